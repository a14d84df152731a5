// DynamicsOutputs.hpp -- the four outputs of DynamicsStep on the device side, like History, Series, Drifters and Stations of
// nextsimdg_amd/outputs.py: each class holds the host object of its output (keys, clock, files: HistoryOutput.hpp, Drifters.hpp,
// Stations.hpp), the list its input file held and its buffers on every row block, and says ONCE how large they are, how a slot is
// addressed and how the blocks' parts become what is written.  The device memory goes with the block it lies on
// (DynamicsBlock::outputBuffer).  A private header of the host sources.
//
// The operations: start(time, blocks) when the run starts; allocate(block) from the block's own thread; afterStep(dt, blocks) after the
// NSDG_PHASE_END mark of every model step -- the sample belongs to no phase and is never part of a captured graph --; atStop(blocks) from
// stop(), which comes twice and writes nothing twice; for the drifters also advance(block, dt) inside every (sub-)step.
#pragma once
#include "BudgetOutput.hpp"
#include "Drifters.hpp"
#include "DynamicsBlock.hpp"
#include "HistoryOutput.hpp"
#include "Stations.hpp"

namespace Nextsim {

//! what a sample reads besides the dynamics' own fields (DynamicsBlock::sources)
struct SampledState {
    bool thermodynamics, advectColumn;
};

//! model.output_period: one plane of the OWNED rows per output field on every block, and one of summed weights if an ice-weighted mean
//! is asked for; a window's record is every block's rows in one host array, finished per statistic
class HistoryChannel {
public:
    HistoryChannel(const HistoryOutput::Config& c, SampledState s) : m_host(c), m_state(s) { }
    void start(long time, std::size_t blocks) { m_host.start(time), m_parts.assign(blocks, Part()); }
    void allocate(DynamicsBlock& b);
    void afterStep(long dt, const DynamicsBlocks& blocks); //!< one sample on every block if the window asks for one, the record if it ends
    void atStop(const DynamicsBlocks& blocks); //!< the window's record from the samples it has, if any

private:
    struct Part {
        double *acc = nullptr, *weight = nullptr;
    };
    static std::size_t plane(const DynamicsBlock& b) { return (std::size_t)b.ownedRows() * b.nx; }
    HistoryOutput m_host;
    SampledState m_state;
    std::vector<Part> m_parts;
};

//! model.series_file: [model.series_buffer][quantities][owned rows] row totals on every block; the lines add them in global row order
class SeriesChannel {
public:
    SeriesChannel(const SeriesOutput::Config& c, SampledState s, double L) : m_host(c), m_state(s), m_L(L) { }
    void start(long time, std::size_t blocks) { m_host.start(time), m_parts.assign(blocks, nullptr); }
    void allocate(DynamicsBlock& b);
    void afterStep(long dt, const DynamicsBlocks& blocks); //!< one row-totals launch on every block into the next slot, the lines if full
    void atStop(const DynamicsBlocks& blocks); //!< the lines of the pending slots, if any

private:
    std::size_t slotSize(const DynamicsBlock& b) const { return m_host.config().ids.size() * (std::size_t)b.ownedRows(); }
    SeriesOutput m_host;
    SampledState m_state;
    double m_L; // dynamics.domain_size
    std::vector<double*> m_parts;
};

//! model.drifters_file: the whole list [3][n] on every block, twice -- a step is out of place --, and with model.drifters_fields the
//! samples [fields][n] at the current positions; every block holds the same after the merge, block 0 writes
class DriftersChannel {
public:
    DriftersChannel(const DriftersOutput::Config& c, SampledState s, std::vector<double> list) : m_host(c), m_state(s), m_list(std::move(list)) { }
    bool any() const { return !m_list.empty(); }
    void start(long time, std::size_t blocks) { m_host.start(time), m_parts.assign(blocks, Part()); }
    void allocate(DynamicsBlock& b);
    //! inside a (sub-)step, after its transport: the drifters of the owned rows move, the blocks' lists are merged and sampled
    void advance(DynamicsBlock& b, double dt);
    void afterStep(long dt, const DynamicsBlocks& blocks); //!< the block of lines of the current clock if a period ends
    void atStop(const DynamicsBlocks& blocks); //!< the block of lines of the last time, once

private:
    struct Part {
        double* list[2] = { nullptr, nullptr };
        int current = 0; // which half holds the positions
        double* samples = nullptr;
    };
    std::size_t count() const { return m_list.size() / 3; }
    std::size_t samplesSize() const { return m_host.config().fieldIds.size() * count(); }
    void write(const DynamicsBlocks& blocks);
    DriftersOutput m_host;
    SampledState m_state;
    std::vector<double> m_list; // what the input file held, [3][n]
    std::vector<Part> m_parts;
    bool m_sampled = false; // a model step has run: the samples are those of the current positions
};

//! model.stations_file: the positions [2][n] and [model.stations_buffer][fields][n] samples on every block; a station belongs to the block
//! whose rows hold its element, the others hold -inf: the maximum over the blocks is the table, block 0 writes
class StationsChannel {
public:
    StationsChannel(const StationsOutput::Config& c, SampledState s, std::vector<double> xy) : m_host(c), m_state(s), m_xy(std::move(xy)) { }
    void start(long time, std::size_t blocks) { m_host.start(time), m_parts.assign(blocks, Part()); }
    void allocate(DynamicsBlock& b);
    void afterStep(long dt, const DynamicsBlocks& blocks); //!< one point-sample launch on every block into the next slot, the lines if full
    void atStop(const DynamicsBlocks& blocks); //!< the lines of the pending slots, if any

private:
    struct Part {
        double *xy = nullptr, *samples = nullptr;
    };
    std::size_t slotSize() const { return m_host.config().ids.size() * (m_xy.size() / 2); }
    StationsOutput m_host;
    SampledState m_state;
    std::vector<double> m_xy; // what the input file held, [2][n]
    std::vector<Part> m_parts;
};

//! model.budget_file / model.budget_series_file: two planes of the LOCAL lattice per term asked for and, with the series, the row totals
//! [NSDG_BUDGET_QUANTITIES][owned rows] on every block.  Unlike the other outputs it launches INSIDE every (sub-)step, right after the
//! sub-cycle and before the transport moves H and A (launch(), from the block's own thread, in the sub-cycle's phase); afterStep()
//! downloads the totals of the step's last launch, adds them in global row order and writes the planes when a record is due
class BudgetChannel {
public:
    explicit BudgetChannel(const BudgetOutput::Config& c) : m_host(c) { }
    void start(long time, std::size_t blocks) { m_host.start(time), m_parts.assign(blocks, Part()); }
    void allocate(DynamicsBlock& b);
    void launch(DynamicsBlock& b); //!< nsdg_momentum_budget on the owned rows, at the state the sub-cycle has just left
    void afterStep(long dt, const DynamicsBlocks& blocks);
    void atStop(const DynamicsBlocks& blocks); //!< model.budget_period = 0: the one record, once

private:
    struct Part {
        double *planes = nullptr, *power = nullptr;
    };
    void write(const DynamicsBlocks& blocks);
    BudgetOutput m_host;
    std::vector<Part> m_parts;
};

} // namespace Nextsim

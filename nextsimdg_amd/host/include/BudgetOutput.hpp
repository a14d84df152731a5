// BudgetOutput.hpp -- the momentum balance diagnostics of the host (include/nsdg_budget.h): records of the nodal
// forces and a time series of the power of every term.  This class is the part that needs no device: the keys, the refusals, the clock
// and the files.  BudgetChannel (src/DynamicsOutputs.hpp) holds the planes and the row totals on every row block, launches
// nsdg_momentum_budget right after the sub-cycle of every (sub-)step and downloads what is written.
//
// Configuration keys (all optional; without budget_file and budget_series_file nothing is allocated, nothing is launched and nothing of a
// run changes):
//     model.budget_file         the name the record files are made from, as model.output_file: forces.nc gives forces.<time, 10 digits>.nc;
//                               the extension picks the format of the history's record writer (.nc / .h5 / .hdf5: HDF5 subset, else header +
//                               float64)
//     model.budget_terms        comma list of the names of nsdg_budget_term_id (default: all eight); a record holds <term>_x and <term>_y
//     model.budget_period       whole seconds, a multiple of model.time_step: a record after the model step in which the integer model clock
//                               reaches (or passes) a multiple of the period; 0 -- the default -- writes ONE record when the run stops
//     model.budget_series_file  a text file with one line per model step: the header "# time <terms> ke", then the integer model clock
//                               after the step, the domain totals of the power of all eight terms [W] and the kinetic energy [J] as %.17g.
//                               The row totals of the device are added in global row order: the file does not depend on
//                               dynamics.row_blocks
// A record is a snapshot of the last (sub-)step of the model step it is written after: planes on the CG2 lattice, (2 ny + 1) x (2 nx + 1),
// node row 2 i + a of the structure's element row i, in the record's own terms x = 2 nx_rows + 1 node rows and y node columns.
//
// Refused before a device is asked for: a run of several processes (nothing gathers their rows), dynamics.rheology = bbm (the brittle
// sub-cycle packs per sub-step with u0 = 0: this balance does not describe it), and a step that has no momentum equation (HipStep).
#pragma once
#include <string>
#include <vector>

namespace Nextsim {

class BudgetOutput {
public:
    struct Config {
        std::string file, seriesFile;
        std::vector<std::string> terms; //!< names, in the order of the record's planes
        std::vector<int> ids; //!< their ids (nsdg_budget_term_id)
        long period = 0;
        bool on() const { return !file.empty() || !seriesFile.empty(); }
    };
    //! model.budget_*, read and checked; throws std::invalid_argument naming the key.  world: the processes of the run; brittle:
    //! dynamics.rheology = bbm.  Touches no device.
    static Config fromConfiguration(int world, bool brittle);
    //! for a step that has no momentum balance (HipStep): throws std::invalid_argument if any model.budget_* key is given
    static void refuseFor(const std::string& stepName);
    //! "# time wind water coriolis tilt internal basal inertia residual ke"
    static std::string headerLine();
    //! the integer model clock and the nine totals as %.17g
    static std::string formatLine(long time, const std::vector<double>& totals);
    //! the totals of one model step from its row totals rows[q * nrows + r] (q: quantity, r: global row order): the rows are added one
    //! after the other
    static std::vector<double> totals(const double* rows, std::size_t nrows);

    explicit BudgetOutput(const Config& c) : m_c(c) { }
    const Config& config() const { return m_c; }
    //! the integer model clock at the start of the run; truncates the series file to its header
    void start(long time);
    //! a model step of dt seconds has run: advances the clock; true if a record is due
    bool step(long dt);
    //! stop(): true once if a record is due (period 0 and a step has run since the last record)
    bool dueAtStop();
    void appendLine(const std::string& line) const;
    long clock() const { return m_clock; }

private:
    Config m_c;
    long m_clock = 0;
    bool m_pending = false; // a step has run since the last record
};

} // namespace Nextsim

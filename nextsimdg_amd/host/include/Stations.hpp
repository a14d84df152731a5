// Stations.hpp -- the model sampled at fixed points of the C++ host: the keys, the text files and the clock of the output blocks; and the
// list of point fields that the drifters' samples (model.drifters_fields, include/Drifters.hpp) share with them.  Needs no device; the class
// that holds the device buffers (StationsChannel, src/DynamicsOutputs.hpp) samples with nsdg_points_sample after every model step, after its NSDG_PHASE_END mark, like
// the history (include/nsdg.h "point samples").
//
// Keys (all under model.*; with none of them given nothing changes):
//     model.stations_file      the input text file: one station per line, "x y" -- metres in the domain [0, L] x [0, L] (x along the
//                              structure's fast index, as the CG2 lattice); lines that start with # and empty lines are skipped.
//                              Empty (the default): no stations
//     model.stations_output    the output text file, truncated at start(): the header "# time id x y <fields>", then one block per MODEL
//                              STEP -- one line per station, in the order of the input: the integer model clock after the step, the
//                              station's index, x, y and the samples as %.17g
//     model.stations_fields    required with the file: a comma-separated list of the history's field names (hice cice u v speed divergence
//                              shear sigma_n sigma_s hsnow tice damage), each evaluated AT the point; damage needs dynamics.rheology = bbm,
//                              hsnow and tice need dynamics.thermodynamics
//     model.stations_buffer    the model steps kept on the device between two downloads (256)
// Row block 0 writes; a station belongs to the block whose rows hold its element, the others hold -inf, and the maximum is the table.
#pragma once
#include <string>
#include <vector>

namespace Nextsim {

//! a comma-separated list of history field names as NSDG_HIST_* ids; throws std::invalid_argument naming `key` for an empty list, an unknown
//! name, a name given twice, damage without the brittle rheology, hsnow / tice without the column model
std::vector<int> parsePointFields(const std::string& key, const std::string& list, bool thermodynamics, bool brittle, std::vector<std::string>& names);

class StationsOutput {
public:
    struct Config {
        std::string file, output;
        std::vector<std::string> names;
        std::vector<int> ids; //!< their NSDG_HIST_* ids
        long buffer = 256;
        bool on() const { return !file.empty(); }
    };
    //! model.stations_*, read and checked; throws std::invalid_argument naming the key.  world: the processes of the run (> 1 is refused:
    //! nothing gathers a multi-process table into one file); loopback: dynamics.loopback_world is set (refused: its rows wrap around).
    //! Touches no device.
    static Config fromConfiguration(int world, bool loopback, bool thermodynamics, bool brittle);
    //! for a step that samples nothing (HipStep): throws std::invalid_argument if any model.stations_* key is given
    static void refuseFor(const std::string& stepName);

    //! the stations of a text file as two planes [2][n] (x, y); every position must lie in [0, Lx] x [0, Ly], else std::invalid_argument
    //! with the file and the line
    static std::vector<double> read(const std::string& path, double Lx, double Ly);
    //! "# time id x y hice shear"
    static std::string headerLine(const std::vector<std::string>& names);
    //! "480 3 1500 2500 0.31 1e-07": samples[k * stride] for k < nfields
    static std::string formatLine(long time, std::size_t id, double x, double y, const double* samples, std::size_t nfields, std::size_t stride);

    explicit StationsOutput(const Config& c);
    const Config& config() const { return m_c; }
    //! the integer model clock at the start of the run; truncates the output file to its header
    void start(long time);
    //! a model step of dt seconds has run: advances the clock and returns the slot of the device buffer its samples go to
    std::size_t step(long dt);
    bool full() const { return (long)m_times.size() >= m_c.buffer; } //!< flush before the next step
    const std::vector<long>& pending() const { return m_times; } //!< the clock after every step since the last flush, slot by slot
    //! appends the pending blocks: table[(s * nfields + k) * n + p] for slot s, field k, station p, and xy = the planes [2][n]; the slots
    //! are free again
    void write(const std::vector<double>& xy, const std::vector<double>& table);

private:
    Config m_c;
    long m_clock = 0;
    std::vector<long> m_times;
};

} // namespace Nextsim

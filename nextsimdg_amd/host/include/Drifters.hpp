// Drifters.hpp -- Lagrangian drifters of the C++ host: the keys, the text files and the clock of the output blocks.  Needs no device; the
// class that holds the device lists (DriftersChannel, src/DynamicsOutputs.hpp) moves the drifters with nsdg_drifters_advance after every transport step and merges the
// row blocks' lists with nsdg_comm_max_f64_array (include/nsdg.h "drifters").
//
// Keys (all under model.*; with none of them given nothing changes):
//     model.drifters_file      the input text file: one drifter per line, "x y" or "x y status" -- metres in the domain [0, L] x [0, L]
//                              (x along the structure's fast index, as the CG2 lattice), status 0 active (the default), 1 left the domain,
//                              2 lost its ice, 3 on land; lines that start with # and empty lines are skipped.  A line of five columns is a
//                              line of the output file, "time id x y status": time and id are ignored, so the block of the last time of
//                              an output file is a valid input file.  Empty (the default): no drifters
//     model.drifters_output    the output text file, truncated at start(): the header "# time id x y status", then one block per period --
//                              one line per drifter, in the order of the input, the integer model clock, the drifter's index and x, y as
//                              %.17g (the file round-trips exactly)
//     model.drifters_period    seconds between two blocks, a multiple of model.time_step; 0 (the default): one block, at stop().  stop()
//                              always writes the block of its time unless a period has just written it
//     model.drifters_min_conc  the cell-mean concentration below which a drifter has lost its ice (0.15)
//     model.drifters_fields    a comma-separated list of the history's field names (include/Stations.hpp: the list the stations share),
//                              sampled AT the new position of every drifter after every (sub-)step (include/nsdg.h "point samples"): the
//                              header becomes "# time id x y status hice cice shear" and every line ends with the samples as %.17g.  A line
//                              of 5 + k columns is read as an output line whose samples are ignored, where the file's own header names k
//                              fields.  Not given (the default): the file is what it always was
// The restart file holds no drifters: a resumed run names the last block as its model.drifters_file.
#pragma once
#include <string>
#include <vector>

namespace Nextsim {

class DriftersOutput {
public:
    struct Config {
        std::string file, output;
        long period = 0;
        double minConc = 0.15;
        std::vector<std::string> fields; //!< model.drifters_fields: the names ...
        std::vector<int> fieldIds; //!< ... and their NSDG_HIST_* ids; empty: positions only
        bool on() const { return !file.empty(); }
    };
    //! model.drifters_*, read and checked; throws std::invalid_argument naming the key.  world: the processes of the run (> 1 is refused:
    //! nothing gathers a multi-process list into one file); loopback: dynamics.loopback_world is set (refused: its values wrap around).
    //! thermodynamics, brittle: what model.drifters_fields may name (hsnow / tice, damage).  Touches no device.
    static Config fromConfiguration(int world, bool loopback, bool thermodynamics = false, bool brittle = false);
    //! for a step that moves no drifters (HipStep): throws std::invalid_argument if any model.drifters_* key is given
    static void refuseFor(const std::string& stepName);

    //! the drifters of a text file as three planes [3][n] (x, y, status); every position must lie in [0, Lx] x [0, Ly] and every status be
    //! 0, 1, 2 or 3, else std::invalid_argument with the file and the line
    static std::vector<double> read(const std::string& path, double Lx, double Ly);
    static std::string headerLine() { return "# time id x y status"; }
    //! "# time id x y status hice cice shear"
    static std::string headerLine(const std::vector<std::string>& fields);
    static std::string formatLine(long time, std::size_t id, double x, double y, double status);
    //! the line with samples[k * stride], k < nfields, at its end
    static std::string formatLine(long time, std::size_t id, double x, double y, double status, const double* samples, std::size_t nfields, std::size_t stride);

    explicit DriftersOutput(const Config& c);
    const Config& config() const { return m_c; }
    //! the integer model clock at the start of the run; truncates the output file to its header
    void start(long time);
    //! a model step of dt seconds has run: advances the clock; true if a block is due now
    bool step(long dt);
    //! stop(): true if the block of the current clock has not been written yet
    bool dueAtStop() const { return !m_written || m_lastWritten != m_clock; }
    //! appends the block of the current clock: planes [3][n] as the device holds them, and the samples [nfields][n] of model.drifters_fields
    //! (empty without the key)
    void write(const std::vector<double>& planes, const std::vector<double>& samples = std::vector<double>());

private:
    Config m_c;
    long m_clock = 0, m_lastWritten = 0;
    bool m_written = false;
};

} // namespace Nextsim

// HistoryOutput.hpp -- gridded output at a chosen period: time means and snapshots of element fields that the device accumulates
// (include/nsdg.h "history output").  This class is the part that needs no device: the keys, the window
// arithmetic and the record files.  HistoryChannel (src/DynamicsOutputs.hpp) holds the accumulators, samples after every model step and downloads at a window end.
//
// Configuration keys (all optional; the period 0 -- the default -- turns the output off and nothing of a run changes):
//     model.output_period   whole seconds, a multiple of model.time_step
//     model.output_file     the name the record files are made from: ice.nsdg gives ice.<time_end, 10 digits>.nsdg, one per window; a
//                           process of a multi-process run appends .rank<r> and writes its own rows
//     model.output_fields   comma list of the names of nsdg_history_field_name (default hice,cice,u,v); an entry may be field:stat with a
//                           statistic of nsdg_history_stat_name -- hice,speed:ice_mean,hice:max --: mean (what the bare name means),
//                           ice_mean (the mean weighted by the concentration clamped to [0, 1]; NaN where the window saw no ice), min
//                           and max (the extremes of the window's samples).  output_kind = snapshot takes bare names only
//     model.output_kind     mean (default): the mean of the samples taken at the end of every model step of the window;
//                           snapshot: the sample of the window's last step alone
// Windows are aligned to absolute model time: a window ends after the model step in which the integer model clock reaches (or passes) a
// multiple of the period.  A run that starts or stops inside a window writes that window with the samples it has, so a restart at a
// window boundary needs no state of the output in the restart file.
//
// Record file.  The extension picks the format, as in RectGrid::dump: .nc / .h5 / .hdf5 are written through Hdf5Writer -- one float64
// dataset /data/<field> of shape (rows, y) per field and the string attributes time_start, time_end, samples, kind, fields, x, y, row0,
// rows of the group /history --, anything else is the plain form: the line "NSDG-HISTORY 1", the same keys as key=value lines,
// END-HEADER and the planes as float64 in the order of `fields`.  A plane has the orientation of the restart file's hice: element
// (i, j) of the structure at i * y + j, rows [row0, row0 + rows) of the x rows.  The dataset of an entry field:stat is /data/<field>_<stat>
// (speed_ice_mean); the attribute `fields` keeps the entries as configured.
//
// SeriesOutput (below): scalar time series of the whole domain -- ice area, extent, volume, mean drift --, one line of text per model step.
//     model.series_file     the text file (empty -- the default -- turns the series off); truncated at start()
//     model.series_fields   comma list of the names of nsdg_history_series_name (default area,extent,volume)
//     model.series_buffer   model steps whose row totals stay on the device between two flushes (default 256)
// The device leaves one total per row and quantity (nsdg_history_row_totals); a flush adds the rows in global row order, so the lines
// do not depend on the row blocks.  A multi-process run is refused: nothing gathers the processes' rows.
#pragma once
#include <string>
#include <vector>

namespace Nextsim {

class HistoryOutput {
public:
    struct Config {
        long period = 0; //!< seconds; 0: off
        std::string file;
        std::vector<std::string> fields; //!< names, in the order of the record's planes
        std::vector<int> ids; //!< their NSDG_HIST_* ids
        std::vector<int> stats; //!< their NSDG_STAT_* ids (NSDG_STAT_MEAN for a bare name)
        bool snapshot = false;
        bool on() const { return period > 0; }
        //! some entry names a statistic: the sample goes through nsdg_history_accumulate_stats
        bool hasStats() const;
        //! some entry is an ice-weighted mean: a weight plane is kept beside the accumulator
        bool weighted() const;
    };
    //! model.output_*, read and checked against model.time_step and what the step can sample; throws std::invalid_argument naming the
    //! key.  thermodynamics: the column model runs (hsnow, tice exist).  Touches no device.
    static Config fromConfiguration(bool thermodynamics, bool brittle = false); //!< brittle: dynamics.rheology = bbm (the field "damage" exists)
    //! for a step that cannot write history (HipStep): throws std::invalid_argument if any model.output_* key is given
    static void refuseFor(const std::string& stepName);

    //! what to do after a model step
    struct Action {
        bool sample = false; //!< take a sample of the state the step left ...
        bool store = false; //!< ... as the first of its window: overwrite the accumulator
        bool flush = false; //!< the window ends with this step: download and write (if it holds a sample)
    };

    explicit HistoryOutput(const Config& c);
    const Config& config() const { return m_c; }
    //! the integer model clock at the start of the run
    void start(long time);
    //! a model step of dt seconds has run: advances the clock and says what follows; counts the sample it asks for
    Action step(long dt);
    //! the window was written (or dropped): the next sample opens a new one
    void closeWindow();
    long clock() const { return m_clock; }
    long samples() const { return m_samples; }
    long windowStart() const { return m_windowStart; } //!< the clock at the start of the first sampled step of the window
    long windowEnd() const { return m_windowEnd; } //!< the clock after the last sampled step

    struct Record {
        long timeStart = 0, timeEnd = 0, samples = 0;
        std::string kind;
        std::vector<std::string> fields;
        long x = 0, y = 0, row0 = 0, rows = 0; //!< the structure's shape and the rows this file holds
        std::vector<double> data; //!< fields.size() planes of rows * y
    };
    //! ice.nsdg, 480 -> ice.0000000480.nsdg (world > 1: ... .rank<r>)
    static std::string recordPath(const std::string& file, long timeEnd, int rank = 0, int world = 1);
    //! the dataset of an entry of `fields`: hice -> hice, speed:ice_mean -> speed_ice_mean
    static std::string datasetName(const std::string& entry);
    //! what the host makes of a window: `acc` (planes of `plane` values, as the device left them) becomes the record's data -- MEAN
    //! acc / samples, ICE_MEAN acc / wacc where wacc > 0 and NaN elsewhere, MIN / MAX as stored.  wacc may be null without ICE_MEAN
    static void finish(const std::vector<int>& stats, long samples, std::size_t plane, const double* wacc, std::vector<double>& acc);
    //! writes `r` in the format the extension of `formatOf` (the configured model.output_file) asks for
    static void write(const std::string& path, const std::string& formatOf, const Record& r);
    static Record read(const std::string& path);

private:
    Config m_c;
    long m_clock = 0, m_samples = 0, m_windowStart = 0, m_windowEnd = 0;
};

//! scalar time series: the keys, the sums over the rows and the text file; needs no device
class SeriesOutput {
public:
    static constexpr double EXTENT_CONC = 0.15; //!< the ice extent counts the cells of at least this concentration
    struct Config {
        std::string file; //!< empty: off
        std::vector<std::string> names;
        std::vector<int> ids; //!< their NSDG_SERIES_* ids
        long buffer = 256;
        bool on() const { return !file.empty(); }
    };
    //! model.series_*, read and checked; throws std::invalid_argument naming the key.  thermodynamics: the column model runs
    //! (snow_volume exists); world: the processes of the run (> 1 is refused: there is no gather).  Touches no device.
    static Config fromConfiguration(bool thermodynamics, int world);
    //! for a step that cannot write series (HipStep): throws std::invalid_argument if any model.series_* key is given
    static void refuseFor(const std::string& stepName);

    //! "# time area extent volume"
    static std::string headerLine(const std::vector<std::string>& names);
    //! "480 1.25e+10 ...": the integer model clock after the step and the totals as %.17g
    static std::string formatLine(long time, const std::vector<double>& totals);
    //! the inverse of formatLine (false for a comment or a malformed line)
    static bool parseLine(const std::string& line, long& time, std::vector<double>& totals);
    //! the totals of one model step from its row totals rows[k * nrows + r] (k: position in ids, r: global row order): the rows are
    //! added one after the other; area and extent times hx hy [m^2], volume and snow_volume times hx hy [m^3], drift = sum(w speed) /
    //! sum(w) [m/s] (NaN without ice), speed_max and hice_max the NaN-keeping maximum
    static std::vector<double> totals(const std::vector<int>& ids, const double* rows, std::size_t nrows, double hx, double hy);
    //! the file with the header line alone / more lines at its end
    static void truncate(const Config& c);
    static void append(const Config& c, const std::vector<std::string>& lines);

    explicit SeriesOutput(const Config& c);
    const Config& config() const { return m_c; }
    //! the integer model clock at the start of the run; truncates the file
    void start(long time);
    //! a model step of dt seconds has run: advances the clock and returns the slot of the device buffer its row totals go to
    std::size_t step(long dt);
    bool full() const { return (long)m_times.size() >= m_c.buffer; } //!< flush before the next step
    const std::vector<long>& pending() const { return m_times; } //!< the clock after every step since the last flush, slot by slot
    void flushed() { m_times.clear(); }

private:
    Config m_c;
    long m_clock = 0;
    std::vector<long> m_times;
};

} // namespace Nextsim

#include "HistoryOutput.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>

#include "../../../include/nsdg.h"
#include "Configured.hpp"
#include "Hdf5Subset.hpp"

namespace Nextsim {

namespace {
struct Keys { }; // (a tag: the keys live under model.*, which belongs to no step class)
const char* const KEY_PERIOD = "model.output_period";
const char* const KEY_FILE = "model.output_file";
const char* const KEY_FIELDS = "model.output_fields";
const char* const KEY_KIND = "model.output_kind";
const char* const KEY_SERIES_FILE = "model.series_file";
const char* const KEY_SERIES_FIELDS = "model.series_fields";
const char* const KEY_SERIES_BUFFER = "model.series_buffer";
const char* const MAGIC = "NSDG-HISTORY 1";

// a whole number of seconds, or std::invalid_argument naming the key
long wholeSeconds(const std::string& key, const std::string& v)
{
    std::size_t used = 0;
    long k = 0;
    try {
        k = std::stol(v, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (v.empty() || used != v.size())
        throw std::invalid_argument(key + " must be a whole number of seconds, got \"" + v + "\"");
    return k;
}

long floorDiv(long a, long b) { return a / b - ((a % b != 0 && (a < 0) != (b < 0)) ? 1 : 0); }

std::string join(const std::vector<std::string>& v)
{
    std::string s;
    for (const auto& x : v)
        s += (s.empty() ? "" : ",") + x;
    return s;
}

std::vector<std::string> split(const std::string& s)
{
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string item; std::getline(ss, item, ',');) {
        const auto a = item.find_first_not_of(" \t"), b = item.find_last_not_of(" \t");
        out.push_back(a == std::string::npos ? std::string() : item.substr(a, b - a + 1));
    }
    return out;
}

// the header of a record as key -> value, in the order both formats write it
std::vector<std::pair<std::string, std::string>> header(const HistoryOutput::Record& r)
{
    return { { "time_start", std::to_string(r.timeStart) }, { "time_end", std::to_string(r.timeEnd) }, { "samples", std::to_string(r.samples) },
        { "kind", r.kind }, { "fields", join(r.fields) }, { "x", std::to_string(r.x) }, { "y", std::to_string(r.y) }, { "row0", std::to_string(r.row0) },
        { "rows", std::to_string(r.rows) } };
}

void fromHeader(const std::map<std::string, std::string>& h, const std::string& path, HistoryOutput::Record& r)
{
    auto at = [&](const char* k) -> const std::string& {
        const auto it = h.find(k);
        if (it == h.end())
            throw std::runtime_error("history record " + path + " has no " + k);
        return it->second;
    };
    r.timeStart = std::stol(at("time_start")), r.timeEnd = std::stol(at("time_end")), r.samples = std::stol(at("samples"));
    r.kind = at("kind");
    r.fields = split(at("fields"));
    r.x = std::stol(at("x")), r.y = std::stol(at("y")), r.row0 = std::stol(at("row0")), r.rows = std::stol(at("rows"));
}
} // namespace

HistoryOutput::Config HistoryOutput::fromConfiguration(bool thermodynamics, bool brittle)
{
    typedef Configured<Keys> C;
    Config c;
    c.period = wholeSeconds(KEY_PERIOD, C::getConfiguration(std::string(KEY_PERIOD), std::string("0")));
    if (c.period < 0)
        throw std::invalid_argument(std::string(KEY_PERIOD) + " must not be negative (0 turns the output off)");
    if (!c.on())
        return c; // off: the other keys are not looked at
    const long step = wholeSeconds("model.time_step", C::getConfiguration(std::string("model.time_step"), std::string("1")));
    if (step <= 0)
        throw std::invalid_argument("model.time_step must be positive");
    if (c.period % step != 0)
        throw std::invalid_argument(std::string(KEY_PERIOD) + " = " + std::to_string(c.period) + " s is not a whole multiple of model.time_step = "
            + std::to_string(step) + " s");
    c.file = C::getConfiguration(std::string(KEY_FILE), std::string(""));
    if (c.file.empty())
        throw std::invalid_argument(std::string(KEY_PERIOD) + " is set: " + KEY_FILE + " must name the record files");
    const std::string kind = C::getConfiguration(std::string(KEY_KIND), std::string("mean"));
    if (kind != "mean" && kind != "snapshot")
        throw std::invalid_argument(std::string(KEY_KIND) + " must be mean or snapshot, got \"" + kind + "\"");
    c.snapshot = kind == "snapshot";
    c.fields = split(C::getConfiguration(std::string(KEY_FIELDS), std::string("hice,cice,u,v")));
    if (c.fields.empty() || c.fields.size() > NSDG_HISTORY_MAX_FIELDS)
        throw std::invalid_argument(std::string(KEY_FIELDS) + " must name 1 to " + std::to_string(NSDG_HISTORY_MAX_FIELDS) + " fields");
    for (const std::string& entry : c.fields) {
        const std::size_t colon = entry.find(':');
        const std::string name = entry.substr(0, colon);
        int stat = NSDG_STAT_MEAN;
        if (colon != std::string::npos) {
            if (c.snapshot)
                throw std::invalid_argument(std::string(KEY_FIELDS) + ": \"" + entry + "\" names a statistic of a window, but " + KEY_KIND
                    + " = snapshot takes one sample: list the bare field names");
            stat = nsdg_history_stat_id(entry.substr(colon + 1).c_str());
            if (stat < 0) {
                std::string known;
                for (int s = 0; s < NSDG_STAT_COUNT; ++s)
                    known += std::string(s ? " " : "") + nsdg_history_stat_name(s);
                throw std::invalid_argument(std::string(KEY_FIELDS) + ": unknown statistic in \"" + entry + "\" (known: " + known + ")");
            }
        }
        const int id = nsdg_history_field_id(name.c_str());
        if (id < 0) {
            std::string known;
            for (int f = 0; f < NSDG_HIST_COUNT; ++f)
                known += std::string(f ? " " : "") + nsdg_history_field_name(f);
            throw std::invalid_argument(std::string(KEY_FIELDS) + ": unknown field \"" + name + "\" (known: " + known + ")");
        }
        for (std::size_t k = 0; k < c.ids.size(); ++k)
            if (c.ids[k] == id && c.stats[k] == stat)
                throw std::invalid_argument(std::string(KEY_FIELDS) + ": field \"" + entry + "\" is listed twice");
        if ((id == NSDG_HIST_HSNOW || id == NSDG_HIST_TICE) && !thermodynamics)
            throw std::invalid_argument(std::string(KEY_FIELDS) + ": field \"" + name + "\" is column state: it needs dynamics.thermodynamics = true");
        if (id == NSDG_HIST_DAMAGE && !brittle)
            throw std::invalid_argument(std::string(KEY_FIELDS) + ": field \"damage\" belongs to the brittle rheology: it needs dynamics.rheology = bbm");
        c.ids.push_back(id);
        c.stats.push_back(stat);
    }
    return c;
}

bool HistoryOutput::Config::hasStats() const
{
    for (const std::string& entry : fields)
        if (entry.find(':') != std::string::npos)
            return true;
    return false;
}

bool HistoryOutput::Config::weighted() const
{
    for (int s : stats)
        if (s == NSDG_STAT_ICE_MEAN)
            return true;
    return false;
}

std::string HistoryOutput::datasetName(const std::string& entry)
{
    std::string name = entry;
    const std::size_t colon = name.find(':');
    if (colon != std::string::npos)
        name[colon] = '_';
    return name;
}

void HistoryOutput::finish(const std::vector<int>& stats, long samples, std::size_t plane, const double* wacc, std::vector<double>& acc)
{
    const double n = (double)samples;
    for (std::size_t k = 0; k < stats.size(); ++k) {
        double* a = acc.data() + k * plane;
        if (stats[k] == NSDG_STAT_MEAN)
            for (std::size_t i = 0; i < plane; ++i)
                a[i] /= n;
        else if (stats[k] == NSDG_STAT_ICE_MEAN)
            for (std::size_t i = 0; i < plane; ++i)
                a[i] = wacc && wacc[i] > 0. ? a[i] / wacc[i] : std::numeric_limits<double>::quiet_NaN(); // NaN: no ice in the window
    }
}

void HistoryOutput::refuseFor(const std::string& stepName)
{
    std::string raw;
    for (const char* key : { KEY_PERIOD, KEY_FILE, KEY_FIELDS, KEY_KIND })
        if (Configurator::lookup(key, raw))
            throw std::invalid_argument(std::string(key) + " is set, but " + stepName + " writes no history output: select Nextsim::DynamicsStep");
}

// ---- SeriesOutput
SeriesOutput::Config SeriesOutput::fromConfiguration(bool thermodynamics, int world)
{
    typedef Configured<Keys> C;
    Config c;
    c.file = C::getConfiguration(std::string(KEY_SERIES_FILE), std::string(""));
    if (!c.on())
        return c; // off: the other keys are not looked at
    if (world > 1)
        throw std::invalid_argument(std::string(KEY_SERIES_FILE) + " is set in a run of " + std::to_string(world)
            + " processes: there is no gather of the processes' row totals, a series needs a single process (dynamics.row_blocks splits one)");
    c.names = split(C::getConfiguration(std::string(KEY_SERIES_FIELDS), std::string("area,extent,volume")));
    if (c.names.empty() || c.names.size() > NSDG_SERIES_COUNT)
        throw std::invalid_argument(std::string(KEY_SERIES_FIELDS) + " must name 1 to " + std::to_string(NSDG_SERIES_COUNT) + " quantities");
    bool area = false, drift = false;
    for (const std::string& name : c.names) {
        const int id = nsdg_history_series_id(name.c_str());
        if (id < 0) {
            std::string known;
            for (int q = 0; q < NSDG_SERIES_COUNT; ++q)
                known += std::string(q ? " " : "") + nsdg_history_series_name(q);
            throw std::invalid_argument(std::string(KEY_SERIES_FIELDS) + ": unknown quantity \"" + name + "\" (known: " + known + ")");
        }
        for (int other : c.ids)
            if (other == id)
                throw std::invalid_argument(std::string(KEY_SERIES_FIELDS) + ": quantity \"" + name + "\" is listed twice");
        if (id == NSDG_SERIES_SNOW_VOLUME && !thermodynamics)
            throw std::invalid_argument(std::string(KEY_SERIES_FIELDS) + ": quantity \"snow_volume\" is column state: it needs dynamics.thermodynamics = true");
        area = area || id == NSDG_SERIES_AREA, drift = drift || id == NSDG_SERIES_DRIFT;
        c.ids.push_back(id);
    }
    if (drift && !area)
        throw std::invalid_argument(std::string(KEY_SERIES_FIELDS) + ": quantity \"drift\" is the ice-weighted mean speed: it needs \"area\", the sum of the weights, in the list");
    const std::string buffer = C::getConfiguration(std::string(KEY_SERIES_BUFFER), std::string("256"));
    std::size_t used = 0;
    try {
        c.buffer = std::stol(buffer, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (buffer.empty() || used != buffer.size() || c.buffer < 1)
        throw std::invalid_argument(std::string(KEY_SERIES_BUFFER) + " must be a whole number of model steps, at least 1, got \"" + buffer + "\"");
    return c;
}

void SeriesOutput::refuseFor(const std::string& stepName)
{
    std::string raw;
    for (const char* key : { KEY_SERIES_FILE, KEY_SERIES_FIELDS, KEY_SERIES_BUFFER })
        if (Configurator::lookup(key, raw))
            throw std::invalid_argument(std::string(key) + " is set, but " + stepName + " writes no time series: select Nextsim::DynamicsStep");
}

SeriesOutput::SeriesOutput(const Config& c)
    : m_c(c)
{
    if (!c.on())
        throw std::invalid_argument("SeriesOutput: the file must be named");
}

void SeriesOutput::start(long time)
{
    m_clock = time;
    m_times.clear();
    truncate(m_c);
}

std::size_t SeriesOutput::step(long dt)
{
    if (full())
        throw std::logic_error("SeriesOutput::step: the buffer is full, flush first");
    m_clock += dt;
    m_times.push_back(m_clock);
    return m_times.size() - 1;
}

std::string SeriesOutput::headerLine(const std::vector<std::string>& names)
{
    std::string s = "# time";
    for (const std::string& n : names)
        s += " " + n;
    return s;
}

std::string SeriesOutput::formatLine(long time, const std::vector<double>& totals)
{
    std::string s = std::to_string(time);
    char buf[40];
    for (double x : totals) {
        std::snprintf(buf, sizeof buf, " %.17g", x);
        s += buf;
    }
    return s;
}

bool SeriesOutput::parseLine(const std::string& line, long& time, std::vector<double>& totals)
{
    if (line.empty() || line[0] == '#')
        return false;
    std::stringstream ss(line);
    std::string word;
    if (!(ss >> word))
        return false;
    std::size_t used = 0;
    try {
        time = std::stol(word, &used);
    } catch (const std::exception&) {
        return false;
    }
    if (used != word.size())
        return false;
    totals.clear();
    while (ss >> word) { // strtod reads nan and inf as well, which operator>> does not
        char* end = nullptr;
        const double x = std::strtod(word.c_str(), &end);
        if (end == word.c_str() || *end)
            return false;
        totals.push_back(x);
    }
    return true;
}

std::vector<double> SeriesOutput::totals(const std::vector<int>& ids, const double* rows, std::size_t nrows, double hx, double hy)
{
    std::vector<double> out(ids.size(), 0.);
    double area = std::numeric_limits<double>::quiet_NaN();
    for (std::size_t k = 0; k < ids.size(); ++k) {
        const double* r = rows + k * nrows;
        const bool isMax = ids[k] == NSDG_SERIES_SPEED_MAX || ids[k] == NSDG_SERIES_HICE_MAX;
        double t = isMax ? -std::numeric_limits<double>::infinity() : 0.;
        for (std::size_t i = 0; i < nrows; ++i) // one row after the other, in global row order: the same bits for any row blocks
            t = isMax ? ((r[i] > t || r[i] != r[i]) ? r[i] : t) : t + r[i];
        out[k] = t;
        if (ids[k] == NSDG_SERIES_AREA)
            area = t;
    }
    const double cell = hx * hy;
    for (std::size_t k = 0; k < ids.size(); ++k) {
        if (ids[k] == NSDG_SERIES_DRIFT)
            out[k] = area > 0. ? out[k] / area : std::numeric_limits<double>::quiet_NaN();
        else if (ids[k] <= NSDG_SERIES_SNOW_VOLUME)
            out[k] *= cell;
    }
    return out;
}

void SeriesOutput::truncate(const Config& c)
{
    std::ofstream f(c.file, std::ios::trunc);
    f << headerLine(c.names) << "\n";
    f.close();
    if (!f)
        throw std::runtime_error(std::string(KEY_SERIES_FILE) + ": cannot write " + c.file);
}

void SeriesOutput::append(const Config& c, const std::vector<std::string>& lines)
{
    std::ofstream f(c.file, std::ios::app);
    for (const std::string& line : lines)
        f << line << "\n";
    f.close();
    if (!f)
        throw std::runtime_error(std::string(KEY_SERIES_FILE) + ": cannot write " + c.file);
}

HistoryOutput::HistoryOutput(const Config& c)
    : m_c(c)
{
    if (!c.on())
        throw std::invalid_argument("HistoryOutput: the period must be positive");
}

void HistoryOutput::start(long time)
{
    m_clock = time;
    closeWindow();
}

HistoryOutput::Action HistoryOutput::step(long dt)
{
    const long t0 = m_clock, t1 = t0 + dt;
    m_clock = t1;
    Action a;
    a.flush = floorDiv(t1, m_c.period) > floorDiv(t0, m_c.period); // the clock has reached (or passed) a multiple of the period
    a.sample = !m_c.snapshot || a.flush;
    if (a.sample) {
        a.store = m_samples == 0;
        if (m_samples == 0)
            m_windowStart = t0;
        ++m_samples;
        m_windowEnd = t1;
    }
    return a;
}

void HistoryOutput::closeWindow() { m_samples = 0, m_windowStart = m_windowEnd = m_clock; }

std::string HistoryOutput::recordPath(const std::string& file, long timeEnd, int rank, int world)
{
    char stamp[32];
    std::snprintf(stamp, sizeof stamp, "%s%010ld", timeEnd < 0 ? "-" : "", timeEnd < 0 ? -timeEnd : timeEnd);
    const std::size_t slash = file.find_last_of('/'), dot = file.find_last_of('.');
    const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1) && dot > 0;
    std::string path = ext ? file.substr(0, dot) + "." + stamp + file.substr(dot) : file + "." + stamp;
    if (world > 1)
        path += ".rank" + std::to_string(rank);
    return path;
}

void HistoryOutput::write(const std::string& path, const std::string& formatOf, const Record& r)
{
    const std::size_t plane = (std::size_t)r.rows * (std::size_t)r.y;
    if (r.data.size() != plane * r.fields.size())
        throw std::logic_error("HistoryOutput::write: the record's data do not have fields x rows x y values");
    if (Hdf5File::hasHdf5Extension(formatOf)) {
        Hdf5Writer w;
        w.group("/history");
        for (const auto& kv : header(r))
            w.stringAttribute("/history", kv.first, kv.second);
        w.group("/data");
        for (std::size_t k = 0; k < r.fields.size(); ++k)
            w.dataset("/data/" + datasetName(r.fields[k]), { (std::uint64_t)r.rows, (std::uint64_t)r.y },
                std::vector<double>(r.data.begin() + k * plane, r.data.begin() + (k + 1) * plane));
        w.write(path);
        return;
    }
    std::ofstream f(path, std::ios::binary);
    f << MAGIC << "\n";
    for (const auto& kv : header(r))
        f << kv.first << "=" << kv.second << "\n";
    f << "END-HEADER\n";
    f.write(reinterpret_cast<const char*>(r.data.data()), (std::streamsize)(r.data.size() * sizeof(double)));
    f.close();
    if (!f)
        throw std::runtime_error("model.output_file: cannot write " + path);
}

HistoryOutput::Record HistoryOutput::read(const std::string& path)
{
    Record r;
    std::map<std::string, std::string> h;
    if (Hdf5File::isHdf5(path)) {
        const Hdf5File file(path);
        for (const char* k : { "time_start", "time_end", "samples", "kind", "fields", "x", "y", "row0", "rows" })
            if (file.hasAttribute("/history", k))
                h[k] = file.stringAttribute("/history", k);
        fromHeader(h, path, r);
        for (const std::string& entry : r.fields) {
            const std::string name = datasetName(entry);
            const std::vector<std::uint64_t> d = file.dims("/data/" + name);
            if (d.size() != 2 || (long)d[0] != r.rows || (long)d[1] != r.y)
                throw std::runtime_error("history record " + path + ": " + name + " does not have the shape (rows, y)");
            const std::vector<double> v = file.readDoubles("/data/" + name);
            r.data.insert(r.data.end(), v.begin(), v.end());
        }
        return r;
    }
    std::ifstream f(path, std::ios::binary);
    std::string line;
    if (!f || !std::getline(f, line) || line != MAGIC)
        throw std::runtime_error("cannot read history record " + path);
    while (std::getline(f, line) && line != "END-HEADER") {
        const auto eq = line.find('=');
        if (eq != std::string::npos)
            h[line.substr(0, eq)] = line.substr(eq + 1);
    }
    fromHeader(h, path, r);
    r.data.resize(r.fields.size() * (std::size_t)r.rows * (std::size_t)r.y);
    f.read(reinterpret_cast<char*>(r.data.data()), (std::streamsize)(r.data.size() * sizeof(double)));
    if (!f)
        throw std::runtime_error("history record " + path + " is truncated");
    return r;
}

} // namespace Nextsim

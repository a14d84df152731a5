#include "HistoryOutput.hpp"

#include <cstdio>
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

HistoryOutput::Config HistoryOutput::fromConfiguration(bool thermodynamics)
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
    for (const std::string& name : c.fields) {
        const int id = nsdg_history_field_id(name.c_str());
        if (id < 0) {
            std::string known;
            for (int f = 0; f < NSDG_HIST_COUNT; ++f)
                known += std::string(f ? " " : "") + nsdg_history_field_name(f);
            throw std::invalid_argument(std::string(KEY_FIELDS) + ": unknown field \"" + name + "\" (known: " + known + ")");
        }
        for (int other : c.ids)
            if (other == id)
                throw std::invalid_argument(std::string(KEY_FIELDS) + ": field \"" + name + "\" is listed twice");
        if ((id == NSDG_HIST_HSNOW || id == NSDG_HIST_TICE) && !thermodynamics)
            throw std::invalid_argument(std::string(KEY_FIELDS) + ": field \"" + name + "\" is column state: it needs dynamics.thermodynamics = true");
        if (id == NSDG_HIST_DAMAGE)
            throw std::invalid_argument(std::string(KEY_FIELDS) + ": field \"damage\" belongs to the brittle rheology, which this host does not run");
        c.ids.push_back(id);
    }
    return c;
}

void HistoryOutput::refuseFor(const std::string& stepName)
{
    std::string raw;
    for (const char* key : { KEY_PERIOD, KEY_FILE, KEY_FIELDS, KEY_KIND })
        if (Configurator::lookup(key, raw))
            throw std::invalid_argument(std::string(key) + " is set, but " + stepName + " writes no history output: select Nextsim::DynamicsStep");
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
            w.dataset("/data/" + r.fields[k], { (std::uint64_t)r.rows, (std::uint64_t)r.y },
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
        for (const std::string& name : r.fields) {
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

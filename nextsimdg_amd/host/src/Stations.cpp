#include "Stations.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "Configured.hpp"
#include "../../../include/nsdg.h"

namespace Nextsim {

namespace {
struct Keys { }; // (a tag: the keys live under model.*, which belongs to no step class)
const char* const KEY_FILE = "model.stations_file";
const char* const KEY_OUTPUT = "model.stations_output";
const char* const KEY_FIELDS = "model.stations_fields";
const char* const KEY_BUFFER = "model.stations_buffer";
} // namespace

std::vector<int> parsePointFields(const std::string& key, const std::string& list, bool thermodynamics, bool brittle, std::vector<std::string>& names)
{
    std::vector<int> ids;
    names.clear();
    std::stringstream ss(list);
    for (std::string name; std::getline(ss, name, ',');) {
        const auto a = name.find_first_not_of(" \t"), b = name.find_last_not_of(" \t");
        name = a == std::string::npos ? std::string() : name.substr(a, b - a + 1);
        if (name.empty())
            continue;
        const int id = nsdg_history_field_id(name.c_str());
        if (id < 0) {
            std::string known;
            for (int f = 0; f < NSDG_HIST_COUNT; ++f)
                known += std::string(f ? " " : "") + nsdg_history_field_name(f);
            throw std::invalid_argument(key + ": unknown field \"" + name + "\" (known: " + known + ")");
        }
        for (const int seen : ids)
            if (seen == id)
                throw std::invalid_argument(key + ": field \"" + name + "\" is listed twice");
        if (id == NSDG_HIST_DAMAGE && !brittle)
            throw std::invalid_argument(key + ": the field \"damage\" needs dynamics.rheology = bbm: the mEVP sub-cycle has no damage");
        if ((id == NSDG_HIST_HSNOW || id == NSDG_HIST_TICE) && !thermodynamics)
            throw std::invalid_argument(key + ": the field \"" + name + "\" is column state: it needs dynamics.thermodynamics = true");
        ids.push_back(id);
        names.push_back(name);
    }
    if (ids.empty())
        throw std::invalid_argument(key + " names no field");
    return ids;
}

StationsOutput::Config StationsOutput::fromConfiguration(int world, bool loopback, bool thermodynamics, bool brittle)
{
    typedef Configured<Keys> C;
    Config c;
    c.file = C::getConfiguration(std::string(KEY_FILE), std::string(""));
    if (!c.on()) {
        std::string raw;
        for (const char* key : { KEY_OUTPUT, KEY_FIELDS, KEY_BUFFER })
            if (Configurator::lookup(key, raw))
                throw std::invalid_argument(std::string(key) + " is set without " + KEY_FILE + ": there are no stations to sample at");
        return c;
    }
    if (world > 1)
        throw std::invalid_argument(std::string(KEY_FILE) + " is set in a run of " + std::to_string(world)
            + " processes: nothing gathers the processes' samples into one output file, stations need a single process (dynamics.row_blocks splits one)");
    if (loopback)
        throw std::invalid_argument(std::string(KEY_FILE) + " is set with dynamics.loopback_world: the rehearsal's rows wrap around, a station would sample them");
    c.output = C::getConfiguration(std::string(KEY_OUTPUT), std::string(""));
    if (c.output.empty())
        throw std::invalid_argument(std::string(KEY_FILE) + " is set: " + KEY_OUTPUT + " must name the file the samples are written to");
    std::string raw;
    if (!Configurator::lookup(KEY_FIELDS, raw))
        throw std::invalid_argument(std::string(KEY_FILE) + " is set: " + KEY_FIELDS + " must list the fields sampled at the stations");
    c.ids = parsePointFields(KEY_FIELDS, C::getConfiguration(std::string(KEY_FIELDS), std::string("")), thermodynamics, brittle, c.names);
    const std::string buffer = C::getConfiguration(std::string(KEY_BUFFER), std::string("256"));
    std::size_t used = 0;
    try {
        c.buffer = std::stol(buffer, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (buffer.empty() || used != buffer.size() || c.buffer < 1)
        throw std::invalid_argument(std::string(KEY_BUFFER) + " must be a whole number of model steps, at least 1, got \"" + buffer + "\"");
    return c;
}

void StationsOutput::refuseFor(const std::string& stepName)
{
    std::string raw;
    for (const char* key : { KEY_FILE, KEY_OUTPUT, KEY_FIELDS, KEY_BUFFER })
        if (Configurator::lookup(key, raw))
            throw std::invalid_argument(std::string(key) + " is set, but " + stepName + " has no dynamics state to sample: select Nextsim::DynamicsStep");
}

std::vector<double> StationsOutput::read(const std::string& path, double Lx, double Ly)
{
    std::ifstream in(path);
    if (!in)
        throw std::invalid_argument(std::string(KEY_FILE) + ": cannot read " + path);
    std::vector<double> xs, ys;
    std::string line;
    for (long no = 1; std::getline(in, line); ++no) {
        const auto first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#')
            continue;
        const std::string where = std::string(KEY_FILE) + " " + path + ", line " + std::to_string(no) + ": ";
        std::vector<double> v;
        std::stringstream ss(line);
        for (std::string tok; ss >> tok;) {
            char* end = nullptr;
            const double d = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end != '\0')
                throw std::invalid_argument(where + "\"" + tok + "\" is not a number");
            v.push_back(d);
        }
        if (v.size() != 2)
            throw std::invalid_argument(where + std::to_string(v.size()) + " columns; a line is \"x y\"");
        if (!(v[0] >= 0. && v[0] <= Lx && v[1] >= 0. && v[1] <= Ly)) // (a NaN too)
            throw std::invalid_argument(where + "the station is outside the domain [0, " + std::to_string(Lx) + "] x [0, " + std::to_string(Ly) + "] m");
        xs.push_back(v[0]), ys.push_back(v[1]);
    }
    std::vector<double> planes(xs);
    planes.insert(planes.end(), ys.begin(), ys.end());
    return planes;
}

std::string StationsOutput::headerLine(const std::vector<std::string>& names)
{
    std::string h = "# time id x y";
    for (const std::string& n : names)
        h += " " + n;
    return h;
}

std::string StationsOutput::formatLine(long time, std::size_t id, double x, double y, const double* samples, std::size_t nfields, std::size_t stride)
{
    char buf[96];
    std::snprintf(buf, sizeof buf, "%ld %zu %.17g %.17g", time, id, x, y);
    std::string line = buf;
    for (std::size_t k = 0; k < nfields; ++k) {
        std::snprintf(buf, sizeof buf, " %.17g", samples[k * stride]);
        line += buf;
    }
    return line;
}

StationsOutput::StationsOutput(const Config& c)
    : m_c(c)
{
    if (!c.on() || c.output.empty() || c.ids.empty() || c.buffer < 1)
        throw std::invalid_argument("StationsOutput: the input file, the output file and the fields must be named, the buffer hold a step");
}

void StationsOutput::start(long time)
{
    m_clock = time;
    m_times.clear();
    std::ofstream out(m_c.output, std::ios::trunc);
    out << headerLine(m_c.names) << "\n";
    if (!out)
        throw std::runtime_error(std::string(KEY_OUTPUT) + ": cannot write " + m_c.output);
}

std::size_t StationsOutput::step(long dt)
{
    if (full())
        throw std::logic_error("StationsOutput::step: the buffer is full, write() comes first");
    m_clock += dt;
    m_times.push_back(m_clock);
    return m_times.size() - 1;
}

void StationsOutput::write(const std::vector<double>& xy, const std::vector<double>& table)
{
    const std::size_t n = xy.size() / 2, nf = m_c.ids.size();
    if (table.size() != m_times.size() * nf * n)
        throw std::logic_error("StationsOutput::write: the table does not hold slots x fields x stations values");
    std::ofstream out(m_c.output, std::ios::app);
    for (std::size_t s = 0; s < m_times.size(); ++s)
        for (std::size_t p = 0; p < n; ++p)
            out << formatLine(m_times[s], p, xy[p], xy[n + p], table.data() + s * nf * n + p, nf, n) << "\n";
    out.flush();
    if (!out)
        throw std::runtime_error(std::string(KEY_OUTPUT) + ": cannot write " + m_c.output);
    m_times.clear();
}

} // namespace Nextsim

#include "Drifters.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "Configured.hpp"
#include "Stations.hpp"

namespace Nextsim {

namespace {
struct Keys { }; // (a tag: the keys live under model.*, which belongs to no step class)
const char* const KEY_FILE = "model.drifters_file";
const char* const KEY_OUTPUT = "model.drifters_output";
const char* const KEY_PERIOD = "model.drifters_period";
const char* const KEY_MIN_CONC = "model.drifters_min_conc";
const char* const KEY_FIELDS = "model.drifters_fields";

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
} // namespace

DriftersOutput::Config DriftersOutput::fromConfiguration(int world, bool loopback, bool thermodynamics, bool brittle)
{
    typedef Configured<Keys> C;
    Config c;
    c.file = C::getConfiguration(std::string(KEY_FILE), std::string(""));
    if (!c.on()) {
        std::string raw;
        for (const char* key : { KEY_OUTPUT, KEY_PERIOD, KEY_MIN_CONC, KEY_FIELDS })
            if (Configurator::lookup(key, raw))
                throw std::invalid_argument(std::string(key) + " is set without " + KEY_FILE + ": there are no drifters to move");
        return c;
    }
    if (world > 1)
        throw std::invalid_argument(std::string(KEY_FILE) + " is set in a run of " + std::to_string(world)
            + " processes: nothing gathers the processes' drifters into one output file, drifters need a single process (dynamics.row_blocks splits one)");
    if (loopback)
        throw std::invalid_argument(std::string(KEY_FILE) + " is set with dynamics.loopback_world: the rehearsal's ghost rows wrap around, a drifter would follow them");
    c.output = C::getConfiguration(std::string(KEY_OUTPUT), std::string(""));
    if (c.output.empty())
        throw std::invalid_argument(std::string(KEY_FILE) + " is set: " + KEY_OUTPUT + " must name the file the positions are written to");
    c.period = wholeSeconds(KEY_PERIOD, C::getConfiguration(std::string(KEY_PERIOD), std::string("0")));
    if (c.period < 0)
        throw std::invalid_argument(std::string(KEY_PERIOD) + " must not be negative (0: one block, at the end of the run)");
    const long step = wholeSeconds("model.time_step", C::getConfiguration(std::string("model.time_step"), std::string("1")));
    if (step <= 0)
        throw std::invalid_argument("model.time_step must be positive");
    if (c.period % step != 0)
        throw std::invalid_argument(std::string(KEY_PERIOD) + " = " + std::to_string(c.period) + " s is no multiple of model.time_step = " + std::to_string(step) + " s");
    c.minConc = C::getConfiguration(std::string(KEY_MIN_CONC), 0.15);
    if (!std::isfinite(c.minConc))
        throw std::invalid_argument(std::string(KEY_MIN_CONC) + " must be finite");
    std::string raw;
    if (Configurator::lookup(KEY_FIELDS, raw))
        c.fieldIds = parsePointFields(KEY_FIELDS, C::getConfiguration(std::string(KEY_FIELDS), std::string("")), thermodynamics, brittle, c.fields);
    return c;
}

void DriftersOutput::refuseFor(const std::string& stepName)
{
    std::string raw;
    for (const char* key : { KEY_FILE, KEY_OUTPUT, KEY_PERIOD, KEY_MIN_CONC, KEY_FIELDS })
        if (Configurator::lookup(key, raw))
            throw std::invalid_argument(std::string(key) + " is set, but " + stepName + " has no ice velocity to move drifters with: select Nextsim::DynamicsStep");
}

std::vector<double> DriftersOutput::read(const std::string& path, double Lx, double Ly)
{
    std::ifstream in(path);
    if (!in)
        throw std::invalid_argument(std::string(KEY_FILE) + ": cannot read " + path);
    struct Row {
        double x, y, status;
    };
    std::vector<Row> rows;
    std::string line;
    std::size_t extra = 0; // the fields the file's own header names after "# time id x y status": an output line has 5 + extra columns
    for (long no = 1; std::getline(in, line); ++no) {
        const auto first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos)
            continue;
        if (line[first] == '#') {
            std::stringstream hs(line.substr(first));
            std::vector<std::string> words;
            for (std::string w; hs >> w;)
                words.push_back(w);
            const std::vector<std::string> head = { "#", "time", "id", "x", "y", "status" };
            if (words.size() >= head.size() && std::vector<std::string>(words.begin(), words.begin() + head.size()) == head)
                extra = words.size() - head.size();
            continue;
        }
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
        if (extra > 0 && v.size() == 5 + extra) // an output line with samples: they are ignored
            v.resize(5);
        if (v.size() != 2 && v.size() != 3 && v.size() != 5)
            throw std::invalid_argument(where + std::to_string(v.size()) + " columns; a line is \"x y\", \"x y status\" or \"time id x y status\"");
        Row r;
        const std::size_t at = v.size() == 5 ? 2 : 0; // a line of the output file: time and id are ignored
        r.x = v[at], r.y = v[at + 1], r.status = v.size() == 2 ? 0. : v[at + 2];
        if (!(r.x >= 0. && r.x <= Lx && r.y >= 0. && r.y <= Ly)) // (a NaN too)
            throw std::invalid_argument(where + "the position is outside the domain [0, " + std::to_string(Lx) + "] x [0, " + std::to_string(Ly) + "] m");
        if (r.status != 0. && r.status != 1. && r.status != 2. && r.status != 3.)
            throw std::invalid_argument(where + "unknown status; known: 0 active, 1 left the domain, 2 lost its ice, 3 on land");
        rows.push_back(r);
    }
    const std::size_t n = rows.size();
    std::vector<double> planes(3 * n);
    for (std::size_t i = 0; i < n; ++i)
        planes[i] = rows[i].x, planes[n + i] = rows[i].y, planes[2 * n + i] = rows[i].status;
    return planes;
}

std::string DriftersOutput::formatLine(long time, std::size_t id, double x, double y, double status)
{
    char buf[160];
    std::snprintf(buf, sizeof buf, "%ld %zu %.17g %.17g %d", time, id, x, y, (int)status);
    return buf;
}

std::string DriftersOutput::headerLine(const std::vector<std::string>& fields)
{
    std::string h = headerLine();
    for (const std::string& f : fields)
        h += " " + f;
    return h;
}

std::string DriftersOutput::formatLine(long time, std::size_t id, double x, double y, double status, const double* samples, std::size_t nfields,
    std::size_t stride)
{
    std::string line = formatLine(time, id, x, y, status);
    char buf[48];
    for (std::size_t k = 0; k < nfields; ++k) {
        std::snprintf(buf, sizeof buf, " %.17g", samples[k * stride]);
        line += buf;
    }
    return line;
}

DriftersOutput::DriftersOutput(const Config& c)
    : m_c(c)
{
    if (!c.on() || c.output.empty())
        throw std::invalid_argument("DriftersOutput: the input and the output file must be named");
}

void DriftersOutput::start(long time)
{
    m_clock = time;
    m_written = false;
    std::ofstream out(m_c.output, std::ios::trunc);
    out << headerLine(m_c.fields) << "\n";
    if (!out)
        throw std::runtime_error(std::string(KEY_OUTPUT) + ": cannot write " + m_c.output);
}

bool DriftersOutput::step(long dt)
{
    m_clock += dt;
    return m_c.period > 0 && m_clock % m_c.period == 0;
}

void DriftersOutput::write(const std::vector<double>& planes, const std::vector<double>& samples)
{
    const std::size_t n = planes.size() / 3, nf = m_c.fieldIds.size();
    if (samples.size() != nf * n)
        throw std::logic_error("DriftersOutput::write: the samples do not hold fields x drifters values");
    std::ofstream out(m_c.output, std::ios::app);
    for (std::size_t i = 0; i < n; ++i)
        out << formatLine(m_clock, i, planes[i], planes[n + i], planes[2 * n + i], nf ? samples.data() + i : nullptr, nf, n) << "\n";
    out.flush();
    if (!out)
        throw std::runtime_error(std::string(KEY_OUTPUT) + ": cannot write " + m_c.output);
    m_lastWritten = m_clock;
    m_written = true;
}

} // namespace Nextsim

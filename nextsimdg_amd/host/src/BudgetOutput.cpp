#include "BudgetOutput.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "../../../include/nsdg.h"
#include "Configured.hpp"

namespace Nextsim {

namespace {
struct Keys { }; // (a tag: the keys live under model.*)
const char* const KEY_FILE = "model.budget_file";
const char* const KEY_TERMS = "model.budget_terms";
const char* const KEY_PERIOD = "model.budget_period";
const char* const KEY_SERIES = "model.budget_series_file";
const char* const TERMS[NSDG_BUDGET_TERMS] = { "wind", "water", "coriolis", "tilt", "internal", "basal", "inertia", "residual" };

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
} // namespace

BudgetOutput::Config BudgetOutput::fromConfiguration(int world, bool brittle)
{
    typedef Configured<Keys> C;
    Config c;
    c.file = C::getConfiguration(std::string(KEY_FILE), std::string(""));
    c.seriesFile = C::getConfiguration(std::string(KEY_SERIES), std::string(""));
    std::string raw;
    if (!c.on()) {
        for (const char* key : { KEY_TERMS, KEY_PERIOD })
            if (Configurator::lookup(key, raw))
                throw std::invalid_argument(std::string(key) + " is set: " + KEY_FILE + " must name the record files");
        return c;
    }
    const char* first = c.file.empty() ? KEY_SERIES : KEY_FILE;
    if (world > 1)
        throw std::invalid_argument(std::string(first) + " is set in a run of " + std::to_string(world)
            + " processes: there is no gather of the processes' rows, the momentum budget needs a single process (dynamics.row_blocks splits one)");
    if (brittle)
        throw std::invalid_argument(std::string(first) + " is set with dynamics.rheology = bbm: the brittle sub-cycle packs per sub-step with u0 = 0, "
                                                         "this balance does not describe it; the momentum budget needs dynamics.rheology = mevp");
    std::string list = C::getConfiguration(std::string(KEY_TERMS), std::string(""));
    if (list.empty())
        for (const char* t : TERMS)
            list += std::string(list.empty() ? "" : ",") + t;
    std::stringstream ss(list);
    for (std::string item; std::getline(ss, item, ',');) {
        const auto a = item.find_first_not_of(" \t"), b = item.find_last_not_of(" \t");
        const std::string name = a == std::string::npos ? std::string() : item.substr(a, b - a + 1);
        const int id = nsdg_budget_term_id(name.c_str());
        if (id < 0) {
            std::string known;
            for (const char* t : TERMS)
                known += std::string(known.empty() ? "" : " ") + t;
            throw std::invalid_argument(std::string(KEY_TERMS) + ": unknown term \"" + name + "\" (known: " + known + ")");
        }
        for (int other : c.ids)
            if (other == id)
                throw std::invalid_argument(std::string(KEY_TERMS) + ": \"" + name + "\" is named more than once");
        c.terms.push_back(name), c.ids.push_back(id);
    }
    c.period = wholeSeconds(KEY_PERIOD, C::getConfiguration(std::string(KEY_PERIOD), std::string("0")));
    if (c.period < 0)
        throw std::invalid_argument(std::string(KEY_PERIOD) + " must not be negative (0 writes one record at the end)");
    if (c.period > 0) {
        if (c.file.empty())
            throw std::invalid_argument(std::string(KEY_PERIOD) + " is set: " + KEY_FILE + " must name the record files");
        const long step = wholeSeconds("model.time_step", C::getConfiguration(std::string("model.time_step"), std::string("1")));
        if (step <= 0)
            throw std::invalid_argument("model.time_step must be positive");
        if (c.period % step != 0)
            throw std::invalid_argument(std::string(KEY_PERIOD) + " = " + std::to_string(c.period) + " s is not a whole multiple of model.time_step = "
                + std::to_string(step) + " s");
    }
    return c;
}

void BudgetOutput::refuseFor(const std::string& stepName)
{
    std::string raw;
    for (const char* key : { KEY_FILE, KEY_TERMS, KEY_PERIOD, KEY_SERIES })
        if (Configurator::lookup(key, raw))
            throw std::invalid_argument(std::string(key) + " is set, but " + stepName + " has no momentum balance: select Nextsim::DynamicsStep");
}

std::string BudgetOutput::headerLine()
{
    std::string s = "# time";
    for (const char* t : TERMS)
        s += std::string(" ") + t;
    return s + " ke";
}

std::string BudgetOutput::formatLine(long time, const std::vector<double>& totals)
{
    std::string s = std::to_string(time);
    char buf[40];
    for (double v : totals) {
        std::snprintf(buf, sizeof buf, " %.17g", v);
        s += buf;
    }
    return s;
}

std::vector<double> BudgetOutput::totals(const double* rows, std::size_t nrows)
{
    std::vector<double> out(NSDG_BUDGET_QUANTITIES, 0.);
    for (int q = 0; q < NSDG_BUDGET_QUANTITIES; ++q)
        for (std::size_t r = 0; r < nrows; ++r)
            out[q] = out[q] + rows[q * nrows + r];
    return out;
}

void BudgetOutput::start(long time)
{
    m_clock = time, m_pending = false;
    if (!m_c.seriesFile.empty()) {
        std::ofstream f(m_c.seriesFile, std::ios::trunc);
        if (!f)
            throw std::runtime_error(std::string(KEY_SERIES) + ": cannot write " + m_c.seriesFile);
        f << headerLine() << "\n";
    }
}

bool BudgetOutput::step(long dt)
{
    const long before = m_clock;
    m_clock += dt;
    m_pending = true;
    if (m_c.file.empty() || m_c.period <= 0 || floorDiv(m_clock, m_c.period) == floorDiv(before, m_c.period))
        return false;
    m_pending = false;
    return true;
}

bool BudgetOutput::dueAtStop()
{
    const bool due = !m_c.file.empty() && m_c.period == 0 && m_pending;
    m_pending = false;
    return due;
}

void BudgetOutput::appendLine(const std::string& line) const
{
    std::ofstream f(m_c.seriesFile, std::ios::app);
    if (!f)
        throw std::runtime_error(std::string(KEY_SERIES) + ": cannot write " + m_c.seriesFile);
    f << line << "\n";
}

} // namespace Nextsim

#include "ForcingFile.hpp"

#include <cmath>
#include <cstdio>
#include <stdexcept>

#include "Hdf5Subset.hpp"

namespace Nextsim {

namespace {
std::string fmt(double v)
{
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}
} // namespace

const std::vector<std::string>& ForcingFile::columnVariables()
{
    static const std::vector<std::string> v = { "tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall" };
    return v;
}

const std::vector<std::string>& ForcingFile::knownVariables()
{
    static const std::vector<std::string> v = { "tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall", "wind_u", "wind_v", "ocean_u",
        "ocean_v", "sst", "sss", "ssh" };
    return v;
}

ForcingFile::ForcingFile(const std::string& path, bool needColumn)
    : m_path(path)
{
    const std::string where = "dynamics.forcing_file " + path + ": ";
    auto fail = [&](const std::string& what) { throw std::runtime_error(where + what); };
    try {
        const Hdf5File f(path);
        const std::vector<std::string> names = f.listGroup("/");
        if (!f.exists("/time"))
            fail("no variable time");
        const std::vector<std::uint64_t> td = f.dims("/time");
        if (td.size() != 1 || td[0] < 1)
            fail("time must be one-dimensional with at least one record");
        m_time = f.readDoubles("/time");
        for (std::size_t k = 0; k < m_time.size(); ++k) {
            if (!std::isfinite(m_time[k]))
                fail("time of record " + std::to_string(k) + " is not finite");
            if (k > 0 && !(m_time[k] > m_time[k - 1]))
                fail("time is not strictly increasing at record " + std::to_string(k) + " (" + fmt(m_time[k - 1]) + " s, then " + fmt(m_time[k]) + " s)");
        }
        const auto& known = knownVariables();
        for (const std::string& name : names) {
            if (name == "time")
                continue;
            if (name == "lon" || name == "lat" || name == "longitude" || name == "latitude" || name == "x" || name == "y")
                fail("variable " + name + ": coordinate variables are not supported -- the forcing lattice is cell-centred over the model's "
                     "square domain (no lon/lat or other lattices)");
            bool isKnown = false;
            for (const auto& k : known)
                isKnown = isKnown || k == name;
            if (!isKnown) {
                std::string list;
                for (const auto& k : known)
                    list += " " + k;
                fail("unknown variable " + name + " (known: time" + list + ")");
            }
            const std::vector<std::uint64_t> d = f.dims("/" + name);
            if (d.size() != 3 || d[0] != m_time.size() || d[1] < 1 || d[2] < 1)
                fail("variable " + name + " must have the dimensions (nt = " + std::to_string(m_time.size()) + ", nyr, nxr), it has "
                    + std::to_string(d.size()) + " dimension(s)" + (d.empty() ? std::string() : " of which the first is " + std::to_string(d[0])));
            if (m_vars.empty()) {
                if (d[1] > 65536 || d[2] > 65536) // NSDG_FORCING_MAX_LATTICE
                    fail("variable " + name + ": the lattice is larger than 65536 points along an axis");
                m_nyr = (int)d[1], m_nxr = (int)d[2];
            } else if ((int)d[1] != m_nyr || (int)d[2] != m_nxr)
                fail("variable " + name + " is on a " + std::to_string(d[1]) + " x " + std::to_string(d[2]) + " lattice, the others on "
                    + std::to_string(m_nyr) + " x " + std::to_string(m_nxr) + " (nyr x nxr): all variables share one lattice");
            std::vector<double> v = f.readDoubles("/" + name);
            const std::size_t plane = (std::size_t)m_nxr * m_nyr;
            for (std::size_t i = 0; i < v.size(); ++i)
                if (!std::isfinite(v[i])) {
                    const std::size_t k = i / plane, r = i % plane;
                    fail("variable " + name + " has a non-finite value in record " + std::to_string(k) + " at (j, i) = (" + std::to_string(r / m_nxr)
                        + ", " + std::to_string(r % m_nxr) + ")");
                }
            m_vars[name] = std::move(v);
        }
    } catch (const Hdf5Error& e) {
        fail(e.what());
    }
    if (m_vars.empty())
        fail("no forcing variable (known: tair tdew slp qsw qlw mld snowfall wind_u wind_v ocean_u ocean_v sst sss ssh)");
    for (const auto& pair : { std::make_pair("wind_u", "wind_v"), std::make_pair("ocean_u", "ocean_v"), std::make_pair("sst", "sss") })
        if (has(pair.first) != has(pair.second))
            fail(std::string("variable ") + (has(pair.first) ? pair.first : pair.second) + " without " + (has(pair.first) ? pair.second : pair.first)
                + ": the components come as a pair");
    if (needColumn)
        for (const auto& name : columnVariables())
            if (!has(name))
                fail("no variable " + name + ", which the column step needs (dynamics.thermodynamics = true)");
}

bool ForcingFile::hasColumn() const
{
    for (const auto& name : columnVariables())
        if (!has(name))
            return false;
    return true;
}

std::vector<std::string> ForcingFile::variables() const
{
    std::vector<std::string> out;
    for (const auto& name : knownVariables())
        if (has(name))
            out.push_back(name);
    return out;
}

void ForcingFile::bracket(double t, std::size_t& k0, std::size_t& k1, double& w) const
{
    const std::size_t nt = m_time.size();
    if (!(t >= m_time.front() && t <= m_time.back()))
        throw std::runtime_error("dynamics.forcing_file " + m_path + ": model time " + fmt(t) + " s is outside the records [" + fmt(m_time.front())
            + ", " + fmt(m_time.back()) + "] s (no extrapolation)");
    std::size_t lo = 0, hi = nt; // the last k with time[k] <= t: time[lo] <= t < time[hi]
    while (hi - lo > 1) {
        const std::size_t mid = (lo + hi) / 2;
        if (m_time[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    k0 = lo;
    if (k0 == nt - 1) {
        k1 = k0, w = 0.;
        return;
    }
    k1 = k0 + 1;
    w = (t - m_time[k0]) / (m_time[k1] - m_time[k0]);
}

const double* ForcingFile::record(const std::string& var, std::size_t k) const
{
    const auto it = m_vars.find(var);
    if (it == m_vars.end())
        throw std::runtime_error("dynamics.forcing_file " + m_path + ": no variable " + var);
    if (k >= m_time.size())
        throw std::runtime_error("dynamics.forcing_file " + m_path + ": no record " + std::to_string(k) + " of variable " + var);
    return it->second.data() + k * (std::size_t)m_nxr * m_nyr;
}

} // namespace Nextsim

// make_forcing.cpp -- writes the forcing file of dynamics.forcing = file (host/include/ForcingFile.hpp) from .npy arrays, and
// describes one.
//
//     make_forcing --out f.nc --time t.npy tair=tair.npy tdew=tdew.npy ... [wind_u=u.npy wind_v=v.npy] [ocean_u=... ocean_v=...]
//     make_forcing --check f.nc
//
// The arrays are float64 .npy files (little-endian, C order): time of shape (nt), every variable of shape (nt, nyr, nxr).  The
// written file is read back with ForcingFile and checked as a run would check it; a file that fails the check is removed and the
// tool exits with status 1.  --check prints the lattice, the time range and the variables.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "ForcingFile.hpp"
#include "Hdf5Subset.hpp"

using namespace Nextsim;

namespace {

struct Npy {
    std::vector<std::uint64_t> shape;
    std::vector<double> values;
};

// a float64 .npy file (format versions 1-3), little-endian, C order
Npy readNpy(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f)
        throw std::runtime_error("cannot open " + path);
    const std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (b.size() < 10 || std::memcmp(b.data(), "\x93NUMPY", 6) != 0)
        throw std::runtime_error(path + " is not a .npy file");
    const int major = (unsigned char)b[6];
    std::size_t hlen = 0, start = 0;
    if (major == 1) {
        hlen = (unsigned char)b[8] | ((std::size_t)(unsigned char)b[9] << 8), start = 10;
    } else if (major == 2 || major == 3) {
        if (b.size() < 12)
            throw std::runtime_error(path + ": truncated header");
        for (int i = 0; i < 4; ++i)
            hlen |= (std::size_t)(unsigned char)b[8 + i] << (8 * i);
        start = 12;
    } else
        throw std::runtime_error(path + ": .npy format version " + std::to_string(major) + " is not supported");
    if (start + hlen > b.size())
        throw std::runtime_error(path + ": truncated header");
    const std::string h(b.data() + start, hlen);
    auto value = [&](const std::string& key) {
        const std::size_t k = h.find("'" + key + "'");
        if (k == std::string::npos)
            throw std::runtime_error(path + ": no " + key + " in the header");
        std::size_t p = h.find(':', k);
        while (p + 1 < h.size() && h[p + 1] == ' ')
            ++p;
        return p + 1;
    };
    const std::size_t d = value("descr");
    if (h.compare(d, 5, "'<f8'") != 0 && h.compare(d, 5, "'f8'") != 0)
        throw std::runtime_error(path + ": the array must be float64 ('<f8'), the header says " + h.substr(d, 6));
    if (h.compare(value("fortran_order"), 5, "False") != 0)
        throw std::runtime_error(path + ": the array must be in C order");
    const std::size_t s = value("shape");
    const std::size_t e = h.find(')', s);
    if (h[s] != '(' || e == std::string::npos)
        throw std::runtime_error(path + ": unreadable shape");
    Npy out;
    std::uint64_t n = 1;
    for (std::size_t p = s + 1; p < e;) {
        while (p < e && (h[p] == ' ' || h[p] == ','))
            ++p;
        if (p >= e)
            break;
        char* end = nullptr;
        const unsigned long long v = std::strtoull(h.c_str() + p, &end, 10);
        if (end == h.c_str() + p)
            throw std::runtime_error(path + ": unreadable shape");
        out.shape.push_back(v);
        n *= v;
        p = end - h.c_str();
    }
    const std::size_t data = start + hlen;
    if (b.size() - data != n * sizeof(double))
        throw std::runtime_error(path + ": " + std::to_string(b.size() - data) + " bytes of data for " + std::to_string(n) + " float64 values");
    out.values.resize(n);
    std::memcpy(out.values.data(), b.data() + data, n * sizeof(double));
    return out;
}

void usage()
{
    std::cerr << "usage: make_forcing --out FILE --time TIME.npy NAME=ARRAY.npy ...\n"
                 "       make_forcing --check FILE\n"
                 "NAME: tair tdew slp qsw qlw mld snowfall wind_u wind_v ocean_u ocean_v; TIME (nt) in model seconds, every ARRAY\n"
                 "(nt, nyr, nxr) float64 on one cell-centred lattice over the model's square domain\n";
}

int check(const std::string& path)
{
    const ForcingFile f(path, false);
    std::printf("%s: lattice nxr x nyr = %d x %d, %zu record(s), time %.17g .. %.17g s\n", path.c_str(), f.nxr(), f.nyr(), f.records(),
        f.times().front(), f.times().back());
    std::printf("variables:");
    for (const auto& v : f.variables())
        std::printf(" %s", v.c_str());
    std::printf("\ncolumn variables: %s, wind: %s, ocean: %s\n", f.hasColumn() ? "all" : "incomplete", f.hasWind() ? "yes" : "no",
        f.hasOcean() ? "yes" : "no");
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    try {
        std::string out, time;
        std::vector<std::pair<std::string, std::string>> vars;
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            if (a == "--check" && i + 1 < argc && argc == 3)
                return check(argv[i + 1]);
            if (a == "--out" && i + 1 < argc)
                out = argv[++i];
            else if (a == "--time" && i + 1 < argc)
                time = argv[++i];
            else if (a.find('=') != std::string::npos && a[0] != '-')
                vars.emplace_back(a.substr(0, a.find('=')), a.substr(a.find('=') + 1));
            else {
                usage();
                return 2;
            }
        }
        if (out.empty() || time.empty() || vars.empty()) {
            usage();
            return 2;
        }
        Hdf5Writer w;
        const Npy t = readNpy(time);
        if (t.shape.size() != 1)
            throw std::runtime_error(time + ": time must be one-dimensional");
        w.dataset("/time", t.shape, t.values);
        for (const auto& v : vars) {
            if (v.first == "time")
                throw std::runtime_error("time is given with --time");
            const Npy a = readNpy(v.second);
            w.dataset("/" + v.first, a.shape, a.values);
        }
        w.write(out);
        try {
            (void)ForcingFile(out, false);
        } catch (...) {
            std::remove(out.c_str());
            throw;
        }
        return check(out);
    } catch (const std::exception& e) {
        std::cerr << "make_forcing: " << e.what() << std::endl;
        return 1;
    }
}

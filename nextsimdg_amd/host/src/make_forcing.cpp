// make_forcing.cpp -- writes the forcing file of dynamics.forcing = file (host/include/ForcingFile.hpp) from .npy arrays, and
// describes one.
//
//     make_forcing --out f.nc --time t.npy tair=tair.npy tdew=tdew.npy ... [wind_u=u.npy wind_v=v.npy] [ocean_u=... ocean_v=...] [ssh=ssh.npy]
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
#include "NpyFile.hpp"

using namespace Nextsim;

namespace {

void usage()
{
    std::cerr << "usage: make_forcing --out FILE --time TIME.npy NAME=ARRAY.npy ...\n"
                 "       make_forcing --check FILE\n"
                 "NAME: tair tdew slp qsw qlw mld snowfall wind_u wind_v ocean_u ocean_v sst sss ssh; TIME (nt) in model seconds, every ARRAY\n"
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

// forcing_tests.cpp -- tests of the forcing file of dynamics.forcing = file (ForcingFile, make_forcing) on the CPU: a file written
// by make_forcing from .npy arrays reads back bit for bit, the records around a model time are the right ones, and every malformed
// file is refused with an error that names the file, the variable and the record.  Same tiny harness as host_tests: CHECK() records
// failures, the exit code is the number of failures.
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "ForcingFile.hpp"
#include "Hdf5Subset.hpp"

using namespace Nextsim;

static int failures = 0, checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++checks;                                                                \
        if (!(cond)) {                                                           \
            ++failures;                                                          \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
        }                                                                        \
    } while (0)

// the message of the exception `f` throws ("" if it does not throw)
static std::string errorOf(const std::function<void()>& f)
{
    try {
        f();
    } catch (const std::exception& e) {
        return e.what();
    }
    return "";
}
static bool contains(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }
#define CHECK_ERROR(expr, ...)                                                                   \
    do {                                                                                         \
        const std::string msg_ = errorOf([&] { expr; });                                         \
        bool ok_ = !msg_.empty();                                                                \
        for (const char* p_ : { __VA_ARGS__ })                                                   \
            ok_ = ok_ && contains(msg_, p_);                                                     \
        ++checks;                                                                                \
        if (!ok_) {                                                                              \
            ++failures;                                                                          \
            std::printf("FAIL %s:%d: %s: message \"%s\"\n", __FILE__, __LINE__, #expr, msg_.c_str()); \
        }                                                                                        \
    } while (0)

static std::string g_dir, g_tools;

static void writeNpy(const std::string& path, const std::vector<std::uint64_t>& shape, const std::vector<double>& v)
{
    std::string dims;
    for (std::uint64_t d : shape)
        dims += std::to_string(d) + ", ";
    if (shape.size() > 1)
        dims.resize(dims.size() - 2);
    std::string h = "{'descr': '<f8', 'fortran_order': False, 'shape': (" + dims + "), }";
    while ((10 + h.size() + 1) % 64)
        h += ' ';
    h += '\n';
    std::ofstream f(path, std::ios::binary);
    f.write("\x93NUMPY\x01\x00", 8);
    const unsigned char len[2] = { (unsigned char)(h.size() & 0xff), (unsigned char)(h.size() >> 8) };
    f.write(reinterpret_cast<const char*>(len), 2);
    f.write(h.data(), (std::streamsize)h.size());
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
}

// a file of the given variables: values that use every bit (a seeded pattern, negative values, a subnormal)
struct Spec {
    std::vector<double> time;
    int nyr = 3, nxr = 5;
    std::vector<std::string> vars;
};
static std::vector<double> pattern(std::size_t n, unsigned seed)
{
    std::vector<double> v(n);
    unsigned long long x = 0x9e3779b97f4a7c15ULL * (seed + 1);
    for (auto& e : v) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        e = ((double)(x >> 11) / 9007199254740992.0 - 0.3) * 1e3;
    }
    if (n > 3)
        v[3] = 4.9e-324;
    return v;
}
static std::string writeDirect(const std::string& name, const Spec& s, const std::function<void(Hdf5Writer&)>& extra = nullptr)
{
    Hdf5Writer w;
    w.dataset("/time", { s.time.size() }, s.time);
    unsigned seed = 0;
    for (const auto& v : s.vars)
        w.dataset("/" + v, { s.time.size(), (std::uint64_t)s.nyr, (std::uint64_t)s.nxr }, pattern(s.time.size() * s.nyr * s.nxr, seed++));
    if (extra)
        extra(w);
    const std::string path = g_dir + "/" + name;
    w.write(path);
    return path;
}
static const std::vector<std::string> COLUMN = { "tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall" };

static void test_make_forcing_round_trip()
{
    const std::size_t nt = 4;
    const int nyr = 7, nxr = 9;
    std::vector<std::string> vars = COLUMN;
    for (const char* v : { "wind_u", "wind_v", "ocean_u", "ocean_v" })
        vars.push_back(v);
    const std::vector<double> t = { -3600., 0., 1800.5, 86400. };
    writeNpy(g_dir + "/t.npy", { nt }, t);
    std::string cmd = g_tools + "/make_forcing --out " + g_dir + "/made.nc --time " + g_dir + "/t.npy";
    std::vector<std::vector<double>> values;
    for (std::size_t k = 0; k < vars.size(); ++k) {
        values.push_back(pattern(nt * nyr * nxr, 100 + (unsigned)k));
        writeNpy(g_dir + "/" + vars[k] + ".npy", { nt, (std::uint64_t)nyr, (std::uint64_t)nxr }, values.back());
        cmd += " " + vars[k] + "=" + g_dir + "/" + vars[k] + ".npy";
    }
    CHECK(std::system((cmd + " > " + g_dir + "/made.txt 2>&1").c_str()) == 0);
    const ForcingFile f(g_dir + "/made.nc", true);
    CHECK(f.records() == nt && f.nxr() == nxr && f.nyr() == nyr);
    CHECK(std::memcmp(f.times().data(), t.data(), nt * sizeof(double)) == 0);
    CHECK(f.hasColumn() && f.hasWind() && f.hasOcean() && f.variables() == vars);
    for (std::size_t k = 0; k < vars.size(); ++k)
        for (std::size_t r = 0; r < nt; ++r)
            CHECK(std::memcmp(f.record(vars[k], r), values[k].data() + r * nyr * nxr, (std::size_t)nyr * nxr * sizeof(double)) == 0);
    // --check describes it
    CHECK(std::system((g_tools + "/make_forcing --check " + g_dir + "/made.nc > " + g_dir + "/check.txt 2>&1").c_str()) == 0);
    std::ifstream in(g_dir + "/check.txt");
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    CHECK(contains(text, "lattice nxr x nyr = 9 x 7, 4 record(s), time -3600 .. 86400 s"));
    CHECK(contains(text, "variables: tair tdew slp qsw qlw mld snowfall wind_u wind_v ocean_u ocean_v"));
    // make_forcing refuses what a run would refuse, and leaves no file behind: a lone wind_u, a time that goes back
    CHECK(std::system((g_tools + "/make_forcing --out " + g_dir + "/lone.nc --time " + g_dir + "/t.npy wind_u=" + g_dir + "/wind_u.npy > " + g_dir
                          + "/lone.txt 2>&1").c_str()) != 0);
    CHECK(access((g_dir + "/lone.nc").c_str(), F_OK) != 0);
    writeNpy(g_dir + "/back.npy", { nt }, { 0., 10., 5., 20. });
    CHECK(std::system((g_tools + "/make_forcing --out " + g_dir + "/back.nc --time " + g_dir + "/back.npy tair=" + g_dir + "/tair.npy > " + g_dir
                          + "/back.txt 2>&1").c_str()) != 0);
    CHECK(access((g_dir + "/back.nc").c_str(), F_OK) != 0);
}

static void test_bracket()
{
    Spec s;
    s.time = { 0., 3600., 7200. };
    s.vars = COLUMN;
    const ForcingFile f(writeDirect("three.nc", s), true);
    std::size_t k0 = 99, k1 = 99;
    double w = -1.;
    f.bracket(0., k0, k1, w); // the first record itself
    CHECK(k0 == 0 && k1 == 1 && w == 0.);
    f.bracket(1800., k0, k1, w); // between records
    CHECK(k0 == 0 && k1 == 1 && w == 0.5);
    f.bracket(3600., k0, k1, w); // an interior record exactly: that record with weight 0
    CHECK(k0 == 1 && k1 == 2 && w == 0.);
    f.bracket(5000., k0, k1, w);
    CHECK(k0 == 1 && k1 == 2 && w == (5000. - 3600.) / 3600.);
    f.bracket(7200., k0, k1, w); // the last record is allowed
    CHECK(k0 == 2 && k1 == 2 && w == 0.);
    CHECK_ERROR(f.bracket(-1e-9, k0, k1, w), "three.nc", "model time", "outside the records [0, 7200]");
    CHECK_ERROR(f.bracket(7200.000001, k0, k1, w), "three.nc", "outside the records");
    CHECK_ERROR(f.bracket(std::nan(""), k0, k1, w), "three.nc", "outside the records");
    Spec one;
    one.time = { 600. };
    one.vars = { "wind_u", "wind_v" };
    const ForcingFile g(writeDirect("one.nc", one), false);
    g.bracket(600., k0, k1, w);
    CHECK(k0 == 0 && k1 == 0 && w == 0.);
    CHECK_ERROR(g.bracket(601., k0, k1, w), "one.nc", "outside the records");
}

static void test_errors()
{
    const std::string missing = g_dir + "/no_such_forcing.nc";
    CHECK_ERROR(ForcingFile(missing, false), "dynamics.forcing_file", "no_such_forcing.nc");
    Spec s;
    s.time = { 0., 3600., 3600., 7200. };
    s.vars = COLUMN;
    CHECK_ERROR(ForcingFile(writeDirect("flat.nc", s), true), "flat.nc", "time is not strictly increasing at record 2");
    s.time = { 0., 3600., 1800. };
    CHECK_ERROR(ForcingFile(writeDirect("back.nc", s), true), "back.nc", "time is not strictly increasing at record 2");
    s.time = { 0., std::numeric_limits<double>::infinity() };
    CHECK_ERROR(ForcingFile(writeDirect("inftime.nc", s), true), "inftime.nc", "time of record 1 is not finite");
    Spec ok;
    ok.time = { 0., 3600. };
    ok.vars = COLUMN;
    // dimensions: another lattice, another record count, two dimensions
    CHECK_ERROR(ForcingFile(writeDirect("lattice.nc", ok, [](Hdf5Writer& w) { w.dataset("/wind_u", { 2, 3, 6 }, std::vector<double>(36, 1.)); }), false),
        "lattice.nc", "variable wind_u is on a 3 x 6 lattice", "3 x 5");
    CHECK_ERROR(ForcingFile(writeDirect("nt.nc", ok, [](Hdf5Writer& w) { w.dataset("/ocean_u", { 3, 3, 5 }, std::vector<double>(45, 1.)); }), false),
        "nt.nc", "variable ocean_u must have the dimensions (nt = 2, nyr, nxr)");
    CHECK_ERROR(ForcingFile(writeDirect("rank.nc", ok, [](Hdf5Writer& w) { w.dataset("/ocean_v", { 2, 15 }, std::vector<double>(30, 1.)); }), false),
        "rank.nc", "variable ocean_v must have the dimensions");
    // a lone component
    Spec lone = ok;
    lone.vars.push_back("wind_u");
    CHECK_ERROR(ForcingFile(writeDirect("lone.nc", lone), false), "lone.nc", "variable wind_u without wind_v");
    Spec lonev = ok;
    lonev.vars.push_back("ocean_v");
    CHECK_ERROR(ForcingFile(writeDirect("lonev.nc", lonev), false), "lonev.nc", "variable ocean_v without ocean_u");
    // a NaN: the variable, the record and the point
    CHECK_ERROR(ForcingFile(writeDirect("nan.nc", ok, [](Hdf5Writer& w) {
        std::vector<double> v(30, 2.);
        v[15 + 5 + 3] = std::nan("");
        w.dataset("/wind_u", { 2, 3, 5 }, v);
        w.dataset("/wind_v", { 2, 3, 5 }, std::vector<double>(30, 1.));
    }), false),
        "nan.nc", "variable wind_u has a non-finite value in record 1 at (j, i) = (1, 3)");
    // a missing column variable with thermodynamics on; without, the file is fine
    Spec six = ok;
    six.vars.erase(six.vars.begin() + 4); // qlw
    CHECK_ERROR(ForcingFile(writeDirect("six.nc", six), true), "six.nc", "no variable qlw", "dynamics.thermodynamics = true");
    CHECK(errorOf([&] { ForcingFile(g_dir + "/six.nc", false); }).empty());
    // what the reader does not do: coordinate variables (lon / lat or other lattices), unknown variables, no time, no variable
    CHECK_ERROR(ForcingFile(writeDirect("lon.nc", ok, [](Hdf5Writer& w) { w.dataset("/lon", { 5 }, std::vector<double>(5, 0.)); }), false), "lon.nc",
        "variable lon", "lon/lat");
    CHECK_ERROR(ForcingFile(writeDirect("typo.nc", ok, [](Hdf5Writer& w) { w.dataset("/Tair", { 2, 3, 5 }, std::vector<double>(30, 0.)); }), false),
        "typo.nc", "unknown variable Tair");
    {
        Hdf5Writer w;
        w.dataset("/tair", { 1, 1, 1 }, { 1. });
        w.write(g_dir + "/notime.nc");
        CHECK_ERROR(ForcingFile(g_dir + "/notime.nc", false), "notime.nc", "no variable time");
    }
    Spec none;
    none.time = { 0. };
    CHECK_ERROR(ForcingFile(writeDirect("none.nc", none), false), "none.nc", "no forcing variable");
    // not an HDF5 file
    {
        std::ofstream junk(g_dir + "/junk.nc");
        junk << "not a forcing file\n";
    }
    CHECK_ERROR(ForcingFile(g_dir + "/junk.nc", false), "junk.nc", "dynamics.forcing_file");
}

int main(int argc, char** argv)
{
    const std::string self = argv[0];
    g_tools = self.find('/') == std::string::npos ? "." : self.substr(0, self.rfind('/'));
    const char* tmp = std::getenv("TMPDIR");
    std::string templ = std::string(tmp && *tmp ? tmp : "/tmp") + "/forcing_tests.XXXXXX";
    std::vector<char> buf(templ.begin(), templ.end());
    buf.push_back(0);
    if (!mkdtemp(buf.data())) {
        std::printf("FAIL: cannot create a temporary directory\n");
        return 1;
    }
    g_dir = buf.data();
    try {
        test_make_forcing_round_trip();
        test_bracket();
        test_errors();
    } catch (const std::exception& e) {
        std::printf("FAIL: unexpected exception: %s\n", e.what());
        ++failures;
    }
    if (std::system(("rm -rf '" + g_dir + "'").c_str()) != 0)
        std::printf("note: could not remove %s\n", g_dir.c_str());
    std::printf("forcing tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

// basal_tests.cpp -- landfast ice on the host (include/DynamicsStep.hpp "dynamics.bathymetry_file", "[basal]"; include/BathymetryFile.hpp):
// the depth file is read and every bad file or value is refused by a message that names the key, the file and the first offending
// element; land elements are not looked at and stored as 0; the [basal] keys follow the rule of nsdg_basal_params_set and need the file;
// all of it in configure(), before a device is asked for.  Needs no device.  Same tiny harness as host_tests: CHECK() records failures,
// the exit code is the number of failures.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <functional>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/nsdg.h"
#include "BathymetryFile.hpp"
#include "Configurator.hpp"
#include "DynamicsStep.hpp"
#include "LandMaskFile.hpp"
#include "RectGrid.hpp"

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

static bool contains(const std::string& s, const std::string& part) { return s.find(part) != std::string::npos; }

static void configureWith(const std::string& ini)
{
    Configurator::clear();
    Configurator::addStream(std::unique_ptr<std::istream>(new std::stringstream(ini)));
}

// the message of the exception f throws; "" if it throws nothing
static std::string refusal(const std::function<void()>& f)
{
    try {
        f();
    } catch (const std::exception& e) {
        return e.what();
    }
    return "";
}

// configure() never asks for a device: whatever it refuses, it refuses before one
static std::string dyn(const std::string& ini)
{
    configureWith(ini);
    return refusal([] { DynamicsStep().configure(); });
}

static const std::string MODEL = "[model]\ntime_step = 120\n[dynamics]\n";

template <class T>
static void writeNpy(const std::string& path, const std::string& descr, const std::vector<std::size_t>& shape, const std::vector<T>& values)
{
    std::string dims;
    for (std::size_t s : shape)
        dims += std::to_string(s) + ", ";
    std::string header = "{'descr': '" + descr + "', 'fortran_order': False, 'shape': (" + dims + "), }";
    while ((10 + header.size() + 1) % 64)
        header += ' ';
    header += '\n';
    std::ofstream f(path, std::ios::binary);
    const unsigned char magic[8] = { 0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0 };
    f.write(reinterpret_cast<const char*>(magic), 8);
    const unsigned char len[2] = { (unsigned char)(header.size() & 255), (unsigned char)(header.size() >> 8) };
    f.write(reinterpret_cast<const char*>(len), 2);
    f << header;
    f.write(reinterpret_cast<const char*>(values.data()), (std::streamsize)(values.size() * sizeof(T)));
}

static void test_file()
{
    const std::string dir = "/tmp/nsdg_basal_test_", good = dir + "good.npy", mask = dir + "mask.npy";
    std::vector<double> depth(5 * 7, 100.);
    depth[2 * 7 + 3] = 12.5;
    writeNpy(good, "<f8", { 5, 7 }, depth);
    {
        const BathymetryFile b(good, nullptr);
        CHECK(b.rows() == 5 && b.cols() == 7 && b.shallowest() == 12.5 && b.data()[2 * 7 + 3] == 12.5 && b.data()[0] == 100.);
        CHECK(refusal([&] { b.checkShape(5, 7); }) == "");
        const std::string why = refusal([&] { b.checkShape(7, 5); });
        CHECK(contains(why, "dynamics.bathymetry_file " + good) && contains(why, "the shape (5, 7)") && contains(why, "(7, 5)"));
    }
    // a bad value at an ocean element is named with its place; on land it is not looked at and stored as 0
    std::vector<std::uint8_t> land(5 * 7, 0);
    land[4 * 7 + 6] = 1;
    writeNpy(mask, "|u1", { 5, 7 }, land);
    const LandMaskFile m(mask);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (const auto& bad : { std::make_pair(-1., std::string("value -1 at (1, 2)")), std::make_pair(nan, std::string(" at (1, 2)")),
             std::make_pair(inf, std::string("value inf at (1, 2)")) }) {
        std::vector<double> d = depth;
        d[1 * 7 + 2] = bad.first;
        d[3 * 7 + 0] = -5.; // a later offender: the first one is named
        writeNpy(dir + "bad.npy", "<f8", { 5, 7 }, d);
        const std::string why = refusal([&] { BathymetryFile b(dir + "bad.npy", &m); });
        CHECK(contains(why, "dynamics.bathymetry_file " + dir + "bad.npy") && contains(why, bad.second) && contains(why, "finite and >= 0 at ocean elements"));
        d = depth;
        d[4 * 7 + 6] = bad.first; // the land element
        writeNpy(dir + "land.npy", "<f8", { 5, 7 }, d);
        CHECK(refusal([&] { BathymetryFile b(dir + "land.npy", &m); CHECK(b.data()[4 * 7 + 6] == 0. && b.data()[4 * 7 + 5] == 100.); }) == "");
        CHECK(contains(refusal([&] { BathymetryFile b(dir + "land.npy", nullptr); }), " at (4, 6)")); // without the mask it is an ocean element
    }
    CHECK(contains(refusal([&] { BathymetryFile b(dir + "missing.npy", nullptr); }), "dynamics.bathymetry_file " + dir + "missing.npy"));
    writeNpy(dir + "flat.npy", "<f8", { 35 }, depth);
    CHECK(contains(refusal([&] { BathymetryFile b(dir + "flat.npy", nullptr); }), "two-dimensional"));
    writeNpy(dir + "int.npy", "<i8", { 5, 7 }, std::vector<std::int64_t>(35, 10));
    CHECK(contains(refusal([&] { BathymetryFile b(dir + "int.npy", nullptr); }), "dynamics.bathymetry_file " + dir + "int.npy"));
    writeNpy(dir + "other.npy", "<f8", { 7, 5 }, depth);
    const std::string why = refusal([&] { BathymetryFile b(dir + "other.npy", &m); });
    CHECK(contains(why, "the shape (7, 5)") && contains(why, "dynamics.land_mask_file (5, 7)"));
}

static void test_keys()
{
    const std::string dir = "/tmp/nsdg_basal_test_", good = dir + "good.npy", mask = dir + "mask.npy";
    CHECK(dyn(MODEL) == "" && dyn(MODEL + "bathymetry_file = " + good + "\n") == "");
    CHECK(dyn(MODEL + "bathymetry_file = " + good + "\nland_mask_file = " + mask + "\n") == "");
    CHECK(dyn(MODEL + "bathymetry_file = " + good + "\nrheology = bbm\n") == "" && dyn(MODEL + "bathymetry_file = " + good + "\nthermodynamics = true\n") == "");
    CHECK(dyn(MODEL + "bathymetry_file = " + good + "\n[basal]\nk1 = 5\nk2 = 0\nalpha_b = 0\nu0 = 1e-4\n") == ""); // the closed ends are allowed
    for (const std::string bad : { "k1 = 0", "k1 = -2", "k2 = -1", "alpha_b = -0.5", "u0 = 0", "u0 = -1e-5" }) {
        const std::string why = dyn(MODEL + "bathymetry_file = " + good + "\n[basal]\n" + bad + "\n");
        CHECK(contains(why, "[basal]") && contains(why, "basal." + bad.substr(0, bad.find(' '))) && contains(why, "k1 > 0, k2 >= 0, alpha_b >= 0 and u0 > 0"));
    }
    // (a value that is no finite number never becomes a double: the configurator refuses it, by the key's name)
    CHECK(contains(dyn(MODEL + "bathymetry_file = " + good + "\n[basal]\nk1 = nan\n"), "basal.k1") && contains(dyn(MODEL + "bathymetry_file = " + good + "\n[basal]\nk2 = inf\n"), "basal.k2"));
    CHECK(contains(dyn(MODEL + "[basal]\nk2 = 10\n"), "need dynamics.bathymetry_file")); // parameters without a depth
    CHECK(contains(dyn(MODEL + "bathymetry_file = " + dir + "missing.npy\n"), "dynamics.bathymetry_file " + dir + "missing.npy"));
    { // the shape is held against the structure's once there is one
        RectGrid g57, g75;
        g57.resize(5, 7, 1), g75.resize(7, 5, 1);
        configureWith(MODEL + "bathymetry_file = " + good + "\n");
        CHECK(refusal([&] { DynamicsStep s; s.setInitialData(g57); s.configure(); }) == "");
        const std::string why = refusal([&] { DynamicsStep s; s.setInitialData(g75); s.configure(); });
        CHECK(contains(why, "dynamics.bathymetry_file") && contains(why, "(rectgrid.nx, rectgrid.ny) = (7, 5)"));
    }
    Configurator::clear();
}

int main()
{
    test_file();
    test_keys();
    std::printf("host basal tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

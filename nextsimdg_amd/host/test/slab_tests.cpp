// slab_tests.cpp -- the slab ocean on the host (include/DynamicsStep.hpp "dynamics.slab_ocean", "[slabocean]"; include/nsdg_ocean.h):
// the mode needs the column model, the [slabocean] keys follow the rule of nsdg_slab_params_set and need the mode, all of it in
// configure(), before a device is asked for; the forcing file's pair sst, sss comes complete or not at all; sst and sss travel between the
// ranks with the column planes.  Needs no device.  Same tiny harness as host_tests: CHECK() records failures, the exit code is the number
// of failures.
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/nsdg.h"
#include "Configurator.hpp"
#include "DynamicsStep.hpp"
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
static const std::string ON = MODEL + "thermodynamics = true\nslab_ocean = true\n";

static void test_keys()
{
    CHECK(dyn(MODEL) == "" && dyn(ON) == "" && dyn(MODEL + "thermodynamics = true\nslab_ocean = false\n") == "");
    CHECK(dyn(ON + "advect_column_state = true\n") == "" && dyn(ON + "rheology = bbm\n") == "" && dyn(ON + "tracers = age\n") == "");
    // the mode needs the column model: the message names both keys
    for (const std::string& ini : { MODEL + "slab_ocean = true\n", MODEL + "slab_ocean = true\nthermodynamics = false\n" }) {
        const std::string why = dyn(ini);
        CHECK(contains(why, "dynamics.slab_ocean") && contains(why, "dynamics.thermodynamics = true"));
    }
    // the parameters: the closed end 0 is allowed (0 = no relaxation), a negative value is not
    CHECK(dyn(ON + "[slabocean]\nrelax_t = 0\nrelax_s = 864000\nice_salinity = 0\n") == "");
    for (const std::string bad : { "relax_t = -1", "relax_s = -0.5", "ice_salinity = -5" }) {
        const std::string why = dyn(ON + "[slabocean]\n" + bad + "\n");
        CHECK(contains(why, "[slabocean]") && contains(why, "slabocean." + bad.substr(0, bad.find(' ')))
            && contains(why, "relax_t >= 0, relax_s >= 0 and ice_salinity >= 0, all finite"));
    }
    // (a value that is no finite number never becomes a double: the configurator refuses it, by the key's name)
    CHECK(contains(dyn(ON + "[slabocean]\nrelax_t = nan\n"), "slabocean.relax_t") && contains(dyn(ON + "[slabocean]\nice_salinity = inf\n"), "slabocean.ice_salinity"));
    // the keys without the mode, whatever their value
    for (const std::string key : { "relax_t", "relax_s", "ice_salinity" }) {
        for (const std::string& head : { MODEL, MODEL + "thermodynamics = true\n", MODEL + "thermodynamics = true\nslab_ocean = false\n" }) {
            const std::string why = dyn(head + "[slabocean]\n" + key + " = 5\n");
            CHECK(contains(why, "[slabocean]: slabocean." + key) && contains(why, "needs dynamics.slab_ocean = true"));
        }
    }
    Configurator::clear();
}

static void test_forcing_pair()
{
    const std::string dir = "/tmp/nsdg_slab_test_";
    const std::vector<std::uint64_t> dims = { 2, 3, 4 };
    const std::vector<double> plane(24, 1.5);
    auto file = [&](const std::string& name, const std::vector<std::string>& vars) {
        Hdf5Writer w;
        w.dataset("/time", { 2 }, { 0., 600. });
        for (const std::string& v : vars)
            w.dataset("/" + v, dims, plane);
        w.write(dir + name);
        return dir + name;
    };
    {
        const ForcingFile both(file("both.nc", { "wind_u", "wind_v", "sst", "sss" }), false);
        CHECK(both.hasSlabTargets() && both.has("sss") && both.record("sst", 1)[11] == 1.5);
        const std::vector<std::string> vars = both.variables();
        CHECK(vars.size() == 4 && vars[2] == "sst" && vars[3] == "sss"); // after the others: the layout of a file without the pair is as it was
        const ForcingFile none(file("none.nc", { "wind_u", "wind_v" }), false);
        CHECK(!none.hasSlabTargets() && none.variables().size() == 2);
    }
    for (const auto& half : { std::make_pair("sst", "sss"), std::make_pair("sss", "sst") }) {
        const std::string path = file(std::string("half_") + half.first + ".nc", { half.first });
        const std::string why = refusal([&] { ForcingFile f(path, false); });
        CHECK(contains(why, "dynamics.forcing_file " + path) && contains(why, std::string("variable ") + half.first + " without " + half.second)
            && contains(why, "come as a pair"));
    }
    for (const std::string name : { "both.nc", "none.nc", "half_sst.nc", "half_sss.nc" })
        std::remove((dir + name).c_str());
}

static void test_rows_between_the_ranks()
{
    const int nx = 7, ny = 10; // nx = the row length of the dynamics, ny = rows
    FieldStore a, b;
    a.resize((std::size_t)nx * ny, 1), b.resize((std::size_t)nx * ny, 1);
    for (std::size_t e = 0; e < a.n; ++e)
        a.hice[e] = 1. + e, a.sst[e] = -1.5 + 0.001 * e, a.sss[e] = 30. + 0.01 * e, a.newice[e] = 0.5 * e;
    const std::vector<double> plain = DynamicsStep::packRows(a, true, nx, 3, 10), with = DynamicsStep::packRows(a, true, nx, 3, 10, true);
    CHECK(with.size() == plain.size() + 2 * 7 * (std::size_t)nx && plain == DynamicsStep::packRows(a, true, nx, 3, 10, false));
    CHECK(with[5 * 7 * (std::size_t)nx] == a.sst[3 * nx] && with[6 * 7 * (std::size_t)nx] == a.sss[3 * nx]); // after hice, cice, hsnow, tice, newice
    DynamicsStep::placeRows(b, true, nx, 3, 10, with.data(), with.size(), true);
    bool same = true;
    for (std::size_t e = 0; e < a.n; ++e) { // rows nobody sent stay as they were
        const bool sent = e >= 3 * (std::size_t)nx;
        same = same && b.sst[e] == (sent ? a.sst[e] : 0.) && b.sss[e] == (sent ? a.sss[e] : 0.) && b.hice[e] == (sent ? a.hice[e] : 0.)
            && b.newice[e] == (sent ? a.newice[e] : 0.);
    }
    CHECK(same);
    // the two ends must run the same mode: the size gives the other one away
    CHECK(contains(refusal([&] { DynamicsStep::placeRows(b, true, nx, 3, 10, with.data(), with.size(), false); }), "a rank delivered"));
    CHECK(contains(refusal([&] { DynamicsStep::placeRows(b, true, nx, 3, 10, plain.data(), plain.size(), true); }), "a rank delivered"));
    // without thermodynamics the flag still adds exactly the two planes (configure() refuses that combination: the static form is total)
    CHECK(DynamicsStep::packRows(a, false, nx, 3, 10, true).size() == DynamicsStep::packRows(a, false, nx, 3, 10).size() + 2 * 7 * (std::size_t)nx);
}

int main()
{
    test_keys();
    test_forcing_pair();
    test_rows_between_the_ranks();
    std::printf("host slab tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

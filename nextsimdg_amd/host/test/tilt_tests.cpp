// tilt_tests.cpp -- the sea-surface tilt on the host (include/DynamicsStep.hpp "dynamics.tilt", "dynamics.gravity"; include/nsdg_tilt.h):
// the two keys, their defaults and every refusal -- an unknown tilt, a gravity without tilt = ssh, a bad gravity, a forcing file whose
// ocean pair comes without ssh, ssh in the file without tilt = ssh, both keys under Nextsim::HipStep -- all before a device is asked for;
// and ForcingFile with and without the optional variable ssh.  Needs no device.  Same tiny harness as host_tests: CHECK() records failures,
// the exit code is the number of failures.
//
//     tilt_tests DIR        DIR: where the forcing files of the test are written
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
#include "HipStep.hpp"

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
static std::string g_dir;

// a forcing file of two records on a 3 x 5 lattice that holds the named variables
static std::string forcingFile(const std::string& name, const std::vector<std::string>& vars)
{
    Hdf5Writer w;
    w.dataset("/time", { 2 }, { 0., 86400. });
    double seed = 1.;
    for (const auto& v : vars) {
        std::vector<double> a(2 * 3 * 5);
        for (std::size_t i = 0; i < a.size(); ++i)
            a[i] = seed + 0.01 * (double)i;
        seed += 1.;
        w.dataset("/" + v, { 2, 3, 5 }, a);
    }
    const std::string path = g_dir + "/" + name;
    w.write(path);
    return path;
}

static void test_abi()
{
    CHECK(NSDG_GRAVITY == 9.81);
    CHECK(nsdg_tilt_set(nullptr, nullptr, NSDG_GRAVITY) == NSDG_ERR_ARG); // a null context, from every call, without a crash
    CHECK(nsdg_tilt_nodal(nullptr, nullptr, nullptr) == NSDG_ERR_ARG);
    CHECK(nsdg_boxtest_ssh(nullptr, 1., 1e-4, NSDG_GRAVITY, nullptr) == NSDG_ERR_ARG);
    CHECK(nsdg_abi_version() == 6);
}

static void test_keys()
{
    // geostrophic by default, and ssh accepted in every combination the step knows
    CHECK(dyn(MODEL) == "" && dyn(MODEL + "tilt = geostrophic\n") == "");
    CHECK(dyn(MODEL + "tilt = ssh\n") == "" && dyn(MODEL + "tilt = ssh\ngravity = 9.8\n") == "");
    CHECK(dyn(MODEL + "tilt = ssh\nthermodynamics = true\nsnow_load = true\n") == "");
    CHECK(dyn(MODEL + "tilt = ssh\nrheology = bbm\n") == "");
    for (const std::string forcing : { "dummy", "winter", "host" }) // other forcings take the box test's height
        CHECK(dyn(MODEL + "tilt = ssh\nforcing = " + forcing + "\n") == "");
    // an unknown tilt
    CHECK(contains(dyn(MODEL + "tilt = barotropic\n"), "dynamics.tilt must be geostrophic or ssh"));
    // a gravity without the height
    CHECK(contains(dyn(MODEL + "gravity = 9.81\n"), "dynamics.gravity needs dynamics.tilt = ssh"));
    CHECK(contains(dyn(MODEL + "tilt = geostrophic\ngravity = 9.81\n"), "dynamics.gravity needs dynamics.tilt = ssh"));
    // a bad gravity
    for (const std::string bad : { "0", "-9.81", "-1e-300" }) {
        const std::string why = dyn(MODEL + "tilt = ssh\ngravity = " + bad + "\n");
        CHECK(contains(why, "dynamics.gravity") && contains(why, "finite gravity > 0"));
    }
    // (a value that is no finite number never becomes a double: the configurator refuses it, by the key's name)
    CHECK(contains(dyn(MODEL + "tilt = ssh\ngravity = nan\n"), "dynamics.gravity"));
    CHECK(contains(dyn(MODEL + "tilt = ssh\ngravity = inf\n"), "dynamics.gravity"));
    Configurator::clear();
}

static void test_forcing_file()
{
    const std::vector<std::string> wind = { "wind_u", "wind_v" }, ocean = { "ocean_u", "ocean_v" };
    auto with = [](std::vector<std::string> a, const std::vector<std::string>& b) {
        a.insert(a.end(), b.begin(), b.end());
        return a;
    };
    const std::string bare = forcingFile("bare.nc", with(wind, ocean));
    const std::string full = forcingFile("full.nc", with(with(wind, ocean), { "ssh" }));
    const std::string windSsh = forcingFile("wind_ssh.nc", with(wind, { "ssh" }));
    const std::string windOnly = forcingFile("wind.nc", wind);
    {
        const ForcingFile f(bare, false), g(full, false);
        CHECK(!f.hasSsh() && !f.has("ssh") && f.variables().size() == 4);
        CHECK(g.hasSsh() && g.hasOcean() && g.hasWind() && g.variables().size() == 5 && g.variables().back() == "ssh");
        CHECK(g.nxr() == 5 && g.nyr() == 3 && g.record("ssh", 1)[0] == 5. + 0.01 * 15);
        CHECK(contains(refusal([&] { f.record("ssh", 0); }), "no variable ssh"));
        bool known = false;
        for (const auto& k : ForcingFile::knownVariables())
            known = known || k == "ssh";
        CHECK(known);
    }
    {
        // ssh is held to the lattice and to finite values like every variable
        Hdf5Writer w;
        w.dataset("/time", { 2 }, { 0., 1. });
        w.dataset("/wind_u", { 2, 3, 5 }, std::vector<double>(30, 1.));
        w.dataset("/wind_v", { 2, 3, 5 }, std::vector<double>(30, 1.));
        w.dataset("/ssh", { 2, 3, 6 }, std::vector<double>(36, 0.));
        w.write(g_dir + "/lattice.nc");
        CHECK(contains(refusal([&] { ForcingFile(g_dir + "/lattice.nc", false); }), "all variables share one lattice"));
    }
    const std::string file = "forcing = file\nforcing_file = ";
    // the file and the tilt agree on who states it
    CHECK(dyn(MODEL + "tilt = ssh\n" + file + full + "\n") == "");
    CHECK(dyn(MODEL + "tilt = ssh\n" + file + windSsh + "\n") == "");
    CHECK(dyn(MODEL + "tilt = ssh\n" + file + windOnly + "\n") == ""); // no ocean pair: the box test's current and its height
    CHECK(dyn(MODEL + file + bare + "\n") == "" && dyn(MODEL + "tilt = geostrophic\n" + file + bare + "\n") == "");
    {
        const std::string why = dyn(MODEL + "tilt = ssh\n" + file + bare + "\n");
        CHECK(contains(why, "dynamics.tilt = ssh") && contains(why, bare) && contains(why, "holds ocean_u / ocean_v but no ssh"));
    }
    for (const std::string& path : { full, windSsh })
        for (const std::string tilt : { "", "tilt = geostrophic\n" }) {
            const std::string why = dyn(MODEL + tilt + file + path + "\n");
            CHECK(contains(why, path) && contains(why, "holds ssh: it needs dynamics.tilt = ssh"));
        }
    Configurator::clear();
}

static void test_hipstep_refuses_both_keys()
{
    CHECK(DynamicsStep::tiltKeys().size() == 2);
    for (const char* key : { "[dynamics]\ntilt = ssh\n", "[dynamics]\ntilt = geostrophic\n", "[dynamics]\ngravity = 9.81\n" }) {
        configureWith(std::string("[model]\ntime_step = 120\n") + key);
        const std::string why = refusal([] { HipStep().init(); });
        CHECK(contains(why, "dynamics.") && contains(why, "Nextsim::HipStep runs the column step alone"));
    }
    Configurator::clear();
}

int main(int argc, char** argv)
{
    g_dir = argc > 1 ? argv[1] : ".";
    test_abi();
    test_keys();
    test_forcing_file();
    test_hipstep_refuses_both_keys();
    std::printf("host tilt tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

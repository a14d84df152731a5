// snow_tests.cpp -- the snow load on the host (include/DynamicsStep.hpp "dynamics.snow_load", "dynamics.rho_snow"; include/nsdg_snow.h): the
// two keys, their defaults and every refusal -- snow_load without the column model, a bad density, a density without snow_load -- all in
// configure(), before a device is asked for.  Needs no device.  Same tiny harness as host_tests: CHECK() records failures, the exit code
// is the number of failures.
#include <cstdio>
#include <functional>
#include <memory>
#include <sstream>
#include <string>

#include "../../../include/nsdg.h"
#include "Configurator.hpp"
#include "DynamicsStep.hpp"

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

static void test_abi()
{
    CHECK(NSDG_SNOW_DENSITY == 330.0);
    CHECK(nsdg_snow_load_set(nullptr, nullptr, 1, NSDG_SNOW_DENSITY) == NSDG_ERR_ARG); // a null context, from either call, without a crash
    CHECK(nsdg_snow_load_nodal(nullptr, nullptr, nullptr, nullptr) == NSDG_ERR_ARG);
    CHECK(nsdg_abi_version() == 6);
}

static void test_keys()
{
    const std::string THERMO = MODEL + "thermodynamics = true\n";
    // off by default, and accepted with the column model in every combination the step knows
    CHECK(dyn(MODEL) == "" && dyn(MODEL + "snow_load = false\n") == "" && dyn(THERMO + "snow_load = false\n") == "");
    CHECK(dyn(THERMO + "snow_load = true\n") == "");
    CHECK(dyn(THERMO + "snow_load = true\nrho_snow = 250\n") == "" && dyn(THERMO + "snow_load = true\nrho_snow = 0\n") == ""); // the closed end
    CHECK(dyn(THERMO + "snow_load = true\nadvect_column_state = true\n") == "");
    CHECK(dyn(THERMO + "snow_load = true\nrheology = bbm\n") == "");
    CHECK(dyn(THERMO + "snow_load = true\nslab_ocean = true\n") == "");
    // without the column model there is no snow
    for (const std::string& ini : { MODEL + "snow_load = true\n", MODEL + "snow_load = true\nthermodynamics = false\n" }) {
        const std::string why = dyn(ini);
        CHECK(contains(why, "dynamics.snow_load needs dynamics.thermodynamics = true"));
    }
    // a bad density
    for (const std::string bad : { "-1", "-330", "-1e-300" }) {
        const std::string why = dyn(THERMO + "snow_load = true\nrho_snow = " + bad + "\n");
        CHECK(contains(why, "dynamics.rho_snow") && contains(why, "finite density >= 0"));
    }
    // (a value that is no finite number never becomes a double: the configurator refuses it, by the key's name)
    CHECK(contains(dyn(THERMO + "snow_load = true\nrho_snow = nan\n"), "dynamics.rho_snow"));
    CHECK(contains(dyn(THERMO + "snow_load = true\nrho_snow = inf\n"), "dynamics.rho_snow"));
    // a density without the load
    CHECK(contains(dyn(THERMO + "rho_snow = 330\n"), "dynamics.rho_snow needs dynamics.snow_load = true"));
    CHECK(contains(dyn(THERMO + "snow_load = false\nrho_snow = 250\n"), "dynamics.rho_snow needs dynamics.snow_load = true"));
    CHECK(contains(dyn(MODEL + "rho_snow = 330\n"), "dynamics.rho_snow needs dynamics.snow_load = true"));
    Configurator::clear();
}

int main()
{
    test_abi();
    test_keys();
    std::printf("host snow tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

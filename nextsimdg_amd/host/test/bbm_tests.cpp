// bbm_tests.cpp -- the brittle rheology on the host (include/DynamicsStep.hpp "dynamics.rheology"): every refusal of its keys before a
// device is asked for, the library's message for a bad [bbm] value, the history field `damage` with and without the rheology, and the
// optional `damage` row of the restart table through both file formats and between the ranks; needs no device.  Same tiny harness as
// host_tests: CHECK() records failures, the exit code is the number of failures.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/nsdg.h"
#include "Configurator.hpp"
#include "DynamicsStep.hpp"
#include "Hdf5Subset.hpp"
#include "HipStep.hpp"
#include "HistoryOutput.hpp"
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

// the message of the std::invalid_argument f throws; "" if it throws nothing, "other: ..." for another exception
static std::string refusal(const std::function<void()>& f)
{
    try {
        f();
    } catch (const std::invalid_argument& e) {
        return e.what();
    } catch (const std::exception& e) {
        return std::string("other: ") + e.what();
    }
    return "";
}

// configure() never asks for a device: whatever it refuses, it refuses before one
static std::string dyn(const std::string& ini)
{
    configureWith(ini);
    return refusal([] { DynamicsStep().configure(); });
}

static const char* const MODEL = "[model]\ntime_step = 120\n";

static void test_refusals()
{
    const std::string bbm = std::string(MODEL) + "[dynamics]\nrheology = bbm\n";
    CHECK(dyn(MODEL) == "");
    CHECK(dyn(std::string(MODEL) + "[dynamics]\nrheology = mevp\n") == "");
    CHECK(dyn(bbm) == "");
    CHECK(dyn(bbm + "nsub = 40\nbbm_courant = 0.3\nsubsteps = 2\n[bbm]\ncohesion_lab = 5e5\nrelax_exponent = 3\n") == "");
    CHECK(contains(dyn(std::string(MODEL) + "[dynamics]\nrheology = evp\n"), "dynamics.rheology must be mevp or bbm"));
    CHECK(contains(dyn(bbm + "thermodynamics = true\nadvect_column_state = true\n"), "five fields"));
    CHECK(dyn(bbm + "thermodynamics = true\n") == "");
    CHECK(contains(dyn(bbm + "substeps = auto\n"), "strength wave"));
    CHECK(contains(dyn(bbm + "graph = true\n"), "replays no graph"));
    CHECK(contains(dyn(bbm + "bbm_courant = 0\n"), "dynamics.bbm_courant must be positive"));
    // a bad [bbm] value: the library's own message
    const std::string dmax = dyn(bbm + "[bbm]\nd_max = 1.5\n"), expo = dyn(bbm + "[bbm]\nrelax_exponent = 0\n");
    CHECK(contains(dmax, "[bbm]") && contains(dmax, "d_max must lie in (0, 1)") && !contains(dmax, "other:"));
    CHECK(contains(expo, "relax_exponent must be an integer >= 1") && !contains(expo, "other:"));
    CHECK(contains(dyn(bbm + "[bbm]\nyoung = -1\n"), "young, lambda0 and t_heal must be positive"));
    CHECK(dyn(std::string(MODEL) + "[bbm]\nd_max = 1.5\n") == ""); // without the rheology the section is not looked at
    // the library's check needs no context
    nsdg_bbm_params p;
    nsdg_bbm_default_params(&p);
    CHECK(nsdg_bbm_params_check(&p) == NSDG_OK && nsdg_bbm_params_check(nullptr) == NSDG_ERR_ARG && nsdg_bbm_params_set(nullptr, &p) == NSDG_ERR_ARG);
    p.d_max = 1.;
    CHECK(nsdg_bbm_params_check(&p) == NSDG_ERR_ARG);
    // HipStep runs no rheology: any of the keys stops it before it asks for a device
    CHECK(DynamicsStep::brittleKeys().size() == 12);
    for (const char* key : { "[dynamics]\nrheology = bbm\n", "[dynamics]\nrheology = mevp\n", "[dynamics]\nbbm_courant = 0.25\n", "[bbm]\nyoung = 1e9\n", "[bbm]\nrelax_exponent = 5\n" }) {
        configureWith(std::string(MODEL) + key);
        const std::string why = refusal([] { HipStep().init(); });
        CHECK(contains(why, "Nextsim::HipStep runs the column step alone") && !contains(why, "other:"));
    }
    Configurator::clear();
}

static void test_damage_output()
{
    const std::string on = std::string(MODEL) + "output_period = 480\noutput_file = ice.nsdg\n";
    const std::string bbm = "[dynamics]\nrheology = bbm\n";
    CHECK(contains(dyn(on + "output_fields = damage\n"), "brittle rheology"));
    CHECK(contains(dyn(on + "output_fields = damage:max\n"), "brittle rheology"));
    CHECK(contains(dyn(on + "output_fields = damage\n[dynamics]\nrheology = mevp\n"), "brittle rheology"));
    CHECK(dyn(on + "output_fields = damage\n" + bbm) == "");
    CHECK(dyn(on + "output_fields = hice,damage,damage:max,damage:min,damage:ice_mean\n" + bbm) == "");
    CHECK(contains(dyn(on + "output_fields = damage,damage\n" + bbm), "listed twice"));
    const HistoryOutput::Config c = (configureWith(on + "output_fields = damage:max\n"), HistoryOutput::fromConfiguration(false, true));
    CHECK((c.ids == std::vector<int> { NSDG_HIST_DAMAGE }) && (c.stats == std::vector<int> { NSDG_STAT_MAX }));
    CHECK(contains(refusal([] { HistoryOutput::fromConfiguration(false); }), "brittle rheology")); // the default argument: no brittle rheology
    Configurator::clear();
}

static void fillState(FieldStore& f, int nx, int ny, bool damage)
{ // nx = slow ("x" of the file), ny = fast
    f.dyn.resize((std::size_t)nx, (std::size_t)ny);
    f.dyn.damage.assign(damage ? 6 * f.n : 0, 0.);
    auto fill = [&](std::vector<double>& v, double base) {
        for (std::size_t k = 0; k < v.size(); ++k)
            v[k] = base + 1e-3 * (double)k;
    };
    fill(f.dyn.hdg, 1.), fill(f.dyn.adg, 2.), fill(f.dyn.u, 3.), fill(f.dyn.v, 4.), fill(f.dyn.s11, 5.), fill(f.dyn.s12, 6.), fill(f.dyn.s22, 7.);
    fill(f.dyn.damage, 0.25);
    f.dyn.present = true;
}

static void test_restart_table()
{
    for (const bool damage : { false, true })
        for (const char* ext : { ".nc", ".nsdg" }) {
            const std::string path = std::string("/tmp/nsdg_bbm_test_restart") + ext;
            RectGrid g;
            g.resize(5, 7, 2);
            FieldStore& f = g.fields();
            for (std::size_t e = 0; e < f.n; ++e)
                f.hice[e] = 0.1 * e, f.cice[e] = 0.5, f.newice[e] = 1e-5 * e;
            fillState(f, 5, 7, damage);
            g.dump(path);
            auto again = StructureFactory::generateFromFile(path);
            again->init(path);
            const FieldStore& r = again->fields();
            CHECK(r.dyn.present && r.dyn.hdg == f.dyn.hdg && r.dyn.adg == f.dyn.adg && r.dyn.u == f.dyn.u && r.dyn.v == f.dyn.v);
            CHECK(r.dyn.s11 == f.dyn.s11 && r.dyn.s12 == f.dyn.s12 && r.dyn.s22 == f.dyn.s22 && r.newice == f.newice && r.hice == f.hice);
            CHECK(r.dyn.damage == f.dyn.damage && r.dyn.damage.size() == (damage ? 6 * f.n : 0)); // a file without damage leaves it empty
            CHECK(r.dyn.sdg.empty());
            if (Hdf5File::isHdf5(path)) {
                const Hdf5File h(path);
                CHECK(h.exists("/data/damage") == damage && h.exists("/data/dg2full") == damage && !h.exists("/data/hsnow_dg"));
                CHECK(!damage || h.dims("/data/damage") == (std::vector<std::uint64_t> { 6, 5, 7 }));
            } else {
                std::ifstream in(path, std::ios::binary);
                std::string head, line;
                while (std::getline(in, line) && line != "END-HEADER")
                    head += line + "\n";
                CHECK(contains(head, "data.damage=1") == damage && contains(head, ",damage") == damage && !contains(head, "data.snow_dg"));
            }
            std::remove(path.c_str());
        }
    // the rows of a rank travel with the damage, whether or not the receiver has any state yet; a state with the snow instead is told apart
    const int nx = 7, ny = 10; // here nx = the fast dimension of the dynamics (row length), ny = rows
    for (const int kind : { 0, 1, 2 }) { // no optional variable | the damage | the snow
        FieldStore a, b;
        a.resize((std::size_t)nx * ny, 1), b.resize((std::size_t)nx * ny, 1);
        fillState(a, ny, nx, kind == 1);
        if (kind == 2)
            a.dyn.sdg.assign(5 * a.n, 0.125);
        const std::vector<double> rows = DynamicsStep::packRows(a, false, nx, 3, 10);
        DynamicsStep::placeRows(b, false, nx, 3, 10, rows.data(), rows.size());
        CHECK(b.dyn.present && b.dyn.damage.size() == (kind == 1 ? 6 * a.n : 0) && b.dyn.sdg.size() == (kind == 2 ? 5 * a.n : 0));
        bool same = true;
        for (int c = 0; c < 6 && kind == 1; ++c)
            for (std::size_t e = 3 * (std::size_t)nx; e < a.n; ++e)
                same = same && b.dyn.damage[c * a.n + e] == a.dyn.damage[c * a.n + e];
        for (std::size_t e = 3 * (std::size_t)nx; e < a.n; ++e)
            same = same && b.dyn.hdg[4 * a.n + e] == a.dyn.hdg[4 * a.n + e] && b.dyn.s22[7 * a.n + e] == a.dyn.s22[7 * a.n + e];
        CHECK(same);
        CHECK(kind != 1 || b.dyn.damage[0] == 0.); // rows nobody sent stay at zero
    }
}

int main()
{
    test_refusals();
    test_damage_output();
    test_restart_table();
    std::printf("host brittle tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

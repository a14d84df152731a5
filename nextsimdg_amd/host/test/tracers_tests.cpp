// tracers_tests.cpp -- ice tracers on the host (include/DynamicsStep.hpp "dynamics.tracers"): the two keys are parsed and every bad value
// is refused, by a message that names the key, before a device is asked for; the tracer planes go through both restart file formats
// and between the ranks byte for byte, and a file without them reads back without them; needs no device.  Same tiny harness as
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

static const std::string MODEL = "[model]\ntime_step = 120\n[dynamics]\n";

static void writeNpy(const std::string& path, const std::string& descr, std::size_t nx, std::size_t ny, const std::vector<double>& values)
{
    std::string header = "{'descr': '" + descr + "', 'fortran_order': False, 'shape': (" + std::to_string(nx) + ", " + std::to_string(ny) + "), }";
    while ((10 + header.size() + 1) % 64)
        header += ' ';
    header += '\n';
    std::ofstream f(path, std::ios::binary);
    const unsigned char magic[8] = { 0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0 };
    f.write(reinterpret_cast<const char*>(magic), 8);
    const unsigned char len[2] = { (unsigned char)(header.size() & 255), (unsigned char)(header.size() >> 8) };
    f.write(reinterpret_cast<const char*>(len), 2);
    f << header;
    f.write(reinterpret_cast<const char*>(values.data()), (std::streamsize)(values.size() * sizeof(double)));
}

static void test_keys()
{
    typedef std::vector<std::string> Names;
    CHECK(DynamicsStep::tracerNames("").empty());
    CHECK((DynamicsStep::tracerNames("age,origin") == Names { "age", "origin" }));
    CHECK((DynamicsStep::tracerNames(" age , _b2 ,c,d") == Names { "age", "_b2", "c", "d" }));
    CHECK(dyn(MODEL) == "" && dyn(MODEL + "tracers = age,origin\n") == "" && dyn(MODEL + "tracers = age\nthermodynamics = true\n") == "");
    CHECK(dyn(MODEL + "tracers = age\nrheology = bbm\n") == "" && dyn(MODEL + "tracers = a,b\nthermodynamics = true\nadvect_column_state = true\n") == "");
    for (const auto& bad : { std::make_pair("a,b,c,d,e", "at most 4"), std::make_pair("age,age", "more than once"), std::make_pair("2nd", "not an identifier"),
             std::make_pair("my tracer", "not an identifier"), std::make_pair("a,,b", "not an identifier"), std::make_pair("a-b", "not an identifier"),
             std::make_pair("hice", "collides"), std::make_pair("damage", "collides"), std::make_pair("age,u", "collides"), std::make_pair("H", "collides") }) {
        const std::string why = dyn(MODEL + "tracers = " + bad.first + "\n");
        CHECK(contains(why, "dynamics.tracers") && contains(why, bad.second) && !contains(why, "other:"));
    }
    // dynamics.tracer_init: one entry per name, a float64 .npy file of two dimensions or -
    const std::string dir = "/tmp/nsdg_tracers_test_", good = dir + "good.npy", flat = dir + "int.npy";
    writeNpy(good, "<f8", 5, 7, std::vector<double>(35, 2.5));
    writeNpy(flat, "<i8", 5, 7, std::vector<double>(35, 0.));
    CHECK(dyn(MODEL + "tracers = age,origin\ntracer_init = -," + good + "\n") == "");
    CHECK(dyn(MODEL + "tracers = age,origin\ntracer_init = -,-\n") == "");
    for (const std::string& init : std::vector<std::string> { "-", "-,-,-", good, "-," + dir + "missing.npy", "-," + flat }) {
        const std::string why = dyn(MODEL + "tracers = age,origin\ntracer_init = " + init + "\n");
        CHECK(contains(why, "dynamics.tracer_init") && !contains(why, "other:"));
    }
    CHECK(contains(dyn(MODEL + "tracer_init = " + good + "\n"), "dynamics.tracer_init")); // values without names
    { // the shape is held against the structure's once there is one
        RectGrid g57, g75;
        g57.resize(5, 7, 1), g75.resize(7, 5, 1);
        configureWith(MODEL + "tracers = origin\ntracer_init = " + good + "\n");
        CHECK(refusal([&] { DynamicsStep s; s.setInitialData(g57); s.configure(); }) == "");
        const std::string why = refusal([&] { DynamicsStep s; s.setInitialData(g75); s.configure(); });
        CHECK(contains(why, "dynamics.tracer_init") && contains(why, "shape"));
    }
    std::remove(good.c_str()), std::remove(flat.c_str());
    Configurator::clear();
}

static void fillState(FieldStore& f, int nx, int ny, const std::vector<std::string>& tracers)
{ // nx = slow ("x" of the file), ny = fast
    f.dyn.resize((std::size_t)nx, (std::size_t)ny);
    auto fill = [&](std::vector<double>& v, double base) {
        for (std::size_t k = 0; k < v.size(); ++k)
            v[k] = base + 1e-3 * (double)k;
    };
    fill(f.dyn.hdg, 1.), fill(f.dyn.adg, 2.), fill(f.dyn.u, 3.), fill(f.dyn.v, 4.), fill(f.dyn.s11, 5.), fill(f.dyn.s12, 6.), fill(f.dyn.s22, 7.);
    f.dyn.tracers.clear();
    for (std::size_t k = 0; k < tracers.size(); ++k) {
        f.dyn.tracers.push_back({ tracers[k], std::vector<double>(f.n) });
        fill(f.dyn.tracers.back().values, 100. * (double)(k + 1));
    }
    f.dyn.present = true;
}

static bool sameTracers(const FieldStore& a, const FieldStore& b)
{
    bool same = a.dyn.tracers.size() == b.dyn.tracers.size();
    for (std::size_t k = 0; same && k < a.dyn.tracers.size(); ++k)
        same = a.dyn.tracers[k].name == b.dyn.tracers[k].name && a.dyn.tracers[k].values == b.dyn.tracers[k].values;
    return same;
}

static void test_restart_files()
{
    for (const std::vector<std::string>& tracers : { std::vector<std::string> {}, std::vector<std::string> { "age", "origin" } })
        for (const char* ext : { ".nc", ".nsdg" }) {
            const std::string path = std::string("/tmp/nsdg_tracers_test_restart") + ext;
            RectGrid g;
            g.resize(5, 7, 2);
            FieldStore& f = g.fields();
            for (std::size_t e = 0; e < f.n; ++e)
                f.hice[e] = 0.1 * e, f.cice[e] = 0.5;
            fillState(f, 5, 7, tracers);
            g.dump(path);
            // either format gives the tracers dynamics.tracers names, in its order (one the file does not hold is left out); the value is
            // read as DynamicsStep reads it: spaces around a name are not part of it
            configureWith("[dynamics]\ntracers = age, origin ,absent\n");
            auto again = StructureFactory::generateFromFile(path);
            again->init(path);
            const FieldStore& r = again->fields();
            CHECK(r.dyn.present && r.dyn.hdg == f.dyn.hdg && r.dyn.u == f.dyn.u && r.dyn.s22 == f.dyn.s22 && r.hice == f.hice);
            CHECK(sameTracers(r, f) && r.dyn.tracers.size() == tracers.size());
            if (Hdf5File::isHdf5(path)) {
                const Hdf5File h(path);
                CHECK(h.exists("/data/tracer_age") == !tracers.empty() && h.exists("/data/tracer_origin") == !tracers.empty() && !h.exists("/data/tracer_absent"));
                CHECK(tracers.empty() || h.dims("/data/tracer_origin") == (std::vector<std::uint64_t> { 5, 7 }));
            } else {
                std::ifstream in(path, std::ios::binary);
                std::string head, line;
                while (std::getline(in, line) && line != "END-HEADER")
                    head += line + "\n";
                CHECK(contains(head, "data.tracer.age=1\ndata.tracer.origin=1\n") == !tracers.empty() && contains(head, ",tracer_age,tracer_origin") == !tracers.empty());
            }
            {
                configureWith("[dynamics]\ntracers =  origin\n"); // only what the configuration names is kept
                auto one = StructureFactory::generateFromFile(path);
                one->init(path);
                CHECK(one->fields().dyn.tracers.size() == (tracers.empty() ? 0u : 1u));
                CHECK(tracers.empty() || (one->fields().dyn.tracers[0].name == "origin" && one->fields().dyn.tracers[0].values == f.dyn.tracers[1].values));
                configureWith("[dynamics]\ntracers = origin, age\n"); // in the configuration's order
                auto swapped = StructureFactory::generateFromFile(path);
                swapped->init(path);
                const auto& st = swapped->fields().dyn.tracers;
                CHECK(st.size() == tracers.size() && (tracers.empty() || (st[0].name == "origin" && st[1].name == "age" && st[1].values == f.dyn.tracers[0].values)));
                configureWith("[dynamics]\ntracers = 2nd\n"); // a bad value is refused here as it is in the step, by the key
                auto bad = StructureFactory::generateFromFile(path);
                CHECK(contains(refusal([&] { bad->init(path); }), "dynamics.tracers"));
            }
            // a dump of what was read is the same file, byte for byte
            const std::string second = path + ".again";
            configureWith("[dynamics]\ntracers = age,origin\n");
            auto copy = StructureFactory::generateFromFile(path);
            copy->init(path);
            copy->dump(second + ext);
            std::ifstream a(path, std::ios::binary), b(second + ext, std::ios::binary);
            const std::string ba((std::istreambuf_iterator<char>(a)), std::istreambuf_iterator<char>()), bb((std::istreambuf_iterator<char>(b)), std::istreambuf_iterator<char>());
            CHECK(!ba.empty() && ba == bb);
            std::remove(path.c_str()), std::remove((second + ext).c_str());
        }
    Configurator::clear();
    // the rows of a rank travel with its tracers; both ends run the same names
    const int nx = 7, ny = 10; // here nx = the fast dimension of the dynamics (row length), ny = rows
    FieldStore a, b;
    a.resize((std::size_t)nx * ny, 1), b.resize((std::size_t)nx * ny, 1);
    fillState(a, ny, nx, { "age", "origin" });
    fillState(b, ny, nx, { "age", "origin" });
    for (auto& t : b.dyn.tracers)
        t.values.assign(b.n, 0.);
    const std::vector<double> rows = DynamicsStep::packRows(a, false, nx, 3, 10);
    FieldStore none;
    none.resize((std::size_t)nx * ny, 1);
    fillState(none, ny, nx, {});
    CHECK(rows.size() == DynamicsStep::packRows(none, false, nx, 3, 10).size() + 2 * 7 * (std::size_t)nx);
    DynamicsStep::placeRows(b, false, nx, 3, 10, rows.data(), rows.size());
    bool same = true;
    for (std::size_t k = 0; k < 2; ++k)
        for (std::size_t e = 0; e < a.n; ++e)
            same = same && b.dyn.tracers[k].values[e] == (e < 3 * (std::size_t)nx ? 0. : a.dyn.tracers[k].values[e]); // rows nobody sent stay at zero
    CHECK(same && b.dyn.hdg[4 * a.n + a.n - 1] == a.dyn.hdg[4 * a.n + a.n - 1]);
    CHECK(contains(refusal([&] { DynamicsStep::placeRows(none, false, nx, 3, 10, rows.data(), rows.size()); }), "other: DynamicsStep: a rank delivered"));
}

int main()
{
    test_keys();
    test_restart_files();
    std::printf("host tracer tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

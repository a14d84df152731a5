// points_tests.cpp -- point samples on the host (include/Stations.hpp, include/Drifters.hpp "model.drifters_fields"): every refusal of the keys
// before a device is asked for, the header lines, the reader's handling of output lines with 5 + k columns, and the clock of the stations'
// blocks; needs no device.  Same tiny harness as host_tests: CHECK() records failures, the exit code is the number of failures.
#include <algorithm>
#include <cmath>
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
#include "Drifters.hpp"
#include "DynamicsStep.hpp"
#include "HipStep.hpp"
#include "Stations.hpp"

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

static std::string dir;
static std::string path(const std::string& name) { return dir + "/" + name; }

static void writeFile(const std::string& name, const std::string& text)
{
    std::ofstream out(path(name), std::ios::trunc);
    out << text;
}

static std::string readFile(const std::string& name)
{
    std::ifstream in(path(name));
    std::stringstream ss;
    ss << in.rdbuf();
    return ss.str();
}

static std::string model() // the domain is [0, 8000]^2
{
    return "[model]\ntime_step = 120\ndrifters_file = " + path("seeds.txt") + "\ndrifters_output = " + path("track.txt") + "\nstations_file = "
        + path("stations.txt") + "\nstations_output = " + path("moorings.txt") + "\n";
}

static void test_refusals()
{
    writeFile("seeds.txt", "100 200\n3.5e3 4e3 2\n");
    writeFile("stations.txt", "# x y\n100 200\n\n8000 8000\n0 0\n");
    const std::string dynamics = "[dynamics]\ndomain_size = 8000\n";
    const std::string good = model() + "drifters_fields = hice, cice,shear\nstations_fields = u,v,sigma_n\n";
    CHECK(dyn(good + dynamics) == "");
    CHECK(dyn(good + "stations_buffer = 2\n" + dynamics) == "");
    // a multi-process run and the rehearsal
    setenv("WORLD_SIZE", "2", 1);
    setenv("RANK", "0", 1);
    CHECK(contains(dyn("[model]\ntime_step = 120\nstations_file = " + path("stations.txt") + "\nstations_output = x\nstations_fields = u\n" + dynamics),
        "model.stations_file is set in a run of 2 processes"));
    unsetenv("WORLD_SIZE");
    unsetenv("RANK");
    CHECK(contains(dyn("[model]\ntime_step = 120\nstations_file = " + path("stations.txt") + "\nstations_output = x\nstations_fields = u\n" + dynamics
                       + "loopback_world = 3\n"),
        "model.stations_file is set with dynamics.loopback_world"));
    // the keys that go together
    const std::string st = "[model]\ntime_step = 120\nstations_file = " + path("stations.txt") + "\n";
    CHECK(contains(dyn(st + dynamics), "model.stations_output must name the file"));
    CHECK(contains(dyn(st + "stations_output = x\n" + dynamics), "model.stations_fields must list the fields"));
    CHECK(contains(dyn("[model]\ntime_step = 120\nstations_fields = u\n" + dynamics), "model.stations_fields is set without model.stations_file"));
    CHECK(contains(dyn("[model]\ntime_step = 120\nstations_buffer = 4\n" + dynamics), "model.stations_buffer is set without model.stations_file"));
    CHECK(contains(dyn("[model]\ntime_step = 120\ndrifters_fields = hice\n" + dynamics), "model.drifters_fields is set without model.drifters_file"));
    CHECK(contains(dyn(st + "stations_output = x\nstations_fields = u\nstations_buffer = 0\n" + dynamics), "model.stations_buffer must be a whole number"));
    CHECK(contains(dyn(st + "stations_output = x\nstations_fields = u\nstations_buffer = 2.5\n" + dynamics), "model.stations_buffer must be a whole number"));
    // the fields, for both consumers
    for (const std::string key : { "stations_fields", "drifters_fields" }) {
        const std::string other = key == "stations_fields" ? "drifters_fields = hice\n" : "stations_fields = hice\n";
        const std::string base = model() + other + key + " = ";
        CHECK(contains(dyn(base + "hice,thickness\n" + dynamics), "model." + key + ": unknown field \"thickness\" (known: hice cice u v"));
        CHECK(contains(dyn(base + "hice,u,hice\n" + dynamics), "model." + key + ": field \"hice\" is listed twice"));
        CHECK(contains(dyn(base + "damage\n" + dynamics), "model." + key + ": the field \"damage\" needs dynamics.rheology = bbm"));
        CHECK(dyn(base + "damage\n" + dynamics + "rheology = bbm\n") == "");
        CHECK(contains(dyn(base + "hsnow\n" + dynamics), "model." + key + ": the field \"hsnow\" is column state: it needs dynamics.thermodynamics"));
        CHECK(contains(dyn(base + "u,tice\n" + dynamics), "model." + key + ": the field \"tice\" is column state"));
        CHECK(dyn(base + "hsnow,tice\n" + dynamics + "thermodynamics = true\n") == "");
        CHECK(contains(dyn(base + " , \n" + dynamics), "model." + key + " names no field"));
    }
    // the stations' file
    writeFile("stations.txt", "100 200\n100 8000.5\n");
    CHECK(contains(dyn(good + dynamics), "stations.txt, line 2: the station is outside the domain"));
    writeFile("stations.txt", "nan 2\n");
    CHECK(contains(dyn(good + dynamics), "stations.txt, line 1: the station is outside the domain"));
    writeFile("stations.txt", "1 2 0\n");
    CHECK(contains(dyn(good + dynamics), "stations.txt, line 1: 3 columns; a line is \"x y\""));
    writeFile("stations.txt", "1 two\n");
    CHECK(contains(dyn(good + dynamics), "stations.txt, line 1: \"two\" is not a number"));
    std::remove(path("stations.txt").c_str());
    CHECK(contains(dyn(good + dynamics), "model.stations_file: cannot read"));
    writeFile("stations.txt", "100 200\n");
    // HipStep samples nothing: any of the new keys stops it before it asks for a device
    for (const std::string key : { "stations_file = a", "stations_output = a", "stations_fields = u", "stations_buffer = 3", "drifters_fields = u" }) {
        configureWith("[model]\n" + key + "\n");
        const std::string why = refusal([] { HipStep().init(); });
        CHECK(contains(why, "model." + key.substr(0, key.find(' ')) + " is set, but Nextsim::HipStep") && !contains(why, "other:"));
    }
    Configurator::clear();
}

static void test_header_lines_and_the_reader()
{
    CHECK(DriftersOutput::headerLine() == "# time id x y status");
    CHECK(DriftersOutput::headerLine({}) == "# time id x y status");
    CHECK(DriftersOutput::headerLine({ "hice", "cice", "shear" }) == "# time id x y status hice cice shear");
    CHECK(StationsOutput::headerLine({ "u", "sigma_n" }) == "# time id x y u sigma_n");
    const double smp[4] = { 0.1, 99., -2.5e-7, 99. };
    CHECK(DriftersOutput::formatLine(480, 3, 1500., 0.1, 2.) == "480 3 1500 0.10000000000000001 2");
    CHECK(DriftersOutput::formatLine(480, 3, 1500., 0.1, 2., nullptr, 0, 7) == DriftersOutput::formatLine(480, 3, 1500., 0.1, 2.));
    CHECK(DriftersOutput::formatLine(480, 3, 1500., 0.1, 2., smp, 2, 2) == "480 3 1500 0.10000000000000001 2 0.10000000000000001 -2.4999999999999999e-07");
    CHECK(StationsOutput::formatLine(120, 0, 8000., 0., smp, 2, 2) == "120 0 8000 0 0.10000000000000001 -2.4999999999999999e-07");
    const double special[2] = { -INFINITY, NAN };
    CHECK(StationsOutput::formatLine(120, 1, 1., 2., special, 2, 1) == "120 1 1 2 -inf nan");

    // an output block with k = 3 extra columns is an input file: the samples are ignored
    writeFile("block.txt", "# time id x y status hice cice shear\n480 0 100 200 0 0.3 0.9 1e-7\n480 1 3500 4000 2 0.5 1 nan\n");
    const std::vector<double> d = DriftersOutput::read(path("block.txt"), 8000., 8000.);
    CHECK(d == std::vector<double>({ 100., 3500., 200., 4000., 0., 2. }));
    // ... only with the header that names them, and only for exactly 5 + k columns: the messages for other counts stay as they are
    writeFile("block.txt", "480 0 100 200 0 0.3 0.9 1e-7\n");
    CHECK(contains(refusal([] { DriftersOutput::read(path("block.txt"), 8000., 8000.); }), "line 1: 8 columns; a line is \"x y\", \"x y status\" or \"time id x y status\""));
    writeFile("block.txt", "# time id x y status hice cice shear\n480 0 100 200 0 0.3 0.9\n");
    CHECK(contains(refusal([] { DriftersOutput::read(path("block.txt"), 8000., 8000.); }), "line 2: 7 columns"));
    writeFile("block.txt", "# time id x y status hice\n480 0 100 200 0 0.3\n100 200\n5 6 1\n480 7 300 400 3\n1 2 3 4\n");
    CHECK(contains(refusal([] { DriftersOutput::read(path("block.txt"), 8000., 8000.); }), "line 6: 4 columns"));
    writeFile("block.txt", "# time id x y status hice\n480 0 100 200 0 0.3\n100 200\n5 6 1\n480 7 300 400 3\n");
    CHECK(DriftersOutput::read(path("block.txt"), 8000., 8000.).size() == 12);
    writeFile("block.txt", "# my buoys\n# time id x y status\n480 0 100 200 0 0.3\n");
    CHECK(contains(refusal([] { DriftersOutput::read(path("block.txt"), 8000., 8000.); }), "line 3: 6 columns"));
    writeFile("block.txt", "# time id x y status hice\n480 0 100 200 5 0.3\n");
    CHECK(contains(refusal([] { DriftersOutput::read(path("block.txt"), 8000., 8000.); }), "line 2: unknown status"));

    // the stations' reader
    writeFile("stations.txt", "# x y\n100 200\n\n8000 8000\n0 0\n");
    CHECK(StationsOutput::read(path("stations.txt"), 8000., 8000.) == std::vector<double>({ 100., 8000., 0., 200., 8000., 0. }));
}

static void test_files_and_the_block_clock()
{
    // the drifters' file: with fields the header and the lines grow, without them the file is what it was
    DriftersOutput::Config dc;
    dc.file = path("seeds.txt"), dc.output = path("track.txt");
    {
        DriftersOutput plain(dc);
        plain.start(0);
        CHECK(!plain.step(120) && plain.dueAtStop());
        plain.write({ 100., 3500., 200., 4000., 0., 2. });
        CHECK(readFile("track.txt") == "# time id x y status\n120 0 100 200 0\n120 1 3500 4000 2\n");
        CHECK(contains(refusal([&] { plain.write({ 1., 2., 0. }, { 5. }); }), "other: DriftersOutput::write"));
    }
    dc.fields = { "hice", "shear" }, dc.fieldIds = { NSDG_HIST_HICE, NSDG_HIST_SHEAR };
    {
        DriftersOutput with(dc);
        with.start(240);
        with.step(120);
        with.write({ 100., 3500., 200., 4000., 0., 2. }, { 0.25, 0.5, 1e-7, 2e-7 });
        CHECK(readFile("track.txt") == "# time id x y status hice shear\n360 0 100 200 0 0.25 9.9999999999999995e-08\n360 1 3500 4000 2 0.5 1.9999999999999999e-07\n");
        CHECK(DriftersOutput::read(path("track.txt"), 8000., 8000.) == std::vector<double>({ 100., 3500., 200., 4000., 0., 2. })); // fed back in
        CHECK(contains(refusal([&] { with.write({ 1., 2., 0. }); }), "other: DriftersOutput::write"));
    }
    // the stations: one block per model step on the integer clock, slots counted by the host
    StationsOutput::Config sc;
    sc.file = path("stations.txt"), sc.output = path("moorings.txt"), sc.names = { "u", "hice" }, sc.ids = { NSDG_HIST_U, NSDG_HIST_HICE }, sc.buffer = 2;
    StationsOutput st(sc);
    st.start(600);
    CHECK(readFile("moorings.txt") == "# time id x y u hice\n");
    CHECK(st.step(120) == 0 && !st.full());
    CHECK(st.step(120) == 1 && st.full());
    CHECK(st.pending() == std::vector<long>({ 720, 840 }));
    CHECK(contains(refusal([&] { st.step(120); }), "other: StationsOutput::step"));
    const std::vector<double> xy = { 100., 8000., 200., 0. }; // two stations
    CHECK(contains(refusal([&] { st.write(xy, { 1., 2. }); }), "other: StationsOutput::write"));
    st.write(xy, { 0.5, -0.5, 1., 2., 0.25, -0.25, 3., 4. }); // [slot][field][station]
    CHECK(st.pending().empty() && !st.full());
    CHECK(readFile("moorings.txt")
        == "# time id x y u hice\n720 0 100 200 0.5 1\n720 1 8000 0 -0.5 2\n840 0 100 200 0.25 3\n840 1 8000 0 -0.25 4\n");
    CHECK(st.step(120) == 0);
    st.write(xy, { 7., 8., 9., 10. });
    CHECK(contains(readFile("moorings.txt"), "\n960 1 8000 0 8 10\n"));
    st.write(xy, {}); // nothing pending (a second stop()): nothing is written
    const std::string all = readFile("moorings.txt");
    CHECK(std::count(all.begin(), all.end(), '\n') == 7);
    sc.buffer = 0;
    CHECK(contains(refusal([&] { StationsOutput bad(sc); }), "StationsOutput:"));
}

int main()
{
    const char* tmp = std::getenv("TMPDIR");
    char name[512];
    std::snprintf(name, sizeof name, "%s/nsdg_points_tests_XXXXXX", tmp ? tmp : "/tmp");
    if (!mkdtemp(name)) {
        std::printf("cannot create a temporary directory\n");
        return 1;
    }
    dir = name;
    test_refusals();
    test_header_lines_and_the_reader();
    test_files_and_the_block_clock();
    for (const char* f : { "seeds.txt", "stations.txt", "track.txt", "moorings.txt", "block.txt" })
        std::remove(path(f).c_str());
    std::remove(dir.c_str());
    std::printf("host point-sample tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

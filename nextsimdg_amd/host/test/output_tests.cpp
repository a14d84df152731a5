// output_tests.cpp -- history output on the host (include/HistoryOutput.hpp): the window arithmetic, every refusal of the keys before a
// device is touched, both record formats read back, and a window that is flushed once; needs no device.  Same tiny harness as
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

static HistoryOutput::Config config(long period, bool snapshot = false)
{
    HistoryOutput::Config c;
    c.period = period, c.file = "ice.nsdg", c.fields = { "hice" }, c.ids = { NSDG_HIST_HICE }, c.snapshot = snapshot;
    return c;
}

// a run of `steps` model steps of dt from `start`, as DynamicsStep drives the object: "time_start-time_end:samples" of every record
// written, the stores as 's' / adds as 'a' in `trace`
static std::vector<std::string> run(HistoryOutput& h, long start, long dt, int steps, std::string* trace = nullptr, int stops = 1)
{
    std::vector<std::string> records;
    auto flush = [&] {
        if (h.samples() > 0)
            records.push_back(std::to_string(h.windowStart()) + "-" + std::to_string(h.windowEnd()) + ":" + std::to_string(h.samples()));
        h.closeWindow();
    };
    h.start(start);
    for (int k = 0; k < steps; ++k) {
        const HistoryOutput::Action a = h.step(dt);
        if (trace)
            *trace += a.sample ? (a.store ? 's' : 'a') : '.';
        if (a.flush)
            flush();
    }
    for (int k = 0; k < stops; ++k) // stop(), and writeRestartFile() reaches stop() again
        flush();
    return records;
}

static void test_windows()
{
    typedef std::vector<std::string> V;
    std::string trace;
    HistoryOutput h(config(480));
    CHECK((run(h, 0, 120, 8, &trace) == V { "0-480:4", "480-960:4" }));
    CHECK(trace == "saaasaaa"); // the first sample of a window stores, the others add
    CHECK(h.clock() == 960);
    // a start inside a window: the window ends at the multiple of the period, with the samples it has
    CHECK((run(h, 240, 120, 6) == V { "240-480:2", "480-960:4" }));
    // a stop inside a window writes it with the samples it has -- once, however often stop() comes
    CHECK((run(h, 0, 120, 6, nullptr, 2) == V { "0-480:4", "480-720:2" }));
    CHECK((run(h, 0, 120, 4, nullptr, 2) == V { "0-480:4" })); // a stop at a window boundary leaves nothing to flush
    // 8 steps == 4 steps + restart + 4 steps
    V both = run(h, 0, 120, 4);
    for (const std::string& r : run(h, 480, 120, 4))
        both.push_back(r);
    CHECK((both == run(h, 0, 120, 8)));
    // period = time step: every step is a window of its own, every sample stores
    HistoryOutput every(config(120));
    trace.clear();
    CHECK((run(every, 0, 120, 3, &trace) == V { "0-120:1", "120-240:1", "240-360:1" }));
    CHECK(trace == "sss");
    // a negative clock: windows stay aligned to absolute time
    CHECK((run(h, -600, 120, 5) == V { "-600--480:1", "-480-0:4" }));
    // a snapshot samples the last step of a window alone, and a stop inside a window has nothing to write
    HistoryOutput snap(config(480, true));
    trace.clear();
    CHECK((run(snap, 0, 120, 10, &trace) == V { "360-480:1", "840-960:1" }));
    CHECK(trace == "...s...s..");
    CHECK(refusal([] { HistoryOutput off(config(0)); }) != "");
}

static void test_paths()
{
    CHECK(HistoryOutput::recordPath("ice.nsdg", 480) == "ice.0000000480.nsdg");
    CHECK(HistoryOutput::recordPath("/tmp/run.1/ice.nc", 86400) == "/tmp/run.1/ice.0000086400.nc");
    CHECK(HistoryOutput::recordPath("/tmp/run.1/ice", 120) == "/tmp/run.1/ice.0000000120");
    CHECK(HistoryOutput::recordPath("ice.nsdg", 480, 3, 8) == "ice.0000000480.nsdg.rank3");
    CHECK(HistoryOutput::recordPath("ice.nsdg", -120) == "ice.-0000000120.nsdg");
}

static const char* const MODEL = "[model]\ntime_step = 120\n";

static void test_refusals()
{
    auto dyn = [](const std::string& ini) {
        configureWith(ini);
        return refusal([] { DynamicsStep().configure(); });
    };
    const std::string on = std::string(MODEL) + "output_period = 480\noutput_file = ice.nsdg\n";
    CHECK(dyn(MODEL) == ""); // off by default
    CHECK(dyn(std::string(MODEL) + "output_period = 0\noutput_fields = nonsense\n") == ""); // off: the other keys are not looked at
    CHECK(dyn(on) == "");
    CHECK(dyn(on + "output_fields = hice,speed,divergence,shear,sigma_n,sigma_s\noutput_kind = snapshot\n") == "");
    CHECK(contains(dyn(std::string(MODEL) + "output_period = 500\noutput_file = ice.nsdg\n"), "not a whole multiple of model.time_step"));
    CHECK(contains(dyn(std::string(MODEL) + "output_period = 480.5\noutput_file = ice.nsdg\n"), "whole number of seconds"));
    CHECK(contains(dyn(std::string(MODEL) + "output_period = -480\noutput_file = ice.nsdg\n"), "must not be negative"));
    CHECK(contains(dyn(std::string(MODEL) + "output_period = 480\n"), "model.output_file must name the record files"));
    CHECK(contains(dyn(on + "output_fields = hice,thickness\n"), "unknown field \"thickness\""));
    CHECK(contains(dyn(on + "output_fields = hice,u,hice\n"), "\"hice\" is listed twice"));
    CHECK(contains(dyn(on + "output_fields = hice,hsnow\n"), "\"hsnow\" is column state"));
    CHECK(contains(dyn(on + "output_fields = tice\n"), "\"tice\" is column state"));
    CHECK(dyn(on + "output_fields = hice, hsnow, tice\n[dynamics]\nthermodynamics = true\n") == "");
    CHECK(contains(dyn(on + "output_fields = damage\n"), "brittle rheology"));
    CHECK(contains(dyn(on + "output_kind = maximum\n"), "must be mean or snapshot"));
    // HipStep writes no history: any of the keys stops it before it asks for a device
    for (const char* key : { "output_period = 480\n", "output_file = ice.nsdg\n", "output_fields = hice\n", "output_kind = mean\n" }) {
        configureWith(std::string(MODEL) + key);
        const std::string why = refusal([] { HipStep().init(); });
        CHECK(contains(why, "Nextsim::HipStep writes no history output") && !contains(why, "other:"));
    }
    Configurator::clear();
    const HistoryOutput::Config def = (configureWith(on), HistoryOutput::fromConfiguration(false));
    CHECK((def.fields == std::vector<std::string> { "hice", "cice", "u", "v" }) && !def.snapshot && def.period == 480);
    CHECK((def.ids == std::vector<int> { NSDG_HIST_HICE, NSDG_HIST_CICE, NSDG_HIST_U, NSDG_HIST_V }));
    Configurator::clear();
}

static void test_field_names()
{
    const char* const names[NSDG_HIST_COUNT] = { "hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s", "hsnow", "tice", "damage" };
    for (int f = 0; f < NSDG_HIST_COUNT; ++f)
        CHECK(std::string(nsdg_history_field_name(f)) == names[f] && nsdg_history_field_id(names[f]) == f);
    CHECK(nsdg_history_field_name(NSDG_HIST_COUNT) == nullptr && nsdg_history_field_id("thickness") == -1 && nsdg_history_field_id(nullptr) == -1);
    CHECK(nsdg_history_accumulate(nullptr, 0, 0, 1, nullptr, nullptr, 1, 0, 0, nullptr) == NSDG_ERR_ARG);
}

static void test_round_trip(const std::string& dir)
{
    HistoryOutput::Record r;
    r.timeStart = 480, r.timeEnd = 960, r.samples = 4, r.kind = "mean";
    r.fields = { "hice", "speed", "sigma_n" };
    r.x = 7, r.y = 5, r.row0 = 2, r.rows = 3;
    for (std::size_t k = 0; k < r.fields.size() * 15; ++k)
        r.data.push_back(1.0 / 3.0 * (double)(k + 1) - 2.0);
    for (const char* name : { "ice.nsdg", "ice.nc", "ice.h5", "ice.hdf5" }) {
        const std::string file = dir + "/" + name, path = HistoryOutput::recordPath(file, r.timeEnd);
        HistoryOutput::write(path, file, r);
        CHECK(Hdf5File::isHdf5(path) == (std::string(name) != "ice.nsdg"));
        const HistoryOutput::Record b = HistoryOutput::read(path);
        CHECK(b.timeStart == 480 && b.timeEnd == 960 && b.samples == 4 && b.kind == "mean" && b.fields == r.fields);
        CHECK(b.x == 7 && b.y == 5 && b.row0 == 2 && b.rows == 3 && b.data == r.data); // bit for bit
        if (Hdf5File::isHdf5(path)) { // one dataset per field, the attributes beside them
            const Hdf5File h(path);
            CHECK((h.dims("/data/speed") == std::vector<std::uint64_t> { 3, 5 }));
            CHECK(h.stringAttribute("/history", "fields") == "hice,speed,sigma_n" && h.stringAttribute("/history", "kind") == "mean");
            CHECK(h.readDoubles("/data/sigma_n") == std::vector<double>(r.data.begin() + 30, r.data.end()));
        }
    }
    // a rank's file: the format is that of the configured name, whatever the suffix
    const std::string file = dir + "/part.nc", path = HistoryOutput::recordPath(file, 960, 1, 2);
    HistoryOutput::write(path, file, r);
    CHECK(contains(path, "part.0000000960.nc.rank1") && Hdf5File::isHdf5(path) && HistoryOutput::read(path).data == r.data);
    {
        std::ofstream cut(dir + "/cut.nsdg", std::ios::binary);
        cut << "NSDG-HISTORY 1\ntime_start=0\ntime_end=1\nsamples=1\nkind=mean\nfields=hice\nx=2\ny=2\nrow0=0\nrows=2\nEND-HEADER\nabc";
    }
    bool threw = false;
    try {
        HistoryOutput::read(dir + "/cut.nsdg");
    } catch (const std::runtime_error& e) {
        threw = contains(e.what(), "truncated");
    }
    CHECK(threw);
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    test_windows();
    test_paths();
    test_refusals();
    test_field_names();
    test_round_trip(dir);
    std::printf("output tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

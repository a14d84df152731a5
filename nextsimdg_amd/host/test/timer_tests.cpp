// timer_tests.cpp -- the timer's device-time nodes (Timer::setDeviceNode / setDeviceTime, PhaseTiming) fed synthetic numbers, and the
// argument checks of the library's phase entry points; needs no device.  Same tiny harness as host_tests: CHECK() records failures,
// the exit code is the number of failures.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/nsdg.h"
#include "PhaseTiming.hpp"
#include "Timer.hpp"

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
static std::vector<std::string> lines(const std::string& s)
{
    std::vector<std::string> out;
    std::istringstream is(s);
    for (std::string l; std::getline(is, l);)
        out.push_back(l);
    return out;
}

static void test_null_context()
{
    nsdg_phase_table t;
    CHECK(nsdg_phase_timing_set(nullptr, 1) == NSDG_ERR_ARG);
    CHECK(contains(nsdg_last_error(), "nsdg_phase_timing_set"));
    CHECK(nsdg_phase_mark(nullptr, NSDG_PHASE_COLUMN) == NSDG_ERR_ARG);
    CHECK(contains(nsdg_last_error(), "nsdg_phase_mark"));
    CHECK(nsdg_phase_times(nullptr, &t, 0) == NSDG_ERR_ARG);
    CHECK(contains(nsdg_last_error(), "nsdg_phase_times"));
}

static void test_device_nodes()
{
    Timer t("root");
    int syncs = 0;
    t.tick("run");
    for (int k = 0; k < 4; ++k) {
        t.tick("iterate");
        CHECK((t.currentPath() == std::vector<std::string> { "run", "iterate" }));
        t.tock("iterate"); // no hook was set: nothing to call, and nothing crashes
    }
    t.tock("run");
    CHECK(syncs == 0);
    CHECK(t.deviceSeconds({ "run", "iterate" }) < 0);
    const std::vector<std::string> it = { "run", "iterate" };
    // 4 steps: total 2 s on the device; phases 0.25 + 1.25 + 0.5 = 2 s, mentioned in this order; an overlapped exchange under sub-cycle
    t.setDeviceTime(it, 2.0);
    t.setDeviceNode(it, "forcing", 0.25, 4);
    t.setDeviceNode(it, "sub-cycle", 1.25, 4);
    t.setDeviceNode(it, "transport", 0.5, 8);
    t.setDeviceNode({ "run", "iterate", "sub-cycle" }, "exchange", 0.75, 120, true);
    t.setDeviceNode(it, "forcing", 0.25, 4); // a second resolution updates, it does not duplicate
    CHECK(t.ticks({ "run", "iterate" }) == 4);
    CHECK(t.ticks({ "run", "iterate", "transport" }) == 8);
    CHECK(t.deviceSeconds({ "run", "iterate", "sub-cycle" }) == 1.25);
    std::ostringstream os;
    t.report(os);
    const std::vector<std::string> l = lines(os.str());
    CHECK(l.size() == 7);
    if (l.size() == 7) {
        // the host-clocked lines keep their format
        CHECK(l[0].rfind("root: ticks = 1 wall time ", 0) == 0 && contains(l[0], " cpu time "));
        CHECK(l[1].rfind("`- run: ticks = 1 wall time ", 0) == 0);
        CHECK(l[2].rfind("   `- iterate: ticks = 4 wall time ", 0) == 0 && contains(l[2], "% of parent) cpu time ") && contains(l[2], " ms/tick"));
        // the device-time lines: same shape, "device time", the share from DEVICE times (0.25 / 2, 1.25 / 2, 0.5 / 2), first-mention order
        CHECK(l[3] == "      +- forcing: ticks = 4 device time 0.250000 s (12.5% of parent) 62.500 ms/tick");
        CHECK(l[4] == "      +- sub-cycle: ticks = 4 device time 1.250000 s (62.5% of parent) 312.500 ms/tick");
        CHECK(l[5] == "      |  `- exchange: ticks = 120 device time 0.750000 s (overlapped, in no sum) 6.250 ms/tick");
        CHECK(l[6] == "      `- transport: ticks = 8 device time 0.500000 s (25.0% of parent) 62.500 ms/tick");
    }
    if (failures)
        std::printf("%s", os.str().c_str());
    // a hook that IS set is called at every tock -- and only then
    t.setDeviceSync([&] { ++syncs; });
    t.tick("a");
    t.tock();
    CHECK(syncs == 1);
}

static void test_phase_timing_helpers()
{
    CHECK(std::string(PhaseTiming::phaseName(NSDG_PHASE_SUBCYCLE)) == "sub-cycle");
    CHECK(std::string(PhaseTiming::phaseName(NSDG_PHASE_REDUCTION)) == "reduction");
    CHECK(std::string(PhaseTiming::phaseName(9)) == "phase 9");
    // two blocks: the tree takes the slower block per phase; the file has both
    std::vector<PhaseBlockTimes> blocks(2);
    blocks[0].block = 0, blocks[1].block = 1;
    for (int k = 0; k < 2; ++k) {
        nsdg_phase_table& tb = blocks[k].table;
        tb.ms[NSDG_PHASE_FORCING] = 10. + k, tb.count[NSDG_PHASE_FORCING] = 2;
        tb.ms[NSDG_PHASE_SUBCYCLE] = 100. - 10 * k, tb.count[NSDG_PHASE_SUBCYCLE] = 2;
        tb.total_ms = 110. + k, tb.spans = 2;
        blocks[k].hasExchange = true;
        blocks[k].subcycleExchange.exchanges = 30, blocks[k].subcycleExchange.ms = 5. + k;
    }
    Timer t("root");
    t.tick("iterate");
    t.tock();
    PhaseTiming::toTimer(t, { "iterate" }, blocks);
    CHECK(t.deviceSeconds({ "iterate" }) == 1e-3 * 111.);
    CHECK(t.deviceSeconds({ "iterate", "forcing" }) == 1e-3 * 11.);
    CHECK(t.deviceSeconds({ "iterate", "sub-cycle" }) == 1e-3 * 100.);
    CHECK(t.deviceSeconds({ "iterate", "sub-cycle", "exchange" }) == 1e-3 * 6.);
    CHECK(t.ticks({ "iterate", "transport" }) == 0); // a phase that never ran has no node
    const std::string js = PhaseTiming::json(0, 1, 2, 2, blocks);
    CHECK(contains(js, "\"steps\": 2") && contains(js, "\"block\": 1") && contains(js, "\"sub-cycle\": {\"ms\": 90, \"count\": 2, \"exchange\": {"));
    CHECK(contains(js, "\"total_ms\": 111, \"spans\": 2") && !contains(js, "transport"));
}

int main()
{
    try {
        test_null_context();
        test_device_nodes();
        test_phase_timing_helpers();
    } catch (const std::exception& e) {
        std::printf("FAIL: unexpected exception: %s\n", e.what());
        ++failures;
    }
    std::printf("timer tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

// budget_tests.cpp -- the momentum budget on the host (include/BudgetOutput.hpp; include/nsdg_budget.h): the four keys, their defaults and
// every refusal -- a run of several processes, dynamics.rheology = bbm, an unknown or repeated term, a period without a file or off the
// time step, every key under Nextsim::HipStep --, the clock that says when a record is due, the series' header, line and row-order sum.
// Needs no device.  Same tiny harness as host_tests: CHECK() records failures, the exit code is the number of failures.
#include <cstdio>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/nsdg.h"
#include "BudgetOutput.hpp"
#include "Configurator.hpp"

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

static std::string refusal(const std::function<void()>& f)
{
    try {
        f();
    } catch (const std::invalid_argument& e) {
        return e.what();
    }
    return "";
}

int main()
{
    // off: nothing is read, and the keys that need a file say so
    configureWith("[model]\ntime_step = 120\n");
    CHECK(!BudgetOutput::fromConfiguration(1, false).on());
    CHECK(!BudgetOutput::fromConfiguration(4, true).on()); // without the keys neither refusal fires
    configureWith("[model]\ntime_step = 120\nbudget_terms = wind\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, false); }), "model.budget_file must name the record files"));

    // defaults: all eight terms in id order, period 0
    configureWith("[model]\ntime_step = 120\nbudget_file = forces.nc\n");
    BudgetOutput::Config c = BudgetOutput::fromConfiguration(1, false);
    CHECK(c.on() && c.terms.size() == NSDG_BUDGET_TERMS && c.terms[0] == "wind" && c.terms[7] == "residual" && c.period == 0 && c.seriesFile.empty());
    for (int k = 0; k < NSDG_BUDGET_TERMS; ++k)
        CHECK(c.ids[k] == k && nsdg_budget_term_id(c.terms[k].c_str()) == k);
    configureWith("[model]\ntime_step = 120\nbudget_file = forces.nc\nbudget_terms = wind, water,internal,residual\nbudget_period = 240\nbudget_series_file = p.txt\n");
    c = BudgetOutput::fromConfiguration(1, false);
    CHECK(c.ids == std::vector<int>({ 0, 1, 4, 7 }) && c.period == 240 && c.seriesFile == "p.txt");

    // refusals
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(2, false); }), "model.budget_file is set in a run of 2 processes"));
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, true); }), "dynamics.rheology = bbm"));
    configureWith("[model]\ntime_step = 120\nbudget_series_file = p.txt\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(3, false); }), "model.budget_series_file is set in a run of 3 processes"));
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, true); }), "model.budget_series_file is set with dynamics.rheology = bbm"));
    CHECK(BudgetOutput::fromConfiguration(1, false).file.empty());
    configureWith("[model]\ntime_step = 120\nbudget_file = f.nc\nbudget_terms = wind,friction\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, false); }), "unknown term \"friction\" (known: wind water coriolis tilt internal basal inertia residual)"));
    configureWith("[model]\ntime_step = 120\nbudget_file = f.nc\nbudget_terms = wind,wind\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, false); }), "named more than once"));
    configureWith("[model]\ntime_step = 120\nbudget_file = f.nc\nbudget_period = 100\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, false); }), "not a whole multiple of model.time_step"));
    configureWith("[model]\ntime_step = 120\nbudget_file = f.nc\nbudget_period = -1\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, false); }), "must not be negative"));
    configureWith("[model]\ntime_step = 120\nbudget_series_file = p.txt\nbudget_period = 240\n");
    CHECK(contains(refusal([] { BudgetOutput::fromConfiguration(1, false); }), "model.budget_file must name the record files"));
    for (const char* key : { "budget_file = f.nc", "budget_terms = wind", "budget_period = 0", "budget_series_file = p.txt" }) {
        configureWith(std::string("[model]\ntime_step = 120\n") + key + "\n");
        CHECK(contains(refusal([] { BudgetOutput::refuseFor("Nextsim::HipStep"); }), "Nextsim::HipStep has no momentum balance"));
    }
    configureWith("[model]\ntime_step = 120\n");
    CHECK(refusal([] { BudgetOutput::refuseFor("Nextsim::HipStep"); }).empty());

    // the clock: a record after the step in which the clock reaches a multiple of the period; period 0: one at the stop, once
    BudgetOutput::Config p;
    p.file = "f.nsdg", p.period = 240;
    BudgetOutput o(p);
    o.start(0);
    CHECK(!o.step(120) && o.step(120) && !o.step(120) && o.clock() == 360 && !o.dueAtStop());
    p.period = 0;
    BudgetOutput e(p);
    e.start(600);
    CHECK(!e.dueAtStop()); // no step has run
    CHECK(!e.step(120) && !e.step(120) && e.dueAtStop() && !e.dueAtStop());

    // the series: header, line, and rows added one after the other
    CHECK(BudgetOutput::headerLine() == "# time wind water coriolis tilt internal basal inertia residual ke");
    CHECK(BudgetOutput::formatLine(480, { 1., -0.5 }) == "480 1 -0.5");
    CHECK(BudgetOutput::formatLine(0, { 0.1 }) == "0 0.10000000000000001");
    std::vector<double> rows(NSDG_BUDGET_QUANTITIES * 3, 0.);
    rows[0] = 1., rows[1] = 0x1p-53, rows[2] = 0x1p-53; // (1 + 2^-53) + 2^-53 = 1 in row order; another order gives 1 + 2^-52
    rows[8 * 3 + 2] = 7.;
    const std::vector<double> t = BudgetOutput::totals(rows.data(), 3);
    CHECK(t.size() == NSDG_BUDGET_QUANTITIES && t[0] == 1. && t[1] == 0. && t[8] == 7.);

    std::printf("host budget tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

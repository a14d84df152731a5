// output_stats_tests.cpp -- history statistics and time series on the host (include/HistoryOutput.hpp): the field:stat entries of
// model.output_fields and the model.series_* keys with everything they refuse before a device is touched, the dataset names of a record,
// what the host makes of a window per statistic, and the series lines written, appended and read back; needs no device.  The harness
// of output_tests: CHECK() records failures, the exit code is the number of failures.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <limits>
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

static const char* const MODEL = "[model]\ntime_step = 120\n";
static const double NaN = std::numeric_limits<double>::quiet_NaN();

static std::string dyn(const std::string& ini)
{
    configureWith(ini);
    return refusal([] { DynamicsStep().configure(); });
}

static void test_names()
{
    const char* const stats[NSDG_STAT_COUNT] = { "mean", "ice_mean", "min", "max" };
    for (int s = 0; s < NSDG_STAT_COUNT; ++s)
        CHECK(std::string(nsdg_history_stat_name(s)) == stats[s] && nsdg_history_stat_id(stats[s]) == s);
    const char* const series[NSDG_SERIES_COUNT] = { "area", "extent", "volume", "snow_volume", "drift", "speed_max", "hice_max" };
    for (int q = 0; q < NSDG_SERIES_COUNT; ++q)
        CHECK(std::string(nsdg_history_series_name(q)) == series[q] && nsdg_history_series_id(series[q]) == q);
    CHECK(nsdg_history_stat_name(NSDG_STAT_COUNT) == nullptr && nsdg_history_stat_id("median") == -1 && nsdg_history_stat_id(nullptr) == -1);
    CHECK(nsdg_history_series_name(NSDG_SERIES_COUNT) == nullptr && nsdg_history_series_id("mass") == -1 && nsdg_history_series_id(nullptr) == -1);
    CHECK(nsdg_history_accumulate_stats(nullptr, 0, 0, 1, nullptr, nullptr, nullptr, 1, 0, 0, nullptr, nullptr) == NSDG_ERR_ARG);
    CHECK(nsdg_history_row_totals(nullptr, 0, 0, 1, nullptr, nullptr, 0.15, 0, 0, nullptr) == NSDG_ERR_ARG);
    CHECK(NSDG_HIST_COUNT == 12 && NSDG_HISTORY_MAX_FIELDS == 16 && nsdg_abi_version() == 6);
}

static void test_field_statistics()
{
    const std::string on = std::string(MODEL) + "output_period = 480\noutput_file = ice.nsdg\n";
    CHECK(dyn(on + "output_fields = hice,speed:ice_mean,hice:max\n") == "");
    CHECK(dyn(on + "output_fields = hice, hice:min, hice:max, hice:ice_mean\n") == ""); // one field under several statistics
    CHECK(contains(dyn(on + "output_fields = hice,hice:median\n"), "unknown statistic in \"hice:median\""));
    CHECK(contains(dyn(on + "output_fields = thickness:max\n"), "unknown field \"thickness\""));
    CHECK(contains(dyn(on + "output_fields = hice:max,u,hice:max\n"), "\"hice:max\" is listed twice"));
    CHECK(contains(dyn(on + "output_fields = hice,hice:mean\n"), "listed twice")); // the bare name IS the mean
    CHECK(contains(dyn(on + "output_fields = hice,speed:max\noutput_kind = snapshot\n"), "\"speed:max\" names a statistic of a window"));
    CHECK(contains(dyn(on + "output_fields = hsnow:max\n"), "\"hsnow\" is column state"));
    CHECK(contains(dyn(on + "output_fields = damage:max\n"), "brittle rheology"));
    const HistoryOutput::Config c = (configureWith(on + "output_fields = hice,speed:ice_mean,hice:max\n"), HistoryOutput::fromConfiguration(false));
    CHECK((c.fields == std::vector<std::string> { "hice", "speed:ice_mean", "hice:max" })); // as configured
    CHECK((c.ids == std::vector<int> { NSDG_HIST_HICE, NSDG_HIST_SPEED, NSDG_HIST_HICE }));
    CHECK((c.stats == std::vector<int> { NSDG_STAT_MEAN, NSDG_STAT_ICE_MEAN, NSDG_STAT_MAX }) && c.hasStats() && c.weighted());
    const HistoryOutput::Config plain = (configureWith(on), HistoryOutput::fromConfiguration(false));
    CHECK(!plain.hasStats() && !plain.weighted() && plain.stats == std::vector<int>(4, NSDG_STAT_MEAN));
    const HistoryOutput::Config ext = (configureWith(on + "output_fields = hice:max,u:min\n"), HistoryOutput::fromConfiguration(false));
    CHECK(ext.hasStats() && !ext.weighted());
    Configurator::clear();
}

static void test_finish()
{
    // three samples; planes of four values: mean, ice_mean, min, max
    std::vector<double> acc = { 3, 6, 9, NaN, /**/ 1.5, 0, 2, 4, /**/ -1, -2, -3, NaN, /**/ 7, 8, 9, NaN };
    const std::vector<double> wacc = { 3, 0, 0.5, -0.0 };
    HistoryOutput::finish({ NSDG_STAT_MEAN, NSDG_STAT_ICE_MEAN, NSDG_STAT_MIN, NSDG_STAT_MAX }, 3, 4, wacc.data(), acc);
    CHECK(acc[0] == 1 && acc[1] == 2 && acc[2] == 3 && std::isnan(acc[3]));
    CHECK(acc[4] == 0.5 && std::isnan(acc[5]) && acc[6] == 4 && std::isnan(acc[7])); // NaN exactly where the weights are not positive
    CHECK(acc[8] == -1 && acc[9] == -2 && acc[10] == -3 && std::isnan(acc[11]) && acc[12] == 7 && acc[14] == 9 && std::isnan(acc[15]));
    std::vector<double> plain = { 3, 6 };
    HistoryOutput::finish({ NSDG_STAT_MEAN }, 3, 2, nullptr, plain);
    CHECK(plain[0] == 1 && plain[1] == 2);
}

static void test_dataset_names(const std::string& dir)
{
    CHECK(HistoryOutput::datasetName("hice") == "hice" && HistoryOutput::datasetName("speed:ice_mean") == "speed_ice_mean");
    CHECK(HistoryOutput::datasetName("sigma_n:max") == "sigma_n_max");
    HistoryOutput::Record r;
    r.timeStart = 0, r.timeEnd = 480, r.samples = 4, r.kind = "mean";
    r.fields = { "hice", "speed:ice_mean", "hice:max" };
    r.x = 4, r.y = 3, r.row0 = 0, r.rows = 2;
    for (std::size_t k = 0; k < r.fields.size() * 6; ++k)
        r.data.push_back(k % 5 == 0 ? NaN : 1.0 / 7.0 * (double)k);
    auto same = [](const std::vector<double>& a, const std::vector<double>& b) { // bit for bit, NaN included
        return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin(), [](double x, double y) { return (std::isnan(x) && std::isnan(y)) || x == y; });
    };
    for (const char* name : { "stat.nsdg", "stat.nc" }) {
        const std::string file = dir + "/" + name, path = HistoryOutput::recordPath(file, r.timeEnd);
        HistoryOutput::write(path, file, r);
        const HistoryOutput::Record b = HistoryOutput::read(path);
        CHECK(b.fields == r.fields && b.samples == 4 && same(b.data, r.data));
        if (Hdf5File::isHdf5(path)) {
            const Hdf5File h(path);
            CHECK(h.stringAttribute("/history", "fields") == "hice,speed:ice_mean,hice:max"); // the configured strings
            CHECK((h.dims("/data/speed_ice_mean") == std::vector<std::uint64_t> { 2, 3 }) && (h.dims("/data/hice_max") == std::vector<std::uint64_t> { 2, 3 }));
            CHECK(same(h.readDoubles("/data/hice_max"), std::vector<double>(r.data.begin() + 12, r.data.end())));
            CHECK(same(h.readDoubles("/data/hice"), std::vector<double>(r.data.begin(), r.data.begin() + 6)));
        }
    }
}

static void test_series_keys()
{
    const std::string on = std::string(MODEL) + "series_file = totals.txt\n";
    CHECK(dyn(MODEL) == ""); // off by default
    CHECK(dyn(std::string(MODEL) + "series_fields = nonsense\nseries_buffer = -3\n") == ""); // off: the other keys are not looked at
    CHECK(dyn(on) == "");
    CHECK(dyn(on + "series_fields = area, extent, volume, drift, speed_max, hice_max\nseries_buffer = 1\n") == "");
    CHECK(contains(dyn(on + "series_fields = area,mass\n"), "unknown quantity \"mass\""));
    CHECK(contains(dyn(on + "series_fields = area,volume,area\n"), "\"area\" is listed twice"));
    CHECK(contains(dyn(on + "series_fields = drift,volume\n"), "\"drift\" is the ice-weighted mean speed: it needs \"area\""));
    CHECK(contains(dyn(on + "series_fields = snow_volume\n"), "\"snow_volume\" is column state"));
    CHECK(dyn(on + "series_fields = snow_volume\n[dynamics]\nthermodynamics = true\n") == "");
    CHECK(contains(dyn(on + "series_fields =\n"), "must name 1 to 7 quantities"));
    for (const char* bad : { "0", "-4", "2.5", "many" })
        CHECK(contains(dyn(on + "series_buffer = " + bad + "\n"), "model.series_buffer must be a whole number of model steps"));
    // a multi-process run: there is no gather
    configureWith(on);
    CHECK(contains(refusal([] { SeriesOutput::fromConfiguration(false, 4); }), "no gather"));
    CHECK(refusal([] { SeriesOutput::fromConfiguration(false, 1); }) == "");
    configureWith(MODEL);
    CHECK(refusal([] { SeriesOutput::fromConfiguration(false, 4); }) == ""); // off: nothing to refuse
    setenv("WORLD_SIZE", "2", 1), setenv("RANK", "1", 1);
    CHECK(contains(dyn(on), "model.series_file is set in a run of 2 processes: there is no gather"));
    unsetenv("WORLD_SIZE"), unsetenv("RANK");
    // HipStep writes no series: any of the keys stops it before it asks for a device
    for (const char* key : { "series_file = totals.txt\n", "series_fields = area\n", "series_buffer = 8\n" }) {
        configureWith(std::string(MODEL) + key);
        const std::string why = refusal([] { HipStep().init(); });
        CHECK(contains(why, "Nextsim::HipStep writes no time series") && !contains(why, "other:"));
    }
    const SeriesOutput::Config def = (configureWith(on), SeriesOutput::fromConfiguration(false, 1));
    CHECK((def.names == std::vector<std::string> { "area", "extent", "volume" }) && def.buffer == 256 && def.file == "totals.txt");
    CHECK((def.ids == std::vector<int> { NSDG_SERIES_AREA, NSDG_SERIES_EXTENT, NSDG_SERIES_VOLUME }));
    Configurator::clear();
}

static void test_series_totals()
{
    const std::vector<int> ids = { NSDG_SERIES_VOLUME, NSDG_SERIES_AREA, NSDG_SERIES_DRIFT, NSDG_SERIES_SPEED_MAX, NSDG_SERIES_EXTENT };
    // three rows whose sum remembers its order: (1e16 + 1) + 1 != 1e16 + (1 + 1)
    const std::vector<double> rows = { 1e16, 1, 1, /**/ 0.5, 0.25, 0.25, /**/ 0.1, 0.2, 0.1, /**/ 0.3, 0.7, 0.2, /**/ 2, 3, 4 };
    const std::vector<double> t = SeriesOutput::totals(ids, rows.data(), 3, 100., 50.);
    CHECK(t.size() == 5 && t[0] == ((1e16 + 1.) + 1.) * 5000. && t[0] != (1e16 + (1. + 1.)) * 5000.); // one row after the other
    CHECK(t[1] == 5000. && t[2] == ((0.1 + 0.2) + 0.1) / 1.0 && t[3] == 0.7 && t[4] == 9. * 5000.);
    const std::vector<double> none = { 0, 0, 0, /**/ 0, 0, 0, /**/ 0, 0, 0, /**/ 0.1, NaN, 0.2, /**/ 0, 0, 0 };
    const std::vector<double> z = SeriesOutput::totals(ids, none.data(), 3, 100., 50.);
    CHECK(z[0] == 0 && z[1] == 0 && std::isnan(z[2]) && std::isnan(z[3]) && z[4] == 0); // no ice: no drift; a NaN row keeps the maximum NaN
}

static void test_series_file(const std::string& dir)
{
    CHECK(SeriesOutput::headerLine({ "area", "extent", "volume" }) == "# time area extent volume");
    CHECK(SeriesOutput::formatLine(480, { 1.5, 0.1, NaN }) == "480 1.5 0.10000000000000001 nan");
    CHECK(SeriesOutput::formatLine(-120, {}) == "-120");
    SeriesOutput::Config c;
    c.file = dir + "/totals.txt", c.names = { "area", "drift" }, c.ids = { NSDG_SERIES_AREA, NSDG_SERIES_DRIFT };
    {
        std::ofstream old(c.file);
        old << "what an earlier run left\n";
    }
    const std::vector<std::vector<double>> want = { { 1.0 / 3.0, 5e-324 }, { 1.7976931348623157e308, NaN }, { -0.0, 123456789.125 } };
    SeriesOutput::truncate(c);
    SeriesOutput::append(c, { SeriesOutput::formatLine(120, want[0]) });
    SeriesOutput::append(c, { SeriesOutput::formatLine(240, want[1]), SeriesOutput::formatLine(360, want[2]) });
    std::ifstream f(c.file);
    std::string line;
    CHECK(std::getline(f, line) && line == "# time area drift");
    long time = 0;
    std::vector<double> got;
    CHECK(!SeriesOutput::parseLine(line, time, got) && !SeriesOutput::parseLine("", time, got) && !SeriesOutput::parseLine("12x 1", time, got));
    CHECK(!SeriesOutput::parseLine("12 1.5e", time, got));
    for (std::size_t k = 0; k < want.size(); ++k) { // %.17g reads back bit for bit
        CHECK(std::getline(f, line) && SeriesOutput::parseLine(line, time, got) && time == 120 * (long)(k + 1) && got.size() == 2);
        for (std::size_t i = 0; i < 2 && i < got.size(); ++i)
            CHECK((std::isnan(want[k][i]) && std::isnan(got[i])) || (got[i] == want[k][i] && std::signbit(got[i]) == std::signbit(want[k][i])));
    }
    CHECK(!std::getline(f, line));
    SeriesOutput::Config nowhere = c;
    nowhere.file = dir + "/no/such/directory/totals.txt";
    bool threw = false;
    try {
        SeriesOutput::truncate(nowhere);
    } catch (const std::runtime_error& e) {
        threw = contains(e.what(), "model.series_file: cannot write");
    }
    CHECK(threw);
}

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    test_names();
    test_field_statistics();
    test_finish();
    test_dataset_names(dir);
    test_series_keys();
    test_series_totals();
    test_series_file(dir);
    std::printf("output stats tests: %d checks, %d failures\n", checks, failures);
    return failures;
}

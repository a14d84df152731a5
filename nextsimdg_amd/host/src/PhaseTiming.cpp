#include "PhaseTiming.hpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "Configured.hpp"

namespace Nextsim {

namespace {
struct Keys { }; // (a tag: the keys live under model.*, which belongs to no step class)
const char* const NAMES[] = { "forcing", "column", "prepare", "sub-cycle", "transport", "reduction" };
// the order a model step runs its phases in: the reduction of the sub-stepping rule comes first
const int ORDER[] = { NSDG_PHASE_REDUCTION, NSDG_PHASE_FORCING, NSDG_PHASE_COLUMN, NSDG_PHASE_PREPARE, NSDG_PHASE_SUBCYCLE, NSDG_PHASE_TRANSPORT };

std::vector<int> phaseOrder()
{
    std::vector<int> ids(ORDER, ORDER + sizeof ORDER / sizeof ORDER[0]);
    for (int id = 0; id < NSDG_PHASE_MAX; ++id)
        if (id >= (int)(sizeof NAMES / sizeof NAMES[0]))
            ids.push_back(id);
    return ids;
}

std::string num(double v)
{
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", v);
    return buf;
}

const nsdg_halo_stats* exchangeOf(const PhaseBlockTimes& b, int id)
{
    if (!b.hasExchange)
        return nullptr;
    return id == NSDG_PHASE_SUBCYCLE ? &b.subcycleExchange : id == NSDG_PHASE_TRANSPORT ? &b.transportExchange : nullptr;
}
} // namespace

bool PhaseTiming::enabled() { return Configured<Keys>::getConfiguration(std::string("model.phase_timing"), false); }

std::string PhaseTiming::file() { return Configured<Keys>::getConfiguration(std::string("model.phase_timing_file"), std::string("")); }

const char* PhaseTiming::phaseName(int id)
{
    static thread_local char other[24];
    if (id >= 0 && id < (int)(sizeof NAMES / sizeof NAMES[0]))
        return NAMES[id];
    std::snprintf(other, sizeof other, "phase %d", id);
    return other;
}

void PhaseTiming::toTimer(Timer& timer, const std::vector<Timer::Key>& iteratePath, const std::vector<PhaseBlockTimes>& blocks)
{
    if (blocks.empty())
        return;
    double total = 0.;
    for (const auto& b : blocks)
        total = std::max(total, b.table.total_ms);
    timer.setDeviceTime(iteratePath, 1e-3 * total);
    for (int id : phaseOrder()) {
        const PhaseBlockTimes* slowest = nullptr;
        for (const auto& b : blocks)
            if (b.table.count[id] > 0 && (!slowest || b.table.ms[id] > slowest->table.ms[id]))
                slowest = &b;
        if (!slowest)
            continue;
        const std::string name = phaseName(id);
        timer.setDeviceNode(iteratePath, name, 1e-3 * slowest->table.ms[id], (int)slowest->table.count[id]);
        const nsdg_halo_stats* ex = nullptr;
        for (const auto& b : blocks) {
            const nsdg_halo_stats* e = exchangeOf(b, id);
            if (e && e->exchanges > 0 && (!ex || e->ms > ex->ms))
                ex = e;
        }
        if (ex) {
            std::vector<Timer::Key> path = iteratePath;
            path.push_back(name);
            timer.setDeviceNode(path, "exchange", 1e-3 * ex->ms, (int)ex->exchanges, true);
        }
    }
}

std::string PhaseTiming::json(int rank, int world, long steps, long substeps, const std::vector<PhaseBlockTimes>& blocks)
{
    std::ostringstream os;
    os << "{\"rank\": " << rank << ", \"world\": " << world << ", \"steps\": " << steps << ", \"substeps\": " << substeps << ", \"blocks\": [";
    for (std::size_t k = 0; k < blocks.size(); ++k) {
        const PhaseBlockTimes& b = blocks[k];
        os << (k ? ",\n  " : "\n  ") << "{\"block\": " << b.block << ", \"total_ms\": " << num(b.table.total_ms) << ", \"spans\": " << b.table.spans
           << ", \"phases\": {";
        bool first = true;
        for (int id : phaseOrder()) {
            if (b.table.count[id] <= 0)
                continue;
            os << (first ? "" : ", ") << "\"" << phaseName(id) << "\": {\"ms\": " << num(b.table.ms[id]) << ", \"count\": " << b.table.count[id];
            if (const nsdg_halo_stats* e = exchangeOf(b, id))
                os << ", \"exchange\": {\"overlapped\": true, \"exchanges\": " << e->exchanges << ", \"untimed\": " << e->untimed << ", \"ms\": " << num(e->ms)
                   << ", \"bytes_sent\": " << e->bytes_sent << ", \"bytes_received\": " << e->bytes_received << "}";
            os << "}";
            first = false;
        }
        os << "}}";
    }
    os << "\n]}\n";
    return os.str();
}

void PhaseTiming::write(const std::string& path, int rank, int world, long steps, long substeps, const std::vector<PhaseBlockTimes>& blocks)
{
    const std::string name = world > 1 ? path + ".rank" + std::to_string(rank) : path;
    std::ofstream out(name);
    out << json(rank, world, steps, substeps, blocks);
    if (!out)
        throw std::runtime_error("model.phase_timing_file: cannot write " + name);
}

} // namespace Nextsim

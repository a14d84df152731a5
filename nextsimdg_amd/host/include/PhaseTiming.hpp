// PhaseTiming.hpp -- what the model steps do with the library's per-phase device timing (include/nsdg.h "per-phase device timing"):
// the two configuration keys, and the two outputs of the tables read at the end of a run.
//     model.phase_timing       = true   the step marks its phases on every block's context (nsdg_phase_mark: one event per mark on the
//                                       block's stream, no synchronisation) and the timer tree gains the phases as device-time
//                                       children of `iterate`; works with either value of model.timing and installs no device-sync hook
//     model.phase_timing_file  = PATH   the same numbers as JSON, per block (a process of a multi-process run appends .rank<r>):
//         {"rank": r, "world": w, "steps": model steps, "substeps": sub-steps run,
//          "blocks": [{"block": k, "total_ms": t, "spans": s,
//                      "phases": {"forcing": {"ms": m, "count": c}, ..., "sub-cycle": {"ms": m, "count": c, "exchange": {...}}}}]}
// A phase's `ms` is device time between its mark and the next one, summed over `count` intervals; total_ms is the time from the first
// mark of a model step to its end mark, from that pair of events, summed over `spans` model steps.  `exchange` (under sub-cycle and
// transport, blocks with neighbours only) is the event timing of the ghost exchanges (nsdg_rb_mevp_stats / nsdg_rb_transport_stats): they
// run on the communication stream BESIDE the compute phases, so they are in no sum.
// With several blocks in one process the tree shows, per phase, the LARGEST value over the blocks -- the slowest block sets the pace --
// and the file has every block's table.  Blocks that share one device see each other's work inside their intervals.
#pragma once
#include <string>
#include <vector>

#include "../../../include/nsdg.h"
#include "Timer.hpp"

namespace Nextsim {

struct PhaseBlockTimes {
    int block = 0;
    nsdg_phase_table table {};
    bool hasExchange = false; // the block has neighbours: the two exchange records are valid
    nsdg_halo_stats subcycleExchange {}, transportExchange {};
};

class PhaseTiming {
public:
    static bool enabled(); //!< model.phase_timing
    static std::string file(); //!< model.phase_timing_file ("" = none)
    static const char* phaseName(int id); //!< "forcing", "column", ... ; "phase <id>" beyond the shared ids
    //! the phases as device-time children of the node at `iteratePath`, in id order of their first interval; per phase the largest time
    //! over the blocks (with that block's count), the node's own device time = the largest total
    static void toTimer(Timer& timer, const std::vector<Timer::Key>& iteratePath, const std::vector<PhaseBlockTimes>& blocks);
    static std::string json(int rank, int world, long steps, long substeps, const std::vector<PhaseBlockTimes>& blocks);
    static void write(const std::string& path, int rank, int world, long steps, long substeps, const std::vector<PhaseBlockTimes>& blocks);
};

} // namespace Nextsim

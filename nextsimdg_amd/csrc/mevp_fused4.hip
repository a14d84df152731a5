// mevp_fused4.hip -- the stage-per-wave pipeline of the mEVP sub-cycle: up to FOUR sub-iterations per kernel pass, one pipeline stage
// per wave of a four-wave workgroup, hand-over POINT TO POINT (round 5).  A workgroup marches through a strip of 57 owned columns x
// R rows; wave s performs sub-iteration p + s; the hand-over between two waves -- 24 stress coefficients and u, v at the 4 owned
// nodes per lane -- goes through LDS.  Redundancy instead of synchronisation BETWEEN workgroups: lanes 0-3 / 61-63 recompute the
// columns beside the owned ones, stage s of a pass of n sub-iterations runs on the rows y0 - n + s .. y1 + n - 2 - s.
//
// The round-4 kernel (git history: csrc/mevp_fused4.hip before round 5) synchronised its four stage waves with ONE workgroup barrier per march step.  A barrier is
// a rendez-vous of all four waves, so a link of the pipeline can only be as short as "write, barrier, read": every link was three
// march steps deep, a strip of R rows took R + 16 steps, a row's ice strength and nodal coefficients were in flight for ten steps
// -- re-read from the Infinity Cache by each of the stages 1-3 (3.4 of the 6.7 GB a pass moves, -13.5 % without them) -- and the
// three rotating slots per link filled the LDS (144 of 160 KB).  Here a stage waits for exactly what it needs and nothing else:
//
//   * every link has two counters in LDS.  done[k] = the last row stage k has handed over, read[k] = the last row stage k + 1 has
//     taken.  Stage k + 1 starts row r when done[k] >= r + 1 (it needs the bottom nodes of the row above); stage k writes row r
//     into slot r % 2 when read[k] >= r - 2.  A link is TWO steps deep -- the minimum the scheme allows: the velocity of the top
//     node row of element row r is updated by row r + 1 -- a strip takes R + 13 steps (R + 7 rows of stage 0, six steps of lag),
//     and two slots per link are enough: 96 KB for the three hand-overs.
//   * the freed LDS holds two RINGS of seven rows: the loader (stage 0) reads a row's ice strength (nine Gauss-point values) and
//     packed nodal coefficients from memory once and writes the ice strength and ONE of the three coefficient pairs (u_ocean,
//     v_ocean of the 4 owned nodes) into the rings, the stages 1-3 take them from there: 136 of the 264 bytes per element each of
//     them used to re-read.  The other two pairs (128 B) are still re-read from memory -- a ring for them needs another 2 x 28 KB
//     and the LDS is full: 96 + 31.5 + 28 = 155.5 of 160 KB (profiles/r05_fused4_p2p.md: what fits, what was measured).
//   * no barrier after the prologue: the waves run as far apart as their dependencies allow, idle steps do not exist.
//   * the last stage issues the 12 streaming stores of a row's stress right after the relaxation, under the contributions and node
//     updates that only read those registers (NSDG_P2P_EARLY bit 2, mevp_p2p.h; -1.7 ... -1.9 % per step).  The same move for the
//     hand-over between the stages (bit 1: slot wait and the 12 LDS writes right after the relaxation) is built and off: it asks for
//     the slot before the consumer has freed it and costs 6.9 % (profiles/r15_early_stress_writes.md).
//   * the loader (stage 0) never polls, so it paces every row.  Where it requests its loads and where they land is stated by hand
//     (NSDG_P2P_LAND, mevp_p2p.h; the table above p2p_row): the coefficient pair goes to its ring behind the projected stress, the
//     next row's stress is requested at the very end of the row into the registers the row's own stress has just left (-3.7 ...
//     -3.8 % per step, 68 fewer registers per wave; profiles/r16_loader_landing.md).
//
// Memory ordering of the hand-over, the bounded wait and how a wait that gave up becomes an error status: mevp_p2p.h.  Every wait is
// on an event that is strictly earlier in the dependency graph of the march (row r of stage k + 1 waits for row r + 1 of stage k; row r
// of stage k waits for row r - 2 of stage k + 1, which waited for row r - 1 of stage k), so no wave can wait for ever.
//
// The arithmetic is the same sequence of inlined functions as in every other variant: bit-identical to four passes of variant 1.
//
// THIS FILE IS COMPILED TWICE.  As itself it holds the instantiations without the seabed stress; mevp_fused4_basal.hip includes it with
// NSDG_FUSED4_BASAL_TU defined and holds the BASAL ones (landfast ice), so that this file's own listing keeps the
// four kernels its resource tests and tools/isa_flops.py read.  Two consequences for whoever edits it: (1) every definition here that is
// not a template or inline is defined in BOTH translation units and collides at link time unless it is guarded by
// #ifndef NSDG_FUSED4_BASAL_TU, as the launcher's head and the stamped build's readers are; (2) the stamped diagnostic build
// (NSDG_P2P_SPINSTAT) is undefined in the second translation unit: its counters and phase stamps do NOT cover the BASAL kernels.
#include "mevp_p2p.h"

namespace nsdg_mevp_detail {

#ifdef NSDG_P2P_SPINSTAT
// diagnostic build only (tools/ab_build.sh spin -DNSDG_P2P_SPINSTAT; tools/p2p_spinstat.py): polls per stage and kind of wait -- 0 the
// previous stage's hand-over, 1 a free hand-over slot, 2 a free ring slot -- and the rows the stage worked on in [3]
__device__ unsigned long long nsdg_p2p_spin_dev[4][4];
__device__ unsigned long long nsdg_p2p_phase_dev[4][8]; // shader cycles per stage and phase of a row (s_memtime, fenced)
__device__ unsigned long long nsdg_p2p_land_dev[4]; // shader cycles the loader spent at each of its landing points (s_memtime around the s_waitcnt, no fence)
#define NSDG_SPIN_ARG , unsigned (&spins)[3], unsigned (&phase)[8], unsigned& stamp_last, unsigned (&landc)[4]
#define NSDG_SPIN_PASS , spins, phase, stamp_last, landc
#define NSDG_SPIN_COUNT(k, n) spins[k] += (n)
#if NSDG_P2P_SPINSTAT + 0 == 2 // -DNSDG_P2P_SPINSTAT=2: the polls and the landing points only -- no phase stamps, whose fences change the schedule
#define NSDG_PHASE(k)
#else
#define NSDG_PHASE(k)                                                   \
    do {                                                                \
        __builtin_amdgcn_sched_barrier(0);                              \
        const unsigned now_ = (unsigned)__builtin_amdgcn_s_memtime();   \
        phase[k] += now_ - stamp_last;                                  \
        stamp_last = now_;                                              \
        __builtin_amdgcn_sched_barrier(0);                              \
    } while (0)
#endif
// a landing point between two s_memtime: what is added to landc[k] is the stall at its s_waitcnt plus the two stamps' own ~12 cycles
#define NSDG_LAND_TIMED(k, ...)                                                     \
    do {                                                                            \
        const unsigned land0_ = (unsigned)__builtin_amdgcn_s_memtime();             \
        __VA_ARGS__;                                                                \
        landc[k] += (unsigned)__builtin_amdgcn_s_memtime() - land0_;                \
    } while (0)
#else
#define NSDG_PHASE(k)
#define NSDG_SPIN_ARG
#define NSDG_SPIN_PASS
#define NSDG_SPIN_COUNT(k, n) (void)(n) /* the wait itself is the argument: it must stay */
#define NSDG_LAND_TIMED(k, ...) __VA_ARGS__
#endif
// the stamped build with the switch at 0 has no landing point of its own to time: it waits, timed, where and for as many loads as the
// compiler does in the product (the three s_waitcnt vmcnt of the loader's loop, table above p2p_row)
#if defined(NSDG_P2P_SPINSTAT) && NSDG_P2P_LAND == 0
#define NSDG_LAND_PROBE(k, n) NSDG_LAND_TIMED(k, p2p_wait_vm<n>())
#else
#define NSDG_LAND_PROBE(k, n)
#endif

constexpr int P4_OWNED = 57, P4_LEFT = 4; // lanes 4 .. 60 own a column (four sub-iterations reach four columns / rows)
constexpr int P4_HAND = 32; // doubles per lane and hand-over slot: 24 stress coefficients + u, v at the 4 owned nodes
constexpr int P4_SLOT = P4_HAND * 64; // value k of lane l at (k / 2) * 128 + 2 l + k % 2 (16-byte pairs)
constexpr int P4_HSLOTS = 2; // slots per link
constexpr int P4_PRING = 7; // rows in each of the two rings (a row is in flight for ~5.7 march steps; 7 x (4.6 + 4) KB is what fits)
constexpr int P4_PSLOT = P2P_PSLOT; // ice strength (mevp_p2p.h)
constexpr int P4_CSLOT = 8 * 64; // third pair of the nodal coefficients (u_ocean, v_ocean): node n of lane l at n * 128 + 2 l
constexpr int P4_LDS = 3 * P4_HSLOTS * P4_SLOT + P4_PRING * (P4_PSLOT + P4_CSLOT); // doubles: 96 + 31.5 + 28 KB of the 160 KB of a CU

struct Fetch {
    double P[9]; // ice strength at the Gauss points of the row the stage works on next
    double c[4][6]; // packed momentum coefficients of its 4 owned nodes
    double tb[4]; // BASAL only: their seventh coefficient, the critical stress T_b of the seabed stress (mevp_common.h: node_update)
    double s11[8], s12[8], s22[8]; // stage 0 only: the stress the pass starts from
    double ub[3], vb[3], um[3], vm[3], ut[3], vt[3]; // stage 0 only: u, v of the pass's start on the three node rows
};

struct Stage {
    int s; // pipeline stage of this wave = sub-iteration p + s
    int nst; // stages of this pass = its sub-iterations (4; 3 or 2 for what is left of a sub-cycle whose length is no multiple of 4)
    int first, last; // element rows this stage works on
    int last_prev; // last row of the previous stage
    int last_final; // last row of the last stage (the loader's ring wait)
    int upd0; // node updates from this row on
};

// counters: done[k] at k, read[k] at 3 + k, the sticky give-up flag at 6
struct Flags {
    int v[8];
};

__device__ __forceinline__ int ring_slot(int row) { return row % P4_PRING; } // row >= 0
// the third pair (u_ocean, v_ocean) of the 4 owned nodes of a row from / to its ring
__device__ __forceinline__ void ring_read_c(const double* __restrict__ cring, int row, int lane, double (&c)[4][6])
{
    const double* s = cring + ring_slot(row) * P4_CSLOT + 2 * lane;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const double2 t = *reinterpret_cast<const double2*>(s + n * 128);
        c[n][4] = t.x, c[n][5] = t.y;
    }
}
__device__ __forceinline__ void ring_write_c(double* __restrict__ cring, int row, int lane, const double (&c)[4][6])
{
    double* s = cring + ring_slot(row) * P4_CSLOT + 2 * lane;
#pragma unroll
    for (int n = 0; n < 4; ++n)
        *reinterpret_cast<double2*>(s + n * 128) = make_double2(c[n][4], c[n][5]);
}
// the first two pairs of the nodal coefficients from memory (the third comes from the ring)
__device__ __forceinline__ void load_nodal2(const double* __restrict__ packed, long plane, long n, double (&c)[6])
{
    const double* p = packed + nodal_off(n);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double2 t = *reinterpret_cast<const double2*>(p + k * plane);
        c[2 * k] = t.x, c[2 * k + 1] = t.y;
    }
}
__device__ __forceinline__ void load_owned_nodal2(const MarchConst& M, int nrow, double (&c)[4][6], const double* __restrict__ packed)
{
    const long nVn = (long)(2 * nrow) * M.nn + 2 * M.ix;
    load_nodal2(packed, M.nplane, nVn, c[0]);
    load_nodal2(packed, M.nplane, nVn + 1, c[1]);
    load_nodal2(packed, M.nplane, nVn + M.nn, c[2]);
    load_nodal2(packed, M.nplane, nVn + M.nn + 1, c[3]);
}
// the 24 stress coefficients of a row into its hand-over slot (pairs 0 .. 11) / to memory (the last stage)
__device__ __forceinline__ void hand_stress(double* out, const double (&s11)[8], const double (&s12)[8], const double (&s22)[8])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lds_pair(out, k, s11[2 * k], s11[2 * k + 1]);
        lds_pair(out, 4 + k, s12[2 * k], s12[2 * k + 1]);
        lds_pair(out, 8 + k, s22[2 * k], s22[2 * k + 1]);
    }
}
__device__ __forceinline__ void store_stress(const StressPtrs& S, long ts, const double (&s11)[8], const double (&s12)[8], const double (&s22)[8])
{
    tile_store8_nt<(NSDG_P2P_NT & 2) != 0>(S.o11, ts, s11);
    tile_store8_nt<(NSDG_P2P_NT & 2) != 0>(S.o12, ts, s12);
    tile_store8_nt<(NSDG_P2P_NT & 2) != 0>(S.o22, ts, s22);
}
// The loader's loads and where they land (NSDG_P2P_LAND, mevp_p2p.h).  During row r the loader requests the inputs of row r + 1 in four
// groups; vmcnt counts a wave's loads in the order of their issue, so a landing point is "at most N loads younger than the group":
//
//   group  loads                                   issued in row r                                      consumed in row r + 1
//   A   5  ice strength P (4 x 16 B, 1 x 8 B)      ring block, after the ring write of P(r)             projected stress
//   B   8  u, v, two node rows (4 x (16 + 8 B))    ring block, after A                                  projected stress
//   C  12  stress (3 x 4 x 16 B)                   after the relaxation | bit 2: behind the hand-over   relaxation
//   D  12  nodal coefficients (4 x 3 x 16 B)       request_c, after the node updates                    ring write of the pair, node updates
//      +4  BASAL: the fourth pair (4 x 16 B), issued behind the twelve: the group is 16 loads           node updates
//
// Bit 2 requests C at the very end of the row, behind the hand-over of the row's own stress: the working registers are dead there, the
// request can take them and the compiler has no copy to make (requested anywhere earlier the new stress needs a second register set,
// and the copies between the two sets at the end of the row are what the compiler's waits stand in front of).  The lead of C shrinks
// from a row to the top of the next row plus its projected stress.
//
//   issue order over the rows:   ... A B C D | A' B' C' D' ...        bit 2:   ... A B D C | A' B' D' C' ...
//
//   landing point                                     lands    younger loads in flight                        N
//   L1  ring write of the pair (bit 1), behind the    D        A' B'                                         13
//         projected stress                                     bit 2: C A' B'                                25
//   the stress copy (bit 2: in front of the relaxation) and every other use: the compiler's own waits, which with bit 2 are 28 at the
//   top of the row (A and 4 of B; the rest of B lands in the ring block) and 24 ... 13 in front of the relaxation (C, behind A' B')
//
// With the switch at 0 the compiler waits three times per row (adaptive form: vmcnt(12) at the top -- A, B and C; vmcnt(5) in the ring
// block behind the issue of A' -- C, D; vmcnt(4) before request_c -- A', B' and 8 of the 12 loads of C', whose destination it copies
// out of the accumulation registers there); the stamped build times those three (NSDG_LAND_PROBE).  With a bit set the prologue of the
// march lets all its loads land before the first row, so the loop's waits are those of its own requests; in the last row of a stage
// nrow == row and the same loads are issued once more.
//
// BASAL (the fourth pair, landfast ice): every stage reads it from memory in request_c, beside the pairs it reads there anyway; there is no
// ring for it (the LDS is full).  In the loader the four loads join group D, so every count of the table stands: L1 counts the loads
// YOUNGER than D (C A' B' = 25, or A' B' = 13), and D growing from 12 to 16 loads does not change what is younger than it; the prologue's
// p2p_land<0> waits for everything whatever was requested.  T_b is consumed at the node updates, behind L1 and behind the relaxation's
// wait for C, and vmcnt retires loads in order: the fourth pair, older than C, has landed there and the compiler's own wait costs nothing.
// The counts of the stamped build's probes (12 at the top, P4_NA in the ring block, 4 before request_c) restate the compiler's waits of
// the switch-at-0 build without a depth array and are not launched with one.  The stages 1-3 have no hand-placed count.
constexpr int P4_NA = 5, P4_NB = 8, P4_NC = 12;
constexpr bool P4_LAND_COEFF = (NSDG_P2P_LAND & 1) != 0, P4_LAND_ORDER = (NSDG_P2P_LAND & 2) != 0;
constexpr int P4_L1 = P4_LAND_ORDER ? P4_NC + P4_NA + P4_NB : P4_NA + P4_NB;
// the loader's stress request (group C)
__device__ __forceinline__ void request_stress(const StressPtrs& S, long ts, Fetch& f)
{
    tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i11, ts, f.s11);
    tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i12, ts, f.s12);
    tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i22, ts, f.s22);
}
// One row of one stage.  FIRST: the loader (stage 0): inputs from memory, ice strength into the ring.
template <bool FIRST, bool AD, bool LAND, bool BASAL>
__device__ __forceinline__ void p2p_row(const MarchConst& M, const Stage& G, int row, Fetch& f, TopCarry& carry, double* __restrict__ lds,
    volatile lds_int* flags, const P2PReport& rep, const StressPtrs& S, const double* __restrict__ u_old, const double* __restrict__ v_old,
    const double* __restrict__ packed, const double* __restrict__ pg, double* __restrict__ u_new, double* __restrict__ v_new NSDG_SPIN_ARG)
{
    const int stage = FIRST ? 0 : G.s;
    const int nrow = min(row + 1, G.last); // the row this stage works on next: its inputs are requested during this one
    const int ix = M.ix, nn = M.nn;
    double* const ring = lds + 3 * P4_HSLOTS * P4_SLOT;
    double* const cring = ring + P4_PRING * P4_PSLOT;
    // the coefficients of row r: a stage >= 1 takes two pairs from memory and the third from the ring; BASAL: every stage takes the
    // fourth from memory
    auto request_c = [&](int r) {
        if (FIRST)
            load_owned_nodal(M, r, f.c, packed);
        else
            load_owned_nodal2(M, r, f.c, packed);
        if constexpr (BASAL)
            load_owned_nodal_tb(M, r, f.tb, packed);
        if (!FIRST)
            ring_read_c(cring, r, M.lane, f.c);
    };
    const long nVn = (long)(2 * nrow) * nn + 2 * ix; // vertex node of the next row
    double s11[8], s12[8], s22[8], uu[4], vv[4], ul[9], vl[9], un[4], vn[4];
    // ------------------------------------------------------------------------------------------ inputs of the row
    if (FIRST) {
        NSDG_LAND_PROBE(0, 12);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            ul[a] = f.ub[a], ul[3 + a] = f.um[a], ul[6 + a] = f.ut[a];
            vl[a] = f.vb[a], vl[3 + a] = f.vm[a], vl[6 + a] = f.vt[a];
        }
        uu[0] = ul[0], uu[1] = ul[1], uu[2] = ul[3], uu[3] = ul[4];
        vv[0] = vl[0], vv[1] = vl[1], vv[2] = vl[3], vv[3] = vl[4];
    } else {
        // the previous stage has handed over this row and the row above it (whose bottom nodes are this row's top nodes)
        NSDG_SPIN_COUNT(0, flag_wait(flags, stage - 1, min(row + 1, G.last_prev), rep));
        if (row == G.first) { // wave-uniform: the first row of the stage has no predecessor that requested its inputs
            ring_read_P<P4_PRING>(ring, row, M.lane, f.P);
            request_c(row);
        }
        const double* in = lds + ((stage - 1) * P4_HSLOTS + (row & 1)) * P4_SLOT + 2 * M.lane;
        const double* top = lds + ((stage - 1) * P4_HSLOTS + ((row + 1) & 1)) * P4_SLOT + 2 * M.lane;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double2 a = lds_pair(in, 12 + k), b = lds_pair(in, 14 + k);
            uu[2 * k] = a.x, uu[2 * k + 1] = a.y, vv[2 * k] = b.x, vv[2 * k + 1] = b.y;
        }
        double2 tu = lds_pair(top, 12), tv = lds_pair(top, 14);
        if (row + 1 > G.last_prev) // wave-uniform: node row 2*ny is the top boundary
            tu = tv = make_double2(0., 0.);
        gather_nodes(M, uu, tu.x, tu.y, ul);
        gather_nodes(M, vv, tv.x, tv.y, vl);
    }
    NSDG_PHASE(0); // inputs of the row (stages >= 1: the wait for the previous stage, LDS reads)
    // ------------------------------------------------------------------------------------------ stress update
    double r11[8], r12[8], r22[8];
    double qe = 0., ialpha = M.ialpha; // adaptive form: this element's offer q_e = alpha_e h'_c and 1 / alpha_e of this sub-iteration (the centre node's h' is coefficient [0] of node 3)
    if constexpr (AD)
        stress_projected_adaptive(ul, vl, f.P, M.ihx, M.ihy, M.dmin2, f.c[3][0], M.AC, r11, r12, r22, qe, ialpha);
    else
        stress_projected(ul, vl, f.P, M.ihx, M.ihy, M.ialpha, M.dmin2, r11, r12, r22);
    __builtin_amdgcn_sched_barrier(0);
    NSDG_PHASE(1); // projected stress
    if (FIRST) {
        // the ice strength of this row goes to the ring for the stages 1-3 (slot of row - 8: stage 3 has passed it), then the
        // register set takes the next row's; u, v of the next row
        NSDG_SPIN_COUNT(2, flag_wait(flags, 3 + G.nst - 2, min(row - P4_PRING, G.last_final), rep)); // read[] of the LAST link: the last stage has passed that row
        ring_write_P<P4_PRING>(ring, row, M.lane, f.P);
#if defined(NSDG_P2P_SPINSTAT) && NSDG_P2P_LAND == 0
        // the product's compiled order: the requests of P issue above the wait for the coefficients
        tile_load9_nt<(NSDG_P2P_NT & 4) != 0>(pg, tile_off(ix, nrow, M.ntx, 9), ix & 63, f.P);
        NSDG_LAND_PROBE(1, P4_NA);
        ring_write_c(cring, row, M.lane, f.c);
#else
        if constexpr (!P4_LAND_COEFF)
            ring_write_c(cring, row, M.lane, f.c); // this row's coefficients were requested a step ago; the stages 1-3 take the pair from here
        tile_load9_nt<(NSDG_P2P_NT & 4) != 0>(pg, tile_off(ix, nrow, M.ntx, 9), ix & 63, f.P);
#endif
        if (nrow > row) { // wave-uniform: the top node row of this element row is the bottom one of the next
#pragma unroll
            for (int a = 0; a < 3; ++a)
                f.ub[a] = f.ut[a], f.vb[a] = f.vt[a];
        }
        fetch_nodes(u_old, nVn + nn, f.um);
        fetch_nodes(v_old, nVn + nn, f.vm);
        fetch_nodes(u_old, nVn + 2 * nn, f.ut);
        fetch_nodes(v_old, nVn + 2 * nn, f.vt);
        if constexpr (!P4_LAND_ORDER) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                s11[i] = f.s11[i], s12[i] = f.s12[i], s22[i] = f.s22[i];
        }
    } else {
        ring_read_P<P4_PRING>(ring, nrow, M.lane, f.P); // written by the loader before it handed row nrow over: done[stage - 1] >= row + 1 implies done[0] >= nrow
        const double* in = lds + ((stage - 1) * P4_HSLOTS + (row & 1)) * P4_SLOT + 2 * M.lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double2 a = lds_pair(in, k), b = lds_pair(in, 4 + k), c = lds_pair(in, 8 + k);
            s11[2 * k] = a.x, s11[2 * k + 1] = a.y, s12[2 * k] = b.x, s12[2 * k + 1] = b.y, s22[2 * k] = c.x, s22[2 * k + 1] = c.y;
        }
        // this row's slot (stress, u, v) and the next row's ice strength have been taken: the producer may write row + 2 into the slot
        flag_publish(flags, 3 + stage - 1, row);
    }
    NSDG_PHASE(2); // loader: ring wait, ring writes, requests of P, u, v; stages: ring read, stress read, read[] published
    if constexpr (FIRST && P4_LAND_COEFF) {
        // L1: the projected stress is complete (its registers are named, so the arithmetic stays above), then this row's coefficients
        // land and the pair goes to the ring -- its slot is free since the ring wait above
        p2p_name(r11), p2p_name(r12), p2p_name(r22);
        NSDG_LAND_TIMED(1, p2p_land<P4_L1>(f.c));
        ring_write_c(cring, row, M.lane, f.c);
    }
    if constexpr (FIRST && P4_LAND_ORDER) { // the stress copy, in front of the relaxation that consumes it: its request is the youngest but A', B'
#pragma unroll
        for (int i = 0; i < 8; ++i)
            s11[i] = f.s11[i], s12[i] = f.s12[i], s22[i] = f.s22[i];
    }
    stress_relax(ialpha, r11, r12, r22, s11, s12, s22); // AD: alpha_e of this element; else ialpha = M.ialpha
    __builtin_amdgcn_sched_barrier(0);
    if (FIRST && !P4_LAND_ORDER) { // stress of the next row
        const long ts = tile_off(ix, nrow, M.ntx, 8);
        tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i11, ts, f.s11);
        tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i12, ts, f.s12);
        tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i22, ts, f.s22);
    }
    // the 24 stress coefficients are final here: with NSDG_P2P_EARLY (mevp_p2p.h) they leave now, under the node arithmetic below
    constexpr bool EARLY_HAND = (NSDG_P2P_EARLY & 1) != 0, EARLY_STORE = (NSDG_P2P_EARLY & 2) != 0;
    if constexpr (EARLY_HAND) {
        if (FIRST || stage < G.nst - 1) { // the same condition as at the end of the row (read[stage] >= row - 2), tested earlier
            NSDG_SPIN_COUNT(1, flag_wait(flags, 3 + stage, row - P4_HSLOTS, rep));
            hand_stress(lds + (stage * P4_HSLOTS + (row & 1)) * P4_SLOT + 2 * M.lane, s11, s12, s22);
        }
    }
    if constexpr (EARLY_STORE) {
        if (!(FIRST || stage < G.nst - 1) && M.own && row >= M.y0)
            store_stress(S, tile_off(ix, row, M.ntx, 8), s11, s12, s22);
    }
    NSDG_PHASE(3); // relaxation, (loader) stress request; NSDG_P2P_EARLY: slot wait and stress hand-over (bit 1), stress stores (bit 2)
    // ------------------------------------------------------------------------------------------ contributions, node updates
    {
        double cx[9], cy[9];
        node_contrib_all(s11, s12, s22, M.hx, M.hy, cx, cy);
        owned_node_updates<AD, LAND, BASAL>(M, row > 0, f.c, uu, vv, carry, cx, cy, un, vn, qe, f.tb);
        if (row < G.upd0) { // wave-uniform: the first row of a stage only feeds the carried contributions
#pragma unroll
            for (int k = 0; k < 4; ++k)
                un[k] = vn[k] = 0.;
        }
        carry_top<AD>(carry, cx, cy, qe);
    }
    __builtin_amdgcn_sched_barrier(0);
    NSDG_PHASE(4); // contributions, node updates (the wait for the nodal coefficients is here)
    if (FIRST) {
        NSDG_LAND_PROBE(3, 4);
    }
    request_c(nrow); // nodal coefficients of the next row
    NSDG_PHASE(5); // request of the coefficients
    // ------------------------------------------------------------------------------------------ outputs
    if (FIRST || stage < G.nst - 1) {
        if constexpr (!EARLY_HAND)
            NSDG_SPIN_COUNT(1, flag_wait(flags, 3 + stage, row - P4_HSLOTS, rep)); // the consumer has taken the row this slot held
        double* out = lds + (stage * P4_HSLOTS + (row & 1)) * P4_SLOT + 2 * M.lane;
        if constexpr (!EARLY_HAND)
            hand_stress(out, s11, s12, s22);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            lds_pair(out, 12 + k, un[2 * k], un[2 * k + 1]);
            lds_pair(out, 14 + k, vn[2 * k], vn[2 * k + 1]);
        }
        flag_publish(flags, stage, row); // its lgkmcnt(0) covers the early writes of the row too
        if constexpr (FIRST && P4_LAND_ORDER) // the stress of the next row: this row's has left, the request may take its registers
            request_stress(S, tile_off(ix, nrow, M.ntx, 8), f);
    } else if (M.own && row >= M.y0) { // the last stage runs on rows y0-1 .. y1-1
        const long ts = tile_off(ix, row, M.ntx, 8);
        const long nV = (long)(2 * row) * nn + 2 * ix;
        if constexpr (!EARLY_STORE)
            store_stress(S, ts, s11, s12, s22);
        store_owned_nodes(nV, nn, M.lastcol, row == M.ny - 1, un, vn, u_new, v_new);
    }
    NSDG_PHASE(6); // outputs: slot wait, LDS writes, done[] published / global stores (what NSDG_P2P_EARLY has not moved to phase 3)
}

// LAND: the instantiation that holds land nodes at 0 (mevp_common.h: node_update), launched after a packing that saw a land mask
// BASAL: the instantiation with the seabed stress (mevp_common.h: node_update), launched after a packing that saw a depth array
template <bool AD, bool LAND, bool BASAL>
__global__ __launch_bounds__(256) void mevp_fused4_kernel(NodalConstsOf<BASAL> K, AdaptConsts AC, int nst, int nx, int ny, int j0, int j1, int j0b, int j1b, int nsA, int R, int ncw,
    double hx, double hy, double ialpha, double dmin2, P2PReport rep, StressPtrs S, const double* __restrict__ u_old, const double* __restrict__ v_old,
    const double* __restrict__ packed, const double* __restrict__ pg, double* __restrict__ u_new, double* __restrict__ v_new)
{
    __shared__ __attribute__((aligned(16))) double lds[P4_LDS]; // 96 KB of hand-over slots + 31.5 + 28 KB of rings (ice strength, one coefficient pair)
    __shared__ Flags flagmem;
    volatile lds_int* flags = (volatile lds_int*)flagmem.v;
    const int lane = threadIdx.x & 63;
    const int group = xcd_contiguous_block(blockIdx.x, gridDim.x);
    int strip = group / ncw;
    const int cw = group - strip * ncw;
    if (strip >= nsA) { // workgroup-uniform: a strip of the second range
        strip -= nsA;
        j0 = j0b, j1 = j1b;
    }
    MarchConst M;
    M.y0 = j0 + strip * R;
    if (M.y0 >= j1)
        return; // workgroup-uniform: no wave of this workgroup reaches the barrier or a counter
    M.y1 = min(M.y0 + R, j1);
    march_frame<P4_OWNED, P4_LEFT>(M, K, AC, nx, ny, lane, cw, hx, hy, ialpha, dmin2, nodal_u0<BASAL>(K));

    // a pass of nst sub-iterations (2 <= nst <= 4): stage s works on the rows y0 - nst + s .. y1 + nst - 2 - s, the last one (nst - 1)
    // on y0 - 1 .. y1 - 1; the waves s >= nst have nothing to do
    Stage G;
    G.s = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    G.nst = nst;
    auto first_of = [&](int s) { return max(M.y0 - nst + s, 0); };
    auto last_of = [&](int s) { return min(M.y1 + nst - 2 - s, ny - 1); };
    G.first = first_of(G.s);
    G.last = last_of(G.s);
    G.last_prev = last_of(G.s - 1);
    G.last_final = last_of(nst - 1);
    G.upd0 = G.s == 0 ? 0 : M.y0 - (nst - 1) + G.s;

    // counters: done[k] = first row of stage k - 1 (nothing handed over yet), read[k] = first row of stage k + 1 - 1 (every row
    // below the consumer's first one counts as taken: the consumer never looks at it)
    if (threadIdx.x < 3) {
        flags[threadIdx.x] = first_of(threadIdx.x) - 1;
        flags[3 + threadIdx.x] = first_of(threadIdx.x + 1) - 1;
    }
    if (threadIdx.x == P2P_GIVEUP)
        flags[P2P_GIVEUP] = 0;
    __syncthreads(); // the only barrier of the kernel
    if (G.s >= nst)
        return; // wave-uniform

    Fetch f;
    TopCarry carry; // zero by its member initialisers: the first row of a stage adds nothing from a row below
#ifdef NSDG_P2P_SPINSTAT
    unsigned spins[3] = { 0, 0, 0 }, phase[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    unsigned stamp_last = (unsigned)__builtin_amdgcn_s_memtime();
    unsigned landc[4] = { 0, 0, 0, 0 };
#endif
    if (G.s == 0) {
        const int row = G.first;
        const long nV = (long)(2 * row) * M.nn + 2 * M.ix, ts = tile_off(M.ix, row, M.ntx, 8);
        fetch_nodes(u_old, nV, f.ub);
        fetch_nodes(v_old, nV, f.vb);
        fetch_nodes(u_old, nV + M.nn, f.um);
        fetch_nodes(v_old, nV + M.nn, f.vm);
        fetch_nodes(u_old, nV + 2 * M.nn, f.ut);
        fetch_nodes(v_old, nV + 2 * M.nn, f.vt);
        tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i11, ts, f.s11);
        tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i12, ts, f.s12);
        tile_load8_nt<(NSDG_P2P_NT & 1) != 0>(S.i22, ts, f.s22);
        tile_load9_nt<(NSDG_P2P_NT & 4) != 0>(pg, tile_off(M.ix, row, M.ntx, 9), M.ix & 63, f.P);
        load_owned_nodal(M, row, f.c, packed);
        if constexpr (BASAL)
            load_owned_nodal_tb(M, row, f.tb, packed);
        if constexpr (NSDG_P2P_LAND != 0) {
            // everything the prologue requested lands here, once per strip: a load still in flight at the head of the loop is one
            // the compiler has to assume in flight in every row, and it waits for it wherever a later row reuses the register
            p2p_land<0>(f.P, f.ub, f.vb, f.um, f.vm, f.ut, f.vt, f.s11, f.s12, f.s22, f.c);
#pragma unroll
            for (int n = 0; n < 4; ++n)
                p2p_name(f.c[n][0], f.c[n][1], f.c[n][2], f.c[n][3]);
        }
        for (int row = G.first; row <= G.last; ++row)
            p2p_row<true, AD, LAND, BASAL>(M, G, row, f, carry, lds, flags, rep, S, u_old, v_old, packed, pg, u_new, v_new NSDG_SPIN_PASS);
    } else {
        for (int row = G.first; row <= G.last; ++row)
            p2p_row<false, AD, LAND, BASAL>(M, G, row, f, carry, lds, flags, rep, S, u_old, v_old, packed, pg, u_new, v_new NSDG_SPIN_PASS);
    }
#ifdef NSDG_P2P_SPINSTAT
    if (lane == 0) {
        for (int k = 0; k < 3; ++k)
            atomicAdd(&nsdg_p2p_spin_dev[G.s][k], (unsigned long long)spins[k]);
        atomicAdd(&nsdg_p2p_spin_dev[G.s][3], (unsigned long long)(G.last - G.first + 1));
        for (int k = 0; k < 8; ++k)
            atomicAdd(&nsdg_p2p_phase_dev[G.s][k], (unsigned long long)phase[k]);
        if (G.s == 0)
            for (int k = 0; k < 4; ++k)
                atomicAdd(&nsdg_p2p_land_dev[k], (unsigned long long)landc[k]);
    }
#endif
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

#ifdef NSDG_P2P_SPINSTAT
extern "C" int nsdg_debug_p2p_spinstat(unsigned long long* out48) // [16] polls, then [32] phase cycles
{
    static const unsigned long long zero[32] = { 0 };
    hipError_t e = hipMemcpyFromSymbol(out48, HIP_SYMBOL(nsdg_p2p_spin_dev), 16 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemcpyFromSymbol(out48 + 16, HIP_SYMBOL(nsdg_p2p_phase_dev), 32 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemcpyToSymbol(HIP_SYMBOL(nsdg_p2p_spin_dev), zero, 16 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemcpyToSymbol(HIP_SYMBOL(nsdg_p2p_phase_dev), zero, 32 * sizeof(unsigned long long));
    return (int)e;
}
extern "C" int nsdg_debug_p2p_landstat(unsigned long long* out4) // cycles at the loader's landing points: [1] L1; switch at 0: [0] the top of the row, [1] the ring write of the pair, [3] before request_c
{
    static const unsigned long long zero[4] = { 0 };
    hipError_t e = hipMemcpyFromSymbol(out4, HIP_SYMBOL(nsdg_p2p_land_dev), 4 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemcpyToSymbol(HIP_SYMBOL(nsdg_p2p_land_dev), zero, 4 * sizeof(unsigned long long));
    return (int)e;
}
#endif

// The launcher.  This file is compiled twice: as itself, with the instantiations without the seabed stress -- the kernels of a context
// without a depth array, the ones its resource tests and tools/isa_flops.py list --, and through mevp_fused4_basal.hip, which defines
// NSDG_FUSED4_BASAL_TU and holds the BASAL instantiations behind nsdg_launch_mevp_fused4_basal_ranges.
#ifdef NSDG_FUSED4_BASAL_TU
int nsdg_launch_mevp_fused4_basal_ranges(nsdg_ctx* ctx, bool land, int nst, int j0, int j1, int j0b, int j1b, const nsdg_mevp_bufs& b)
{
    constexpr bool BASAL = true;
#else
int nsdg_launch_mevp_fused4_ranges(nsdg_ctx* ctx, bool land, bool basal, int nst, int j0, int j1, int j0b, int j1b, const nsdg_mevp_bufs& b)
{
    constexpr bool BASAL = false;
    if (basal)
        return nsdg_launch_mevp_fused4_basal_ranges(ctx, land, nst, j0, j1, j0b, j1b, b);
#endif
    const int ncw = nsdg_div_up(ctx->nx, P4_OWNED);
    const int rowsB = j0b < j1b ? j1b - j0b : 0;
    int R = ctx->strip_rows;
    if (R <= 0) {
        // a strip of R rows takes about R + 4 nst - 3 march steps (R + 2 nst - 1 rows of stage 0, 2 (nst - 1) steps of lag: R + 13 for
        // four sub-iterations); one resident workgroup per CU (LDS)
        const double extra = 4. * nst - 3.;
        const long slots = ctx->num_cus;
        double best = 1e30;
        R = 64;
        for (int r = 1; r <= 4096; ++r) {
            const long groups = ((long)nsdg_div_up(j1 - j0, r) + nsdg_div_up(rowsB, r)) * ncw;
            const long rounds = (groups + slots - 1) / slots;
            const double cost = rounds * (r + extra);
            if (cost < best) {
                best = cost;
                R = r;
            }
            if (groups <= ncw * (rowsB ? 2 : 1))
                break; // one strip per range: taller strips change nothing
        }
    }
    const int nsA = nsdg_div_up(j1 - j0, R), nsB = nsdg_div_up(rowsB, R);
    const long ngroups = (long)ncw * (nsA + nsB);
    const StressPtrs S = { b.s11i, b.s12i, b.s22i, b.s11, b.s12, b.s22 };
    const NodalConstsBasal K = nsdg_nodal_consts_basal(ctx);
    const AdaptConsts AC = nsdg_adapt_consts(ctx);
    const P2PReport rep = { ctx->p2p_count_dev, ctx->p2p_flag_dev };
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ngroups), dim3(256), 0, ctx->stream, K, AC, nst, ctx->nx, ctx->ny, j0, j1, j0b, j1b, nsA, R, ncw, ctx->hx, ctx->hy,
            1. / ctx->mevp.alpha, ctx->mevp.delta_min * ctx->mevp.delta_min, rep, S, b.u_old, b.v_old, b.packed, b.pg, b.u_new, b.v_new);
    };
    // adaptive: local, solution-adaptive alpha and beta (mevp_common.h); land: the packing flagged land nodes; BASAL: it stored T_b from a
    // depth array (nsdg_mevp_pass)
    if (!land)
        nsdg_adaptive(ctx) ? launch(mevp_fused4_kernel<true, false, BASAL>) : launch(mevp_fused4_kernel<false, false, BASAL>);
    else
        nsdg_adaptive(ctx) ? launch(mevp_fused4_kernel<true, true, BASAL>) : launch(mevp_fused4_kernel<false, true, BASAL>);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

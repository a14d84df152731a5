// mevp_p2p.h -- what the stage-per-wave pipeline of the mEVP sub-cycle (mevp_fused4.hip) adds to the shared march (mevp_pipeline.h): the
// point-to-point hand-over between the waves of a workgroup -- counters in LDS, a bounded wait, the report of a wait that gave up --,
// the 16-byte pairs of a hand-over slot, the ring of a row's ice strength in LDS, and the streaming (non-temporal) accesses to the
// data a pass touches once.
//
// Memory ordering.  All hand-over traffic is LDS traffic of ONE compute unit; the LDS executes the instructions of a wave in order.
// A producer waits for its own LDS writes (s_waitcnt lgkmcnt(0)) before it raises its counter; a consumer reads the counter,
// waits for that read, and only then issues its reads of the slot -- the pattern of an LDS-scope release / acquire, written out
// with compiler barriers around it.  Counters only ever increase.
//
// A wait that gives up (NSDG_P2P_SPIN_LIMIT polls: never in a correct program) raises the workgroup's sticky flag, which releases
// every other wait of the workgroup, counts the event in the context's device counter and sets the context's flag in HOST memory:
// the next nsdg_ctx_synchronize / nsdg_mevp_subcycle / nsdg_rb_mevp_run on the context returns NSDG_ERR_HIP (nsdg_ctx.hip:
// nsdg_p2p_check).  A wrong result that is reported as an error, never a hung GPU.
#pragma once
#include "mevp_pipeline.h"

namespace nsdg_mevp_detail {

#ifndef NSDG_P2P_SPIN_LIMIT
#define NSDG_P2P_SPIN_LIMIT (1 << 20) // polls of ~0.2 us: a fifth of a second; a legitimate wait is a few march steps (a few microseconds)
#endif

// where a wait that gave up is reported: both belong to the context (nsdg_internal.h)
struct P2PReport {
    unsigned* count; // device memory: events since the last nsdg_mevp_pipeline_health
    unsigned* flag; // host memory mapped into the device: non-zero = at least one event
};

constexpr int P2P_GIVEUP = 6; // index of the sticky give-up flag among a workgroup's counters

// the counters are accessed through LDS-typed pointers: a volatile access through a generic pointer would be a FLAT instruction, which
// counts on vmcnt as well and so waits for every global load in flight
typedef __attribute__((address_space(3))) int lds_int;
__device__ __forceinline__ int flag_peek(const volatile lds_int* p)
{
    asm volatile("" ::: "memory");
    const int x = *p;
    asm volatile("" ::: "memory");
    return __builtin_amdgcn_readfirstlane(x);
}
// the counter flags[which] has reached `need` (or the workgroup has given up)
__device__ __forceinline__ int flag_wait(volatile lds_int* flags, int which, int need, const P2PReport& rep) // returns the polls it took beyond the first
{
    if (flag_peek(flags + which) >= need)
        return 0;
    for (int spin = 0; spin < NSDG_P2P_SPIN_LIMIT; ++spin) {
        __builtin_amdgcn_s_sleep(1);
        if (flag_peek(flags + which) >= need || flag_peek(flags + P2P_GIVEUP) != 0)
            return spin + 1;
    }
    flags[P2P_GIVEUP] = 1; // give up: release everybody, report the event
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(rep.count, 1u);
        __hip_atomic_store(rep.flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return NSDG_P2P_SPIN_LIMIT;
}
// everything this wave has written to (or read from) LDS so far is complete before the counter moves
__device__ __forceinline__ void flag_publish(volatile lds_int* flags, int which, int value)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    flags[which] = value;
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ double2 lds_pair(const double* slot, int k) { return *reinterpret_cast<const double2*>(slot + k * 128); }
__device__ __forceinline__ void lds_pair(double* slot, int k, double a, double b) { *reinterpret_cast<double2*>(slot + k * 128) = make_double2(a, b); }

// Streaming accesses (NSDG_P2P_NT bits: 1 the loader's stress loads, 2 the last stage's stress stores, 4 the loader's ice-strength
// loads): data a pass touches exactly once need not displace the coefficient rows the later stages re-read through the L2.  Measured
// on one box, three alternations (profiles/r05_fused4_p2p.md section 3): 0 0.8727-0.8741 ms per pass at 2048^2, 2 0.8609-0.8679,
// 3 0.8619-0.8702, 7 0.8641-0.8708 -- the same bits in memory, about 1 % less time: 3 is the default.
#ifndef NSDG_P2P_NT
#define NSDG_P2P_NT 3
#endif
// When the stress of a row leaves its stage (NSDG_P2P_EARLY bits: 1 the stages that hand over wait for their free slot and write the 12
// stress pairs into it right after the relaxation, 2 the last stage issues its stress stores there).  The stress registers are final
// after stress_relax; the contributions and node updates that follow only read them, so the writes can issue under that arithmetic.
// 0: everything leaves at the end of the row.  Measured against the parent on one box, five alternations in both orders
// (profiles/r15_early_stress_writes.md): 2 28.21-28.37 -> 27.71-27.88 ms per step at 2048^2 (-1.7 ... -1.9 %, the parent's own spread
// 0.03-0.07 ms), 7.66-7.80 -> 7.54-7.70 at 1024^2; 1 +6.9 % and 3 +8.0 %: the slot is asked for ~2000 cycles sooner, before the consumer
// has freed it, so the loader -- which never waits for a slot at the end of the row -- polls 4.8 times per row and paces the pipeline.
// 2 is the default.
#ifndef NSDG_P2P_EARLY
#define NSDG_P2P_EARLY 2
#endif
// Where the loader's loads land (NSDG_P2P_LAND bits; the row's issue order and the counts: mevp_fused4.hip, above p2p_row).  The loader
// (stage 0) never polls: the stages 1-3 wait for it, so a cycle it stalls at an s_waitcnt is a cycle of every wave.  With the switch at
// 0 the compiler alone decides where a load has to have landed; a bit states one placement by hand:
//   1 coefficients:  the ring write of the coefficient pair, and with it the landing point of the row's coefficients, moves behind
//                    the projected-stress arithmetic (the loader itself needs them only at the node updates);
//   2 request order: the stress of the next row is requested at the very end of the row, behind the hand-over of the row's own
//                    stress, not after the relaxation: the request takes the working registers, 48 registers are free under the
//                    node updates and no copy between two register sets is left; it lands in front of the relaxation.
// Either bit also lets everything the prologue requested land before the first row.  No formula, wait between waves, counter, slot or
// LDS layout changes.  With the switch at 0 the loader stalls ~45 + ~170 + ~160 shader cycles of its ~6600-cycle row at the compiler's
// three waits; with 3 its one stated landing point costs nothing beyond the stamps.  Measured against the parent on one box, five
// alternations in both orders (profiles/r16_loader_landing.md): 3 28.26-28.38 -> 27.19-27.36 ms per step at 2048^2 (-3.7 ... -3.8 %,
// the parent's own spread 0.08-0.09 ms), 7.64-7.91 -> 7.31-7.56 at 1024^2; 1 alone -2.1 %, 2 alone -2.6 % at 2048^2.  Registers per
// wave 364 / 346 -> 296 / 292 (adaptive / uniform).  3 is the default.
#ifndef NSDG_P2P_LAND
#define NSDG_P2P_LAND 3
#endif
// A landing point: at most N vector-memory loads of this wave are still in flight behind it, and the registers named after it are
// opaque to the compiler there ("+v": consumed here), so their data is not used earlier.  The loads are ordinary ones the compiler
// counts itself: its own s_waitcnt in front of the naming statement can only ask for the same or less, never for data that has not
// landed.
template <int N>
__device__ __forceinline__ void p2p_wait_vm()
{
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void p2p_name(double& a, double& b, double& c, double& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
__device__ __forceinline__ void p2p_name(double& a, double& b, double& c) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c)); }
__device__ __forceinline__ void p2p_name(double& a) { asm volatile("" : "+v"(a)); }
__device__ __forceinline__ void p2p_name(double (&x)[3]) { p2p_name(x[0], x[1], x[2]); }
__device__ __forceinline__ void p2p_name(double (&x)[8]) { p2p_name(x[0], x[1], x[2], x[3]), p2p_name(x[4], x[5], x[6], x[7]); }
__device__ __forceinline__ void p2p_name(double (&x)[9]) { p2p_name(x[0], x[1], x[2], x[3]), p2p_name(x[4], x[5], x[6], x[7]), p2p_name(x[8]); }
__device__ __forceinline__ void p2p_name(double (&c)[4][6]) // the pair a ring takes: [n][4], [n][5]
{
    p2p_name(c[0][4], c[0][5], c[1][4], c[1][5]), p2p_name(c[2][4], c[2][5], c[3][4], c[3][5]);
}
template <int N, class... T>
__device__ __forceinline__ void p2p_land(T&... x)
{
    p2p_wait_vm<N>();
    (p2p_name(x), ...);
}

typedef double nsdg_pair16 __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ void tile_load8_nt(const double* __restrict__ a, long t, double (&c)[8])
{
    if (!NT)
        return tile_load8(a, t, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const nsdg_pair16 v = __builtin_nontemporal_load(reinterpret_cast<const nsdg_pair16*>(a + t + 128 * k));
        c[2 * k] = v.x, c[2 * k + 1] = v.y;
    }
}
template <bool NT>
__device__ __forceinline__ void tile_load9_nt(const double* __restrict__ a, long t, int l, double (&c)[9])
{
    if (!NT)
        return tile_load9(a, t, l, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const nsdg_pair16 v = __builtin_nontemporal_load(reinterpret_cast<const nsdg_pair16*>(a + t + 128 * k));
        c[2 * k] = v.x, c[2 * k + 1] = v.y;
    }
    c[8] = __builtin_nontemporal_load(a + t + 512 - l);
}
template <bool NT>
__device__ __forceinline__ void tile_store8_nt(double* __restrict__ a, long t, const double (&c)[8])
{
    if (!NT)
        return tile_store8(a, t, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nsdg_pair16 v;
        v.x = c[2 * k], v.y = c[2 * k + 1];
        __builtin_nontemporal_store(v, reinterpret_cast<nsdg_pair16*>(a + t + 128 * k));
    }
}
typedef double nsdg_pair8 __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ void fetch_nodes(const double* __restrict__ w, long n, double (&o)[3])
{
    const nsdg_pair8 a = *reinterpret_cast<const nsdg_pair8*>(w + n);
    o[0] = a.x, o[1] = a.y, o[2] = w[n + 2];
}

// Rings of NR rows in LDS.  Ice strength: a row takes 9 * 64 doubles, pairs k < 4 of lane l at k * 128 + 2 l, the ninth value at 512 + l.
constexpr int P2P_PSLOT = 9 * 64;
template <int NR>
__device__ __forceinline__ void ring_read_P(const double* __restrict__ ring, int row, int lane, double (&P)[9]) // row >= 0
{
    const double* s = ring + (row % NR) * P2P_PSLOT;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double2 t = *reinterpret_cast<const double2*>(s + k * 128 + 2 * lane);
        P[2 * k] = t.x, P[2 * k + 1] = t.y;
    }
    P[8] = s[512 + lane];
}
template <int NR>
__device__ __forceinline__ void ring_write_P(double* __restrict__ ring, int row, int lane, const double (&P)[9])
{
    double* s = ring + (row % NR) * P2P_PSLOT;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        *reinterpret_cast<double2*>(s + k * 128 + 2 * lane) = make_double2(P[2 * k], P[2 * k + 1]);
    s[512 + lane] = P[8];
}

} // namespace nsdg_mevp_detail

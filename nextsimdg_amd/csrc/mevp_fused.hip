// mevp_fused.hip -- variant 1 of the mEVP sub-iteration: ONE kernel per sub-iteration.
//
// A wave owns a strip of 63 element columns x R element rows and marches through it bottom to top,
// one element per lane per row.  Per row each lane
//   1. gathers its 9 nodal velocities, the 9 Gauss-point strengths and the 24 old stress coefficients,
//   2. relaxes the stress (same inlined stress_update as the two-kernel variant) and stores it,
//   3. forms the element's 18 contributions -(sigma, grad phi_a) to its 9 nodes in registers,
//   4. assembles the divergence at its 4 bottom-left-owned nodes from
//        - its own contributions,
//        - the left neighbour's right-column contributions   -> one-lane wavefront shift (DPP/bpermute),
//        - the contributions of the row below to its top nodes -> carried in registers from the
//          previous iteration of the march (and shifted by one lane for the below-left element),
//      and applies the momentum update to those 4 nodes.
// Nothing but the final stress and velocity ever goes to memory: per element-sub-iteration the kernel
// moves 8 (u,v) + 9 (P) + 24 (S in) + 24 (nodal coefficients) loads and 24 + 8 stores = 776 B of
// unique data, below the 896 B algorithmic figure of SURVEY.md section 8(d) (which counts H, A instead of the
// pre-evaluated P), against 1152 B for the two-kernel variant.
//
// Redundancy instead of synchronisation: lane 0 of every wave recomputes the column left of the
// strip (so 63 of 64 lanes own a column) and every strip recomputes the row below it (R+1 rows of
// stress for R rows of output).  The recomputed values are bit-identical to their owner's, which is
// why the stress is updated out of place (S_in -> S_out): a recomputing strip must never read a value
// its owner has already overwritten.  No barrier, no atomics, no inter-workgroup communication: every
// wave is independent and runs to completion.
//
// The march itself is the one of mevp_pipeline.h: the frame of a wave (march_frame, shared with the stage-per-wave pipeline,
// mevp_fused4.hip: a pass of n sub-iterations there is bit-identical to n launches of this kernel) and the row loop with the prologue
// row, the velocity gather, the carried contributions, the update of the four owned nodes and their store (march_strip, shared with the
// brittle rheology's kernel, bbm.hip).  What is this file's own is the mEVP element step handed to that loop -- where its inputs come from
// (memory, every row) and the order of its loads per register budget -- and the strip height of a single-iteration march
// (nsdg_march_strip_rows, which bbm.hip calls at its one wave per SIMD).
#include "mevp_pipeline.h"

namespace nsdg_mevp_detail {

// MINW: the register budget, 1 or 2 waves per SIMD; AD: local, solution-adaptive alpha and beta (mevp_common.h)
// LAND: the instantiation that holds land nodes at 0 (mevp_common.h: node_update), launched after a packing that saw a land mask
// BASAL: the instantiation with the seabed stress (mevp_common.h: node_update), launched after a packing that saw a depth array
template <int MINW, bool AD, bool LAND, bool BASAL>
__global__ __launch_bounds__(256, MINW) void mevp_fused_kernel(NodalConstsOf<BASAL> K, AdaptConsts AC, int nx, int ny, int k0, int j0, int j1, int R, int ncw, double hx,
    double hy, double ialpha, double dmin2, StressPtrs S, const double* __restrict__ u_old, const double* __restrict__ v_old,
    const double* __restrict__ packed, const double* __restrict__ pg, double* __restrict__ u_new, double* __restrict__ v_new)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int strip = wave / ncw, cw = wave - strip * ncw;
    MarchConst M;
    M.y0 = k0 + strip * R;
    if (M.y0 >= j1)
        return; // wave-uniform
    M.y1 = min(M.y0 + R, j1);
    march_frame<63, 1>(M, K, AC, nx, ny, lane, cw, hx, hy, ialpha, dmin2, nodal_u0<BASAL>(K)); // 63 owned columns, lane 0 recomputes the column left of them

    // the element step of the mEVP rheology: the stress is relaxed in registers, stored, and is itself what the momentum equation takes
    march_strip<AD, LAND, MINW >= 2, BASAL>(M, k0, j0, u_old, v_old, packed, u_new, v_new,
        [&](int iy, bool store, long nV, const double (&ul)[9], const double (&vl)[9], double (&s11)[8], double (&s12)[8], double (&s22)[8], double& qe) {
            const long ts = tile_off(M.ix, iy, M.ntx, 8), tp = tile_off(M.ix, iy, M.ntx, 9);
            double Pq[9];
            tile_load9(pg, tp, M.ix & 63, Pq);
            if constexpr (AD) {
                // local, solution-adaptive alpha (mevp_common.h); h' of the element's centre node is its packed coefficient [0]
                const double hc = packed[nodal_off(nV + M.nn + 1)];
                double r11[8], r12[8], r22[8], ialpha_e;
                stress_projected_adaptive(ul, vl, Pq, M.ihx, M.ihy, dmin2, hc, AC, r11, r12, r22, qe, ialpha_e);
                tile_load8(S.i11, ts, s11);
                tile_load8(S.i12, ts, s12);
                tile_load8(S.i22, ts, s22);
                stress_relax(ialpha_e, r11, r12, r22, s11, s12, s22);
            } else if constexpr (MINW >= 2) {
                // 2 waves/SIMD build: stage the loads so that the live set stays under 256 registers -- the old
                // stress is fetched only after the projected stress is formed, the partner wave covers the latency
                double r11[8], r12[8], r22[8];
                stress_projected(ul, vl, Pq, M.ihx, M.ihy, ialpha, dmin2, r11, r12, r22);
                asm volatile("" ::: "memory");
                tile_load8(S.i11, ts, s11);
                tile_load8(S.i12, ts, s12);
                tile_load8(S.i22, ts, s22);
                stress_relax(ialpha, r11, r12, r22, s11, s12, s22);
            } else {
                tile_load8(S.i11, ts, s11);
                tile_load8(S.i12, ts, s12);
                tile_load8(S.i22, ts, s22);
                stress_update(ul, vl, Pq, M.ihx, M.ihy, ialpha, dmin2, s11, s12, s22);
            }
            if (store) {
                tile_store8(S.o11, ts, s11);
                tile_store8(S.o12, ts, s12);
                tile_store8(S.o22, ts, s22);
            }
        });
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

int nsdg_march_strip_rows(const nsdg_ctx* ctx, int rows, int ncw, int waves_per_simd)
{
    int R = ctx->strip_rows;
    if (R <= 0) {
        // Automatic strip height.  Every wave marches R+1 rows (one redundant), and the launch runs in
        // ceil(waves / resident wave slots) rounds, so the time is ~ rounds * (R+1) row-times: pick the R
        // that minimises it (measured on 2048^2: R = 17 -> 2 full rounds, 8 % faster than R = 4 with its
        // 8.25 rounds and 25 % redundant rows).  A single round is charged 1.5 row-times because one
        // straggling wave then ends the launch alone.
        const long slots = (long)waves_per_simd * 4 * ctx->num_cus;
        double best = 1e30;
        R = 4;
        for (int r = 2; r <= 64; ++r) {
            const long waves = (long)nsdg_div_up(rows, r) * ncw;
            const long rounds = (waves + slots - 1) / slots;
            const double cost = rounds * (r + 1.0) + (rounds == 1 ? 1.5 : 0.0);
            if (cost < best) {
                best = cost;
                R = r;
            }
        }
    }
    return R;
}

int nsdg_launch_mevp_fused(nsdg_ctx* ctx, bool land, bool basal, int k0, int j0, int j1, const nsdg_mevp_bufs& b)
{
    const int ncw = nsdg_div_up(ctx->nx, 63); // 63 owned columns per wave
    const int R = nsdg_march_strip_rows(ctx, j1 - k0, ncw, 2); // 2 waves per SIMD at ~204 VGPRs
    const int nstrips = nsdg_div_up(j1 - k0, R);
    const long nwaves = (long)ncw * nstrips;
    const StressPtrs S = { b.s11i, b.s12i, b.s22i, b.s11, b.s12, b.s22 };
    const NodalConstsBasal K = nsdg_nodal_consts_basal(ctx);
    const AdaptConsts AC = nsdg_adapt_consts(ctx);
    const double ialpha = 1. / ctx->mevp.alpha, dmin2 = ctx->mevp.delta_min * ctx->mevp.delta_min;
    const dim3 grid(nsdg_div_up(nwaves, 4)), block(256);
    // two register budgets of the same kernel: 1 wave/SIMD (no spills) or 2 waves/SIMD (a few scratch spills); the adaptive form (local
    // alpha, beta: mevp_common.h) runs at 1 wave/SIMD
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, K, AC, ctx->nx, ctx->ny, k0, j0, j1, R, ncw, ctx->hx, ctx->hy, ialpha, dmin2, S, b.u_old, b.v_old,
            b.packed, b.pg, b.u_new, b.v_new);
    };
    auto pick = [&](auto minw, auto ad) {
        constexpr int W = decltype(minw)::value;
        constexpr bool A = decltype(ad)::value;
        if (basal)
            land ? launch(mevp_fused_kernel<W, A, true, true>) : launch(mevp_fused_kernel<W, A, false, true>);
        else
            land ? launch(mevp_fused_kernel<W, A, true, false>) : launch(mevp_fused_kernel<W, A, false, false>);
    };
    if (nsdg_adaptive(ctx))
        pick(std::integral_constant<int, 1>(), std::true_type());
    else if (ctx->fused_min_waves >= 2)
        pick(std::integral_constant<int, 2>(), std::false_type());
    else
        pick(std::integral_constant<int, 1>(), std::false_type());
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

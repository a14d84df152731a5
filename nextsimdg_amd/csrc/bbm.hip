// bbm.hip -- the brittle Bingham-Maxwell (BBM) sub-cycle: ONE kernel per sub-iteration, a sibling of mevp_fused.hip.
//
// No counterpart in the reference snapshot (its dynamics component is commented out); the scheme is stated in include/nsdg.h "brittle
// rheology" and DESIGN.md section 3.8 from the published formulation (Olason et al. 2022; Dansereau et al. 2016), parity unpinned.
//
// The march is the one of mevp_pipeline.h, all of it: the frame of a wave that owns 63 element columns x R element rows (march_frame), the
// row loop with its prologue row, velocity gather, carried contributions, update of the four owned nodes by
// owned_node_updates<false, LAND, BASAL> with the BBM launch constants K1 = K2 = rho_i / dt_s (explicit in stress and Coriolis, implicit in ocean
// drag) and their store (march_strip); the strip height is the rule of mevp_fused.hip at this kernel's one wave per SIMD
// (nsdg_march_strip_rows), the checks of a pass those of nsdg_pass_check (mevp.hip).  What is this file's own is the element step inside
// the march (bbm_common.h: bbm_element_step): elastic predictor, Maxwell relaxation, Mohr-Coulomb test and damage update at the 3x3 Gauss
// points, with the loads and stores of its state -- and the damage, which the mEVP pass does not know.
//
// Stress AND damage are out of place (S_in -> S_out, D_in -> D_out): a strip that recomputes a row must never read what its owner has
// overwritten.  No barrier, no atomics: every wave is independent.
//
// Traffic per element-sub-iteration, unique data: loads 8 (u, v) + 27 (hg, eg, pm) + 24 (S in) + 6 (D in) + 24 (nodal coefficients),
// stores 24 (S out) + 6 (D out) + 8 (u, v) = 127 doubles = 1016 B, against 776 B of the mEVP kernel (which reads one Gauss array
// instead of three and no damage).
#include <cmath>
#include <initializer_list>

#include "bbm_common.h"
#include "mevp_pipeline.h"

namespace nsdg_mevp_detail {

// 1 wave per SIMD: the element step holds 9 Gauss points x (3 strain rates + 3 stresses + damage + 3 per-step values) beside the march's
// carried contributions (resource figures: profiles/r09_bbm.md)
// LAND: the instantiation that holds land nodes at 0 (mevp_common.h: node_update), launched after a packing that saw a land mask
// BASAL: the instantiation with the seabed stress (mevp_common.h: node_update), launched after a packing that saw a depth array
template <bool LAND, bool BASAL>
__global__ __launch_bounds__(256, 1) void bbm_fused_kernel(NodalConstsOf<BASAL> K, BbmConsts B, int nx, int ny, int k0, int j0, int j1, int R, int ncw,
    double hx, double hy, StressPtrs S, const double* __restrict__ D_in, double* __restrict__ D_out, const double* __restrict__ u_old,
    const double* __restrict__ v_old, const double* __restrict__ packed, const double* __restrict__ hgp, const double* __restrict__ egp,
    const double* __restrict__ pmp, double* __restrict__ u_new, double* __restrict__ v_new)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int strip = wave / ncw, cw = wave - strip * ncw;
    MarchConst M;
    M.y0 = k0 + strip * R;
    if (M.y0 >= j1)
        return; // wave-uniform
    M.y1 = min(M.y0 + R, j1);
    march_frame<63, 1>(M, K, AdaptConsts { 0., 0., 0. }, nx, ny, lane, cw, hx, hy, 0., 0., nodal_u0<BASAL>(K)); // 63 owned columns, lane 0 recomputes the column left of them
    const long N = (long)nx * ny;

    march_strip<false, LAND, false, BASAL>(M, k0, j0, u_old, v_old, packed, u_new, v_new,
        [&](int iy, bool store, long, const double (&ul)[9], const double (&vl)[9], double (&m11)[8], double (&m12)[8], double (&m22)[8], double&) {
            const long ts = tile_off(M.ix, iy, M.ntx, 8), tp = tile_off(M.ix, iy, M.ntx, 9), e = (long)iy * nx + M.ix;
            double hg[9], eg[9], pm[9], s11[8], s12[8], s22[8], d[6];
            tile_load9(hgp, tp, M.ix & 63, hg);
            tile_load9(egp, tp, M.ix & 63, eg);
            tile_load9(pmp, tp, M.ix & 63, pm);
            tile_load8(S.i11, ts, s11);
            tile_load8(S.i12, ts, s12);
            tile_load8(S.i22, ts, s22);
            plane_load6(D_in, N, e, d);
            bbm_element_step(B, ul, vl, M.ihx, M.ihy, hg, eg, pm, s11, s12, s22, d, m11, m12, m22);
            if (store) {
                tile_store8(S.o11, ts, s11);
                tile_store8(S.o12, ts, s12);
                tile_store8(S.o22, ts, s22);
                plane_store6(D_out, N, e, d);
            }
        });
}

// what the sub-cycle does not change, once per model step: hg = max(H, 0), eg = exp(-C (1 - clamp(A, 0, 1))), pm = p0 hg^(3/2) eg at the
// 3x3 Gauss points (the points and clamps of mevp_common.h: clamp_thickness_conc, as the ice strength), tiled like pg
__global__ __launch_bounds__(256) void bbm_prepare_kernel(int nx, int ny, int j0, int j1, double p0, double compaction,
    const double* __restrict__ H, const double* __restrict__ A, double* __restrict__ hgp, double* __restrict__ egp, double* __restrict__ pmp)
{
    const int ix = blockIdx.x * 64 + threadIdx.x;
    const int iy = j0 + blockIdx.y * 4 + threadIdx.y;
    if (ix >= nx || iy >= j1)
        return;
    const long N = (long)nx * ny;
    const long e = (long)iy * nx + ix;
    const long tp = tile_off(ix, iy, tiles_per_row(nx), 9);
    double hc[6], ac[6];
    plane_load6(H, N, e, hc);
    plane_load6(A, N, e, ac);
    double hg[9], eg[9], pm[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        double h, a;
        gauss_thickness_conc(q, hc, ac, h, a);
        clamp_thickness_conc(h, a);
        hg[q] = h;
        eg[q] = exp(-compaction * (1. - a));
        pm[q] = p0 * h * sqrt(h) * eg[q];
    }
    tile_store9(hgp, tp, ix & 63, hg);
    tile_store9(egp, tp, ix & 63, eg);
    tile_store9(pmp, tp, ix & 63, pm);
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

// launch constants of the element step from the context's parameters and the packing's time step
static BbmConsts nsdg_bbm_consts(const nsdg_ctx* ctx)
{
    const nsdg_bbm_params& P = ctx->bbm;
    const double h = std::min(ctx->hx, ctx->hy), dts = ctx->pack_dt;
    BbmConsts B;
    B.dts = dts;
    B.heal = dts / P.t_heal;
    B.d_max = P.d_max;
    B.young = P.young, B.lambda0 = P.lambda0;
    B.k1 = 1. / (1. + P.nu), B.k2 = P.nu / (1. - P.nu * P.nu);
    B.tan_phi = P.tan_phi, B.coh = P.cohesion_lab * std::sqrt(0.1 / h), B.N = P.compr_strength;
    B.rc = dts / (h * std::sqrt(2. * (1. + P.nu) * ctx->mevp.rho_ice));
    B.nrelax = P.relax_exponent - 1;
    return B;
}

extern "C" {

void nsdg_bbm_default_params(nsdg_bbm_params* p)
{
    p->young = 5.9605e8;
    p->nu = 1. / 3.;
    p->p0 = 1e4;
    p->lambda0 = 1e7;
    p->tan_phi = 0.7;
    p->cohesion_lab = 2e6;
    p->compr_strength = 1e10;
    p->t_heal = 1e5;
    p->d_max = 1. - 1e-6;
    p->relax_exponent = 5;
    p->reserved = 0;
}

int nsdg_bbm_params_check(const nsdg_bbm_params* p)
{ // host only, no context: what nsdg_bbm_params_set refuses
    NSDG_CHECK_ARG(p, "null argument");
    for (double x : { p->young, p->nu, p->p0, p->lambda0, p->tan_phi, p->cohesion_lab, p->compr_strength, p->t_heal, p->d_max })
        NSDG_CHECK_ARG(std::isfinite(x), "non-finite parameter");
    NSDG_CHECK_ARG(p->relax_exponent >= 1, "relax_exponent must be an integer >= 1");
    NSDG_CHECK_ARG(p->d_max > 0. && p->d_max < 1., "d_max must lie in (0, 1)");
    NSDG_CHECK_ARG(p->young > 0. && p->lambda0 > 0. && p->t_heal > 0., "young, lambda0 and t_heal must be positive");
    return NSDG_OK;
}

int nsdg_bbm_params_set(nsdg_ctx* ctx, const nsdg_bbm_params* p)
{
    NSDG_CHECK_ARG(ctx && p, "null argument");
    const int rc = nsdg_bbm_params_check(p);
    if (rc != NSDG_OK)
        return rc;
    ctx->bbm = *p;
    return NSDG_OK;
}

int nsdg_bbm_prepare(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* hg, double* eg, double* pm)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && A && hg && eg && pm, "null field pointer");
    NSDG_CHECK_ARG(nsdg_aligned16({ hg, eg, pm }), "tiled arrays must be 16-byte aligned");
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(ctx->nx, 64), nsdg_div_up(j1 - j0, 4));
    hipLaunchKernelGGL(bbm_prepare_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, j0, j1, ctx->bbm.p0, ctx->mevp.compaction, H, A, hg, eg, pm);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_bbm_iterate(nsdg_ctx* ctx, int32_t k0, int32_t j0, int32_t j1, const double* s11_in, const double* s12_in, const double* s22_in,
    double* s11_out, double* s12_out, double* s22_out, const double* D_in, double* D_out, const double* u_old, const double* v_old, double* u_new,
    double* v_new, const double* packed, const double* hg, const double* eg, const double* pm)
{
    // the damage is this rheology's own; everything else is a single-iteration pass like nsdg_mevp_iterate's, with three Gauss arrays
    // where that has the ice strength
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(D_in && D_out, "null field pointer");
    NSDG_CHECK_ARG(D_out != D_in, "the output damage must not alias the input damage");
    bool run;
    const int checked = nsdg_pass_check(ctx, __func__, 1, k0, j0, j1, false, 0, 0,
        { s11_in, s12_in, s22_in, s11_out, s12_out, s22_out, u_old, v_old, u_new, v_new, packed, /* pg: none */ nullptr }, { hg, eg, pm }, &run);
    if (!run)
        return checked;
    const int ncw = nsdg_div_up(ctx->nx, 63); // 63 owned columns per wave
    const int R = nsdg_march_strip_rows(ctx, j1 - k0, ncw, 1);
    const long nwaves = (long)ncw * nsdg_div_up(j1 - k0, R);
    const StressPtrs S = { s11_in, s12_in, s22_in, s11_out, s12_out, s22_out };
    // the BBM momentum step: the mEVP node update with K1 = K2 = rho_i / dt_s (and u0 = v0 = 0 in the packing)
    const double rdt = ctx->mevp.rho_ice / ctx->pack_dt;
    const NodalConstsBasal K = { { rdt, rdt, ctx->mevp.rho_ice * ctx->mevp.fc, rdt }, ctx->basal.u0 };
    const BbmConsts B = nsdg_bbm_consts(ctx);
    const dim3 grid(nsdg_div_up(nwaves, 4)), block(256);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, K, B, ctx->nx, ctx->ny, k0, j0, j1, R, ncw, ctx->hx, ctx->hy, S, D_in, D_out, u_old, v_old, packed,
            hg, eg, pm, u_new, v_new);
    };
    // masked or not, with the seabed stress or not: the instantiation goes with the packing the pass reads, as in nsdg_mevp_pass
    if (ctx->pack_basal)
        ctx->pack_land ? launch(bbm_fused_kernel<true, true>) : launch(bbm_fused_kernel<false, true>);
    else
        ctx->pack_land ? launch(bbm_fused_kernel<true, false>) : launch(bbm_fused_kernel<false, false>);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_bbm_substep_count(const nsdg_bbm_params* p, double rho_ice, double h, double dt, double courant, int32_t max_nsub, int32_t* nsub)
{
    NSDG_CHECK_ARG(p && nsub, "null argument");
    NSDG_CHECK_ARG(std::isfinite(p->young) && p->young > 0. && std::isfinite(p->nu) && p->nu > -1. && p->nu < 1., "young must be positive, nu in (-1, 1)");
    NSDG_CHECK_ARG(std::isfinite(rho_ice) && rho_ice > 0. && std::isfinite(h) && h > 0. && std::isfinite(dt) && dt > 0. && std::isfinite(courant) && courant > 0.,
        "rho_ice, cell size, time step and courant must be finite and positive");
    NSDG_CHECK_ARG(max_nsub >= 1, "max_nsub must be >= 1");
    const double speed = std::sqrt(p->young / (rho_ice * (1. - p->nu * p->nu)));
    const double need = std::max(1., std::ceil(dt * speed / (courant * h)));
    if (!(need <= (double)max_nsub)) {
        nsdg_set_error("nsdg_bbm_substep_count: the elastic wave of %.6g m/s crosses %.6g cells per step of %g s on cells of %g m: that needs nsub = %.0f "
                       "sub-iterations at courant %g, more than max_nsub = %d",
            speed, speed * dt / h, dt, h, need, courant, (int)max_nsub);
        return NSDG_ERR_ARG;
    }
    *nsub = (int32_t)need;
    return NSDG_OK;
}

} // extern "C"

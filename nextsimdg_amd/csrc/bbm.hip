// bbm.hip -- the brittle Bingham-Maxwell (BBM) sub-cycle: ONE kernel per sub-iteration, a sibling of mevp_fused.hip.
//
// No counterpart in the reference snapshot (its dynamics component is commented out); the scheme is stated in include/nsdg.h "brittle
// rheology" and DESIGN.md section 3.8 from the published formulation (Olason et al. 2022; Dansereau et al. 2016), parity unpinned.
//
// The march is the one of mevp_pipeline.h, unchanged: a wave owns a strip of 63 element columns x R element rows, one element per lane
// per row; lane 0 recomputes the column left of the strip and every strip recomputes the row below it as a prologue; the contributions of
// a row to its top nodes are carried in registers to the next row; the four owned nodes are updated by owned_node_updates<false, LAND>
// with the BBM launch constants K1 = K2 = rho_i / dt_s (explicit in stress and Coriolis, implicit in ocean drag) and stored by
// store_owned_nodes.  What is this kernel's own is the element step (bbm_common.h: bbm_element_step): elastic predictor, Maxwell
// relaxation, Mohr-Coulomb test and damage update at the 3x3 Gauss points.
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

// DG2 field in plane layout: the 6 coefficients of element e, N elements per plane
__device__ __forceinline__ void plane_load6(const double* __restrict__ f, long N, long e, double (&c)[6])
{
#pragma unroll
    for (int k = 0; k < 6; ++k)
        c[k] = f[k * N + e];
}
__device__ __forceinline__ void plane_store6(double* __restrict__ f, long N, long e, const double (&c)[6])
{
#pragma unroll
    for (int k = 0; k < 6; ++k)
        f[k * N + e] = c[k];
}

// 1 wave per SIMD: the element step holds 9 Gauss points x (3 strain rates + 3 stresses + damage + 3 per-step values) beside the march's
// carried contributions (resource figures: profiles/r09_bbm.md)
// LAND: the instantiation that holds land nodes at 0 (mevp_common.h: node_update), launched after a packing that saw a land mask
template <bool LAND>
__global__ __launch_bounds__(256, 1) void bbm_fused_kernel(NodalConsts K, BbmConsts B, int nx, int ny, int k0, int j0, int j1, int R, int ncw,
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
    const int ixr = cw * 63 - 1 + lane;
    const bool valid = ixr >= 0 && ixr < nx; // lanes outside the array load a clamped column and store nothing
    M.K = K, M.AC = AdaptConsts { 0., 0., 0. };
    M.nx = nx, M.ny = ny, M.lane = lane;
    M.own = valid && lane > 0;
    M.ix = min(max(ixr, 0), nx - 1);
    M.hasL = M.ix > 0, M.lastcol = M.ix == nx - 1;
    M.ntx = tiles_per_row(nx);
    M.nn = 2 * nx + 1;
    M.nplane = nodal_plane((long)M.nn * (2 * ny + 1));
    M.hx = hx, M.hy = hy, M.ihx = 1. / hx, M.ihy = 1. / hy, M.iarea = M.ihx * M.ihy;
    M.ialpha = 0., M.dmin2 = 0.;
    const int ix = M.ix, nn = M.nn;
    const long N = (long)nx * ny;

    TopCarry carry; // zero by its member initialisers: the first row of the march adds nothing from a row below

    for (int iy = (M.y0 > k0 ? M.y0 - 1 : M.y0); iy < M.y1; ++iy) {
        const bool prologue = iy < M.y0; // recomputed row owned by the strip below: nothing is stored
        const long ts = tile_off(ix, iy, M.ntx, 8), tp = tile_off(ix, iy, M.ntx, 9);
        const long nV = (long)(2 * iy) * nn + 2 * ix, e = (long)iy * nx + ix;
        double ul[9], vl[9], hg[9], eg[9], pm[9], s11[8], s12[8], s22[8], d[6], m11[8], m12[8], m22[8];
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const long n = nV + (a / 3) * nn + a % 3;
            ul[a] = u_old[n];
            vl[a] = v_old[n];
        }
        tile_load9(hgp, tp, ix & 63, hg);
        tile_load9(egp, tp, ix & 63, eg);
        tile_load9(pmp, tp, ix & 63, pm);
        tile_load8(S.i11, ts, s11);
        tile_load8(S.i12, ts, s12);
        tile_load8(S.i22, ts, s22);
        plane_load6(D_in, N, e, d);
        bbm_element_step(B, ul, vl, M.ihx, M.ihy, hg, eg, pm, s11, s12, s22, d, m11, m12, m22);
        if (!prologue && M.own) {
            tile_store8(S.o11, ts, s11);
            tile_store8(S.o12, ts, s12);
            tile_store8(S.o22, ts, s22);
            plane_store6(D_out, N, e, d);
        }
        double cx[9], cy[9];
        node_contrib_all(m11, m12, m22, hx, hy, cx, cy);

        if (!prologue && iy >= j0) { // wave-uniform
            double c[4][6], un[4], vn[4];
            load_owned_nodal(M, iy, c, packed);
            const double uu[4] = { ul[0], ul[1], ul[3], ul[4] }, vv[4] = { vl[0], vl[1], vl[3], vl[4] };
            owned_node_updates<false, LAND>(M, iy > 0, c, uu, vv, carry, cx, cy, un, vn);
            if (M.own)
                store_owned_nodes(nV, nn, M.lastcol, iy == ny - 1, un, vn, u_new, v_new);
        }
        carry_top<false>(carry, cx, cy); // the top-row contributions go to the next row of the march
    }
}

// what the sub-cycle does not change, once per model step: hg = max(H, 0), eg = exp(-C (1 - clamp(A, 0, 1))), pm = p0 hg^(3/2) eg at the
// 3x3 Gauss points (the points and clamps of ice_strength_kernel, mevp.hip), tiled like pg
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
        double h = 0., a = 0.;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            FMA_TAB(h, PSI_G3[q][c], hc[c]);
            FMA_TAB(a, PSI_G3[q][c], ac[c]);
        }
        h = fmax(h, 0.);
        a = fmin(fmax(a, 0.), 1.);
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

static inline bool bbm_aligned16(std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15)
            return false;
    return true;
}

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

int nsdg_bbm_params_set(nsdg_ctx* ctx, const nsdg_bbm_params* p)
{
    NSDG_CHECK_ARG(ctx && p, "null argument");
    for (double x : { p->young, p->nu, p->p0, p->lambda0, p->tan_phi, p->cohesion_lab, p->compr_strength, p->t_heal, p->d_max })
        NSDG_CHECK_ARG(std::isfinite(x), "non-finite parameter");
    NSDG_CHECK_ARG(p->relax_exponent >= 1, "relax_exponent must be an integer >= 1");
    NSDG_CHECK_ARG(p->d_max > 0. && p->d_max < 1., "d_max must lie in (0, 1)");
    NSDG_CHECK_ARG(p->young > 0. && p->lambda0 > 0. && p->t_heal > 0., "young, lambda0 and t_heal must be positive");
    ctx->bbm = *p;
    return NSDG_OK;
}

int nsdg_bbm_prepare(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* hg, double* eg, double* pm)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && A && hg && eg && pm, "null field pointer");
    NSDG_CHECK_ARG(bbm_aligned16({ hg, eg, pm }), "tiled arrays must be 16-byte aligned");
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
    NSDG_NEED_GRID(ctx);
    const int ny = ctx->ny;
    NSDG_CHECK_ARG(0 <= k0 && k0 <= j0 && j0 <= j1 && j1 <= ny, "need 0 <= k0 <= j0 <= j1 <= ny");
    NSDG_CHECK_ARG(k0 == j0 - 1 || (k0 == 0 && j0 == 0), "need k0 == j0 - 1 (one ghost row below) or k0 == j0 == 0");
    NSDG_CHECK_ARG(s11_in && s12_in && s22_in && s11_out && s12_out && s22_out && D_in && D_out && u_old && v_old && u_new && v_new && packed && hg
            && eg && pm,
        "null field pointer");
    NSDG_CHECK_ARG(bbm_aligned16({ s11_in, s12_in, s22_in, s11_out, s12_out, s22_out, hg, eg, pm }), "tiled arrays (stress, Gauss arrays) must be 16-byte aligned");
    NSDG_CHECK_ARG(u_new != u_old && v_new != v_old, "u_new/v_new must not alias u_old/v_old");
    NSDG_CHECK_ARG(s11_out != s11_in && s12_out != s12_in && s22_out != s22_in, "the output stress must not alias the input stress");
    NSDG_CHECK_ARG(D_out != D_in, "the output damage must not alias the input damage");
    if (k0 == j1)
        return NSDG_OK;
    if (!(ctx->pack_dt > 0)) {
        nsdg_set_error("nsdg_bbm_iterate: nsdg_mevp_prepare / nsdg_mevp_pack_nodal was not called on this context");
        return NSDG_ERR_STATE;
    }
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const int ncw = nsdg_div_up(ctx->nx, 63); // 63 owned columns per wave
    int R = ctx->strip_rows;
    if (R <= 0) {
        // the automatic strip height of the mEVP kernel (mevp_fused.hip: rounds of resident waves times R + 1 rows each) at this kernel's
        // 1 wave per SIMD
        const long slots = 4L * ctx->num_cus;
        const int rows = j1 - k0;
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
    const long nwaves = (long)ncw * nsdg_div_up(j1 - k0, R);
    const StressPtrs S = { s11_in, s12_in, s22_in, s11_out, s12_out, s22_out };
    // the BBM momentum step: the mEVP node update with K1 = K2 = rho_i / dt_s (and u0 = v0 = 0 in the packing)
    const double rdt = ctx->mevp.rho_ice / ctx->pack_dt;
    const NodalConsts K = { rdt, rdt, ctx->mevp.rho_ice * ctx->mevp.fc, rdt };
    const BbmConsts B = nsdg_bbm_consts(ctx);
    const dim3 grid(nsdg_div_up(nwaves, 4)), block(256);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, K, B, ctx->nx, ny, k0, j0, j1, R, ncw, ctx->hx, ctx->hy, S, D_in, D_out, u_old, v_old, packed,
            hg, eg, pm, u_new, v_new);
    };
    // masked or not: the instantiation goes with the packing the pass reads, as in nsdg_mevp_pass
    ctx->pack_land ? launch(bbm_fused_kernel<true>) : launch(bbm_fused_kernel<false>);
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

// budget.hip -- momentum balance diagnostics: the nodal forces of the sea-ice momentum equation and their power.
//
// No counterpart in the reference snapshot; the arithmetic is stated in include/nsdg_budget.h.  One launch after the sub-cycle evaluates
// every term of the nodal balance at the state the sub-cycle left -- (u, v), S -- with the coefficients of the packing it ran with.  It
// reads what nsdg_mevp_velocity reads (the stress of the four elements round a node, the packed coefficients, the velocity) and the wind,
// the concentration and the sea-surface height beside; it writes up to sixteen nodal planes and nine totals per element row.  Nothing of
// the sub-cycle changes: no kernel, plan, pass or packed layout.
//
// One kernel, two launch geometries.  With totals: one wave64 per element row, four rows per workgroup, the wave strides over the row's
// tiles -- the order of the sums in the header comes for free.  Without: one lane per element, the geometry of nsdg_mevp_velocity
// (profiles/momentum_budget.md has both measured).
#include <cstring>

#include "mevp_common.h"

// how a plane value is stored: plain by default; -DNSDG_BUDGET_NT_STORES: non-temporal (nobody re-reads the planes on the device) -- measured
// and not adopted, profiles/momentum_budget.md
#ifdef NSDG_BUDGET_NT_STORES
#define NSDG_BUDGET_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
#else
#define NSDG_BUDGET_STORE(ptr, val) (*(ptr) = (val))
#endif

namespace nsdg_mevp_detail {

struct BudgetConsts {
    double rho_ice, f_atm, k3, dt; // of the packing: rho_ice, c_atm rho_atm, rho_ice f_c, pack_dt
    double u0; // the speed of the seabed stress (BASAL)
    double g; // gravity (with a sea-surface height)
    bool basal; // the packing stored T_b
};

struct BudgetPlanes {
    double* p[2 * NSDG_BUDGET_TERMS]; // [2 t + (0: x, 1: y)], null: not stored
};

// the sixteen forces of one node that is neither a Dirichlet node of the lattice edge nor (the select at the end) a land node; m = the
// nodal mass per area, (uu, vv) = the velocity the power is taken with: 0 at a land node
__device__ __forceinline__ void budget_node(const BudgetConsts& B, int nx, int ny, int gx, int gy, long n, long nplane, double divx, double divy,
    double ilumped, const double* __restrict__ A, const double* __restrict__ ua, const double* __restrict__ va, const double* __restrict__ u,
    const double* __restrict__ v, const double* __restrict__ packed, const double* __restrict__ ssh, double hx, double hy, double (&f)[16],
    double& m, double& uu, double& vv)
{
    double c[6];
    load_nodal(packed, nplane, n, c);
    uu = u[n], vv = v[n];
    const bool land = c[1] < 0.;
    const bool ice_free = c[0] > 0x1p50;
    const double s = ice_free ? 0x1p-100 : 1.;
    const double hp = s * c[0], cd = s * c[1], c2 = s * c[2], c3 = s * c[3];
    m = B.rho_ice * hp;
    double a = 1.;
    if (!ice_free)
        a = fmin(fmax(node_average(nx, ny, 6, A, gx, gy), 0.), 1.);
    // wind
    double tax, tay;
    wind_tau(B.f_atm, ua[n], va[n], tax, tay);
    const double wx = a * tax;
    const double wy = a * tay;
    // water drag: the expressions of node_update
    const double du = c[4] - uu, dv = c[5] - vv;
    const double drag = cd * fast_sqrt(du * du + dv * dv);
    const double qx = drag * du;
    const double qy = drag * dv;
    // Coriolis
    const double cor = B.k3 * hp;
    const double cx = cor * vv;
    const double cu = cor * uu;
    const double cy = -cu;
    // sea-surface tilt
    double tx, ty;
    if (ssh) {
        double sx = 0., sy = 0.;
        if (!land) // a land node reads nothing of eta
            tilt_gradient(2 * nx + 1, 2 * ny + 1, gx, gy, hx, hy, [&](int x, int y) { return ssh[(long)y * (2 * nx + 1) + x]; }, sx, sy);
        const double m_g = m * B.g;
        const double gx_ = m_g * sx;
        const double gy_ = m_g * sy;
        tx = -gx_, ty = -gy_;
    } else {
        const double gv = cor * c[5];
        const double gu = cor * c[4];
        tx = -gv, ty = gu;
    }
    // internal stress divergence: an ice-free node does not feel it
    const double dx_ = divx * ilumped;
    const double dy_ = divy * ilumped;
    const double ix_ = ice_free ? 0. : dx_, iy_ = ice_free ? 0. : dy_;
    // seabed stress
    double bx = 0., by = 0.;
    if (B.basal) {
        const double tb = load_nodal_tb(packed, nplane, n);
        const double cb = tb * fast_rcp(fast_sqrt(uu * uu + vv * vv) + B.u0);
        const double bu = cb * uu;
        const double bv = cb * vv;
        bx = -bu, by = -bv;
    }
    // inertia and residual
    const double mdt = m / B.dt;
    const double mu = mdt * uu;
    const double mv = mdt * vv;
    const double ex = c2 - wx - tx;
    const double ey = c3 - wy - ty;
    double rx = c2 - mu, ry = c3 - mv;
    rx = rx + qx, ry = ry + qy;
    rx = rx + cx, ry = ry + cy;
    rx = rx + ix_, ry = ry + iy_;
    rx = rx + bx, ry = ry + by;
    f[0] = wx, f[1] = wy, f[2] = qx, f[3] = qy, f[4] = cx, f[5] = cy, f[6] = tx, f[7] = ty;
    f[8] = ix_, f[9] = iy_, f[10] = bx, f[11] = by, f[12] = ex - mu, f[13] = ey - mv, f[14] = rx, f[15] = ry;
    if (land) { // selects, as node_update<LAND>: NaN forcing on land reaches nothing
#pragma unroll
        for (int k = 0; k < 16; ++k)
            f[k] = 0.;
        uu = vv = 0.;
    }
}

// Element (ix, iy) = its four owned nodes (vertex, bottom edge, left edge, centre), the ownership of mevp_velocity_body; the wave strides
// over the row by 64 gridDim.x elements.  The totals need gridDim.x == 1 -- the wave then holds the whole row -- and are written only then.
__global__ __launch_bounds__(256) void momentum_budget_kernel(BudgetConsts B, int nx, int ny, int j0, int j1, double hx, double hy,
    const double* __restrict__ A, const double* __restrict__ ua, const double* __restrict__ va, const double* __restrict__ S11,
    const double* __restrict__ S12, const double* __restrict__ S22, const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ packed, const double* __restrict__ ssh, BudgetPlanes out, double* __restrict__ power_arg, long power_stride, int row0)
{
    // the totals are a wave's fold over its WHOLE row: a launch with more than one workgroup column (the tile geometry) writes none, whatever
    // it was handed -- nsdg_momentum_budget launches one column whenever it passes `power`
    double* __restrict__ const power = gridDim.x == 1 ? power_arg : nullptr;
    const int iy = j0 + blockIdx.y * 4 + threadIdx.y;
    if (iy >= j1) // the whole wave
        return;
    const int ntx = tiles_per_row(nx);
    const int nn = 2 * nx + 1;
    const long nplane = nodal_plane((long)nn * (2 * ny + 1));
    const double area = hx * hy;
    const double iarea = 1. / area;
    // lumped masses and their inverses: 4, 2, 2, 1 adjacent elements times LUMP = 1/36, 1/9, 1/9, 4/9 of the cell area
    const double il[4] = { 9. * iarea, 4.5 * iarea, 4.5 * iarea, 2.25 * iarea };
    const double ml[4] = { area / 9., area / 4.5, area / 4.5, area / 2.25 };
    const bool hasB = iy > 0;
    double acc[NSDG_BUDGET_QUANTITIES];
#pragma unroll
    for (int q = 0; q < NSDG_BUDGET_QUANTITIES; ++q)
        acc[q] = 0.;
    for (int ix = blockIdx.x * 64 + threadIdx.x; ix < nx; ix += 64 * (int)gridDim.x) {
        // the gather of mevp_velocity_body (mevp.hip), statement for statement: node sums accumulated in the order below-left, below, left, own
        double s11[8], s12[8], s22[8];
        double cx, cy;
        double divx[4] = { 0., 0., 0., 0. }, divy[4] = { 0., 0., 0., 0. };
        const bool hasL = ix > 0;
        if (hasL && hasB) {
            const long ts = tile_off(ix - 1, iy - 1, ntx, 8);
            tile_load8(S11, ts, s11), tile_load8(S12, ts, s12), tile_load8(S22, ts, s22);
            node_contrib<8>(s11, s12, s22, hx, hy, cx, cy);
            divx[0] += cx, divy[0] += cy;
        }
        if (hasB) {
            const long ts = tile_off(ix, iy - 1, ntx, 8);
            tile_load8(S11, ts, s11), tile_load8(S12, ts, s12), tile_load8(S22, ts, s22);
            node_contrib<6>(s11, s12, s22, hx, hy, cx, cy);
            divx[0] += cx, divy[0] += cy;
            node_contrib<7>(s11, s12, s22, hx, hy, cx, cy);
            divx[1] += cx, divy[1] += cy;
        }
        if (hasL) {
            const long ts = tile_off(ix - 1, iy, ntx, 8);
            tile_load8(S11, ts, s11), tile_load8(S12, ts, s12), tile_load8(S22, ts, s22);
            node_contrib<2>(s11, s12, s22, hx, hy, cx, cy);
            divx[0] += cx, divy[0] += cy;
            node_contrib<5>(s11, s12, s22, hx, hy, cx, cy);
            divx[2] += cx, divy[2] += cy;
        }
        {
            const long ts = tile_off(ix, iy, ntx, 8);
            tile_load8(S11, ts, s11), tile_load8(S12, ts, s12), tile_load8(S22, ts, s22);
            node_contrib<0>(s11, s12, s22, hx, hy, cx, cy);
            divx[0] += cx, divy[0] += cy;
            node_contrib<1>(s11, s12, s22, hx, hy, cx, cy);
            divx[1] += cx, divy[1] += cy;
            node_contrib<3>(s11, s12, s22, hx, hy, cx, cy);
            divx[2] += cx, divy[2] += cy;
            node_contrib<4>(s11, s12, s22, hx, hy, divx[3], divy[3]);
        }
        const long nV = (long)(2 * iy) * nn + 2 * ix; // vertex; EX = nV+1; EY = nV+nn; C = nV+nn+1
        // the Dirichlet nodes of the lattice edge: where mevp_velocity_body writes its zeros
        const bool dirichlet[4] = { !(hasL && hasB), !hasB, !hasL, false };
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ox = k & 1, oy = k >> 1;
            const long n = nV + oy * nn + ox;
            double f[16], m = 0., uu = 0., vv = 0.;
            if (dirichlet[k]) {
#pragma unroll
                for (int t = 0; t < 16; ++t)
                    f[t] = 0.;
            } else
                budget_node(B, nx, ny, 2 * ix + ox, 2 * iy + oy, n, nplane, divx[k], divy[k], il[k], A, ua, va, u, v, packed, ssh, hx, hy, f, m, uu, vv);
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (out.p[t]) // uniform over the launch
                    NSDG_BUDGET_STORE(out.p[t] + n, f[t]);
            if (power) {
#pragma unroll
                for (int t = 0; t < NSDG_BUDGET_TERMS; ++t) {
                    const double pa = uu * f[2 * t];
                    const double pb = vv * f[2 * t + 1];
                    const double ps = pa + pb;
                    const double p = ml[k] * ps;
                    acc[t] = acc[t] + p;
                }
                const double qa = uu * uu;
                const double qb = vv * vv;
                const double qs = qa + qb;
                const double e = m * qs;
                const double eh = 0.5 * e;
                const double ke = ml[k] * eh;
                acc[NSDG_BUDGET_KE] = acc[NSDG_BUDGET_KE] + ke;
            }
        }
        // the zeros of the nodes nobody owns: the right column of the last element column, the top row of the last element row, their corner
        const bool lastcol = ix == nx - 1, toprow = iy == ny - 1;
        if (lastcol || toprow) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                double* __restrict__ p = out.p[t];
                if (!p)
                    continue;
                if (lastcol)
                    p[nV + 2] = 0., p[nV + nn + 2] = 0.;
                if (toprow) {
                    p[nV + 2 * nn] = 0., p[nV + 2 * nn + 1] = 0.;
                    if (lastcol)
                        p[nV + 2 * nn + 2] = 0.;
                }
            }
        }
    }
    if (power) {
        // the lanes folded by halves, p_l = p_l + p_(l + s) for s = 32 ... 1: no LDS, no atomics; lane 0 stores
#pragma unroll
        for (int q = 0; q < NSDG_BUDGET_QUANTITIES; ++q) {
            double r = acc[q];
            for (int s = 32; s >= 1; s >>= 1) {
                const double other = __shfl_down(r, s, 64);
                r = r + other;
            }
            if (threadIdx.x == 0)
                power[q * power_stride + (iy - row0)] = r;
        }
    }
}

struct byte_range {
    uintptr_t lo, hi;
};
static inline byte_range range_of(const void* p, long doubles) { return { (uintptr_t)p, (uintptr_t)p + (uintptr_t)doubles * sizeof(double) }; }
static inline bool overlap(const byte_range& a, const byte_range& b) { return a.lo < b.hi && b.lo < a.hi; }

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

extern "C" {

int nsdg_budget_term_id(const char* name)
{
    static const char* const names[NSDG_BUDGET_TERMS] = { "wind", "water", "coriolis", "tilt", "internal", "basal", "inertia", "residual" };
    if (!name)
        return -1;
    for (int t = 0; t < NSDG_BUDGET_TERMS; ++t)
        if (!std::strcmp(name, names[t]))
            return t;
    return -1;
}

int nsdg_momentum_budget(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, const double* ua, const double* va,
    const double* s11, const double* s12, const double* s22, const double* u, const double* v, const double* packed, const nsdg_budget_out* out)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && A && ua && va && s11 && s12 && s22 && u && v && packed && out, "null field pointer");
    NSDG_CHECK_TILED(s11, s12, s22);
    NSDG_CHECK_ARG(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    const long nnodes = (long)(2 * ctx->nx + 1) * (2 * ctx->ny + 1), N = (long)ctx->nx * ctx->ny, M = nsdg_tiled_len(ctx->nx, ctx->ny, 8);
    BudgetPlanes planes;
    double* const given[2 * NSDG_BUDGET_TERMS] = { out->wind_x, out->wind_y, out->water_x, out->water_y, out->coriolis_x, out->coriolis_y, out->tilt_x,
        out->tilt_y, out->internal_x, out->internal_y, out->basal_x, out->basal_y, out->inertia_x, out->inertia_y, out->residual_x, out->residual_y };
    // what is read, and what is written: no output may overlap an input, the packing, the sea-surface height or another output
    // (H is not read: it takes no part)
    byte_range reads[12] = { { 0, 0 }, range_of(A, 6 * N), range_of(ua, nnodes), range_of(va, nnodes), range_of(s11, M), range_of(s12, M),
        range_of(s22, M), range_of(u, nnodes), range_of(v, nnodes), range_of(packed, 8 * nnodes), range_of(ctx->ssh, ctx->ssh ? nnodes : 0), { 0, 0 } };
    byte_range writes[2 * NSDG_BUDGET_TERMS + 1];
    int nwrites = 0;
    for (int t = 0; t < 2 * NSDG_BUDGET_TERMS; ++t) {
        planes.p[t] = given[t];
        if (given[t])
            writes[nwrites++] = range_of(given[t], nnodes);
    }
    if (out->power) {
        NSDG_CHECK_ARG(out->power_stride >= j1 - j0, "power_stride is smaller than the number of rows");
        NSDG_CHECK_ARG(out->row0 <= j0 && j1 - out->row0 <= out->power_stride, "the rows [j0, j1) do not lie in [row0, row0 + power_stride)");
        writes[nwrites++] = range_of(out->power, NSDG_BUDGET_QUANTITIES * out->power_stride);
    }
    for (int a = 0; a < nwrites; ++a) {
        for (const byte_range& r : reads)
            NSDG_CHECK_ARG(!overlap(writes[a], r), "an output overlaps an input, packed or the sea-surface height");
        for (int b = 0; b < a; ++b)
            NSDG_CHECK_ARG(!overlap(writes[a], writes[b]), "two outputs overlap");
    }
    if (!(ctx->pack_dt > 0)) {
        nsdg_set_error("nsdg_momentum_budget: no packing on this context (nsdg_mevp_prepare / nsdg_mevp_pack_nodal)");
        return NSDG_ERR_STATE;
    }
    if (j0 == j1 || nwrites == 0)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const nsdg_mevp_params& P = ctx->mevp;
    const BudgetConsts B { P.rho_ice, P.c_atm * P.rho_atm, P.rho_ice * P.fc, ctx->pack_dt, ctx->basal.u0, ctx->gravity, ctx->pack_basal };
    // with totals one wave holds a whole row -- ONE workgroup column, which is what makes the kernel write them --; without, one lane per element
    const dim3 block(64, 4), grid(out->power ? 1 : nsdg_div_up(ctx->nx, 64), nsdg_div_up(j1 - j0, 4));
    hipLaunchKernelGGL(momentum_budget_kernel, grid, block, 0, ctx->stream, B, ctx->nx, ctx->ny, j0, j1, ctx->hx, ctx->hy, A, ua, va, s11, s12, s22, u, v,
        packed, ctx->ssh, planes, out->power, (long)out->power_stride, (int)out->row0);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

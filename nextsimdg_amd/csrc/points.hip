// points.hip -- the model sampled at points: along a drifter's track and at fixed stations (include/nsdg.h "point samples").
//
// What did the buoy see, what passed over the mooring?  Everything a sample needs sits on the device at the end of a step and is local to the
// point's own element: the DG coefficients of thickness, concentration and damage, the 3 x 3 CG2 nodes of the velocity, the eight stress
// coefficients.  One launch, one lane per point, evaluates the requested fields AT THE POINT -- not at the cell centre -- for every point whose
// element lies in the rows [j0, j1) and writes -inf for every other point, so that the elementwise maximum over the launches of a
// decomposition is the whole table: the ownership device of drifters.hip, with the same rule for the element and the same launch shape.  No
// atomics, no LDS; only the point's own element is read, so no ghost row is involved.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "nsdg_internal.h"

namespace {

constexpr int POINTS_BLOCK = 256; // lanes per workgroup, as drifters.hip (abi.POINTS_BLOCK: the tests straddle it)

// what a field list reads: one bit per GROUP of source values of a point's element, so that the kernel loads each value at most once
enum : unsigned {
    RD_H = 1u << 0, RD_A = 1u << 1, RD_D = 1u << 2, // the DG coefficients of the order
    RD_U = 1u << 3, RD_V = 1u << 4, // the 3 x 3 nodes of the element
    RD_S11 = 1u << 5, RD_S12 = 1u << 6, RD_S22 = 1u << 7, // the eight coefficients of a stress component
    RD_HS = 1u << 8, RD_T = 1u << 9
};

const unsigned FIELD_READS[NSDG_HIST_COUNT] = { RD_H, RD_A, RD_U, RD_V, RD_U | RD_V, RD_U | RD_V, RD_U | RD_V, RD_S11 | RD_S22,
    RD_S11 | RD_S12 | RD_S22, RD_HS, RD_T, RD_D };

struct points_grid {
    int nx, ny; // local element array
    int row0, ny_glob; // its placement in the global domain
    double hx, hy;
};

struct points_list {
    int32_t n;
    int32_t id[NSDG_HISTORY_MAX_FIELDS];
};

// rule 1, the rule of drifters.hip: min(n - 1, (int)floor(x / h)) by IEEE division, never below 0 (a NaN gives 0)
__device__ __forceinline__ int locate(double x, double h, int n)
{
    const double f = floor(x / h);
    return f >= (double)(n - 1) ? n - 1 : (f > 0. ? (int)f : 0);
}

// the Lagrange weights of the nodes at -1/2, 0, +1/2 at the local coordinate t, as drifters.hip forms them, and their derivatives
__device__ __forceinline__ void weights(double t, double* w, double* d)
{
    const double s = 2. * t * t;
    w[0] = s - t;
    w[1] = 1. - 2. * s;
    w[2] = s + t;
    d[0] = 4. * t - 1.;
    d[1] = -8. * t;
    d[2] = 4. * t + 1.;
}

// a DG field of 1 / 3 / 6 coefficient planes at (xi, eta): c0 + c1 xi + c2 eta + c3 (xi^2 - 1/12) + c4 (eta^2 - 1/12) + c5 xi eta
__device__ __forceinline__ double dg_value(const double* __restrict__ f, long N, long e, int order, double xi, double eta, double bx, double by)
{
    double s = f[e];
    if (order >= 1) {
        s = s + f[N + e] * xi;
        s = s + f[2 * N + e] * eta;
    }
    if (order >= 2) {
        s = s + f[3 * N + e] * bx;
        s = s + f[4 * N + e] * by;
        s = s + f[5 * N + e] * (xi * eta);
    }
    return s;
}

// a component of the tiled stress at (xi, eta) with all eight basis functions; t: the address of coefficient 0, a[T + 2 l]; the
// coefficients travel in pairs (16-byte aligned by the layout)
__device__ __forceinline__ double stress_value(const double* __restrict__ a, long t, double xi, double eta, double bx, double by)
{
    const double2 c01 = *reinterpret_cast<const double2*>(a + t);
    const double2 c23 = *reinterpret_cast<const double2*>(a + t + 128);
    const double2 c45 = *reinterpret_cast<const double2*>(a + t + 256);
    const double2 c67 = *reinterpret_cast<const double2*>(a + t + 384);
    double s = c01.x;
    s = s + c01.y * xi;
    s = s + c23.x * eta;
    s = s + c23.y * bx;
    s = s + c45.x * by;
    s = s + c45.y * (xi * eta);
    s = s + c67.x * (eta * bx);
    s = s + c67.y * (xi * by);
    return s;
}

__global__ __launch_bounds__(POINTS_BLOCK) void points_sample_kernel(points_grid g, int j0, int j1, int order, long n, const double* __restrict__ px,
    const double* __restrict__ py, unsigned reads, points_list list, nsdg_history_sources src, long out_stride, double* __restrict__ out)
{
    const long stride = (long)gridDim.x * blockDim.x;
    const double ninf = -__builtin_huge_val();
    const long W = 2L * g.nx + 1; // nodes per row of the CG2 lattice
    const long ntx = (g.nx + 63) / 64; // stress tiles per element row
    const long N = (long)g.nx * g.ny; // a coefficient plane of a DG field
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double x = px[i], y = py[i];
        // 1, 2: the element and who owns it
        const int ix = locate(x, g.hx, g.nx), iyg = locate(y, g.hy, g.ny_glob);
        const int iy = iyg - g.row0;
        if (!(iy >= j0 && iy < j1)) {
            for (int k = 0; k < list.n; ++k)
                out[k * out_stride + i] = ninf;
            continue;
        }
        // 3: the local coordinates
        const double xi = x / g.hx - (double)ix - 0.5, eta = y / g.hy - (double)iyg - 0.5;
        const double bx = xi * xi - 1. / 12., by = eta * eta - 1. / 12.;
        const long e = (long)iy * g.nx + ix;
        // 4: every group of sources the list reads is loaded once and reduced to its values at the point (`reads` is uniform over the launch)
        double h = 0., a = 0., d = 0., hs = 0., ti = 0.;
        if (reads & RD_H) h = dg_value(src.H, N, e, order, xi, eta, bx, by);
        if (reads & RD_A) a = dg_value(src.A, N, e, order, xi, eta, bx, by);
        if (reads & RD_D) d = dg_value(src.D, N, e, order, xi, eta, bx, by);
        if (reads & RD_HS) hs = src.hsnow[e];
        if (reads & RD_T) ti = src.tice[e];
        double uu = 0., vv = 0., e11 = 0., e22 = 0., gg = 0.;
        if (reads & (RD_U | RD_V)) {
            double ax[3], dx[3], ay[3], dy[3];
            weights(xi, ax, dx);
            weights(eta, ay, dy);
            const long n0 = 2L * iy * W + 2L * ix;
            double u_x = 0., u_y = 0., v_x = 0., v_y = 0.; // the derivatives in local coordinates
#pragma unroll
            for (int r = 0; r < 3; ++r) { // the rows bottom to top, a row west to east
                if (reads & RD_U) {
                    const double* ur = src.u + n0 + r * W;
                    const double w0 = ur[0], w1 = ur[1], w2 = ur[2];
                    const double su = ax[0] * w0 + ax[1] * w1 + ax[2] * w2;
                    const double du = dx[0] * w0 + dx[1] * w1 + dx[2] * w2;
                    uu = uu + ay[r] * su;
                    u_x = u_x + ay[r] * du;
                    u_y = u_y + dy[r] * su;
                }
                if (reads & RD_V) {
                    const double* vr = src.v + n0 + r * W;
                    const double w0 = vr[0], w1 = vr[1], w2 = vr[2];
                    const double sv = ax[0] * w0 + ax[1] * w1 + ax[2] * w2;
                    const double dv = dx[0] * w0 + dx[1] * w1 + dx[2] * w2;
                    vv = vv + ay[r] * sv;
                    v_x = v_x + ay[r] * dv;
                    v_y = v_y + dy[r] * sv;
                }
            }
            e11 = u_x / g.hx;
            e22 = v_y / g.hy;
            gg = u_y / g.hy + v_x / g.hx;
        }
        double s11 = 0., s12 = 0., s22 = 0.;
        if (reads & (RD_S11 | RD_S12 | RD_S22)) {
            const long t = ((iy * ntx + ix / 64) * 8) * 64 + 2 * (ix % 64);
            if (reads & RD_S11) s11 = stress_value(src.s11, t, xi, eta, bx, by);
            if (reads & RD_S12) s12 = stress_value(src.s12, t, xi, eta, bx, by);
            if (reads & RD_S22) s22 = stress_value(src.s22, t, xi, eta, bx, by);
        }
        for (int k = 0; k < list.n; ++k) {
            double s;
            switch (list.id[k]) {
            case NSDG_HIST_HICE: s = h; break;
            case NSDG_HIST_CICE: s = a; break;
            case NSDG_HIST_U: s = uu; break;
            case NSDG_HIST_V: s = vv; break;
            case NSDG_HIST_SPEED: s = sqrt(uu * uu + vv * vv); break;
            case NSDG_HIST_DIVERGENCE: s = e11 + e22; break;
            case NSDG_HIST_SHEAR: {
                const double dd = e11 - e22;
                s = sqrt(dd * dd + gg * gg);
                break;
            }
            case NSDG_HIST_SIGMA_N: s = 0.5 * (s11 + s22); break;
            case NSDG_HIST_SIGMA_S: {
                const double dd = s11 - s22;
                s = sqrt(0.25 * (dd * dd) + s12 * s12);
                break;
            }
            case NSDG_HIST_HSNOW: s = hs; break;
            case NSDG_HIST_TICE: s = ti; break;
            default: s = d; break; // NSDG_HIST_DAMAGE: the host has checked the ids
            }
            out[k * out_stride + i] = s;
        }
    }
}

// the source pointer a field misses, by name, or null
const char* missing_reads(unsigned r, const nsdg_history_sources& s)
{
    if ((r & RD_H) && !s.H) return "H";
    if ((r & RD_A) && !s.A) return "A";
    if ((r & RD_U) && !s.u) return "u";
    if ((r & RD_V) && !s.v) return "v";
    if ((r & RD_S11) && !s.s11) return "s11";
    if ((r & RD_S12) && !s.s12) return "s12";
    if ((r & RD_S22) && !s.s22) return "s22";
    if ((r & RD_HS) && !s.hsnow) return "hsnow";
    if ((r & RD_T) && !s.tice) return "tice";
    if ((r & RD_D) && !s.D) return "D";
    return nullptr;
}

} // namespace

extern "C" {

int nsdg_points_sample(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t order, int64_t n, const double* x, const double* y, int32_t nfields,
    const int32_t* fields, const nsdg_history_sources* src, int64_t out_stride, double* out)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    NSDG_CHECK_ARG(n >= 0, "n must be >= 0");
    NSDG_CHECK_ARG(nfields >= 1 && nfields <= NSDG_HISTORY_MAX_FIELDS, "nfields must be in [1, NSDG_HISTORY_MAX_FIELDS]");
    NSDG_CHECK_ARG(fields && src, "null pointer");
    points_list list;
    unsigned reads = 0;
    bool seen[NSDG_HIST_COUNT] = {};
    list.n = nfields;
    for (int k = 0; k < nfields; ++k) {
        const int32_t f = fields[k];
        NSDG_CHECK_ARG_IN(__func__, f >= 0 && f < NSDG_HIST_COUNT, "unknown field id %d at position %d", (int)f, k);
        NSDG_CHECK_ARG_IN(__func__, !seen[f], "field '%s' is listed twice", nsdg_history_field_name(f));
        const char* miss = missing_reads(FIELD_READS[f], *src);
        NSDG_CHECK_ARG_IN(__func__, !miss, "field '%s' needs the source %s, which is a null pointer", nsdg_history_field_name(f), miss);
        seen[f] = true;
        reads |= FIELD_READS[f];
        list.id[k] = f;
    }
    for (int k = nfields; k < NSDG_HISTORY_MAX_FIELDS; ++k)
        list.id[k] = 0;
    // stress_value loads the coefficients of the tiled stress in pairs: the components the list reads, and no other
    NSDG_CHECK_TILED((reads & RD_S11) ? src->s11 : nullptr, (reads & RD_S12) ? src->s12 : nullptr, (reads & RD_S22) ? src->s22 : nullptr);
    NSDG_CHECK_ARG(out_stride >= n, "out_stride is smaller than the n points of one field");
    points_grid g;
    g.nx = ctx->nx, g.ny = ctx->ny, g.row0 = ctx->row0;
    g.ny_glob = ctx->ny_global > 0 ? ctx->ny_global : ctx->ny;
    NSDG_CHECK_ARG(g.row0 + ctx->ny <= g.ny_glob, "nsdg_block_set: the local array does not fit into the global row count");
    if (n == 0)
        return NSDG_OK;
    NSDG_CHECK_ARG(x && y && out, "null pointer");
    g.hx = ctx->hx, g.hy = ctx->hy;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    // j0 == j1 is launched too: an empty range owns nothing and says so with -inf in every slot
    const int blocks = (int)std::min<long>(nsdg_div_up(n, POINTS_BLOCK), 1L << 20);
    hipLaunchKernelGGL(points_sample_kernel, dim3((unsigned)blocks), dim3(POINTS_BLOCK), 0, ctx->stream, g, (int)j0, (int)j1, (int)order, (long)n, x, y,
        reads, list, *src, (long)out_stride, out);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

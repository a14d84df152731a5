// drifters.hip -- Lagrangian drifters advected on the device by the ice velocity (include/nsdg.h "drifters").
//
// A drifter is a point (x, y) in global domain coordinates and a status.  One launch moves every drifter whose element lies in the rows
// [j0, j1) of the local array by one Heun step of the biquadratic CG2 velocity and writes -inf for every other drifter, so that the
// elementwise maximum over the launches of a decomposition (nsdg_comm_max_f64_array) is the whole list: who owns a drifter is decided
// from its OLD position by IEEE arithmetic on the global coordinates, the same decision on every rank.  One lane per drifter, no atomics,
// out of place.  Everything a lane reads lies in the 3 x 3 elements around the drifter's own: the predictor is clamped to them.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "nsdg_internal.h"

namespace {

constexpr int DRIFTERS_BLOCK = 256; // lanes per workgroup (abi.DRIFTERS_BLOCK: the tests straddle it)

struct drifter_grid {
    int nx, ny; // local element array
    int row0, ny_glob; // its placement in the global domain
    double hx, hy, Lx, Ly;
};

// rule 1 of the header: the element index of a coordinate, min(n - 1, (int)floor(x / h)) by IEEE division; additionally never below 0
// (a coordinate below 0 or a NaN, which the hosts refuse, must not become an address)
__device__ __forceinline__ int locate(double x, double h, int n)
{
    const double f = floor(x / h);
    return f >= (double)(n - 1) ? n - 1 : (f > 0. ? (int)f : 0);
}

// the three Lagrange weights of the nodes at -1/2, 0, +1/2 at the local coordinate xi
__device__ __forceinline__ void weights(double xi, double& lm, double& l0, double& lp)
{
    const double t = 2. * xi * xi;
    lm = t - xi;
    l0 = 1. - 2. * t;
    lp = t + xi;
}

// rule 5: the biquadratic CG2 velocity of the local element (ix, iy) at (x, y), iyg = the element's global row; the rows bottom to top,
// within a row west to east
__device__ __forceinline__ void velocity(const drifter_grid& g, const double* __restrict__ u, const double* __restrict__ v, int ix, int iy, int iyg,
    double x, double y, double& uu, double& vv)
{
    double ax[3], ay[3];
    weights(x / g.hx - (double)ix - 0.5, ax[0], ax[1], ax[2]);
    weights(y / g.hy - (double)iyg - 0.5, ay[0], ay[1], ay[2]);
    const long W = 2L * g.nx + 1;
    const long n0 = 2L * iy * W + 2L * ix;
    uu = 0., vv = 0.;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double* ur = u + n0 + r * W;
        const double* vr = v + n0 + r * W;
        const double su = ax[0] * ur[0] + ax[1] * ur[1] + ax[2] * ur[2];
        const double sv = ax[0] * vr[0] + ax[1] * vr[1] + ax[2] * vr[2];
        uu = uu + ay[r] * su;
        vv = vv + ay[r] * sv;
    }
}

__global__ __launch_bounds__(DRIFTERS_BLOCK) void drifters_advance_kernel(drifter_grid g, int j0, int j1, double dt, double min_conc, long n,
    const uint8_t* __restrict__ land, const double* __restrict__ u, const double* __restrict__ v, const double* __restrict__ A,
    const double* __restrict__ d_in, double* __restrict__ d_out)
{
    const long stride = (long)gridDim.x * blockDim.x;
    const double ninf = -__builtin_huge_val();
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double x = d_in[i], y = d_in[n + i], st = d_in[2 * n + i];
        // 1, 2: the element and who owns it
        const int ix = locate(x, g.hx, g.nx), iyg = locate(y, g.hy, g.ny_glob);
        const int iy = iyg - g.row0;
        double xo = ninf, yo = ninf, so = ninf;
        if (iy >= j0 && iy < j1) {
            xo = x, yo = y, so = st;
            if (st == 0.) { // 3: a stopped drifter is copied through
                const long e = (long)iy * g.nx + ix;
                if (land && land[e]) // 4: the status at the start
                    so = 3.;
                else if (A[e] < min_conc)
                    so = 2.;
                else {
                    double u1, v1, u2, v2;
                    velocity(g, u, v, ix, iy, iyg, x, y, u1, v1); // 5
                    // 6: the predictor, clamped to the 3 x 3 elements around the drifter's own
                    const int ixa = max(ix - 1, 0), ixb = min(ix + 1, g.nx - 1);
                    const int iya = max(iyg - 1, 0), iyb = min(iyg + 1, g.ny_glob - 1);
                    double xp = x + dt * u1, yp = y + dt * v1;
                    const double xlo = (double)ixa * g.hx, xhi = (double)(ixb + 1) * g.hx;
                    const double ylo = (double)iya * g.hy, yhi = (double)(iyb + 1) * g.hy;
                    xp = xp < xlo ? xlo : (xp > xhi ? xhi : xp);
                    yp = yp < ylo ? ylo : (yp > yhi ? yhi : yp);
                    if (xp != xp) xp = x; // a NaN velocity: the step below stops the drifter, nothing is read out of place
                    if (yp != yp) yp = y;
                    // 7: its element, limited to those 3 x 3 (a predictor on the upper limit is on the closed edge of the last of them)
                    const int ix2 = min(max(locate(xp, g.hx, g.nx), ixa), ixb);
                    const int iyg2 = min(max(locate(yp, g.hy, g.ny_glob), iya), iyb);
                    velocity(g, u, v, ix2, iyg2 - g.row0, iyg2, xp, yp, u2, v2);
                    // 8: Heun
                    const double xn = x + (0.5 * dt) * (u1 + u2);
                    const double yn = y + (0.5 * dt) * (v1 + v2);
                    if (!(0. <= xn && xn <= g.Lx && 0. <= yn && yn <= g.Ly))
                        so = 1.;
                    else
                        xo = xn, yo = yn;
                }
            }
        }
        d_out[i] = xo;
        d_out[n + i] = yo;
        d_out[2 * n + i] = so;
    }
}

} // namespace

extern "C" {

int nsdg_drifters_advance(nsdg_ctx* ctx, int32_t j0, int32_t j1, double dt, double min_conc, int64_t n, const double* u, const double* v,
    const double* A, const double* d_in, double* d_out)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(n >= 0, "n must be >= 0");
    NSDG_CHECK_ARG(std::isfinite(dt) && std::isfinite(min_conc), "dt and min_conc must be finite");
    drifter_grid g;
    g.nx = ctx->nx, g.ny = ctx->ny, g.row0 = ctx->row0;
    g.ny_glob = ctx->ny_global > 0 ? ctx->ny_global : ctx->ny;
    NSDG_CHECK_ARG(g.row0 + ctx->ny <= g.ny_glob, "nsdg_block_set: the local array does not fit into the global row count");
    if (n == 0)
        return NSDG_OK;
    NSDG_CHECK_ARG(u && v && A && d_in && d_out, "null pointer");
    NSDG_CHECK_ARG(d_in != d_out, "d_out must not be d_in: the call is out of place");
    if (j0 < j1) {
        // a drifter of row iy reads the velocity of the rows iy - 1 and iy + 1 where the domain has them
        NSDG_CHECK_ARG_IN(__func__, j0 >= 1 || g.row0 + j0 == 0, "the ghost row below row %d is missing: the range starts at the first row of a local array "
            "that does not start at the domain's first row (row0 = %d)", (int)j0, g.row0);
        NSDG_CHECK_ARG_IN(__func__, j1 <= ctx->ny - 1 || g.row0 + j1 == g.ny_glob, "the ghost row above row %d is missing: the range ends at the last row of a "
            "local array that does not end at the domain's last row (row0 = %d, ny_global = %d)", (int)j1 - 1, g.row0, g.ny_glob);
    }
    g.hx = ctx->hx, g.hy = ctx->hy;
    g.Lx = (double)g.nx * g.hx, g.Ly = (double)g.ny_glob * g.hy;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const int blocks = (int)std::min<long>(nsdg_div_up(n, DRIFTERS_BLOCK), 1L << 20);
    hipLaunchKernelGGL(drifters_advance_kernel, dim3((unsigned)blocks), dim3(DRIFTERS_BLOCK), 0, ctx->stream, g, (int)j0, (int)j1, dt, min_conc, (long)n,
        ctx->land, u, v, A, d_in, d_out);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

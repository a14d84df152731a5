// landmask.hip -- land mask of the dynamics core: coastlines as fixed nodes of the mEVP sub-cycle.
//
// No counterpart in the reference snapshot.  An element mask land[iy * nx + ix] (1 = land) is given on the local array, ghost rows
// included; a CG2 node is a LAND NODE if any element adjacent to it inside the local array is land (mevp_common.h: land_node), and a
// land node holds u = v = 0 in every sub-iteration, exactly as the nodes on the array edge do.  That is all the sub-cycle knows: the
// packing (mevp.hip: pack_node) marks a land node inside the six coefficients the passes load anyway, and the LAND instantiations of
// the passes test the mark.  Nothing else changes: an ocean node has only ocean elements around it, so its nodal means are what they
// were; a coast edge has three land nodes, so no flux crosses it and the unchanged transport keeps land elements that start at
// H = A = 0 at exactly 0.
//
// Here: the mask's registration on the context and the two clears a host applies where values ARRIVE on land from outside the scheme
// (a loaded state, the column step's result): stores of 0 -- not multiplications -- so that a NaN is cleared as well.
#include "mevp_common.h"

namespace nsdg_mevp_detail {

// one lane per element of the rows [j0, j1): f[c * nx * ny + e] = 0 for c < nplanes where e is land
__global__ __launch_bounds__(256) void land_clear_kernel(int nx, int ny, int j0, int j1, int nplanes, const uint8_t* __restrict__ land, double* __restrict__ f)
{
    const int ix = blockIdx.x * 64 + threadIdx.x;
    const int iy = j0 + blockIdx.y * 4 + threadIdx.y;
    if (ix >= nx || iy >= j1)
        return;
    const long N = (long)nx * ny, e = (long)iy * nx + ix;
    if (!land[e])
        return;
    for (int c = 0; c < nplanes; ++c)
        f[c * N + e] = 0.;
}

// one lane per CG2 node of the local array
__global__ __launch_bounds__(256) void land_clear_nodes_kernel(int nx, int ny, const uint8_t* __restrict__ land, double* __restrict__ u, double* __restrict__ v)
{
    const int gx = blockIdx.x * 64 + threadIdx.x;
    const int gy = blockIdx.y * 4 + threadIdx.y;
    const int nn = 2 * nx + 1, nm = 2 * ny + 1;
    if (gx >= nn || gy >= nm)
        return;
    if (!land_node(land, nx, ny, gx, gy))
        return;
    const long n = (long)gy * nn + gx;
    u[n] = 0.;
    v[n] = 0.;
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

extern "C" {

int nsdg_land_mask_set(nsdg_ctx* ctx, const uint8_t* land)
{
    NSDG_NEED_GRID(ctx); // the mask is nx * ny bytes: the shape comes first
    ctx->land = land; // the next packing sees it (or its absence); the passes follow the packing they read (nsdg_ctx.pack_land)
    return NSDG_OK;
}

int nsdg_land_clear(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nplanes, double* f)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(nplanes >= 1, "nplanes must be at least 1");
    NSDG_CHECK_ARG(f != nullptr, "null field pointer");
    if (!ctx->land || j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(ctx->nx, 64), nsdg_div_up(j1 - j0, 4));
    hipLaunchKernelGGL(land_clear_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, j0, j1, nplanes, ctx->land, f);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_land_clear_nodes(nsdg_ctx* ctx, double* u, double* v)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(u && v, "null field pointer");
    if (!ctx->land)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    hipLaunchKernelGGL(land_clear_nodes_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, ctx->land, u, v);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

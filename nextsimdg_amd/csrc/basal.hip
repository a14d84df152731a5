// basal.hip -- landfast ice: grounding on shoals as a basal stress in the momentum update.
//
// No counterpart in the reference snapshot; the scheme is the one of Lemieux et al. (2015, JGR 120; 2016, JGR 121), stated in
// include/nsdg_basal.h.  A static water depth per element of the local array, ghost rows included, gives every CG2 node a critical stress
// T_b (mevp_common.h: basal_critical_stress) at packing time.  The packing (mevp.hip: pack_node) stores it as the seventh of the eight
// packed coefficients a node has room for, and the BASAL instantiations of the passes add C_b = T_b / (|u| + u0) to the denominator of
// the node update (mevp_common.h: node_update).  That is all the sub-cycle knows: no buffer, descriptor or plan changes, and a context
// without a depth array runs the kernels it ran before.
//
// Here: the parameters and the depth array's registration on the context, and the diagnostic T_b.
#include <cmath>

#include "mevp_common.h"

namespace nsdg_mevp_detail {

// one lane per CG2 node of the local array: what the next packing would store in pair 3
template <bool LAND>
__global__ __launch_bounds__(256) void basal_critical_kernel(nsdg_mevp_params P, nsdg_basal_params B, int nx, int ny, const uint8_t* __restrict__ land,
    const double* __restrict__ depth, const double* __restrict__ cgh, const double* __restrict__ cga, double* __restrict__ tb)
{
    const int gx = blockIdx.x * 64 + threadIdx.x;
    const int gy = blockIdx.y * 4 + threadIdx.y;
    const int nn = 2 * nx + 1, nm = 2 * ny + 1;
    if (gx >= nn || gy >= nm)
        return;
    const long n = (long)gy * nn + gx;
    bool is_land = false;
    if constexpr (LAND)
        is_land = land_node(land, nx, ny, gx, gy);
    const double hwn = node_mean_of(nx, ny, gx, gy, [&](int ix, int iy) { return depth[(long)iy * nx + ix]; });
    tb[n] = basal_critical_stress(P, B, cgh[n], cga[n], hwn, is_land);
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

extern "C" {

void nsdg_basal_default_params(nsdg_basal_params* p)
{
    // Lemieux et al. 2015, table 1
    p->k1 = 8.;
    p->k2 = 15.;
    p->alpha_b = 20.;
    p->u0 = 5e-5;
}

int nsdg_basal_params_set(nsdg_ctx* ctx, const nsdg_basal_params* p)
{
    NSDG_CHECK_ARG(ctx && p, "null argument");
    NSDG_CHECK_ARG(std::isfinite(p->k1) && std::isfinite(p->k2) && std::isfinite(p->alpha_b) && std::isfinite(p->u0), "non-finite parameter");
    NSDG_CHECK_ARG(p->k1 > 0. && p->k2 >= 0. && p->alpha_b >= 0. && p->u0 > 0., "need k1 > 0, k2 >= 0, alpha_b >= 0 and u0 > 0");
    ctx->basal = *p; // the next packing stores T_b from them; u0 is a launch constant of the passes (mevp_common.h: nsdg_nodal_consts)
    return NSDG_OK;
}

int nsdg_basal_depth_set(nsdg_ctx* ctx, const double* depth)
{
    NSDG_NEED_GRID(ctx); // the array is nx * ny doubles: the shape comes first
    ctx->depth = depth; // the next packing sees it (or its absence); the passes follow the packing they read (nsdg_ctx.pack_basal)
    return NSDG_OK;
}

int nsdg_basal_critical(nsdg_ctx* ctx, const double* cgh, const double* cga, double* tb)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(cgh && cga && tb, "null field pointer");
    if (!ctx->depth) {
        nsdg_set_error("nsdg_basal_critical: no depth array is set (nsdg_basal_depth_set)");
        return NSDG_ERR_STATE;
    }
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, ctx->mevp, ctx->basal, ctx->nx, ctx->ny, ctx->land, ctx->depth, cgh, cga, tb);
    };
    ctx->land ? launch(basal_critical_kernel<true>) : launch(basal_critical_kernel<false>);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

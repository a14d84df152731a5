// snowload.hip -- snow load: the momentum equation feels the snow's weight.
//
// No counterpart in the reference snapshot; the arithmetic is stated in include/nsdg_snow.h.  A snow field on the context -- the column
// plane hsnow or the DG field S of the column-state transport, on the local array, ghost rows included -- gives every CG2 node that is
// neither land nor ice-free the thickness hl = cgH + (rho_snow / rho_ice) max(cgS, 0) in place of cgH where the packing forms the mass
// (mevp.hip: pack_node, mevp_common.h: snow_loaded_thickness).  That is all the sub-cycle knows: the passes read c[0] = h' as ever, no
// buffer, descriptor, plan or flag of the packing changes, and a context without a field runs the kernels it ran before.
//
// Here: the field's registration on the context, the check the packing calls make of it, and the diagnostic h'.
#include <cmath>

#include "mevp_common.h"

namespace nsdg_mevp_detail {

// one lane per CG2 node of the local array: what the next packing would store as c[0] before its 2^100 scaling
template <bool LAND>
__global__ __launch_bounds__(256) void snow_load_nodal_kernel(nsdg_mevp_params P, int nx, int ny, const uint8_t* __restrict__ land,
    const double* __restrict__ snow, int ncs, double r, const double* __restrict__ cgh, const double* __restrict__ cga, double* __restrict__ hload)
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
    double h = P.h_min; // a land node
    if (!is_land) {
        h = fmax(cgh[n], P.h_min);
        if (!ice_free_node(P, cgh[n], cga[n])) {
            // the nodal mean of the snow: nsdg_dg_to_cg's own function
            h = fmax(snow_loaded_thickness(cgh[n], r, node_average(nx, ny, ncs, snow, gx, gy)), P.h_min);
        }
    }
    hload[n] = h;
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

int nsdg_snow_check_packed(const nsdg_ctx* ctx, const char* fn, const double* packed)
{
    if (!ctx->snow)
        return NSDG_OK;
    const uintptr_t s0 = (uintptr_t)ctx->snow, s1 = s0 + (uintptr_t)ctx->snow_ncoef * ctx->nx * ctx->ny * sizeof(double);
    const uintptr_t p0 = (uintptr_t)packed, p1 = p0 + (uintptr_t)8 * (2 * ctx->nx + 1) * (2 * ctx->ny + 1) * sizeof(double);
    NSDG_CHECK_ARG_IN(fn, s1 <= p0 || p1 <= s0, "the snow field (nsdg_snow_load_set) overlaps packed");
    return NSDG_OK;
}

extern "C" {

int nsdg_snow_load_set(nsdg_ctx* ctx, const double* snow, int32_t ncoef, double rho_snow)
{
    NSDG_NEED_GRID(ctx); // the field is ncoef planes of nx * ny doubles: the shape comes first
    if (!snow) {
        ctx->snow = nullptr; // the next packing launches the instantiations without the load
        return NSDG_OK;
    }
    NSDG_CHECK_ARG(ncoef == 1 || ncoef == 3 || ncoef == 6, "ncoef must be 1, 3 or 6");
    NSDG_CHECK_ARG(std::isfinite(rho_snow) && rho_snow >= 0., "rho_snow must be finite and >= 0");
    ctx->snow = snow;
    ctx->snow_ncoef = ncoef;
    ctx->rho_snow = rho_snow;
    return NSDG_OK;
}

int nsdg_snow_load_nodal(nsdg_ctx* ctx, const double* cgh, const double* cga, double* hload)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(cgh && cga && hload, "null field pointer");
    if (!ctx->snow) {
        nsdg_set_error("nsdg_snow_load_nodal: no snow field is set (nsdg_snow_load_set)");
        return NSDG_ERR_STATE;
    }
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, ctx->mevp, ctx->nx, ctx->ny, ctx->land, ctx->snow, ctx->snow_ncoef, nsdg_snow_ratio(ctx), cgh,
            cga, hload);
    };
    ctx->land ? launch(snow_load_nodal_kernel<true>) : launch(snow_load_nodal_kernel<false>);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

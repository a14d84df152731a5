// tilt.hip -- sea-surface tilt from a sea-surface height.
//
// No counterpart in the reference snapshot; the arithmetic is stated in include/nsdg_tilt.h.  A sea-surface height on the context -- one
// double per CG2 node of the local array, ghost rows included -- makes the packing write the tilt force of a node as -m g grad(eta), from
// the centred difference of mevp_common.h: tilt_gradient, in place of the Coriolis terms of the ocean current (mevp.hip: pack_node).  That
// is all the sub-cycle knows: the passes read c2, c3 as ever, no buffer, descriptor, plan or flag of the packing changes, and a context
// without a field runs the kernels it ran before.
//
// Here: the field's registration on the context, the check the packing calls make of it, the diagnostic gradient, and the height whose
// geostrophic current is the box test's gyre.
#include <cmath>

#include "mevp_common.h"

namespace nsdg_mevp_detail {

// one lane per CG2 node of the local array: the gradient the next packing would use, at every node
__global__ __launch_bounds__(256) void tilt_nodal_kernel(int nx, int ny, double hx, double hy, const double* __restrict__ ssh,
    double* __restrict__ sx, double* __restrict__ sy)
{
    const int gx = blockIdx.x * 64 + threadIdx.x;
    const int gy = blockIdx.y * 4 + threadIdx.y;
    const int nn = 2 * nx + 1, nm = 2 * ny + 1;
    if (gx >= nn || gy >= nm)
        return;
    const long n = (long)gy * nn + gx;
    double dx, dy;
    tilt_gradient(nn, nm, gx, gy, hx, hy, [&](int x, int y) { return ssh[(long)y * nn + x]; }, dx, dy);
    sx[n] = dx;
    sy[n] = dy;
}

// eta = -(fc / g) (0.01 / L) [x (x - L) + y (y - L)] at the nodes of the local array: x, y are the expressions of forcing.hip:
// boxtest_forcing_kernel, so that a row block evaluates what the single domain evaluates, bit for bit
__global__ __launch_bounds__(256) void boxtest_ssh_kernel(int nx, int ny, int row0, int ny_glob, double L, double k, double* __restrict__ ssh)
{
    const int gx = blockIdx.x * 64 + threadIdx.x;
    const int gy = blockIdx.y * 4 + threadIdx.y;
    const int nn = 2 * nx + 1, nm = 2 * ny + 1;
    if (gx >= nn || gy >= nm)
        return;
    const double x = gx * (L / (2 * nx)), y = (gy + 2 * row0) * (L / (2 * ny_glob));
    ssh[(long)gy * nn + gx] = k * (x * (x - L) + y * (y - L));
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

int nsdg_tilt_check_packed(const nsdg_ctx* ctx, const char* fn, const double* packed)
{
    if (!ctx->ssh)
        return NSDG_OK;
    const uintptr_t nodes = (uintptr_t)(2 * ctx->nx + 1) * (2 * ctx->ny + 1);
    const uintptr_t s0 = (uintptr_t)ctx->ssh, s1 = s0 + nodes * sizeof(double);
    const uintptr_t p0 = (uintptr_t)packed, p1 = p0 + 8 * nodes * sizeof(double);
    NSDG_CHECK_ARG_IN(fn, s1 <= p0 || p1 <= s0, "the sea-surface height (nsdg_tilt_set) overlaps packed");
    return NSDG_OK;
}

extern "C" {

int nsdg_tilt_set(nsdg_ctx* ctx, const double* ssh, double gravity)
{
    NSDG_NEED_GRID(ctx); // the field is (2nx+1)(2ny+1) doubles: the shape comes first
    if (!ssh) {
        ctx->ssh = nullptr; // the next packing launches the instantiations without the field: the tilt of the geostrophic current
        return NSDG_OK;
    }
    NSDG_CHECK_ARG(std::isfinite(gravity) && gravity > 0., "gravity must be finite and > 0");
    ctx->ssh = ssh;
    ctx->gravity = gravity;
    return NSDG_OK;
}

int nsdg_tilt_nodal(nsdg_ctx* ctx, double* sx, double* sy)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(sx && sy, "null field pointer");
    if (!ctx->ssh) {
        nsdg_set_error("nsdg_tilt_nodal: no sea-surface height is set (nsdg_tilt_set)");
        return NSDG_ERR_STATE;
    }
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    hipLaunchKernelGGL(tilt_nodal_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, ctx->hx, ctx->hy, ctx->ssh, sx, sy);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_boxtest_ssh(nsdg_ctx* ctx, double domain_size, double fc, double gravity, double* ssh)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(domain_size > 0, "domain size must be positive");
    NSDG_CHECK_ARG(std::isfinite(fc), "fc must be finite");
    NSDG_CHECK_ARG(std::isfinite(gravity) && gravity > 0., "gravity must be finite and > 0");
    NSDG_CHECK_ARG(ssh != nullptr, "null field pointer");
    // where the local array sits in the global domain (nsdg_block_set), as nsdg_boxtest_forcing places it
    const int row0 = ctx->row0, ny_glob = ctx->ny_global > 0 ? ctx->ny_global : ctx->ny;
    NSDG_CHECK_ARG(row0 + ctx->ny <= ny_glob, "nsdg_block_set: the local array does not fit into the global row count");
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    const double k = -(fc / gravity) * (0.01 / domain_size);
    hipLaunchKernelGGL(boxtest_ssh_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, row0, ny_glob, domain_size, k, ssh);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

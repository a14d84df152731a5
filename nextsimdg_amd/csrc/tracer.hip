// tracer.hip -- the column state that rides on the moving ice (include/nsdg.h "column state transport").
//
// The snow volume hsnow is a DG2 field of its own and is advected like H; the surface temperature tice0 is intensive and travels as the
// conserved product Q = H T, weighted by the ice VOLUME H: the ridging cap changes the mean of A but never the mean of H, and the
// Zhang-Shu limiter changes no cell mean, so sum_e mean(H)_e T_e is what the transport conserves.  nsdg_tracer_weight forms Q before the
// step, nsdg_tracer_recover divides the means back after it.  Both are strictly element-local: a host runs them on its ghost rows too
// (redundantly, as the column step), which keeps the ghost rows bit-identical to their owners without a message.
#include <algorithm>
#include <cstdint>

#include "nsdg_internal.h"

namespace {

// one lane per element of rows [e0, e1) (grid-stride): Q[c N + e] = T[e] * H[c N + e] for the NC coefficient planes (all loads of an
// element issued before its stores)
template <int NC>
__global__ __launch_bounds__(256) void tracer_weight_kernel(long e0, long e1, long N, const double* __restrict__ H, const double* __restrict__ T,
    double* __restrict__ Q)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        const double t = T[e];
        double h[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            h[c] = H[c * N + e];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            Q[c * N + e] = t * h[c];
    }
}

// one lane per element: T = mean(Q) / mean(H) where the element holds ice after the step (the ice-free test of the closure, DESIGN
// section 3.3); elsewhere T keeps its value -- the column step ignores it there
__global__ __launch_bounds__(256) void tracer_recover_kernel(long e0, long e1, const double* __restrict__ H, const double* __restrict__ A,
    const double* __restrict__ Q, double min_conc, double min_thick, double* __restrict__ T)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        const double h = H[e], a = A[e];
        if (h > 0. && a >= min_conc && h >= min_thick * a) // false for a NaN in any of them
            T[e] = Q[e] / h;
    }
}

int launch_blocks(const nsdg_ctx* ctx, long n)
{
    // a few workgroups per CU, each lane walking the rows (concentration_max_kernel's shape): the accesses stay coalesced per plane
    return (int)std::min<long>(nsdg_div_up(n, 256), 8L * ctx->num_cus);
}

// the na doubles at a and the nb doubles at b share an address
bool overlap(const double* a, long na, const double* b, long nb) { return a < b + nb && b < a + na; }

} // namespace

extern "C" {

int nsdg_tracer_weight(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, const double* T, double* Q)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && T && Q, "null pointer");
    const long N = (long)ctx->nx * ctx->ny, e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    const long nc = nsdg_nc(order);
    NSDG_CHECK_ARG(!overlap(Q, nc * N, H, nc * N) && !overlap(Q, nc * N, T, N), "Q must not alias or overlap H or T");
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)launch_blocks(ctx, e1 - e0)), block(256);
    nsdg_with_order(order, [&](auto O) {
        hipLaunchKernelGGL(tracer_weight_kernel<nsdg_nc(decltype(O)::value)>, grid, block, 0, ctx->stream, e0, e1, N, H, T, Q);
    });
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_tracer_recover(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, const double* A, const double* Q,
    double min_conc, double min_thick, double* T)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && A && Q && T, "null pointer");
    const long N = (long)ctx->nx * ctx->ny, e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    const long nc = nsdg_nc(order);
    NSDG_CHECK_ARG(!overlap(T, N, H, nc * N) && !overlap(T, N, A, nc * N) && !overlap(T, N, Q, nc * N), "T must not alias or overlap H, A or Q");
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(tracer_recover_kernel, dim3((unsigned)launch_blocks(ctx, e1 - e0)), dim3(256), 0, ctx->stream, e0, e1, H, A, Q, min_conc,
        min_thick, T);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

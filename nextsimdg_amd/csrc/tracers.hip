// tracers.hip -- named tracers that ride on the moving ice (include/nsdg_tracers.h, the "ice tracers" section of include/nsdg.h).
//
// The scheme of tracer.hip for up to NSDG_TRACERS_MAX intensive quantities at once: each travels as the conserved product Q_k = H T_k with
// the ice volume, formed before a transport step (nsdg_tracers_weight) and divided back after it (nsdg_tracers_recover, which also ages the
// tracer of the kind NSDG_TRACER_AGE by dt and clears every tracer where no ice is left).  nsdg_tracers_dilute is the thermodynamic source:
// ice that grows carries the value 0.  All three are element-local, so a host runs them on its ghost rows too.  The planes an element
// shares between its tracers -- the coefficients of H, the means of H and A -- are loaded once and serve all of them.
#include <algorithm>
#include <cstdint>

#include "nsdg_internal.h"

namespace {

template <class P>
struct Planes {
    P p[NSDG_TRACERS_MAX];
};

// one lane per element of rows [e0, e1) (grid-stride): Q_k[c N + e] = T_k[e] * H[c N + e] for the NC coefficient planes and the NT tracers
// (all loads of an element issued before its stores; the NC loads of H serve the NT tracers)
template <int NC, int NT>
__global__ __launch_bounds__(256) void tracers_weight_kernel(long e0, long e1, long N, const double* __restrict__ H, Planes<const double*> T,
    Planes<double*> Q)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        double t[NT], h[NC];
#pragma unroll
        for (int k = 0; k < NT; ++k)
            t[k] = T.p[k][e];
#pragma unroll
        for (int c = 0; c < NC; ++c)
            h[c] = H[c * N + e];
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int c = 0; c < NC; ++c)
                Q.p[k][c * N + e] = t[k] * h[c];
    }
}

// one lane per element: the ice test of tracer_recover_kernel on the means of H and A (loaded once); where it holds T_k = mean(Q_k) / mean(H),
// plus dt for the ageing kind; elsewhere T_k = 0
template <int NT>
__global__ __launch_bounds__(256) void tracers_recover_kernel(long e0, long e1, const double* __restrict__ H, const double* __restrict__ A,
    Planes<const double*> Q, Planes<int> kind, double dt, double min_conc, double min_thick, Planes<double*> T)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        const double h = H[e], a = A[e];
        double t[NT];
        if (h > 0. && a >= min_conc && h >= min_thick * a) { // false for a NaN in any of them
            double q[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k)
                q[k] = Q.p[k][e];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const double r = q[k] / h;
                t[k] = kind.p[k] == NSDG_TRACER_AGE ? r + dt : r;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NT; ++k)
                t[k] = 0.;
        }
#pragma unroll
        for (int k = 0; k < NT; ++k)
            T.p[k][e] = t[k];
    }
}

// one lane per element: growth from hb = max(h_before, 0) to ha > hb mixes the tracer with new ice of the value 0; no ice afterwards: 0
template <int NT>
__global__ __launch_bounds__(256) void tracers_dilute_kernel(long e0, long e1, const double* __restrict__ h_before,
    const double* __restrict__ h_after, Planes<double*> T)
{
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        const double b = h_before[e], ha = h_after[e];
        const double hb = b > 0. ? b : 0.; // (a NaN counts as no ice before)
        if (!(ha > 0.)) {
#pragma unroll
            for (int k = 0; k < NT; ++k)
                T.p[k][e] = 0.;
        } else if (ha > hb) {
            double t[NT];
#pragma unroll
            for (int k = 0; k < NT; ++k)
                t[k] = T.p[k][e];
#pragma unroll
            for (int k = 0; k < NT; ++k) {
                const double m = t[k] * hb;
                T.p[k][e] = m / ha;
            }
        }
    }
}

// the launch shape of tracer.hip's launch_blocks: a few workgroups per CU, each lane walking the rows, coalesced per plane
int launch_blocks(const nsdg_ctx* ctx, long n) { return (int)std::min<long>(nsdg_div_up(n, 256), 8L * ctx->num_cus); }

// the na doubles at a and the nb doubles at b share an address
bool overlap(const double* a, long na, const double* b, long nb) { return a < b + nb && b < a + na; }

// f(std::integral_constant<int, n>) for a checked 1 <= n <= NSDG_TRACERS_MAX
template <class F>
void with_count(int n, F&& f)
{
    switch (n) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 4>());
    }
}
static_assert(NSDG_TRACERS_MAX == 4, "with_count lists the tracer counts");

template <class P, class S>
Planes<P> planes(S* const* src, int n)
{
    Planes<P> out {};
    for (int k = 0; k < n; ++k)
        out.p[k] = src[k];
    return out;
}

} // namespace

#define TRACERS_COMMON_CHECKS()                                                                            \
    NSDG_NEED_GRID(ctx);                                                                                   \
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");             \
    NSDG_CHECK_ARG(n >= 1 && n <= NSDG_TRACERS_MAX, "the number of tracers must be 1 .. NSDG_TRACERS_MAX")

extern "C" {

int nsdg_tracers_weight(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, int32_t n, const double* const* T,
    double* const* Q)
{
    TRACERS_COMMON_CHECKS();
    NSDG_CHECK_ARG(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    NSDG_CHECK_ARG(H && T && Q, "null pointer");
    for (int k = 0; k < n; ++k)
        NSDG_CHECK_ARG(T[k] && Q[k], "null pointer");
    const long N = (long)ctx->nx * ctx->ny, e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    const long nc = nsdg_nc(order);
    for (int k = 0; k < n; ++k) {
        NSDG_CHECK_ARG(!overlap(Q[k], nc * N, H, nc * N), "Q must not alias or overlap H, any T or another Q");
        for (int j = 0; j < n; ++j)
            NSDG_CHECK_ARG(!overlap(Q[k], nc * N, T[j], N) && (j == k || !overlap(Q[k], nc * N, Q[j], nc * N)),
                "Q must not alias or overlap H, any T or another Q");
    }
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)launch_blocks(ctx, e1 - e0)), block(256);
    const auto t = planes<const double*>(T, n);
    const auto q = planes<double*>(Q, n);
    nsdg_with_order(order, [&](auto O) {
        with_count(n, [&](auto NT) {
            hipLaunchKernelGGL((tracers_weight_kernel<nsdg_nc(decltype(O)::value), decltype(NT)::value>), grid, block, 0, ctx->stream, e0, e1, N, H, t,
                q);
        });
    });
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_tracers_recover(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, const double* A, int32_t n,
    const double* const* Q, const int32_t* kind, double dt, double min_conc, double min_thick, double* const* T)
{
    TRACERS_COMMON_CHECKS();
    NSDG_CHECK_ARG(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    NSDG_CHECK_ARG(H && A && Q && kind && T, "null pointer");
    for (int k = 0; k < n; ++k) {
        NSDG_CHECK_ARG(Q[k] && T[k], "null pointer");
        NSDG_CHECK_ARG(kind[k] == NSDG_TRACER_PASSIVE || kind[k] == NSDG_TRACER_AGE, "unknown tracer kind");
    }
    const long N = (long)ctx->nx * ctx->ny, e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    const long nc = nsdg_nc(order);
    for (int k = 0; k < n; ++k) {
        NSDG_CHECK_ARG(!overlap(T[k], N, H, nc * N) && !overlap(T[k], N, A, nc * N), "T must not alias or overlap H, A, any Q or another T");
        for (int j = 0; j < n; ++j)
            NSDG_CHECK_ARG(!overlap(T[k], N, Q[j], nc * N) && (j == k || !overlap(T[k], N, T[j], N)),
                "T must not alias or overlap H, A, any Q or another T");
    }
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)launch_blocks(ctx, e1 - e0)), block(256);
    const auto q = planes<const double*>(Q, n);
    const auto t = planes<double*>(T, n);
    Planes<int> kinds {};
    for (int k = 0; k < n; ++k)
        kinds.p[k] = kind[k];
    with_count(n, [&](auto NT) {
        hipLaunchKernelGGL(tracers_recover_kernel<decltype(NT)::value>, grid, block, 0, ctx->stream, e0, e1, H, A, q, kinds, dt, min_conc, min_thick,
            t);
    });
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_tracers_dilute(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* h_before, const double* h_after, int32_t n, double* const* T)
{
    TRACERS_COMMON_CHECKS();
    NSDG_CHECK_ARG(h_before && h_after && T, "null pointer");
    for (int k = 0; k < n; ++k)
        NSDG_CHECK_ARG(T[k], "null pointer");
    const long N = (long)ctx->nx * ctx->ny, e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    for (int k = 0; k < n; ++k) {
        NSDG_CHECK_ARG(!overlap(T[k], N, h_before, N) && !overlap(T[k], N, h_after, N), "T must not alias or overlap h_before, h_after or another T");
        for (int j = 0; j < k; ++j)
            NSDG_CHECK_ARG(!overlap(T[k], N, T[j], N), "T must not alias or overlap h_before, h_after or another T");
    }
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)launch_blocks(ctx, e1 - e0)), block(256);
    const auto t = planes<double*>(T, n);
    with_count(n, [&](auto NT) {
        hipLaunchKernelGGL(tracers_dilute_kernel<decltype(NT)::value>, grid, block, 0, ctx->stream, e0, e1, h_before, h_after, t);
    });
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

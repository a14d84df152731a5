// substep.hip -- the model time step split by the ice's own strength wave speed (include/nsdg.h "sub-stepping").
//
// The explicit coupling of ice strength and transport (Lipscomb et al. 2007) goes unstable when the plastic wave
// speed crosses more than about 1.5 cells per step (profiles/r06_adaptive_noise.md).  The wave speed is a function of
// the local concentration only, c^2 = (1 + C a) P* exp(-C (1 - a)) / (2 rho_ice), monotone in a: the largest c of a
// state is c(max a).  nsdg_concentration_max measures max a on the device (one launch, one 8-byte result),
// nsdg_substep_count turns it into a number of sub-steps (host only).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "dg_tables.h"
#include "mevp_common.h"
#include "nsdg_internal.h"

namespace {

using namespace nsdg_mevp_detail;

// The result slot holds the bit pattern of a non-negative double: for those the unsigned order of the patterns is the
// order of the values, so atomicMax on the pattern is the exact maximum whatever the order of the workgroups.  A
// non-finite input is reported in the same slot as a negative quiet NaN carrying the element index in its payload:
// 0xFFF8... is above every non-negative double's pattern, so it survives the maximum (the largest bad index wins).
constexpr unsigned long long BAD_MARK = 0xFFF8000000000000ull;
constexpr unsigned long long BAD_INDEX_MASK = (1ull << 51) - 1;

// one lane per element of the owned rows (grid-stride); the clamped concentration at the 9 Gauss points (mevp_common.h:
// gauss_thickness_conc, clamp_thickness_conc: what ice_strength_kernel sees), counted where the clamped thickness there is > 0
__global__ __launch_bounds__(256) void concentration_max_kernel(long e0, long e1, long N, const double* __restrict__ H,
    const double* __restrict__ A, unsigned long long* __restrict__ out)
{
    unsigned long long best = 0; // +0.0
    const long stride = (long)gridDim.x * blockDim.x;
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        double hc[6], ac[6];
        plane_load6(H, N, e, hc);
        plane_load6(A, N, e, ac);
        bool finite = true;
#pragma unroll
        for (int c = 0; c < 6; ++c)
            finite = finite && std::isfinite(hc[c]) && std::isfinite(ac[c]);
        double amax = 0.;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            double h, a;
            gauss_thickness_conc(q, hc, ac, h, a);
            // the raw values are checked BEFORE the clamp: fmax(NaN, 0) is 0
            finite = finite && std::isfinite(h) && std::isfinite(a);
            clamp_thickness_conc(h, a);
            if (h > 0. && a > amax) // only positive values enter: the pattern of -0 would be read as a bad mark
                amax = a;
        }
        const unsigned long long v = finite ? (unsigned long long)__double_as_longlong(amax) : (BAD_MARK | ((unsigned long long)e & BAD_INDEX_MASK));
        best = v > best ? v : best;
    }
    // wave64 maximum with cross-lane moves, then one partial per workgroup
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(best, m, 64);
        best = o > best ? o : best;
    }
    __shared__ unsigned long long part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        part[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = part[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            b = part[w] > b ? part[w] : b;
        if (b != 0)
            atomicMax(out, b);
    }
}

} // namespace

extern "C" {

int nsdg_concentration_max(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* amax_host)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && A && amax_host, "null pointer");
    *amax_host = 0.;
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(ctx->scalar_dev);
    const long N = (long)ctx->nx * ctx->ny, e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    // a few workgroups per CU, each lane walking the rows: few atomics on the one slot, the reads stay coalesced per plane
    const long blocks = std::min<long>(nsdg_div_up(e1 - e0, 256), 4L * ctx->num_cus);
    NSDG_CHECK_HIP(hipMemsetAsync(slot, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(concentration_max_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, e0, e1, N, H, A, slot);
    NSDG_CHECK_LAUNCH();
    NSDG_CHECK_HIP(hipMemcpyAsync(ctx->scalar_host, slot, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->comm) { // a dead neighbour must give an error status, never a hang
        const int rc = nsdg_comm_bounded_drain(ctx);
        if (rc != NSDG_OK)
            return rc;
    } else
        NSDG_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    unsigned long long bits;
    std::memcpy(&bits, ctx->scalar_host, sizeof bits);
    if ((bits & BAD_MARK) == BAD_MARK) {
        const long e = (long)(bits & BAD_INDEX_MASK);
        nsdg_set_error("nsdg_concentration_max: non-finite H or A in element %ld (ix %ld, iy %ld of the local array)", e, e % ctx->nx, e / ctx->nx);
        return NSDG_ERR_ARG;
    }
    double a;
    std::memcpy(&a, &bits, sizeof a);
    *amax_host = a;
    return NSDG_OK;
}

int nsdg_substep_count(const nsdg_mevp_params* p, double amax, double h, double dt, double courant, int32_t max_substeps, int32_t* n, double* c)
{
    NSDG_CHECK_ARG(p && n, "null argument");
    NSDG_CHECK_ARG(std::isfinite(amax) && amax >= 0. && amax <= 1., "amax must be a concentration in [0, 1]");
    NSDG_CHECK_ARG(std::isfinite(h) && h > 0. && std::isfinite(dt) && dt > 0. && std::isfinite(courant) && courant > 0.,
        "cell size, time step and courant must be finite and positive");
    NSDG_CHECK_ARG(std::isfinite(p->pstar) && p->pstar > 0. && std::isfinite(p->rho_ice) && p->rho_ice > 0. && std::isfinite(p->compaction)
            && p->compaction >= 0.,
        "pstar and rho_ice must be positive, compaction >= 0");
    NSDG_CHECK_ARG(max_substeps >= 1, "max_substeps must be >= 1");
    const double C = p->compaction;
    const double speed = std::sqrt((1. + C * amax) * p->pstar * std::exp(-C * (1. - amax)) / (2. * p->rho_ice));
    if (c)
        *c = speed;
    const double need = std::max(1., std::ceil(speed * dt / (courant * h)));
    if (!(need <= (double)max_substeps)) {
        nsdg_set_error("nsdg_substep_count: the wave speed %.6g m/s (max concentration %.17g) crosses %.6g cells per step of %g s on cells of %g m: "
                       "that needs n = %.0f sub-steps at courant %g, more than max_substeps = %d",
            speed, amax, speed * dt / h, dt, h, need, courant, (int)max_substeps);
        return NSDG_ERR_ARG;
    }
    *n = (int32_t)need;
    return NSDG_OK;
}

} // extern "C"

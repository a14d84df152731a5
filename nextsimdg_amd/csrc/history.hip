// history.hip -- history output accumulated on the device (include/nsdg.h "history output").
//
// The fields people look at -- mean thickness and concentration, drift, deformation rates, stress invariants, damage -- are element-local
// functions of arrays that sit on the device at the end of every model step.  One streaming launch per step adds (or stores) one sample of
// every requested field into accumulator planes the host owns; the host downloads them once per output window and divides by the count.
// The accumulation of an element is sequential in time and touches nothing but that element's own samples, so a mean does not depend on the
// row range, the strip or the decomposition the samples were taken under.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "nsdg_internal.h"

namespace {

const char* const FIELD_NAMES[NSDG_HIST_COUNT] = { "hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s", "hsnow", "tice",
    "damage" };

// what a field list reads: one bit per source VALUE of an element, so that the kernel loads each of them at most once
enum : unsigned {
    RD_H = 1u << 0, RD_A = 1u << 1, RD_UC = 1u << 2, RD_VC = 1u << 3, // cell means of H and A; u, v at the centre node
    RD_UEW = 1u << 4, RD_VNS = 1u << 5, RD_UNS = 1u << 6, RD_VEW = 1u << 7, // the mid-edge nodes east / west and north / south
    RD_S11 = 1u << 8, RD_S12 = 1u << 9, RD_S22 = 1u << 10, RD_HS = 1u << 11, RD_T = 1u << 12, RD_D = 1u << 13
};

const unsigned FIELD_READS[NSDG_HIST_COUNT] = { RD_H, RD_A, RD_UC, RD_VC, RD_UC | RD_VC, RD_UEW | RD_VNS, RD_UEW | RD_VNS | RD_UNS | RD_VEW,
    RD_S11 | RD_S22, RD_S11 | RD_S12 | RD_S22, RD_HS, RD_T, RD_D };

struct history_list {
    int32_t n;
    int32_t id[NSDG_HISTORY_MAX_FIELDS];
};

// one lane per element of rows [e0 / nx, e1 / nx) (grid-stride): every source value the list needs is loaded once (`reads` is uniform over
// the launch), then one sample per field is stored into / added to its accumulator plane.  The samples are the header's, to the letter.
__global__ __launch_bounds__(256) void history_accumulate_kernel(long e0, long e1, int nx, double hx, double hy, unsigned reads, history_list list,
    nsdg_history_sources src, int store, long acc0, long plane_stride, double* __restrict__ acc)
{
    const long stride = (long)gridDim.x * blockDim.x;
    const long W = 2L * nx + 1; // nodes per row of the CG2 lattice
    const long ntx = (nx + 63) / 64; // stress tiles per element row
    for (long e = e0 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < e1; e += stride) {
        const long iy = e / nx;
        const long ix = e - iy * nx;
        const long n = (2 * iy + 1) * W + 2 * ix + 1; // the centre node
        const long t = ((iy * ntx + ix / 64) * 8) * 64 + 2 * (ix % 64); // coefficient 0 of the tiled stress: a[T + 2 l]
        double h = 0., a = 0., uc = 0., vc = 0., uE = 0., uW = 0., vN = 0., vS = 0., uN = 0., uS = 0., vE = 0., vW = 0.;
        double s11 = 0., s12 = 0., s22 = 0., hs = 0., ti = 0., d = 0.;
        if (reads & RD_H) h = src.H[e];
        if (reads & RD_A) a = src.A[e];
        if (reads & RD_UC) uc = src.u[n];
        if (reads & RD_VC) vc = src.v[n];
        if (reads & RD_UEW) { uE = src.u[n + 1]; uW = src.u[n - 1]; }
        if (reads & RD_VNS) { vN = src.v[n + W]; vS = src.v[n - W]; }
        if (reads & RD_UNS) { uN = src.u[n + W]; uS = src.u[n - W]; }
        if (reads & RD_VEW) { vE = src.v[n + 1]; vW = src.v[n - 1]; }
        if (reads & RD_S11) s11 = src.s11[t];
        if (reads & RD_S12) s12 = src.s12[t];
        if (reads & RD_S22) s22 = src.s22[t];
        if (reads & RD_HS) hs = src.hsnow[e];
        if (reads & RD_T) ti = src.tice[e];
        if (reads & RD_D) d = src.D[e];
        const double e11 = (uE - uW) / hx, e22 = (vN - vS) / hy;
        double* out = acc + (e - acc0);
        for (int k = 0; k < list.n; ++k) {
            double x;
            switch (list.id[k]) {
            case NSDG_HIST_HICE: x = h; break;
            case NSDG_HIST_CICE: x = a; break;
            case NSDG_HIST_U: x = uc; break;
            case NSDG_HIST_V: x = vc; break;
            case NSDG_HIST_SPEED: x = sqrt(uc * uc + vc * vc); break;
            case NSDG_HIST_DIVERGENCE: x = e11 + e22; break;
            case NSDG_HIST_SHEAR: {
                const double g = (uN - uS) / hy + (vE - vW) / hx, dd = e11 - e22;
                x = sqrt(dd * dd + g * g);
                break;
            }
            case NSDG_HIST_SIGMA_N: x = 0.5 * (s11 + s22); break;
            case NSDG_HIST_SIGMA_S: {
                const double dd = s11 - s22;
                x = sqrt(0.25 * (dd * dd) + s12 * s12);
                break;
            }
            case NSDG_HIST_HSNOW: x = hs; break;
            case NSDG_HIST_TICE: x = ti; break;
            default: x = d; break; // NSDG_HIST_DAMAGE: the host has checked the ids
            }
            double* p = out + k * plane_stride;
            *p = store ? x : *p + x; // store: a NaN left in acc is dropped, no memset is needed
        }
    }
}

// the source pointer a field misses, by name, or null
const char* missing_source(int32_t field, const nsdg_history_sources& s)
{
    const unsigned r = FIELD_READS[field];
    if ((r & RD_H) && !s.H) return "H";
    if ((r & RD_A) && !s.A) return "A";
    if ((r & (RD_UC | RD_UEW | RD_UNS)) && !s.u) return "u";
    if ((r & (RD_VC | RD_VNS | RD_VEW)) && !s.v) return "v";
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

const char* nsdg_history_field_name(int32_t field)
{
    return field >= 0 && field < NSDG_HIST_COUNT ? FIELD_NAMES[field] : nullptr;
}

int nsdg_history_field_id(const char* name)
{
    if (name)
        for (int f = 0; f < NSDG_HIST_COUNT; ++f)
            if (!std::strcmp(name, FIELD_NAMES[f]))
                return f;
    return -1;
}

int nsdg_history_accumulate(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nfields, const int32_t* fields, const nsdg_history_sources* src,
    int32_t store, int32_t row0, int64_t plane_stride, double* acc)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(nfields >= 1 && nfields <= NSDG_HISTORY_MAX_FIELDS, "nfields must be in [1, NSDG_HISTORY_MAX_FIELDS]");
    NSDG_CHECK_ARG(fields && src && acc, "null pointer");
    history_list list;
    unsigned reads = 0, seen = 0;
    list.n = nfields;
    for (int k = 0; k < nfields; ++k) {
        const int32_t f = fields[k];
        NSDG_CHECK_ARG_IN(__func__, f >= 0 && f < NSDG_HIST_COUNT, "unknown field id %d at position %d", (int)f, k);
        NSDG_CHECK_ARG_IN(__func__, !(seen & (1u << f)), "field '%s' is listed twice", FIELD_NAMES[f]);
        const char* miss = missing_source(f, *src);
        NSDG_CHECK_ARG_IN(__func__, !miss, "field '%s' needs the source %s, which is a null pointer", FIELD_NAMES[f], miss);
        seen |= 1u << f;
        reads |= FIELD_READS[f];
        list.id[k] = f;
    }
    for (int k = nfields; k < NSDG_HISTORY_MAX_FIELDS; ++k)
        list.id[k] = 0;
    NSDG_CHECK_ARG(0 <= row0 && row0 <= j0, "row0 must be in [0, j0]: the accumulator starts at or below the first row of the range");
    NSDG_CHECK_ARG(plane_stride >= ((int64_t)j1 - row0) * ctx->nx, "plane_stride is smaller than the rows [row0, j1) of one accumulator plane");
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const long e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    // the launch shape of tracer.hip: a few workgroups per CU, each lane walking the rows
    const int blocks = (int)std::min<long>(nsdg_div_up(e1 - e0, 256), 8L * ctx->num_cus);
    hipLaunchKernelGGL(history_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, e0, e1, ctx->nx, ctx->hx, ctx->hy, reads, list,
        *src, (int)(store != 0), (long)row0 * ctx->nx, (long)plane_stride, acc);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

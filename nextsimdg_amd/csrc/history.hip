// history.hip -- history output accumulated on the device (include/nsdg.h "history output").
//
// The fields people look at -- mean thickness and concentration, drift, deformation rates, stress invariants, damage -- are element-local
// functions of arrays that sit on the device at the end of every model step.  One streaming launch per step adds (or stores) one sample of
// every requested field into accumulator planes the host owns; the host downloads them once per output window and divides by the count.
// The accumulation of an element is sequential in time and touches nothing but that element's own samples, so a mean does not depend on the
// row range, the strip or the decomposition the samples were taken under.
//
// Two additions keep that property.  nsdg_history_accumulate_stats is the same launch with a statistic per plane: the plain sum, the sum
// weighted by the clamped concentration (with one plane of summed weights beside it), and the minimum and the maximum of the window.
// nsdg_history_row_totals reduces every row of the array to a handful of scalars -- ice area, extent, volume, drift -- with ONE wave64 per
// row in a fixed order of additions, so that a row's total depends on the row's values alone and the host can add the rows of any
// decomposition in global row order.
#include <algorithm>
#include <cmath>
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

const char* const STAT_NAMES[NSDG_STAT_COUNT] = { "mean", "ice_mean", "min", "max" };
const char* const SERIES_NAMES[NSDG_SERIES_COUNT] = { "area", "extent", "volume", "snow_volume", "drift", "speed_max", "hice_max" };
const unsigned SERIES_READS[NSDG_SERIES_COUNT] = { RD_A, RD_A, RD_H, RD_HS, RD_A | RD_UC | RD_VC, RD_UC | RD_VC, RD_H };

const unsigned FIELD_READS[NSDG_HIST_COUNT] = { RD_H, RD_A, RD_UC, RD_VC, RD_UC | RD_VC, RD_UEW | RD_VNS, RD_UEW | RD_VNS | RD_UNS | RD_VEW,
    RD_S11 | RD_S22, RD_S11 | RD_S12 | RD_S22, RD_HS, RD_T, RD_D };

struct history_list {
    int32_t n;
    int32_t id[NSDG_HISTORY_MAX_FIELDS];
};

// the statistic of every plane of a history_list (all NSDG_STAT_MEAN under nsdg_history_accumulate, which does not read it)
struct history_stats {
    int32_t stat[NSDG_HISTORY_MAX_FIELDS];
    int32_t weighted; // some plane is NSDG_STAT_ICE_MEAN: the weight plane is written
};

// the weight of an ice-weighted mean and the ice area of an element: the concentration clamped to [0, 1]; a NaN stays a NaN
__device__ __forceinline__ double ice_weight(double a) { return a < 0. ? 0. : (a > 1. ? 1. : a); }

// one lane per element of rows [e0 / nx, e1 / nx) (grid-stride): every source value the list needs is loaded once (`reads` is uniform over
// the launch), then one sample per field is stored into / added to its accumulator plane.  The samples are the header's, to the letter.
// STATS: every plane has a statistic of its own (nsdg_history_accumulate_stats); without it the kernel is the plain sum it always was.
template <bool STATS>
__global__ __launch_bounds__(256) void history_accumulate_kernel(long e0, long e1, int nx, double hx, double hy, unsigned reads, history_list list,
    history_stats stats, nsdg_history_sources src, int store, long acc0, long plane_stride, double* __restrict__ acc, double* __restrict__ wacc)
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
            if (!STATS) {
                *p = store ? x : *p + x; // store: a NaN left in acc is dropped, no memset is needed
                continue;
            }
            switch (stats.stat[k]) {
            case NSDG_STAT_MEAN: *p = store ? x : *p + x; break;
            case NSDG_STAT_ICE_MEAN: {
                const double wx = ice_weight(a) * x; // rounded as a statement of its own: never fused into the sum
                *p = store ? wx : *p + wx;
                break;
            }
            case NSDG_STAT_MIN: {
                const double m = *p;
                *p = (store || x < m || x != x) ? x : m; // a NaN sample makes the extreme NaN, and it stays: nothing compares below a NaN
                break;
            }
            default: { // NSDG_STAT_MAX: the host has checked the ids
                const double m = *p;
                *p = (store || x > m || x != x) ? x : m;
                break;
            }
            }
        }
        if (STATS && stats.weighted) {
            const double w = ice_weight(a);
            double* p = wacc + (e - acc0);
            *p = store ? w : *p + w;
        }
    }
}

// the NaN-propagating maximum of the row totals, the MAX statistic's own rule: (a, b) -> b where b is larger or a NaN
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }

struct series_list {
    int32_t slot[NSDG_SERIES_COUNT]; // quantity id -> its position in the caller's list, -1: not asked for
};

// One wave64 per row, four rows per workgroup, grid-stride over the rows [j0, j1).  The order is the header's: lane l folds the elements
// ix = l, l + 64, ... in ascending order from the identity, then the lanes are folded by halves, p_l = op(p_l, p_(l + s)) for s = 32 ... 1
// (__shfl_down: no LDS, no atomics), and lane 0 stores.  Every term is a statement of its own, so no product is fused into a sum.
__global__ __launch_bounds__(256) void history_row_totals_kernel(int j0, int j1, int nx, unsigned reads, series_list list, nsdg_history_sources src,
    double extent_conc, int row0, long q_stride, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int rows_per_pass = (int)gridDim.x * 4;
    const long W = 2L * nx + 1;
    const double ninf = -__builtin_huge_val();
    for (int iy = j0 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); iy < j1; iy += rows_per_pass) {
        double p[NSDG_SERIES_COUNT] = { 0., 0., 0., 0., 0., ninf, ninf };
        const long e_row = (long)iy * nx, n_row = (2L * iy + 1) * W + 1;
        for (int ix = lane; ix < nx; ix += 64) {
            double h = 0., a = 0., uc = 0., vc = 0., hs = 0.;
            if (reads & RD_H) h = src.H[e_row + ix];
            if (reads & RD_A) a = src.A[e_row + ix];
            if (reads & RD_HS) hs = src.hsnow[e_row + ix];
            if (reads & RD_UC) uc = src.u[n_row + 2 * ix];
            if (reads & RD_VC) vc = src.v[n_row + 2 * ix];
            const double w = ice_weight(a);
            const double speed = sqrt(uc * uc + vc * vc); // the sample of NSDG_HIST_SPEED
            const double in_extent = a >= extent_conc ? 1. : 0.;
            const double vol = h < 0. ? 0. : h, snow = hs < 0. ? 0. : hs;
            const double ws = w * speed;
            p[NSDG_SERIES_AREA] = p[NSDG_SERIES_AREA] + w;
            p[NSDG_SERIES_EXTENT] = p[NSDG_SERIES_EXTENT] + in_extent;
            p[NSDG_SERIES_VOLUME] = p[NSDG_SERIES_VOLUME] + vol;
            p[NSDG_SERIES_SNOW_VOLUME] = p[NSDG_SERIES_SNOW_VOLUME] + snow;
            p[NSDG_SERIES_DRIFT] = p[NSDG_SERIES_DRIFT] + ws;
            p[NSDG_SERIES_SPEED_MAX] = max_nan(p[NSDG_SERIES_SPEED_MAX], speed);
            p[NSDG_SERIES_HICE_MAX] = max_nan(p[NSDG_SERIES_HICE_MAX], h);
        }
#pragma unroll
        for (int q = 0; q < NSDG_SERIES_COUNT; ++q) {
            if (list.slot[q] < 0) // uniform over the launch
                continue;
            double r = p[q];
            for (int s = 32; s >= 1; s >>= 1) {
                const double other = __shfl_down(r, s, 64);
                r = q < NSDG_SERIES_SPEED_MAX ? r + other : max_nan(r, other);
            }
            if (lane == 0)
                out[list.slot[q] * q_stride + (iy - row0)] = r;
        }
    }
}

// the source pointer a field misses, by name, or null
const char* missing_reads(unsigned r, const nsdg_history_sources& s)
{
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

// nsdg_history_accumulate (stats == nullptr: the plain sums) and nsdg_history_accumulate_stats: the checks and the launch
int accumulate(const char* func, nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nfields, const int32_t* fields, const int32_t* stats,
    const nsdg_history_sources* src, int32_t store, int32_t row0, int64_t plane_stride, double* acc, double* wacc)
{
    NSDG_CHECK_ARG_IN(func, 0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG_IN(func, nfields >= 1 && nfields <= NSDG_HISTORY_MAX_FIELDS, "nfields must be in [1, NSDG_HISTORY_MAX_FIELDS]");
    NSDG_CHECK_ARG_IN(func, fields && src && acc, "null pointer");
    history_list list;
    history_stats st;
    unsigned reads = 0, seen[NSDG_HIST_COUNT] = {};
    list.n = nfields;
    st.weighted = 0;
    for (int k = 0; k < nfields; ++k) {
        const int32_t f = fields[k];
        NSDG_CHECK_ARG_IN(func, f >= 0 && f < NSDG_HIST_COUNT, "unknown field id %d at position %d", (int)f, k);
        const int32_t s = stats ? stats[k] : (int32_t)NSDG_STAT_MEAN;
        NSDG_CHECK_ARG_IN(func, s >= 0 && s < NSDG_STAT_COUNT, "unknown stat id %d at position %d", (int)s, k);
        if (stats)
            NSDG_CHECK_ARG_IN(func, !(seen[f] & (1u << s)), "the pair '%s:%s' is listed twice", FIELD_NAMES[f], STAT_NAMES[s]);
        else
            NSDG_CHECK_ARG_IN(func, !seen[f], "field '%s' is listed twice", FIELD_NAMES[f]);
        const char* miss = missing_reads(FIELD_READS[f], *src);
        NSDG_CHECK_ARG_IN(func, !miss, "field '%s' needs the source %s, which is a null pointer", FIELD_NAMES[f], miss);
        if (s == NSDG_STAT_ICE_MEAN) {
            NSDG_CHECK_ARG_IN(func, src->A, "the ice-weighted mean of field '%s' needs the source A, which is a null pointer", FIELD_NAMES[f]);
            NSDG_CHECK_ARG_IN(func, wacc, "the ice-weighted mean of field '%s' needs the weight plane wacc, which is a null pointer", FIELD_NAMES[f]);
            reads |= RD_A;
            st.weighted = 1;
        }
        seen[f] |= 1u << s;
        reads |= FIELD_READS[f];
        list.id[k] = f;
        st.stat[k] = s;
    }
    for (int k = nfields; k < NSDG_HISTORY_MAX_FIELDS; ++k)
        list.id[k] = 0, st.stat[k] = NSDG_STAT_MEAN;
    NSDG_CHECK_ARG_IN(func, 0 <= row0 && row0 <= j0, "row0 must be in [0, j0]: the accumulator starts at or below the first row of the range");
    NSDG_CHECK_ARG_IN(func, plane_stride >= ((int64_t)j1 - row0) * ctx->nx, "plane_stride is smaller than the rows [row0, j1) of one accumulator plane");
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const long e0 = (long)j0 * ctx->nx, e1 = (long)j1 * ctx->nx;
    // the launch shape of tracer.hip: a few workgroups per CU, each lane walking the rows
    const int blocks = (int)std::min<long>(nsdg_div_up(e1 - e0, 256), 8L * ctx->num_cus);
    if (stats)
        hipLaunchKernelGGL(history_accumulate_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, e0, e1, ctx->nx, ctx->hx, ctx->hy, reads,
            list, st, *src, (int)(store != 0), (long)row0 * ctx->nx, (long)plane_stride, acc, wacc);
    else
        hipLaunchKernelGGL(history_accumulate_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, e0, e1, ctx->nx, ctx->hx, ctx->hy, reads,
            list, st, *src, (int)(store != 0), (long)row0 * ctx->nx, (long)plane_stride, acc, wacc);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
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

const char* nsdg_history_stat_name(int32_t stat)
{
    return stat >= 0 && stat < NSDG_STAT_COUNT ? STAT_NAMES[stat] : nullptr;
}

int nsdg_history_stat_id(const char* name)
{
    if (name)
        for (int s = 0; s < NSDG_STAT_COUNT; ++s)
            if (!std::strcmp(name, STAT_NAMES[s]))
                return s;
    return -1;
}

const char* nsdg_history_series_name(int32_t quantity)
{
    return quantity >= 0 && quantity < NSDG_SERIES_COUNT ? SERIES_NAMES[quantity] : nullptr;
}

int nsdg_history_series_id(const char* name)
{
    if (name)
        for (int q = 0; q < NSDG_SERIES_COUNT; ++q)
            if (!std::strcmp(name, SERIES_NAMES[q]))
                return q;
    return -1;
}

int nsdg_history_accumulate(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nfields, const int32_t* fields, const nsdg_history_sources* src,
    int32_t store, int32_t row0, int64_t plane_stride, double* acc)
{
    NSDG_NEED_GRID(ctx);
    return accumulate(__func__, ctx, j0, j1, nfields, fields, nullptr, src, store, row0, plane_stride, acc, nullptr);
}

int nsdg_history_accumulate_stats(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nfields, const int32_t* fields, const int32_t* stats,
    const nsdg_history_sources* src, int32_t store, int32_t row0, int64_t plane_stride, double* acc, double* wacc)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(stats, "null pointer");
    return accumulate(__func__, ctx, j0, j1, nfields, fields, stats, src, store, row0, plane_stride, acc, wacc);
}

int nsdg_history_row_totals(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nq, const int32_t* quantities, const nsdg_history_sources* src,
    double extent_conc, int32_t row0, int64_t q_stride, double* out)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(nq >= 1 && nq <= NSDG_SERIES_COUNT, "nq must be in [1, NSDG_SERIES_COUNT]");
    NSDG_CHECK_ARG(quantities && src && out, "null pointer");
    series_list list;
    unsigned reads = 0;
    for (int q = 0; q < NSDG_SERIES_COUNT; ++q)
        list.slot[q] = -1;
    for (int k = 0; k < nq; ++k) {
        const int32_t q = quantities[k];
        NSDG_CHECK_ARG_IN(__func__, q >= 0 && q < NSDG_SERIES_COUNT, "unknown quantity id %d at position %d", (int)q, k);
        NSDG_CHECK_ARG_IN(__func__, list.slot[q] < 0, "quantity '%s' is listed twice", SERIES_NAMES[q]);
        const char* miss = missing_reads(SERIES_READS[q], *src);
        NSDG_CHECK_ARG_IN(__func__, !miss, "quantity '%s' needs the source %s, which is a null pointer", SERIES_NAMES[q], miss);
        list.slot[q] = k;
        reads |= SERIES_READS[q];
    }
    NSDG_CHECK_ARG(std::isfinite(extent_conc), "extent_conc must be finite");
    NSDG_CHECK_ARG(0 <= row0 && row0 <= j0, "row0 must be in [0, j0]: the totals start at or below the first row of the range");
    NSDG_CHECK_ARG(q_stride >= (int64_t)j1 - row0, "q_stride is smaller than the rows [row0, j1) of one quantity");
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const int blocks = (int)std::min<long>(nsdg_div_up((long)j1 - j0, 4), 8L * ctx->num_cus);
    hipLaunchKernelGGL(history_row_totals_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (int)j0, (int)j1, ctx->nx, reads, list, *src,
        extent_conc, (int)row0, (long)q_stride, out);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

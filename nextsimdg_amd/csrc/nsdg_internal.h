// nsdg_internal.h -- shared by the translation units of libnsdg.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <type_traits>

#include "../../include/nsdg.h"

struct nsdg_comm; // halo.hip
struct nsdg_phase_timer; // phase_timer.hip

struct nsdg_ctx {
    int device;
    hipStream_t stream;
    nsdg_column_params column;
    nsdg_slab_params slab; // slab ocean (column_step.hip, nsdg_column_step_ocean): relaxation times and the salinity of the ice
    nsdg_mevp_params mevp;
    nsdg_bbm_params bbm; // brittle rheology (bbm.hip)
    int nx, ny; // local element array
    int row0, ny_global; // its placement in the global domain (analytic forcing providers); ny_global 0 = single domain
    double hx, hy;
    int mevp_variant;
    int strip_rows; // rows per strip of the fused marching kernel (0 = chosen per launch)
    int num_cus;
    double pack_dt; // time step the packed nodal coefficients were built for (0 = never packed)
    const uint8_t* land; // element land mask of the local array (landmask.hip), null = none; owned by the caller
    bool pack_land; // the packing saw a mask: land nodes carry the flag cd < 0 and the passes run the LAND instantiations
    nsdg_basal_params basal; // landfast ice (basal.hip): the grounding scheme's parameters
    const double* depth; // water depth per element of the local array, null = none; owned by the caller
    bool pack_basal; // the packing saw a depth array: pair 3 of a node holds (T_b, 0) and the passes run the BASAL instantiations
    // snow load (snowload.hip, include/nsdg_snow.h): the snow's coefficient planes on the local array, null = none, owned by the caller; the
    // packing reads them and the passes read c[0] as ever -- no flag of the packing goes with them
    const double* snow;
    int snow_ncoef; // 1, 3 or 6 planes
    double rho_snow;
    // sea-surface tilt (tilt.hip, include/nsdg_tilt.h): the sea-surface height on the nodes of the local lattice, null = none (the tilt is
    // then that of the geostrophic current, as ever), owned by the caller; the packing reads it -- no flag of the packing goes with it
    const double* ssh;
    double gravity;
    int transport_variant, transport_rows; // transport stage kernel: 0 one element per lane / 2 two elements per lane; rows per workgroup
    int fused_min_waves; // register budget of the fused kernel: 1 or 2 waves per SIMD
    int nbounds; // closure of a transport step: bounds of the advected fields (0 = none), nsdg_transport_bounds_set
    nsdg_field_bounds bounds[4];
    // device scratch for small host->device tables (field pointer lists of the transport stage)
    double** d_ptrs;
    nsdg_comm* comm; // row-block communicator (halo.hip), null until nsdg_comm_init*
    int64_t comm_group; // id of the local group the communicator belongs to
    double comm_deadline_s; // upper bound on any wait for a neighbour (0 = for ever)
    // report channel of the mEVP pipelines' bounded waits (mevp_p2p.h): a device counter and a flag in mapped host memory
    unsigned* p2p_count_dev;
    unsigned* p2p_flag_host; // hipHostMalloc'ed; p2p_flag_dev is its device address
    unsigned* p2p_flag_dev;
    unsigned p2p_given_up; // sticky: events seen so far and not yet taken by nsdg_mevp_pipeline_health
    // two device scalars and their pinned host mirrors: [0] the result of nsdg_concentration_max (substep.hip), [1] the value of
    // nsdg_comm_max_f64 (halo.hip)
    double* scalar_dev;
    double* scalar_host; // hipHostMalloc'ed
    nsdg_phase_timer* phase; // per-phase device timing (phase_timer.hip), null until nsdg_phase_timing_set turns it on
};

void nsdg_set_error(const char* fmt, ...);
// NSDG_ERR_HIP (sticky until nsdg_mevp_pipeline_health) if a bounded wait of an mEVP pipeline launched on this context has given up
// in a launch that has completed; does not synchronise
int nsdg_p2p_check(nsdg_ctx* ctx, const char* where);
int nsdg_comm_bounded_drain(nsdg_ctx* ctx); // halo.hip: drain the context's streams within the communicator's deadline
void nsdg_phase_timer_free(nsdg_ctx* ctx); // phase_timer.hip: the event ring of nsdg_phase_timing_set, if there is one

#define NSDG_CHECK_ARG(cond, msg)                                        \
    do {                                                                 \
        if (!(cond)) {                                                   \
            nsdg_set_error("%s: %s", __func__, msg);                    \
            return NSDG_ERR_ARG;                                         \
        }                                                                \
    } while (0)

// NSDG_CHECK_ARG in a helper that checks on behalf of several exported functions: `fn` is the one the message names, and the
// message is a printf format
#define NSDG_CHECK_ARG_IN(fn, cond, fmt, ...)                            \
    do {                                                                 \
        if (!(cond)) {                                                   \
            nsdg_set_error("%s: " fmt, fn, ##__VA_ARGS__);               \
            return NSDG_ERR_ARG;                                         \
        }                                                                \
    } while (0)

#define NSDG_CHECK_HIP(expr)                                                              \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            nsdg_set_error("%s: %s failed: %s", __func__, #expr, hipGetErrorString(e_)); \
            return NSDG_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

#define NSDG_CHECK_LAUNCH() NSDG_CHECK_HIP(hipGetLastError())

#define NSDG_NEED_GRID(ctx)                                             \
    do {                                                                \
        NSDG_CHECK_ARG(ctx != nullptr, "null context");                 \
        if ((ctx)->nx <= 0) {                                           \
            nsdg_set_error("%s: nsdg_grid_set was not called", __func__); \
            return NSDG_ERR_STATE;                                      \
        }                                                               \
    } while (0)

static inline int nsdg_div_up(long a, long b) { return (int)((a + b - 1) / b); }

// the tiled arrays are accessed 16 bytes at a time
static inline bool nsdg_aligned16(std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15)
            return false;
    return true;
}

// the refusal of an unaligned tiled array, the same words from every entry point that reads one 16 bytes at a time
#define NSDG_TILED_MSG "tiled arrays (stress, ice strength) must be 16-byte aligned"
#define NSDG_CHECK_TILED(...) NSDG_CHECK_ARG(nsdg_aligned16({ __VA_ARGS__ }), NSDG_TILED_MSG)

// coefficients per element of a DG field of the order 0, 1 or 2
constexpr int nsdg_nc(int order) { return order == 0 ? 1 : (order == 1 ? 3 : 6); }

// ONE dispatch from an order the caller has checked (0, 1 or 2) to the instantiation for it: f receives the order as a
// std::integral_constant, `[&](auto O) { constexpr int ORDER = decltype(O)::value; ... }`
template <class F>
inline auto nsdg_with_order(int order, F&& f)
{
    switch (order) {
    case 0: return f(std::integral_constant<int, 0>());
    case 1: return f(std::integral_constant<int, 1>());
    default: return f(std::integral_constant<int, 2>());
    }
}

// ---- snow load (snowload.hip) ---------------------------------------------------------------------------------------------------
// r = rho_snow / rho_ice of the packing being launched: one IEEE division on the host, with the rho_ice the context holds now
static inline double nsdg_snow_ratio(const nsdg_ctx* ctx) { return ctx->snow ? ctx->rho_snow / ctx->mevp.rho_ice : 0.; }
// NSDG_ERR_ARG, reported under `fn`, if the context's snow field overlaps the 8 (2nx+1)(2ny+1) doubles of `packed`; NSDG_OK without a field
int nsdg_snow_check_packed(const nsdg_ctx* ctx, const char* fn, const double* packed);

// ---- sea-surface tilt (tilt.hip) ------------------------------------------------------------------------------------------------
// NSDG_ERR_ARG, reported under `fn`, if the context's sea-surface height overlaps the 8 (2nx+1)(2ny+1) doubles of `packed`; NSDG_OK without one
int nsdg_tilt_check_packed(const nsdg_ctx* ctx, const char* fn, const double* packed);

// ---- mEVP passes (mevp.hip) -----------------------------------------------------------------------------------------------------
// the buffers of a pass: the stress S_in -> S_out (tiled), the velocity u_old -> u_new, the packed nodal coefficients, the ice strength
struct nsdg_mevp_bufs {
    const double *s11i, *s12i, *s22i;
    double *s11, *s12, *s22;
    const double *u_old, *v_old;
    double *u_new, *v_new;
    const double *packed, *pg;
};

// The checks of one marching pass of v sub-iterations, reported under the name `fn` of the entry point it works for: v = 1 on the stress
// rows [k0, j1) and the velocity rows [j0, j1) -- the single-iteration pass of either rheology (nsdg_mevp_iterate, nsdg_bbm_iterate) --,
// v = 2, 3, 4 on the rows [j0, j1) and, for the pair forms, on the disjoint rows [j0b, j1b) as well.  Context and grid, the row ranges,
// nulls, 16-byte alignment of the tiled arrays and aliasing of the stress, the velocity and the packed coefficients of `b` (b.pg is not
// looked at) and of `gauss`, the tiled Gauss-point arrays of the rheology; then, in this order: nothing to do for v = 1 without a stress
// row, the packing's state, nothing to do for v >= 2 on an empty range, the variant, hipSetDevice.  *run: all is well and there is
// something to launch; the result is the caller's either way
int nsdg_pass_check(nsdg_ctx* ctx, const char* fn, int v, int k0, int j0, int j1, bool pair, int j0b, int j1b, const nsdg_mevp_bufs& b,
    std::initializer_list<const void*> gauss, bool* run);

// One checked pass of v sub-iterations, the work of every nsdg_mevp_iterate* entry point and reported under its name: v = 1 on the
// stress rows [k0, j1) and the velocity rows [j0, j1) (nsdg_mevp_iterate); v = 2, 3, 4 on the rows [j0, j1) (nsdg_mevp_iterate2 / 3 / 4)
// and, for the pair forms, on the disjoint rows [j0b, j1b) as well (nsdg_mevp_iterate3_pair / 4_pair)
int nsdg_mevp_pass(nsdg_ctx* ctx, int v, int k0, int j0, int j1, bool pair, int j0b, int j1b, const nsdg_mevp_bufs& b);

// the launchers behind it, unchecked: the fused single-iteration kernel (mevp_fused.hip); the stage-per-wave pipeline of nst = 2, 3
// or 4 sub-iterations on the rows [j0, j1) and, if j0b < j1b, on a second disjoint range (mevp_fused4.hip)
// land: run the instantiation that holds land nodes at 0; basal: the one with the seabed stress -- both chosen in ONE place,
// nsdg_mevp_pass, from what the packing saw
int nsdg_launch_mevp_fused(nsdg_ctx* ctx, bool land, bool basal, int k0, int j0, int j1, const nsdg_mevp_bufs& b);
int nsdg_launch_mevp_fused4_ranges(nsdg_ctx* ctx, bool land, bool basal, int nst, int j0, int j1, int j0b, int j1b, const nsdg_mevp_bufs& b);
// the BASAL instantiations of the pipeline, a translation unit of their own (mevp_fused4_basal.hip); nsdg_launch_mevp_fused4_ranges forwards to it
int nsdg_launch_mevp_fused4_basal_ranges(nsdg_ctx* ctx, bool land, int nst, int j0, int j1, int j0b, int j1b, const nsdg_mevp_bufs& b);

// rows per strip of a single-iteration march over `rows` element rows with ncw column-waves, in a kernel built for `waves_per_simd`
// resident waves: the context's strip_rows, or the automatic height (mevp_fused.hip)
int nsdg_march_strip_rows(const nsdg_ctx* ctx, int rows, int ncw, int waves_per_simd);

// ---- transport (transport.hip) --------------------------------------------------------------------------------------------------
// One checked transport step on the rows [j0, j1) as stage launches, reported under the name `fn` of the entry point it works for:
// the order + 1 stages of the SSP Runge-Kutta tableau -- stage k reads the state (k = 0) or the stage buffer k - 1 and writes the
// stage buffer k (buf0, buf1), the last stage writes `out` -- then the closure on [j0, j1) of `out` if bounds are set.  after_stage(k) runs once stage k has been launched,
// for every stage but the last (a row block exchanges the ghost rows of the buffer just written); a result != NSDG_OK ends the step.
// A stage reads one row on each side of its rows and never the array it writes: `out` may be the state itself from the second stage
// on (the last stage reads the state only at the element it writes), or buf0 from the third
int nsdg_transport_staged_step(nsdg_ctx* ctx, const char* fn, int order, int j0, int j1, double dt, int nfields, const double* const* state,
    double* const* buf0, double* const* buf1, double* const* out, const double* vx_dg, const double* vy_dg, const double* un_x, const double* un_y,
    const std::function<int(int)>& after_stage);

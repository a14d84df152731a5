/*
 * nsdg.h -- C ABI of the MI355X-native sea-ice dynamics / column-physics core (libnsdg.so).
 *
 * This is the drop-in boundary of SURVEY.md section 8(b): a host program that keeps the reference's
 * IModelStep / IStructure / ModuleLoader surfaces (see nextsimdg_amd/host/ and INTEGRATION.md)
 * calls these entry points once per model step; everything behind them is hand-written HIP for
 * gfx950.  No C++ types, exceptions or torch types cross the boundary.
 *
 * Conventions
 *  - Every function returns NSDG_OK (0) or a negative nsdg_status; nsdg_last_error() returns a
 *    thread-local description of the last failure.
 *  - All array arguments are DEVICE pointers to fp64 owned by the caller; the library never frees
 *    or reallocates them.  Calls are asynchronous on the context's stream: a buffer may be reused by
 *    the host after the stream has been synchronised (nsdg_ctx_synchronize or the caller's own sync).
 *  - One context per GPU/stream.  Calls on one context must not be issued concurrently from two
 *    host threads; different contexts are independent.  (The reference is single-threaded and
 *    non-re-entrant: static m_dt / m_freezer, core/src/PrognosticData.cpp:12-13.)
 *  - Streams (held to it on a stream other than the null stream by tests/test_gpu_stream_order.py; its `blocks_host` column is the
 *    tested form of the list below).  Every launch and copy of a call goes to the context's stream, or to one of the library's own
 *    non-blocking streams (the communication stream, the stream a row-block plan replays its graphs on) ordered behind it and joined
 *    back to it with events before the call returns: a call reads what the stream has produced when its work runs, and work enqueued
 *    on the stream behind it sees its results.  Given a stream other than NULL, the library never uses the null stream.
 *    These calls BLOCK the host until the context's stream (and, with a communicator, its communication stream) has drained:
 *    nsdg_ctx_synchronize, nsdg_ctx_destroy, nsdg_mevp_pipeline_health, nsdg_concentration_max, nsdg_phase_times,
 *    nsdg_halo_stats_get and nsdg_rb_mevp_stats / nsdg_rb_bbm_stats / nsdg_rb_transport_stats (they wait for the last exchange),
 *    nsdg_comm_finalize (the communication stream only), and nsdg_comm_max_f64_array on the local transport.  nsdg_phase_mark waits only when its ring is full;
 *    nsdg_halo_start / _finish on the local transport wait for the neighbour THREAD to post, never for the device.  Every other call
 *    returns without waiting for the device.  Setters (nsdg_grid_set, nsdg_*_params_set, nsdg_*_variant_set, nsdg_land_mask_set, ...)
 *    store host state that is read when a later call is MADE, not when its work runs: a setter between two enqueued calls acts on the
 *    second only.
 *    "One context per stream" permits two contexts on two streams of ONE device, driven concurrently (from one host thread or two):
 *    they share no launch constants, scratch or device symbols.
 *  - No clamping or input checking is added to the physics (SURVEY.md section 8b "Errors").  The results follow the
 *    reference's arithmetic, including its Inf / NaN / 0 for mld == 0, dt == 0, vanishing fluxes, zero pressure and
 *    non-finite forcing values: every division either is an IEEE division or ends in the IEEE sequence's special-case
 *    fix-up (csrc/column_step.hip).  The one exclusion: a SUBNORMAL or > 2^1022 value of slp, of an absolute
 *    temperature or of conc + del_c makes the reciprocal-based divisions return NaN where IEEE division scales.
 *
 * Data layout
 *  - element (ix, iy) of an nx x ny local array, ix fastest:  e = iy*nx + ix.  (The reference's
 *    restart layout is the same x-major linear index i*nx + j, core/src/DevGridIO.cpp:107-109.)
 *  - DG field, nc coefficients: coefficient-major planes  f[c*nx*ny + e]   (nc = 1/3/6 for DG0/1/2,
 *    8 for the stress space).
 *  - CG2 nodal field: (2nx+1) x (2ny+1) lattice, node (gx, gy) at  n = gy*(2nx+1) + gx.
 *  - edge-normal velocities at the ng = order+1 edge Gauss points:
 *        un_x[g*(nx+1)*ny + iy*(nx+1) + ex]   (vertical edges, normal = +x)
 *        un_y[g*nx*(ny+1) + ey*nx + ix]       (horizontal edges, normal = +y)
 *  - arrays private to the mEVP sub-cycle -- the stress coefficients s11/s12/s22 (nc = 8) and the ice
 *    strength at the 3x3 Gauss points pg (nc = 9, q = 3*qy + qx) -- use a TILED layout: tiles of 64
 *    consecutive elements of a row with all coefficients of the tile together, the coefficients in pairs
 *    interleaved by element (so that two coefficients travel in one 16-byte access): with the tile base
 *    T = ((iy*ntx + ix/64)*nc)*64, ntx = ceil(nx/64), and l = ix%64,
 *        coefficient c < 2*(nc/2):  a[T + (c/2)*128 + 2*l + c%2]
 *        odd last coefficient (nc = 9, c = 8):  a[T + (nc/2)*128 + l]
 *    nsdg_tiled_len(nx, ny, nc) doubles, 16-byte aligned.  Element rows stay contiguous, so row ranges / ghost
 *    rows work as for the plane layout.  (nextsimdg_amd/abi.py: tile() / untile() convert from / to planes.)
 *  - Row ranges [j0, j1) are ELEMENT rows of the local array; the edges of the local array are the
 *    physical boundary (zero inflow for transport, v = 0 for momentum).  A rank of a row-block
 *    decomposition passes arrays that include its ghost rows and the range of rows it owns.
 */
#ifndef NSDG_H
#define NSDG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6: a pipeline wait that gives up is an error status.  Since then the ABI has only grown, without a new number: nsdg_concentration_max,
 * nsdg_substep_count and nsdg_comm_max_f64 (sub-stepping of the model time step), nsdg_forcing_sample (forcing from a file) and
 * nsdg_tracer_weight / nsdg_tracer_recover (column state transport) and nsdg_phase_timing_set / nsdg_phase_mark / nsdg_phase_times (per-phase
 * device timing) and nsdg_land_mask_set / nsdg_land_clear / nsdg_land_clear_nodes (land mask) and nsdg_bbm_default_params / nsdg_bbm_params_set /
 * nsdg_bbm_prepare / nsdg_bbm_iterate / nsdg_bbm_substep_count (brittle rheology) and nsdg_history_accumulate / nsdg_history_field_name /
 * nsdg_history_field_id, nsdg_history_accumulate_stats / nsdg_history_row_totals / nsdg_history_stat_* / nsdg_history_series_* (history
 * output) and nsdg_drifters_advance / nsdg_comm_max_f64_array (drifters) and nsdg_rb_bbm_create / nsdg_rb_bbm_destroy / nsdg_rb_bbm_run /
 * nsdg_rb_bbm_stats (the brittle sub-cycle of a row block) and nsdg_bbm_params_check and nsdg_points_sample (point samples) are additions, and so are the
 * ice tracers' calls of nsdg_tracers.h;
 * nothing that existed changed. */
#define NSDG_ABI_VERSION 6

typedef enum {
    NSDG_OK = 0,
    NSDG_ERR_ARG = -1, /* bad argument (null pointer, bad size / order / range) */
    NSDG_ERR_HIP = -2, /* a HIP runtime call or kernel launch failed */
    NSDG_ERR_STATE = -3, /* call sequence error (e.g. grid not set) */
    NSDG_ERR_NODEVICE = -4, /* no usable HIP device */
    NSDG_ERR_COMM = -5 /* RCCL missing or an RCCL call failed; a rank of a local group failed */
} nsdg_status;

typedef struct nsdg_ctx nsdg_ctx;

/* ---- context ------------------------------------------------------------------------------
 * Replaces the process-wide static state of the reference (ModuleLoader singleton,
 * core/src/include/ModuleLoader.hpp:22-27; static physics parameters,
 * physics/src/modules/NextsimPhysics.cpp:26-39) by an explicit per-GPU object.
 * `stream` is a hipStream_t (NULL = the device's default stream). */
int nsdg_abi_version(void);
const char* nsdg_last_error(void);
int nsdg_ctx_create(int device_id, void* stream, nsdg_ctx** out);
int nsdg_ctx_destroy(nsdg_ctx* ctx);
/* Waits for everything enqueued on the context's stream (and its communication stream).  On a context with a
 * communicator the wait is BOUNDED by the communicator's deadline (nsdg_comm_deadline_set): if the streams have not
 * drained by then -- a neighbour rank that died leaves ncclRecv waiting for ever -- it returns NSDG_ERR_COMM, the
 * communicator is marked broken (nsdg_comm_finalize then aborts it instead of draining it) and the caller should
 * leave the process with a non-zero status without synchronising the device again. */
int nsdg_ctx_synchronize(nsdg_ctx* ctx);

/* Measurement aid: streaming device copy of n doubles, 16 bytes per lane and access -- the "device-copy peak" that
 * SURVEY.md section 8(d) asks the roofline fraction to be quoted against, measured on the box the bench runs on
 * (bench.py: roofline.copy_peak_GBs).  dst and src 16-byte aligned, not overlapping. */
int nsdg_copy_f64(nsdg_ctx* ctx, double* dst, const double* src, int64_t n);

/* ---- per-phase device timing (csrc/phase_timer.hip; DESIGN.md section 6 "phase timing") -------------------------
 * An opt-in answer to "where does my step go?": the host brackets the parts of its model step with MARKS, each mark records one event
 * on the context's stream, and the device time between two consecutive marks belongs to the phase the first of them opened.  The
 * ids below are shared by both hosts (the C++ DynamicsStep / HipStep and the Python DynamicsCore) so that their tables read alike;
 * any id in [0, NSDG_PHASE_MAX) is accepted.
 *
 * nsdg_phase_timing_set: on / off; a new context starts off.  Turning it on allocates the ring of NSDG_PHASE_RING events, turning it off
 *   discards whatever was pending and zeroes the table.
 * nsdg_phase_mark: closes the running phase, if there is one, and opens `phase`; NSDG_PHASE_END closes the running phase and opens
 *   nothing (and is a no-op when nothing runs) -- the stretch up to the next mark then belongs to no phase.  With timing off it
 *   returns NSDG_OK and does nothing (no event, no allocation): a host can call it unconditionally.  It never waits for recently
 *   enqueued work: intervals whose closing event has completed are harvested with hipEventQuery, and only when every event of the
 *   ring is outstanding does it wait -- for the OLDEST one.  No interval is dropped or counted twice.  On a stream that is being
 *   captured it returns NSDG_ERR_STATE (an event query inside a capture would invalidate the capture): mark between the captured
 *   regions, e.g. around nsdg_rb_mevp_run, never inside one.
 * nsdg_phase_times: waits for the last mark (on a context with a communicator: the bounded drain of nsdg_ctx_synchronize, NSDG_ERR_COMM
 *   on expiry) and returns, per phase id, the accumulated device time and the number of closed intervals.  A SPAN runs from the mark
 *   that opened a phase while none was running to the NSDG_PHASE_END that closes the sequence; total_ms sums hipEventElapsedTime(first,
 *   end) over the spans -- its own pair of events, not the sum of the phases -- so a table can be checked against it.  A phase that is
 *   still open stays open (its interval is counted once it is closed).  reset != 0 zeroes the table after it was copied; reset between
 *   spans (after an NSDG_PHASE_END) if the next table is to add up: a span that is open keeps its first mark.
 * Null context, a phase outside [0, NSDG_PHASE_MAX) other than NSDG_PHASE_END, or a null `out`: NSDG_ERR_ARG. */
enum {
    NSDG_PHASE_FORCING = 0, /* external forcing: box test or file sampling, nsdg_column_forcing, nsdg_column_wind */
    NSDG_PHASE_COLUMN = 1, /* nsdg_column_step */
    NSDG_PHASE_PREPARE = 2, /* nsdg_ice_strength, nsdg_mevp_prepare */
    NSDG_PHASE_SUBCYCLE = 3, /* the mEVP sub-iterations (nsdg_rb_mevp_run / nsdg_mevp_subcycle) */
    NSDG_PHASE_TRANSPORT = 4, /* nsdg_prepare_advection, tracer weight / recover, the transport step */
    NSDG_PHASE_REDUCTION = 5, /* nsdg_concentration_max of the sub-stepping rule */
    NSDG_PHASE_MAX = 16,
    NSDG_PHASE_END = -1
};
#define NSDG_PHASE_RING 256 /* events per context: a mark waits (for the oldest) only when this many are outstanding */
typedef struct {
    double ms[NSDG_PHASE_MAX]; /* accumulated device time of the phase's closed intervals */
    int64_t count[NSDG_PHASE_MAX]; /* closed intervals */
    double total_ms; /* sum over the closed spans of hipEventElapsedTime(first mark, closing NSDG_PHASE_END) */
    int64_t spans;
} nsdg_phase_table;
int nsdg_phase_timing_set(nsdg_ctx* ctx, int32_t enable);
int nsdg_phase_mark(nsdg_ctx* ctx, int32_t phase);
int nsdg_phase_times(nsdg_ctx* ctx, nsdg_phase_table* out, int32_t reset);

/* ---- column physics (the reference's per-element step) ---------------------------------------- */
enum { NSDG_ALBEDO_SMU = 0, NSDG_ALBEDO_SMU2 = 1, NSDG_ALBEDO_CCSM = 2 }; /* physics/src/modules/modules.json:4-8 */
enum { NSDG_FREEZING_LINEAR = 0, NSDG_FREEZING_UNESCO = 1 }; /* core/src/modules/modules.json:4-7 */

/* Every configuration value of the column path:
 * nextsim_thermo.* (physics/src/modules/NextsimPhysics.cpp:50-58,76-82), thermoice0.*
 * (ThermoIce0.cpp:23-31), Hibler.* (HiblerConcentration.cpp:21-29), CCSMIceAlbedo.*
 * (CCSMIceAlbedo.cpp:40-41) and the [Modules] choices of IIceAlbedo / IFreezingPoint. */
typedef struct {
    double drag_ocean_q, drag_ocean_t, drag_ice_t, ocean_albedo, i0, min_conc, min_thick;
    double ks;
    double h0, phi_m;
    double ccsm_ice_albedo, ccsm_snow_albedo;
    int32_t flooding;
    int32_t albedo_kind;
    int32_t freezing_kind;
    int32_t reserved;
} nsdg_column_params;

void nsdg_column_default_params(nsdg_column_params* p);
int nsdg_column_params_set(nsdg_ctx* ctx, const nsdg_column_params* p);

/* optional diagnostics: NSDG_NDIAG planes of n doubles, diag[k*n + e] */
enum {
    NSDG_D_RHO = 0, NSDG_D_QA, NSDG_D_QW, NSDG_D_QI, NSDG_D_CSPEC, NSDG_D_TAU, NSDG_D_HI, NSDG_D_HS,
    NSDG_D_CNEW, NSDG_D_QIA, NSDG_D_QIO, NSDG_D_SUBL, NSDG_D_DQDT, NSDG_D_HIFROMS, NSDG_D_QOW, NSDG_NDIAG
};

/* One model step of the column physics on n independent elements; replaces the element loop of
 * DevStep::iterate (core/src/DevStep.cpp:14-23), i.e. per element
 *   IPhysics1d::updateDerivedData (physics/src/modules/include/IPhysics1d.hpp:33-45),
 *   NextsimPhysics::calculate (physics/src/modules/NextsimPhysics.cpp:116-131),
 *   PrognosticData::updateAndIntegrate (core/src/PrognosticData.cpp:63-71).
 * hice/cice/hsnow/tice0 are updated in place; sst/sss and the forcing are read-only (the reference
 * never updates sst/sss); newice is the per-element persistent NextsimPhysics::m_newice
 * (NextsimPhysics.cpp:244-253) and must be carried by the caller between steps; wind is
 * PhysicsData::windSpeed (physics/src/include/PhysicsData.hpp:44).  diag may be NULL. */
int nsdg_column_step(nsdg_ctx* ctx, int64_t n, double dt, double* hice, double* cice, double* hsnow,
    double* tice0, const double* sst, const double* sss, const double* tair, const double* tdew,
    const double* slp, const double* qsw, const double* qlw, const double* mld, const double* snowfall,
    const double* wind, double* newice, double* diag);

/* ---- dynamics: DG transport + mEVP (no counterpart in the reference snapshot: CMakeLists.txt:43-46
 *      comments the dynamics component out; built from the published formulation)
 * INPUT DOMAIN AND CLOSURE (round 5; the failure it answers: profiles/r04_soak_divergence_cause.md, the runs that now complete:
 * profiles/r05_closure.md).  Without a closure the scheme leaves the physical range once ice converging against a closed wall
 * reaches A = 1 (a one-element band piles up, the unlimited DG2 transport undershoots beside it, a node of floor mass between full
 * elements runs away).  Three pieces close it; none of them has a counterpart in the reference, whose concentration model has no
 * cap either (physics/src/modules/HiblerConcentration.cpp:32-47) -- the shape followed is the column model's own cut-off rule
 * (physics/src/modules/NextsimPhysics.cpp:210-219):
 *   1. ridging: the cell mean of a field with cap_mean != 0 (the concentration, hi = 1) is capped at hi at the end of a transport
 *      step; the mean thickness -- the conserved volume -- is a field of its own and is not touched, so convergence beyond a
 *      closed cover turns into (true) thickness;
 *   2. a Zhang-Shu scaling limiter at the end of a transport step keeps the values of a bounded field at the scheme's quadrature
 *      points (volume and edge Gauss points) and at its corners -- together: at every CG2 node of the element too -- inside [lo, hi]
 *      by scaling its higher coefficients; cell means are never changed;
 *   3. ice-free nodes (nsdg_mevp_params.min_conc / min_thick) are in free drift and do not feel their neighbours' stress.
 * 1 and 2 are per-field properties the host states with nsdg_transport_bounds_set (they are OFF until it does: the library does
 * not know which field is a concentration); 3 is ON by default.
 * What the closure does NOT replace is a sub-cycle that can follow the forcing (profiles/r05_closure.md): a UNIFORM alpha = beta must satisfy
 * alpha beta >= (2.4 pi)^2 P* dt / (2 delta_min rho_ice h^2) (linear stability, with the margin a one-day run needs), and with the
 * literature's delta_min = 2e-9 on a mesh finer than ~2 km that is an alpha of 10^4 ... 10^5, under which 120 sub-iterations
 * move stress and velocity less than 1 % of the way per model step -- a compressible cover (A < 1) then leaves the physical range
 * within a model day or two with or without the closure.  Round 5's hosts kept alpha = beta = 1500 and raised delta_min to the smallest
 * value for which that is stable on the mesh (1.9e-7 / 7.4e-7 / 3.0e-6 1/s at 500 / 250 / 125 m: a viscosity capped 90 to 1500 times
 * lower than the literature's).  Since round 6 the hosts run LOCAL, SOLUTION-ADAPTIVE alpha and beta (nsdg_mevp_params.aevp_c) at
 * delta_min = 2e-9: a uniform cover A = 0.9 then completes 53 model hours at 1024 x 1024 and the model day at 4096 x 4096
 * (profiles/r06_soak_1024_A09_adaptive_1600_steps.txt, r06_config5_one_day_A09_adaptive_host.txt).  nsdg_mevp_stable_params holds the
 * rule and its three forms; the defaults of nsdg_mevp_default_params -- uniform alpha = beta = 1500, delta_min = 2e-9 -- are the
 * literature's and are UNSTABLE below ~2 km: call nsdg_mevp_stable_params.  The calls do not check any of this; both hosts stop
 * loudly on non-finite fields. */
typedef struct {
    double rho_ice, rho_atm, rho_ocean;
    double c_atm, c_ocean;
    double pstar, compaction;
    double delta_min;
    double fc;
    double alpha, beta;
    double h_min; /* floor of the nodal mean thickness in the nodal mass */
    /* ice-free-node rule: a node with mean concentration < min_conc, true thickness cgH / cgA < min_thick or a mean thickness at the
     * mass floor (cgH <= h_min: its mass would be made up) is in free drift (full
     * exposure to wind and ocean drag, Coriolis, floor mass) and the stress divergence of the neighbouring elements is weighted by
     * 2^-100 there.  Defaults: the column model's cut-off values 1e-12 and 0.01 m (nextsim_thermo.min_conc / min_thick,
     * physics/src/modules/NextsimPhysics.cpp:81-82).  Both 0: rule off. */
    double min_conc, min_thick;
    /* LOCAL, SOLUTION-ADAPTIVE alpha and beta (round 6; after Kimmritz, Danilov & Losch 2016, "The adaptive EVP method for solving
     * the sea ice momentum equation", Ocean Modelling 101 -- parity unpinned like the rest of the dynamics).  aevp_c > 0 replaces the
     * uniform alpha, beta above: in every sub-iteration every element takes the alpha its own viscosity asks for,
     *     zeta_e = max over its 9 Gauss points of P / (2 Delta),
     *     alpha_e = sqrt(max(aevp_alpha_min^2, aevp_c zeta_e dt / (rho_ice h'_c hx hy))),
     * h'_c = max(nodal mean thickness at the element's centre node, h_min) (alpha_e = aevp_alpha_min where that node is ice-free), the
     * stress relaxes with 1 / alpha_e, and every node takes beta_n = max(aevp_alpha_min, max over its adjacent elements of alpha_e h'_c(e) / h'_n)
     * (alpha_e weighted by the ratio of the element's mass to the node's: the bound of every element-node pair; alpha_min at an ice-free node).  aevp_c is the
     * stability bound's constant: (2.4 pi)^2 = 56.85 is the bound DESIGN.md section 3.4 states with its margin; aevp_alpha_min must not be
     * chosen small on a fine mesh (nsdg_mevp_stable_params sets both).  Where the ice
     * deforms alpha is small and the stress follows the strain rate within a few sub-iterations, where it is rigid alpha is what the
     * uniform form needs everywhere; the converged sub-cycle solves the same implicit step.  aevp_c = 0 (the default of
     * nsdg_mevp_default_params): uniform alpha, beta -- bit-identical to ABI 5.  The adaptive form exists in the marching kernels
     * (nsdg_mevp_iterate*, nsdg_mevp_subcycle, nsdg_rb_mevp_run); nsdg_mevp_stress / nsdg_mevp_velocity return NSDG_ERR_STATE. */
    double aevp_c, aevp_alpha_min;
} nsdg_mevp_params;

void nsdg_mevp_default_params(nsdg_mevp_params* p);
int nsdg_mevp_params_set(nsdg_ctx* ctx, const nsdg_mevp_params* p);

/* The stability rule of the explicit sub-cycle, stated ONCE (round 5 had a copy in each host): on cells of size h = min(hx, hy) and
 * for a model time step dt the sub-cycle is linearly stable where  alpha beta >= (2.4 pi)^2 zeta dt / (m h^2)  (2.4: the margin a
 * one-day run needs, profiles/r02_alpha_margin.txt), zeta / m <= pstar / (2 delta_min rho_ice).  Three ways to satisfy it, chosen by
 * `mode`; the other members of *p are read (pstar, rho_ice, and what the mode keeps) and left alone:
 *   NSDG_SUBCYCLE_ADAPTIVE       aevp_c = (2.4 pi)^2: alpha_e, beta_n follow the local viscosity of every sub-iteration; delta_min stays (the
 *                                literature's 2e-9 by default); aevp_alpha_min = 50, the constant Kimmritz et al. (2016) publish.  The
 *                                hosts' default since round 6.  On meshes finer than 1 km every deforming element then sits AT its
 *                                stability limit and 120 sub-iterations do not converge: the velocity is noisy at element scale
 *                                (profiles/r06_adaptive_noise.md) -- the runs complete, the noise acts as a viscosity.
 *   NSDG_SUBCYCLE_ADAPTIVE_CONVERGED  the same with aevp_alpha_min = the bound's alpha for the reference strain rate NSDG_AEVP_DELTA_REF
 *                                (500 / 1000 / 2000 at 500 / 250 / 125 m, dt = 120 s; never below 50): the sub-cycle converges (0.1 % /
 *                                2 % of the maximum speed left after 120 sub-iterations at 1024^2 / 2048^2).  A converged plastic
 *                                solution exposes the time-step limit of the explicit strength / transport splitting (Lipscomb et al.
 *                                2007): dt = 120 s is too long for it at 250 m and below (2048^2 leaves the physical range after 11 model
 *                                hours, with dt = 60 s or 30 s it does not: profiles/r06_adaptive_noise.md) -- split the model step with
 *                                nsdg_substep_count below (the hosts' dynamics.substeps = auto / DynamicsCore.advance(substeps="auto")).
 *   NSDG_SUBCYCLE_KEEP_ALPHA     uniform alpha = beta = p->alpha; delta_min is raised to the smallest value for which that is stable
 *                                (never lowered): the viscosity is capped -- below a strain rate of delta_min the ice creeps
 *                                (nsdg_mevp_creep_percent_per_day).  The hosts' default of round 5.
 *   NSDG_SUBCYCLE_KEEP_DELTA_MIN uniform alpha = beta = the bound's value for p->delta_min (at least 1500): rounds 1-4. */
enum { NSDG_SUBCYCLE_ADAPTIVE = 0, NSDG_SUBCYCLE_KEEP_ALPHA = 1, NSDG_SUBCYCLE_KEEP_DELTA_MIN = 2, NSDG_SUBCYCLE_ADAPTIVE_CONVERGED = 3 };
#define NSDG_AEVP_DELTA_REF 1.67e-6 /* 1/s: 14 % per day */
int nsdg_mevp_stable_params(nsdg_mevp_params* p, int32_t mode, double h, double dt);
/* strain rate below which the ice creeps instead of staying rigid (= delta_min), in percent per day */
double nsdg_mevp_creep_percent_per_day(const nsdg_mevp_params* p);

/* ---- sub-stepping: the model time step split by the ice's own strength wave speed (csrc/substep.hip) ----------------------------------
 * The explicit coupling of ice strength and transport (Lipscomb et al. 2007) is stable while the plastic wave of the current state crosses
 * at most about 1.5 cells per step: with the converging sub-cycle at 250 m, dt = 120 s leaves the physical range after 11 model hours and
 * dt = 60 s or 30 s does not, and at 125 m dt = 30 s completes -- the same c dt / h = 1.5 at a = 0.9 (profiles/r06_adaptive_noise.md).
 * The wave speed depends on the local concentration a only and grows with it,
 *     c^2 = (1 + C a) P* exp(-C (1 - a)) / (2 rho_ice)        (C = compaction; P* = 27 500, C = 20, rho_ice = 900: 6.27 m/s at a = 0.9,
 *                                                           17.91 m/s at a = 1),
 * so the fastest wave of a state is c(max a).  A host that opts in measures max a at the start of a model step (nsdg_concentration_max, then
 * nsdg_comm_max_f64 over the row blocks: every block must take the same n or the ghost exchanges stop matching) and runs the step as n
 * sub-steps of dt / n:
 *     n = max(1, ceil(c dt / (courant h))),   h = min(hx, hy),   courant = 1.5 by default (NSDG_SUBSTEP_COURANT)
 * 1.5 is the largest ratio shown to work, read off the record at a = 0.9; the rule takes c at max a, which may reach 1 (the ridging cap
 * allows it), so it can be conservative there: at a = 1 the runs that completed sit at c dt / h = 4.3 (profiles/r07_substeps.md).
 * A step of n = 1 is the unsplit step, bit for bit.
 *
 * nsdg_concentration_max: the largest clamped concentration clamp(A, 0, 1) at the 3x3 Gauss points of the elements of rows [j0, j1) (the
 * points and the clamp of nsdg_ice_strength), over the points where the clamped mean thickness max(H, 0) is > 0; 0 where there are none.
 * Rows outside [j0, j1) (ghost rows) do not count.  H and A are DG2 fields (6 coefficient planes).  Every raw coefficient and every
 * unclamped point value is checked: a non-finite one returns NSDG_ERR_ARG with the element in nsdg_last_error(), never a number.  One
 * launch; the maximum of the bit patterns (exact, independent of the launch order) travels in one 8-byte copy; the call waits for it (on a
 * context with a communicator within the communicator's deadline: NSDG_ERR_COMM on expiry).
 * nsdg_substep_count: n by the rule above for the mEVP parameters' pstar, compaction and rho_ice, and c (may be NULL).  amax in [0, 1], h,
 * dt, courant finite and positive, max_substeps >= 1, else NSDG_ERR_ARG.  If n would exceed max_substeps it returns NSDG_ERR_ARG with the
 * needed n in the message: n is never capped.  Host only: usable without a device. */
#define NSDG_SUBSTEP_COURANT 1.5
int nsdg_concentration_max(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* amax_host);
int nsdg_substep_count(const nsdg_mevp_params* p, double amax, double h, double dt, double courant, int32_t max_substeps, int32_t* n, double* c);

/* number of doubles of a tiled array (see "Data layout") */
int64_t nsdg_tiled_len(int32_t nx, int32_t ny, int32_t nc);

/* shape and cell size of the local element array all following calls refer to */
int nsdg_grid_set(nsdg_ctx* ctx, int32_t nx, int32_t ny, double hx, double hy);

/* kernel variant of the mEVP sub-cycle = the largest number of sub-iterations a kernel pass may perform:
 * 0 = two kernels per sub-iteration (element-wise stress, node-gather velocity); 1 = fused marching kernel, one launch per
 * sub-iteration (the bitwise reference of the multi-iteration passes); 2, 3, 4 = up to that many sub-iterations per pass on the
 * stage-per-wave pipeline (csrc/mevp_fused4.hip: one pipeline stage per wave of a four-wave workgroup, hand-over point to point
 * through LDS; nsdg_mevp_iterate2 / 3 / 4, nsdg_mevp_subcycle; what is left of a sub-cycle whose length is no multiple of the
 * variant runs as a shorter pass of the same kernel, a single sub-iteration on the kernel of variant 1).
 * NSDG_MEVP_DEFAULT_VARIANT (4) is the default of a new context.  Variants 1, 2, 3 and 4 agree bit for bit, variant 0 to fp64
 * round-off.  (Round 6 built passes of EIGHT -- two sub-iterations per stage wave -- bit-exact and slower: profiles/r06_fused8.md.)  (Rounds 1-4 had kernels of their own for 2 and 3 sub-iterations per pass -- two / three stages in ONE wave --
 * and a four-stage kernel with one workgroup barrier per march step: superseded, see the history of csrc/.) */
#define NSDG_MEVP_DEFAULT_VARIANT 4
int nsdg_mevp_variant_set(nsdg_ctx* ctx, int32_t variant);

/* CG2 velocity -> DG(order) velocity and edge-normal velocities used by the transport */
int nsdg_prepare_advection(nsdg_ctx* ctx, int32_t order, const double* u, const double* v, double* vx_dg,
    double* vy_dg, double* un_x, double* un_y);

/* transport stage kernel: 0 = one lane per element gathering all neighbours from memory, 2 (default) = two elements per
 * lane (16-byte accesses, the inner neighbour from registers; falls back to 0 for an odd nx or arrays that are not
 * 16-byte aligned).  Bit-identical results.  (1 was the marching kernel of rounds 1-2: never faster, removed.)
 * strip_rows: rows per workgroup (<= 4), 0 = default. */
int nsdg_transport_variant_set(nsdg_ctx* ctx, int32_t variant, int32_t strip_rows);

/* one Runge-Kutta stage on element rows [j0, j1) for nfields fields advected by the same velocity:
 *   out[f] = a*phi0[f] + b*(phis[f] + dt*L(phis[f]))
 * phi0/phis/out are HOST arrays of nfields DEVICE pointers. */
int nsdg_transport_stage(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, double dt, double a, double b,
    int32_t nfields, const double* const* phi0, const double* const* phis, double* const* out,
    const double* vx_dg, const double* vy_dg, const double* un_x, const double* un_y);

/* full SSP-RK(order+1) step over all rows (single-domain convenience); scratch: 2*nfields*nc*nx*ny */
int nsdg_transport_step(nsdg_ctx* ctx, int32_t order, double dt, int32_t nfields, double* const* phi,
    const double* vx_dg, const double* vy_dg, const double* un_x, const double* un_y, double* scratch);

/* The same step OUT OF PLACE in ONE launch: all Runge-Kutta stages of a step fused as a march -- a wave owns a window of
 * 64 - 2 (order + 1) element columns and a strip of rows and walks up the rows, stage k running k rows behind the newest row
 * read, the neighbours' edge traces taken from the adjacent lanes and from the rows the lane holds: every value is read once per
 * step, nothing goes through LDS, and the columns / rows at the edges of a window / strip are recomputed instead of exchanged.
 * For meshes whose step is bound by launch latency (BASELINE config 2: 512 x 512 DG1) and for callers that ping-pong their
 * fields.  phi_out must not alias phi_in.  Bit-identical to nsdg_transport_step. */
int nsdg_transport_step_oop(nsdg_ctx* ctx, int32_t order, double dt, int32_t nfields, const double* const* phi_in,
    double* const* phi_out, const double* vx_dg, const double* vy_dg, const double* un_x, const double* un_y);

/* The fused step on the rows [j0, j1) of the local array only (a row block's own rows): phi_in must be valid on order + 2 rows
 * below j0 and above j1 where the array has them (the ghost rows of a block whose ghost zone is at least that deep; the array
 * boundary needs none: nothing flows in).  Rows outside [j0, j1) of phi_out are not written. */
int nsdg_transport_step_oop_rows(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, double dt, int32_t nfields,
    const double* const* phi_in, double* const* phi_out, const double* vx_dg, const double* vy_dg, const double* un_x,
    const double* un_y);

/* Closure of a transport step (see "INPUT DOMAIN AND CLOSURE" above): bounds of the advected fields, in the order in which the
 * step entry points receive them.  nfields = 0 (default): no closure.  Once set, nsdg_transport_step, nsdg_transport_step_oop[_rows]
 * and nsdg_rb_transport_run apply cap + limiter to the new state before they return it (the marching launch in its epilogue, at
 * no extra memory traffic); they then require the same number of fields.  nsdg_transport_stage never limits.
 * The bounds are STATE OF THE CONTEXT: they apply to every later step call on it, whatever fields that call advances, until they are
 * set again (nfields = 0 clears them).  A row-block plan can carry its own instead (nsdg_rb_transport_desc.own_bounds), which then
 * neither reads nor changes the context's. */
typedef struct {
    double lo, hi; /* bounds at the quadrature points; hi = +infinity (HUGE_VAL): no upper bound */
    int32_t cap_mean; /* != 0: a cell mean above hi is set to hi (needs a finite hi) */
    int32_t reserved;
} nsdg_field_bounds;
int nsdg_transport_bounds_set(nsdg_ctx* ctx, int32_t nfields, const nsdg_field_bounds* bounds);

/* cap + limiter as a pass of its own, in place on the element rows [j0, j1) -- for callers that compose a step from
 * nsdg_transport_stage calls; bit-identical to what the step entry points apply.  NSDG_ERR_STATE without bounds. */
int nsdg_transport_limit(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, int32_t nfields, double* const* phi);

/* nodal average of a DG field on the CG2 lattice (mean thickness / concentration at the nodes) */
int nsdg_dg_to_cg(nsdg_ctx* ctx, int32_t ncoef, const double* f_dg, double* f_cg);

/* P = pstar * max(H,0) * exp(-C (1 - clamp(A,0,1))) at the 3x3 Gauss points of rows [j0, j1) */
int nsdg_ice_strength(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* pg);

/* ---- column state transport: the snow and the ice surface temperature ride on the moving ice (csrc/tracer.hip) ----------------------
 * In the coupled model the column step's other prognostic state moves with the ice (opt-in in both hosts; off by default).  The snow
 * volume per unit area hsnow is a DG2 field S of its own whose plane 0 IS the column's hsnow (as plane 0 of H is hice), advected with H
 * and A and bounded below by 0.  The surface temperature tice0 is intensive: it travels as the conserved product Q = H T, weighted by
 * the ice VOLUME H (not A: the ridging cap changes the mean of A but never the mean of H, and the scaling limiter changes no cell mean),
 * so sum_e mean(H)_e T_e is conserved by the transport up to rounding.  Q is unbounded (-HUGE_VAL, HUGE_VAL, no cap) and is rebuilt
 * every step.  A coupled transport step is: nsdg_tracer_weight, one transport step of the four fields H, A, S, Q, nsdg_tracer_recover.
 *
 * nsdg_tracer_weight: Q[c*nx*ny + e] = T[e] * H[c*nx*ny + e] for every coefficient c < nc(order) of the elements of rows [j0, j1); T is
 * one plane (tice0 is DG0).  The product of a constant and a DG field is exact: the result is that multiplication, bit for bit.
 * nsdg_tracer_recover: where an element holds ice after the step -- mean(H) > 0, mean(A) >= min_conc and mean(H) >= min_thick * mean(A),
 * the test of the ice-free-node rule (nsdg_mevp_params.min_conc / min_thick), false for a NaN -- T[e] = mean(Q) / mean(H) (plane 0 of
 * each, one IEEE division); everywhere else T[e] keeps its value (the column step ignores tice0 where there is no ice).
 * Both are element-local: a row block runs them on its ghost rows too, which then stay bit-identical to their owners without an
 * exchange.  Stream-ordered, one launch each; Q must not alias H or T, nor T (nsdg_tracer_recover) H, A or Q.  A null pointer, an order
 * outside 0..2, a row range outside the local array or an overlap of those arrays (nc(order) nx ny doubles of a DG field, nx ny of T):
 * NSDG_ERR_ARG, and nothing is launched. */
int nsdg_tracer_weight(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, const double* T, double* Q);
int nsdg_tracer_recover(nsdg_ctx* ctx, int32_t order, int32_t j0, int32_t j1, const double* H, const double* A, const double* Q,
    double min_conc, double min_thick, double* T);

/* ---- ice tracers: ice age and passive tracers ride on the moving ice (csrc/tracers.hip) ------------------------
 * Up to NSDG_TRACERS_MAX intensive planes travel as Q = H T in a transport run of their own: weight before it, recover after it, dilute
 * after the column step.  The three calls, their arithmetic and their checks are declared in nsdg_tracers.h, which this header includes. */
#include "nsdg_tracers.h"

/* ---- external forcing providers, evaluated on the device at the model time of each step (csrc/forcing.hip) ----
 * They replace DummyExternalData::setAll (core/src/include/DummyExternalData.hpp:22-34: the same eight constants in
 * every element, set once) and fill PhysicsData::windSpeed (physics/src/include/PhysicsData.hpp:26,44), which a run
 * of the reference never sets.
 *
 * Placement of the local array in the global domain for these providers: local element row 0 is global row `row0`
 * of `ny_global` rows (defaults 0 and the local ny: a single domain).  A row block then evaluates the very
 * expressions the single domain evaluates, bit for bit. */
int nsdg_block_set(nsdg_ctx* ctx, int32_t row0, int32_t ny_global);

/* Square box test of side domain_size [m] at model time t [s] on the CG2 lattice of the local array: cyclone wind
 * (ua, va), its centre drifting along the diagonal, and circular ocean current (uo, vo); either pair may be NULL. */
int nsdg_boxtest_forcing(nsdg_ctx* ctx, double domain_size, double t, double* ua, double* va, double* uo, double* vo);

/* Thermodynamic forcing planes of the column step (nx*ny doubles each) at model time t [s]:
 * NSDG_FORCING_DUMMY = the reference's constants (tair -1, tdew -4, slp 1e5, qsw 0, qlw 311, mld 10, snowfall 0);
 * NSDG_FORCING_WINTER = smooth winter fields in the ranges of SURVEY.md section 8(d): a synoptic pattern drifting eastwards
 * with a 5-day period and a diurnal cycle of the short-wave flux. */
enum { NSDG_FORCING_DUMMY = 0, NSDG_FORCING_WINTER = 1 };
int nsdg_column_forcing(nsdg_ctx* ctx, int32_t kind, double t, double* tair, double* tdew, double* slp, double* qsw, double* qlw,
    double* mld, double* snowfall);

/* wind speed of the column step = |u_a| at the element centre (CG2 node (2 ix + 1, 2 iy + 1)) */
int nsdg_column_wind(nsdg_ctx* ctx, const double* ua, const double* va, double* wind);

/* Forcing from a file (csrc/forcing_file.hip): two records rec0, rec1 already on the device, each of nfields planes of nyr x nxr
 * doubles (row-major, x fastest) on one lattice, sampled onto the local array and interpolated in time with weight w:
 *     out[k] = lerp(S(rec0[k]), S(rec1[k]), w),   lerp(a, b, f) = a + f (b - a)   (the device may contract it to an FMA)
 * Target (where): NSDG_AT_NODES = the CG2 node lattice, (2 nx + 1) x (2 ny + 1) values per plane (wind and ocean components);
 * NSDG_AT_ELEMENTS = the element centres, nx x ny (column forcing planes).
 * Lattice: cell-centred over the model's square domain, point i at x / L = (i + 1/2) / nxr, the same in y with nyr.
 * S, the bilinear sample: the index-space coordinate of a target point is num / den, computed in integers and divided once --
 *     node gx:    num = gx nxr - nx,            den = 2 nx;     element ix:  num = (2 ix + 1) nxr - nx,  den = 2 nx
 * and in y the same with the GLOBAL row (node row gy + 2 row0, element row iy + row0) and ny_global of nsdg_block_set in place of nx.
 * num <= 0 takes index 0 with weight 0; num >= (nxr - 1) den takes index nxr - 1 with weight 0; otherwise i0 = num / den (integer
 * division), i1 = i0 + 1, f = (double)(num - i0 den) / den.  The sample interpolates along x on rows j0 and j1, then along y:
 *     S = lerp(lerp(r[j0][i0], r[j0][i1], fx), lerp(r[j1][i0], r[j1][i1], fx), fy)
 * Consequences, bit for bit: a constant field comes out constant; w = 0 gives rec0's sample; nxr = 1 (nyr = 1) is constant along x
 * (y); nxr = nx and nyr = ny_global at the element centres is the identity; a row block computes what the whole domain computes for
 * its rows, ghost rows included.
 * Null pointers, nxr or nyr < 1 or > NSDG_FORCING_MAX_LATTICE, nfields outside [1, NSDG_FORCING_MAX_FIELDS], an unknown `where`, or
 * a w that is not finite or outside [0, 1] return NSDG_ERR_ARG.  One launch; asynchronous on the context's stream. */
enum { NSDG_AT_NODES = 0, NSDG_AT_ELEMENTS = 1 };
#define NSDG_FORCING_MAX_FIELDS 8
#define NSDG_FORCING_MAX_LATTICE 65536
int nsdg_forcing_sample(nsdg_ctx* ctx, int32_t where, int32_t nxr, int32_t nyr, int32_t nfields, const double* const* rec0,
    const double* const* rec1, double w, double* const* out);

/* tau_a = c_atm * rho_atm * |u_a| u_a at nnodes nodes */
int nsdg_wind_stress(nsdg_ctx* ctx, int64_t nnodes, const double* ua, const double* va, double* tax, double* tay);

/* mEVP stress update (in place) on element rows [k0, k1):  S <- (1-1/alpha) S + (1/alpha) Proj sigma(v) */
int nsdg_mevp_stress(nsdg_ctx* ctx, int32_t k0, int32_t k1, const double* u, const double* v, const double* pg,
    double* s11, double* s12, double* s22);

/* Per-step coefficients of the momentum update at every CG2 node in an internal packed layout
 * (6 doubles per node, csrc/mevp_common.h), valid for the whole sub-cycle of one time step because
 * u0, v0, the wind stress, the ocean current and the nodal H, A do not change inside it.  The context
 * remembers dt and the mEVP parameters of the packing for the following iterate/velocity calls.
 * `packed` must hold 8*(2nx+1)*(2ny+1) doubles (6 used; 8 with a depth array set, nsdg_basal.h) and be 16-byte aligned. */
int nsdg_mevp_pack_nodal(nsdg_ctx* ctx, double dt, const double* u0, const double* v0, const double* tax,
    const double* tay, const double* uo, const double* vo, const double* cgh, const double* cga, double* packed);

/* The whole per-step nodal preparation in one launch: nodal means of the DG2 fields H and A, wind stress of
 * (ua, va) and coefficient packing -- equivalent to nsdg_dg_to_cg x2 + nsdg_wind_stress + nsdg_mevp_pack_nodal
 * (bit-identical `packed`) without materialising cgH, cgA and tau_a.  u0, v0: velocity at the start of the step. */
int nsdg_mevp_prepare(nsdg_ctx* ctx, double dt, const double* H, const double* A, const double* ua, const double* va,
    const double* uo, const double* vo, const double* u0, const double* v0, double* packed);

/* mEVP velocity update of the nodes owned (bottom-left) by element rows [j0, j1) */
int nsdg_mevp_velocity(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11, const double* s12,
    const double* s22, const double* u_old, const double* v_old, double* u_new, double* v_new,
    const double* packed);

/* one complete sub-iteration: stress on element rows [k0, j1) (S_out <- relax(S_in, u_old)), then the
 * velocity of the nodes owned by rows [j0, j1) from S_out.  Out-of-place in both the stress and the
 * velocity, so a row may be updated redundantly by two owners (a rank and its neighbour, or two row
 * strips of the fused kernel) with bit-identical results.  k0 == j0 - 1 (one redundant ghost row below)
 * or k0 == j0 == 0 (rows start at the physical boundary).  Used by multi-rank drivers that exchange
 * velocity halos between sub-iterations. */
int nsdg_mevp_iterate(nsdg_ctx* ctx, int32_t k0, int32_t j0, int32_t j1, const double* s11_in, const double* s12_in,
    const double* s22_in, double* s11_out, double* s12_out, double* s22_out, const double* u_old,
    const double* v_old, double* u_new, double* v_new, const double* packed, const double* pg);

/* TWO complete sub-iterations in one pass on the owned element rows [j0, j1): reads S_in, u_old on rows
 * j0-2 .. j1 (node rows 2(j0-2) .. 2*j1+2) and writes S_out = S^{p+2} on rows [j0, j1) and u_new = u^{p+2} on
 * the nodes they own; the intermediate stress and velocity never leave the registers.  j0 == 0 (physical
 * boundary) or j0 >= 2 (two ghost rows below); above, one ghost row or the physical boundary (j1 == ny).
 * A multi-rank driver refreshes the ghost rows of S_out and u_new after every pass (or runs k passes on row ranges
 * shrinking by 2 rows per side and pass on a (2k, 2k-1)-row ghost zone).  Requires variant >= 2. */
int nsdg_mevp_iterate2(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11_in, const double* s12_in,
    const double* s22_in, double* s11_out, double* s12_out, double* s22_out, const double* u_old, const double* v_old,
    double* u_new, double* v_new, const double* packed, const double* pg);

/* THREE complete sub-iterations in one pass on the owned element rows [j0, j1): reads S_in, u_old on rows
 * j0-3 .. j1+1 and writes S_out = S^{p+3} on rows [j0, j1) and u_new = u^{p+3} on the nodes they own.  j0 == 0
 * or j0 >= 3 (three ghost rows below); j1 == ny or j1 + 2 <= ny (two ghost rows above).  Requires variant >= 3. */
int nsdg_mevp_iterate3(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11_in, const double* s12_in,
    const double* s22_in, double* s11_out, double* s12_out, double* s22_out, const double* u_old, const double* v_old,
    double* u_new, double* v_new, const double* packed, const double* pg);

/* The same on TWO disjoint row ranges [j0a, j1a) and [j0b, j1b) in ONE launch -- the two bands of rows whose results a row
 * block sends to its neighbours: as one launch they share the resident wave slots instead of paying two pipeline fills
 * one after the other.  Each range obeys the ghost-row conditions of nsdg_mevp_iterate3; bit-identical to two calls. */
int nsdg_mevp_iterate3_pair(nsdg_ctx* ctx, int32_t j0a, int32_t j1a, int32_t j0b, int32_t j1b, const double* s11_in, const double* s12_in,
    const double* s22_in, double* s11_out, double* s12_out, double* s22_out, const double* u_old, const double* v_old, double* u_new,
    double* v_new, const double* packed, const double* pg);

/* FOUR complete sub-iterations in one pass on the owned element rows [j0, j1): reads S_in, u_old on rows
 * j0-4 .. j1+2 and writes S_out = S^{p+4} on rows [j0, j1) and u_new = u^{p+4} on the nodes they own.  j0 == 0
 * or j0 >= 4 (four ghost rows below); j1 == ny or j1 + 3 <= ny (three ghost rows above).  Requires variant 4. */
int nsdg_mevp_iterate4(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11_in, const double* s12_in,
    const double* s22_in, double* s11_out, double* s12_out, double* s22_out, const double* u_old, const double* v_old,
    double* u_new, double* v_new, const double* packed, const double* pg);

/* The same on TWO disjoint row ranges in ONE launch (see nsdg_mevp_iterate3_pair); each range obeys the ghost-row
 * conditions of nsdg_mevp_iterate4; bit-identical to two calls. */
int nsdg_mevp_iterate4_pair(nsdg_ctx* ctx, int32_t j0a, int32_t j1a, int32_t j0b, int32_t j1b, const double* s11_in, const double* s12_in,
    const double* s22_in, double* s11_out, double* s12_out, double* s22_out, const double* u_old, const double* v_old, double* u_new,
    double* v_new, const double* packed, const double* pg);

/* nsub sub-iterations over the whole local array (packs the nodal coefficients, then iterates);
 * result in s11/s12/s22 and u, v (u0/v0 may be the same arrays as u/v).  scratch: 10*(2nx+1)*(2ny+1) + 24*nx*ny doubles, 16-byte aligned
 * (packed coefficients + ping-pong copies of the velocity and the stress). */
int nsdg_mevp_subcycle(nsdg_ctx* ctx, double dt, int32_t nsub, double* s11, double* s12, double* s22, double* u,
    double* v, const double* u0, const double* v0, const double* tax, const double* tay, const double* uo,
    const double* vo, const double* cgh, const double* cga, const double* pg, double* scratch);

/* The waits of the stage-per-wave pipeline (csrc/mevp_fused4.hip, csrc/mevp_p2p.h) are bounded: a wave that waits for
 * a hand-over longer than ~0.2 s gives up, releases the other waits of its workgroup and reports the event -- the launch then finishes
 * with WRONG results instead of hanging the GPU.  The report reaches the host without being asked for: the kernel sets a flag in host
 * memory that belongs to the context, and from then on nsdg_ctx_synchronize (after the launch has completed), nsdg_mevp_subcycle and
 * nsdg_rb_mevp_run (at their next call) return NSDG_ERR_HIP -- sticky, until this call takes the events.  This call waits for the
 * context's stream, returns the number of events since the last call (0 in a correct program), resets the count and clears the
 * error status.  Counter and flag are per context. */
int nsdg_mevp_pipeline_health(nsdg_ctx* ctx, uint32_t* waits_given_up);

/* rows per strip of the fused marching kernel (performance knob; results do not depend on it);
 * 0 (default) = chosen per launch from the row count and the number of resident wave slots */
int nsdg_mevp_strip_rows_set(nsdg_ctx* ctx, int32_t rows);
/* register budget of the fused kernel: 1 or 2 resident waves per SIMD (performance knob) */
int nsdg_mevp_occupancy_set(nsdg_ctx* ctx, int32_t waves_per_simd);

/* ---- land mask: coastlines as fixed nodes of the mEVP sub-cycle (csrc/landmask.hip) ------------------------------
 * No counterpart in the reference snapshot.  land[iy * nx + ix] (1 = land, 0 = ocean) is an element mask on the LOCAL array, ghost rows
 * included.  A CG2 node is a land node if any element adjacent to it inside the local array is land; a land node holds u = v = 0 in every
 * sub-iteration, exactly as the nodes on the array edge do (no-slip coast).  Nothing else changes: an ocean node has only ocean elements
 * around it (its nodal means, the ice-free rule and the adaptive alpha / beta are what they were), no flux crosses a coast edge (three land
 * nodes: the edge-normal velocity at its Gauss points is exactly 0), so the unchanged transport keeps land elements that start at
 * H = A = 0 at exactly 0, and land carries no stress (P = 0, strain rate 0).  The caller starts with H = A = 0, u = v = 0 on land
 * (nsdg_land_clear*) and clears what a source outside the scheme -- the column step -- writes there.
 *
 * nsdg_land_mask_set: `land` is a device pointer to nx * ny bytes, owned by the caller and valid while it is set; stream-ordered like every
 *   other array argument.  NULL clears the mask.  Before nsdg_grid_set: NSDG_ERR_STATE.  An nsdg_grid_set that changes the shape clears the
 *   mask, the same shape keeps it.  The mask acts through the coefficient packing: nsdg_mevp_prepare / nsdg_mevp_pack_nodal (and
 *   nsdg_mevp_subcycle, which packs) mark the land nodes, land taking precedence over the ice-free rule, and every pass that reads that
 *   packing -- nsdg_mevp_iterate*, nsdg_mevp_velocity, nsdg_rb_mevp_run -- holds them at 0.  The passes read no array and no byte they
 *   did not read before; a context without a mask runs the same kernels as ever.
 * nsdg_land_clear: f[c * nx * ny + e] = 0 for c < nplanes at the land elements e of the rows [j0, j1) -- a store, so a NaN is cleared.
 *   Rows outside the local array, nplanes < 1 or a null f: NSDG_ERR_ARG.  Without a mask it does nothing.  One launch.
 * nsdg_land_clear_nodes: u = v = 0 at the land nodes of the local array's CG2 lattice.  Without a mask it does nothing.  One launch. */
int nsdg_land_mask_set(nsdg_ctx* ctx, const uint8_t* land);
int nsdg_land_clear(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nplanes, double* f);
int nsdg_land_clear_nodes(nsdg_ctx* ctx, double* u, double* v);

/* ---- landfast ice: grounding on shoals as a basal stress in the momentum update (csrc/basal.hip) ---------------
 * A static water depth per element makes the packing store the critical stress T_b of Lemieux et al. (2015) as the seventh packed
 * coefficient of a node, and the passes that read such a packing add C_b = T_b / (|u| + u0) to the denominator of the velocity update.
 * The parameters, the depth array, the diagnostic T_b and their checks are declared in nsdg_basal.h, which this header includes. */
#include "nsdg_basal.h"

/* ---- slab ocean: the mixed layer's heat and salt follow the ice (csrc/column_step.hip) ------------------------
 * The column step above leaves sst and sss as it found them.  Its fused twin advances them by the ice-ocean and open-water fluxes and
 * by the fresh water and salt the pack takes up and releases, with an optional relaxation towards external values.  The call, its
 * parameters, its arithmetic and its checks are declared in nsdg_ocean.h, which this header includes. */
#include "nsdg_ocean.h"

/* ---- snow load: the momentum equation feels the snow's weight (csrc/snowload.hip) ------------------------------
 * A snow field on the context makes the packing take the nodal mass from h' = max(cgH + (rho_snow / rho_ice) max(cgS, 0), h_min) where the
 * node is neither land nor ice-free; the passes read c[0] as ever.  The field, the diagnostic h' and their checks are declared in
 * nsdg_snow.h, which this header includes. */
#include "nsdg_snow.h"

/* ---- sea-surface tilt from a sea-surface height (csrc/tilt.hip) ------------------------------------------------
 * A sea-surface height on the context makes the packing write the tilt force as -m g grad(eta), from a centred difference on the CG2
 * lattice, in place of the Coriolis terms of the ocean current; the passes read c2, c3 as ever.  The field, the diagnostic gradient, the box
 * test's height and their checks are declared in nsdg_tilt.h, which this header includes. */
#include "nsdg_tilt.h"

/* ---- momentum balance diagnostics: nodal forces and their power (csrc/budget.hip) ------------------------------
 * One launch after the sub-cycle evaluates every term of the nodal momentum balance -- wind, water drag, Coriolis, sea-surface tilt,
 * internal stress divergence, seabed stress, inertia -- and the residual of the implicit step, at the state the sub-cycle left and with the
 * coefficients of its packing; per element row, the power of every term and the kinetic energy in a fixed order of summation.  The
 * arithmetic, the outputs and their checks are declared in nsdg_budget.h, which this header includes. */
#include "nsdg_budget.h"

/* ---- brittle rheology: the brittle Bingham-Maxwell (BBM) sub-cycle (csrc/bbm.hip, csrc/bbm_common.h) ------------
 * A second rheology beside mEVP: damage, a Mohr-Coulomb envelope, Maxwell relaxation.  No counterpart in the reference snapshot; built from
 * the published formulation (Olason et al. 2022, "A new brittle rheology and numerical framework for large-scale sea-ice models", JAMES;
 * Dansereau et al. 2016) -- parity unpinned like the rest of the dynamics.  The DEFAULTS of nsdg_bbm_default_params follow the publication
 * as far as it could be recalled when this was written; no source at hand confirmed them: check them against the paper before relying on them.
 *
 * State.  sigma: three DG8 stress components in Pa (NOT thickness-integrated), the tiled arrays the mEVP sub-cycle uses.  D: damage in
 * [0, 1], a DG2 field of 6 coefficient planes (plane layout), updated in the sub-cycle and carried by the transport as a third field
 * with the bounds (0, 1, cap_mean = 0).
 *
 * Per model step, nsdg_bbm_prepare writes what the sub-cycle does not change: three tiled 9-component arrays with the layout of pg,
 *     hg_q = max(H(q), 0),   eg_q = exp(-C (1 - clamp(A(q), 0, 1))),   pm_q = p0 hg_q sqrt(hg_q) eg_q
 * (C = nsdg_mevp_params.compaction; the Gauss points and clamps of nsdg_ice_strength), and the caller packs the nodal coefficients with
 * nsdg_mevp_prepare(dt = dt_s, ..., u0 = v0 = an array of zeros): nothing in the packing changes, the term (m / dt) u0 is exactly 0,
 * and ice-free nodes, free drift and land nodes cost the BBM pass nothing new.
 *
 * Per sub-iteration and Gauss point q, in THIS order (dt_s = the packing's time step; the strain rate from u_old, v_old; sigma_q and d
 * from the old coefficients, the damage with coefficients 6 and 7 zero):
 *   1. clamp and heal      d = min(max(d, 0), d_max);   d <- max(0, d - dt_s / t_heal)
 *   2. stiffness           x = (1 - d) eg_q;   E = young x;   lambda = lambda0 x^(n - 1),  n = relax_exponent, by repeated multiplication
 *   3. compressive limit   from the OLD stress: sigma_n = (sigma11 + sigma22) / 2;   Pt = sigma_n < 0 ? min(1, -pm_q / sigma_n) : 0
 *   4. relaxation          m = min(1 - 1e-12, lambda / (lambda + dt_s (1 - Pt)))
 *   5. predictor           k1 = 1 / (1 + nu), k2 = nu / (1 - nu^2), tr = e11 + e22:
 *                          sigma11 <- (sigma11 + dt_s E (k1 e11 + k2 tr)) m;   sigma22 likewise;   sigma12 <- (sigma12 + dt_s E k1 e12) m
 *   6. Mohr-Coulomb        on the new stress: sigma_n as above, sigma_s = sqrt((sigma11 - sigma22)^2 / 4 + sigma12^2),
 *                          den = sigma_s + tan_phi sigma_n,  c = cohesion_lab sqrt(0.1 / h), h = min(hx, hy) (formed on the host per launch);
 *                          sigma_n < -N (N = compr_strength): d_c = -N / sigma_n;   else den > c: d_c = c / den;   else d_c = 1
 *   7. damage              r = min(1, dt_s sqrt(E) / (h sqrt(2 (1 + nu) rho_ice)))  (the sub-step over the time an elastic shear wave needs
 *                          to cross a cell);   f = (1 - d_c) r;   d <- min(d_max, d + (1 - d) f);   sigma <- sigma (1 - f), all three
 *   8. projection          S_out = Proj8(sigma_q);   D_out = coefficients 0..5 of Proj8(d_q) (the basis is orthogonal: the DG2 projection)
 *   9. momentum            the nodal contributions of Proj8(hg_q sigma_q) -- the momentum equation takes the thickness-integrated stress --
 *                          enter the mEVP node update with K1 = K2 = rho_ice / dt_s:
 *                          u' = ((m / dt_s) u + a tau_x + c_d u_o + m f_c (v - v_o) + div_x / M) / (m / dt_s + c_d),
 *                          explicit in stress and Coriolis, implicit in ocean drag.
 * The scheme is discontinuous in two places only: Pt jumps at sigma_n = 0 and d_c jumps at sigma_n = -N; the envelope test is continuous
 * at den = c.  alpha, beta and aevp_* of nsdg_mevp_params are ignored by the BBM pass (an adaptive context may run it); rho_ice, fc, the
 * drags and compaction are those of nsdg_mevp_params.
 *
 * nsdg_bbm_params_set: NSDG_ERR_ARG for a non-finite member, relax_exponent < 1, d_max outside (0, 1) or a non-positive young, lambda0 or
 *   t_heal.
 * nsdg_bbm_params_check: the same checks without a context (host only): a host validates its configuration before it touches a device.
 * nsdg_bbm_iterate: one sub-iteration, the stress and damage on element rows [k0, j1), the velocity of the nodes owned by rows [j0, j1);
 *   the row conventions of nsdg_mevp_iterate (k0 == j0 - 1 or k0 == j0 == 0).  Stress AND damage are out of place: a row may be updated
 *   redundantly by two owners with bit-identical results, so a row block needs no exchange of D inside the sub-cycle.  A null pointer, an
 *   *_out that aliases its *_in or a bad range: NSDG_ERR_ARG; before a packing: NSDG_ERR_STATE.  The instantiation that holds land nodes
 *   at 0 is chosen from what the packing saw, as for the mEVP passes; nsdg_mevp_strip_rows_set applies (results do not depend on it).
 * nsdg_bbm_substep_count: host only, the elastic-wave rule stated once: nsub = max(1, ceil(dt c_E / (courant h))), c_E = sqrt(young /
 *   (rho_ice (1 - nu^2))).  If that exceeds max_nsub: NSDG_ERR_ARG with the needed value in the message; the result is never capped.
 *   NSDG_BBM_COURANT, the default the hosts pass: 0.25, measured (profiles/r09_bbm.md).  On the 64 x 64 box test at 1 km (full undamaged
 *   cover, cyclone wind, 200 model steps of 120 s) all of 1, 0.7, 0.5, 0.35, 0.25 stay finite and below 1 m/s, but only 0.35 and 0.25 agree
 *   with each other (largest speed 1.24e-4 / 1.25e-4 m/s, no damage); at 0.5 and above the sub-cycle rings at element scale, the noise
 *   reaches the envelope and breaks the cover (damage up to 0.86, speeds 100 to 1000 times larger): finite, and wrong.  0.35 is the
 *   largest value that works, 0.25 the next smaller one of the list. */
typedef struct {
    double young; /* Pa, undamaged elastic modulus */
    double nu; /* Poisson ratio */
    double p0; /* scale of the compressive limit pm = p0 h^(3/2) exp(-C (1 - a)) */
    double lambda0; /* s, undamaged relaxation time */
    double tan_phi; /* internal friction */
    double cohesion_lab; /* Pa, cohesion at the laboratory scale of 0.1 m */
    double compr_strength; /* Pa, N */
    double t_heal; /* s */
    double d_max; /* in (0, 1) */
    int32_t relax_exponent; /* n >= 1 */
    int32_t reserved;
} nsdg_bbm_params;
#define NSDG_BBM_COURANT 0.25
void nsdg_bbm_default_params(nsdg_bbm_params* p);
int nsdg_bbm_params_set(nsdg_ctx* ctx, const nsdg_bbm_params* p);
int nsdg_bbm_params_check(const nsdg_bbm_params* p); /* host only, no context: NSDG_OK, or NSDG_ERR_ARG with nsdg_bbm_params_set's message */
int nsdg_bbm_prepare(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* hg, double* eg, double* pm);
int nsdg_bbm_iterate(nsdg_ctx* ctx, int32_t k0, int32_t j0, int32_t j1, const double* s11_in, const double* s12_in, const double* s22_in,
    double* s11_out, double* s12_out, double* s22_out, const double* D_in, double* D_out, const double* u_old, const double* v_old,
    double* u_new, double* v_new, const double* packed, const double* hg, const double* eg, const double* pm);
int nsdg_bbm_substep_count(const nsdg_bbm_params* p, double rho_ice, double h, double dt, double courant, int32_t max_nsub, int32_t* nsub);

/* ---- history output: time means and snapshots accumulated on the device (csrc/history.hip) ----------------------------
 * No counterpart in the reference snapshot, which writes its restart file and nothing else.  The fields below are element-local functions of
 * arrays that sit on the device at the end of every model step, so a host samples them with ONE streaming launch per step into accumulator
 * planes it owns, downloads those once per output window and divides by the number of samples.
 *
 * nsdg_history_accumulate: for every element (iy, ix) of the local rows [j0, j1) and every k < nfields
 *     acc[k * plane_stride + (iy - row0) * nx + ix]  (store ? = : +=)  x_fields[k](e)
 *   One launch on the context's stream, one lane per element; every source value is loaded at most once per element, whatever the list.
 *   The accumulation over time is sequential per element: the result depends on nothing but the samples -- not on the row range, the strip
 *   or the decomposition.  store != 0 OVERWRITES (it does not add to zero): a NaN left in acc is dropped and no memset is needed.  acc is
 *   nfields planes of plane_stride doubles each; row0 is the local row that plane row 0 stands for (a row block passes its first owned
 *   row and keeps planes of its owned rows only).  Rows outside [j0, j1) are not written.
 *
 * The samples x_f(e), normative:
 *   hice, cice, hsnow, tice, damage   H[e], A[e], hsnow[e], tice[e], D[e]: plane 0 of the field -- the cell mean --, unclamped
 *   u, v                              the velocity at the CG2 centre node of the element, n = (2 iy + 1) (2 nx + 1) + 2 ix + 1
 *   speed                             sqrt(u u + v v) at that node
 *   divergence, shear                 with E / W = the nodes (2 iy + 1, 2 ix + 2) / (2 iy + 1, 2 ix) and N / S = (2 iy + 2, 2 ix + 1) / (2 iy, 2 ix + 1):
 *                                         e11 = (uE - uW) / hx,   e22 = (vN - vS) / hy,   g = (uN - uS) / hy + (vE - vW) / hx
 *                                     -- the exact derivatives of the biquadratic velocity at the element centre --
 *                                         divergence = e11 + e22,   shear = sqrt((e11 - e22)^2 + g g)      [1/s]
 *   sigma_n, sigma_s                  (s11_0 + s22_0) / 2  and  sqrt((s11_0 - s22_0)^2 / 4 + s12_0^2)  from coefficient 0 of the tiled stress,
 *                                     a[T + 2 l] in "Data layout": the cell mean, because the other seven basis functions have zero mean.
 *                                     The unit is whatever the rheology stores: the thickness-integrated stress [N/m] of the mEVP
 *                                     sub-cycle, the stress [Pa] of the BBM sub-cycle.
 *   Every operation is one fp64 operation (IEEE add, multiply, divide; the device's square root); the device may contract a product and a
 *   sum into an FMA.
 *
 * Checks, as for nsdg_tracer_*: grid set (else NSDG_ERR_STATE); 0 <= j0 <= j1 <= ny; 1 <= nfields <= NSDG_HISTORY_MAX_FIELDS; known ids, no
 *   id twice; a field whose source pointer is NULL is refused with a message that names the field (sources no listed field reads may be
 *   NULL); 0 <= row0 <= j0 and plane_stride >= (j1 - row0) nx: NSDG_ERR_ARG.  j0 == j1 does nothing.
 * nsdg_history_field_name: the name of an id (NULL for an unknown id); nsdg_history_field_id: the id of a name, -1 if unknown.  Host only.
 * The call belongs to no phase of the phase table: the hosts make it after their NSDG_PHASE_END mark. */
#define NSDG_HISTORY_MAX_FIELDS 16
enum {
    NSDG_HIST_HICE = 0, NSDG_HIST_CICE, NSDG_HIST_U, NSDG_HIST_V, NSDG_HIST_SPEED, NSDG_HIST_DIVERGENCE, NSDG_HIST_SHEAR, NSDG_HIST_SIGMA_N,
    NSDG_HIST_SIGMA_S, NSDG_HIST_HSNOW, NSDG_HIST_TICE, NSDG_HIST_DAMAGE, NSDG_HIST_COUNT
};
typedef struct {
    const double *H, *A; /* DG fields: plane 0 is read (nsdg_points_sample: every plane of its order) */
    const double *u, *v; /* CG2 velocity */
    const double *s11, *s12, *s22; /* tiled stress */
    const double *hsnow, *tice; /* one plane each (plane 0 of the snow field S under column state transport) */
    const double* D; /* damage of the brittle rheology: plane 0 is read */
} nsdg_history_sources;
int nsdg_history_accumulate(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nfields, const int32_t* fields, const nsdg_history_sources* src,
    int32_t store, int32_t row0, int64_t plane_stride, double* acc);
const char* nsdg_history_field_name(int32_t field);
int nsdg_history_field_id(const char* name);

/* nsdg_history_accumulate_stats: nsdg_history_accumulate -- the same single launch, the same samples, every source value still loaded at
 * most once per element -- with a statistic per plane.  For every pair (fields[k], stats[k]), x = x_fields[k](e), p = the element's slot of
 * plane k:
 *   NSDG_STAT_MEAN       p (store ? = : +=) x.  A list of nothing but MEAN equals nsdg_history_accumulate bit for bit.
 *   NSDG_STAT_ICE_MEAN   w = min(max(A[e], 0), 1) from plane 0 of src.A (a NaN stays a NaN);  t = w x, rounded as a statement of its own and
 *                        never fused into the sum;  p (store ? = : +=) t.  The ONE weight plane takes
 *                            wacc[(iy - row0) nx + ix] (store ? = : +=) w
 *                        once per element if any pair of the list is ICE_MEAN, and is not touched otherwise.
 *   NSDG_STAT_MIN / MAX  store: p = x; else MIN: p = (x < p || x != x) ? x : p, MAX: p = (x > p || x != x) ? x : p.  A NaN sample makes the
 *                        extreme NaN and it stays NaN, as the sums keep a NaN.
 * The host finishes a window of n samples: MEAN acc / n; ICE_MEAN acc / wacc where wacc > 0 and NaN elsewhere (no ice in the window);
 * MIN / MAX as stored.  A field may be listed with several statistics; the same pair twice is refused by name.
 * Checks: those of nsdg_history_accumulate, and NSDG_ERR_ARG for an unknown stat id, for ICE_MEAN with src->A == NULL (the message names the
 * field and A) and for ICE_MEAN with wacc == NULL.  wacc may be NULL when no pair is ICE_MEAN.
 *
 * nsdg_history_row_totals: the scalars of a time series, one value per ROW and quantity:
 *     out[k * q_stride + (iy - row0)] = R_quantities[k](iy)   for iy in [j0, j1); always overwrites; no other slot is written.
 *   With w as above and speed = the sample of NSDG_HIST_SPEED, the row terms x(iy, ix) -- each formed in a statement of its own before it
 *   enters the reduction, all dimensionless: the host multiplies by hx hy once -- and their reductions are
 *     area  w, sum      extent  A[e] >= extent_conc ? 1 : 0, sum      volume  max(H[e], 0), sum      snow_volume  max(hsnow[e], 0), sum
 *     drift  w speed, sum      speed_max  speed, max      hice_max  H[e], max         (max: the NaN-propagating rule of NSDG_STAT_MAX)
 *   The order of a row's reduction is normative: lane l of 64 folds ix = l, l + 64, l + 128, ... in ascending order, starting from the
 *   identity (0 for a sum, -inf for a max); then for s = 32, 16, 8, 4, 2, 1: p_l = op(p_l, p_(l + s)) for l < s; R = p_0.  One wave64 per
 *   row, no atomics, no shared memory: R depends on the values of the row alone -- not on the row range, the grid or the decomposition --,
 *   so a host that adds the rows in global row order gets the same total from one block as from N.
 * Checks: grid set; 0 <= j0 <= j1 <= ny; 1 <= nq <= NSDG_SERIES_COUNT; known ids, none twice; a quantity whose source is NULL is refused by
 *   name; extent_conc finite; 0 <= row0 <= j0; q_stride >= j1 - row0: NSDG_ERR_ARG.  j0 == j1 does nothing.
 * nsdg_history_stat_name / _id ("mean" "ice_mean" "min" "max") and nsdg_history_series_name / _id ("area" "extent" "volume" "snow_volume"
 * "drift" "speed_max" "hice_max"): as nsdg_history_field_name / _id.  Host only. */
enum { NSDG_STAT_MEAN = 0, NSDG_STAT_ICE_MEAN, NSDG_STAT_MIN, NSDG_STAT_MAX, NSDG_STAT_COUNT };
enum {
    NSDG_SERIES_AREA = 0, NSDG_SERIES_EXTENT, NSDG_SERIES_VOLUME, NSDG_SERIES_SNOW_VOLUME, NSDG_SERIES_DRIFT, NSDG_SERIES_SPEED_MAX,
    NSDG_SERIES_HICE_MAX, NSDG_SERIES_COUNT
};
int nsdg_history_accumulate_stats(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nfields, const int32_t* fields, const int32_t* stats,
    const nsdg_history_sources* src, int32_t store, int32_t row0, int64_t plane_stride, double* acc, double* wacc);
int nsdg_history_row_totals(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t nq, const int32_t* quantities, const nsdg_history_sources* src,
    double extent_conc, int32_t row0, int64_t q_stride, double* out);
const char* nsdg_history_stat_name(int32_t stat);
int nsdg_history_stat_id(const char* name);
const char* nsdg_history_series_name(int32_t quantity);
int nsdg_history_series_id(const char* name);

/* ---- drifters: Lagrangian points advected by the ice velocity (csrc/drifters.hip) -----------------------------------
 * No counterpart in the reference snapshot.  The state of n drifters is ONE device array d[3][n] of doubles: plane 0 = x [m], plane 1 = y [m],
 * plane 2 = the status as a double.  x and y are GLOBAL domain coordinates: the domain is [0, Lx] x [0, Ly], Lx = nx hx, Ly = ny_global hy
 * (nsdg_block_set; a single domain: ny_global = ny).  Status: 0 active, 1 left the domain, 2 lost its ice, 3 on land.  A drifter whose
 * status is not 0 never moves again.
 *
 * nsdg_drifters_advance: ONE launch on the context's stream, one lane per drifter, no atomics, out of place.  u, v: the CG2 velocity of the
 * local array; A: the concentration, plane 0 (the cell mean) is read.  For every drifter (x, y, s) of d_in, in THIS order:
 *   1. element     ix = min(nx - 1, (int)floor(x / hx)),  iyg = min(ny_global - 1, (int)floor(y / hy))  -- IEEE divisions, never a reciprocal:
 *                  who owns a drifter must be the same decision on every rank; the local row is iy = iyg - row0.  (An index is also never
 *                  below 0: a coordinate below 0 or a NaN, which the hosts refuse, never becomes an address.)
 *   2. ownership   iy outside [j0, j1): the drifter is not this launch's -- all three planes of d_out get -inf.  Every case below writes all
 *                  three planes, so the elementwise maximum over the launches of a decomposition is the whole list.
 *   3. stopped     s != 0: (x, y, s) is copied through.
 *   4. status      the element is land in the context's mask (nsdg_land_mask_set), if one is set: (x, y, 3); else A[iy nx + ix] < min_conc:
 *                  (x, y, 2) -- a NaN concentration is not "<".
 *   5. velocity    (u1, v1) = V(x, y), the biquadratic CG2 velocity of element (ix, iy) from its 3 x 3 nodes (2 ix + c, 2 iy + r): with the local
 *                  coordinates xi = x / hx - ix - 1/2, eta = y / hy - iyg - 1/2 and the weights of the nodes at -1/2, 0, +1/2
 *                      L-(t) = 2 t^2 - t,   L0(t) = 1 - 4 t^2,   L+(t) = 2 t^2 + t,
 *                  V = sum over the rows r bottom to top of L_r(eta) (L-(xi) w_r0 + L0(xi) w_r1 + L+(xi) w_r2), a row west to east.
 *   6. predictor   xp = x + dt u1, yp = y + dt v1, xp clamped to [max(ix - 1, 0) hx, min(ix + 2, nx) hx] and yp to [max(iyg - 1, 0) hy,
 *                  min(iyg + 2, ny_global) hy]: the 3 x 3 elements around the drifter's own.  The clamp is stated in the drifter's own
 *                  element indices: it does not depend on the decomposition, and at any sane Courant number it is never active.
 *   7. velocity    the element of (xp, yp) by rule 1, its indices limited to [max(ix - 1, 0), min(ix + 1, nx - 1)] and [max(iyg - 1, 0),
 *                  min(iyg + 1, ny_global - 1)] (a predictor ON the upper limit of the clamp is on the closed edge of the last of those
 *                  elements, where the continuous velocity has the same value); (u2, v2) = V(xp, yp) there.
 *   8. Heun        xn = x + (0.5 dt) (u1 + u2), yn likewise.  !(0 <= xn <= Lx && 0 <= yn <= Ly) -- a NaN too --: (x, y, 1); else (xn, yn, 0).
 *   Every operation is one fp64 operation; the device may contract a product and a sum into an FMA.
 * Checks, as for the history calls: grid set (else NSDG_ERR_STATE); 0 <= j0 <= j1 <= ny; n >= 0 (n == 0 does nothing); dt and min_conc finite;
 *   non-null pointers; d_out != d_in; every row of [j0, j1) has its neighbour rows inside the local array or at the physical boundary --
 *   j0 >= 1 unless row0 + j0 == 0, j1 <= ny - 1 unless row0 + j1 == ny_global --, else NSDG_ERR_ARG with a message that names the missing ghost
 *   row.  The velocity must be valid on those rows (node rows 2 (j0 - 1) .. 2 (j1 + 1)).  The call belongs to no phase of the phase table. */
int nsdg_drifters_advance(nsdg_ctx* ctx, int32_t j0, int32_t j1, double dt, double min_conc, int64_t n, const double* u, const double* v,
    const double* A, const double* d_in, double* d_out);

/* ---- point samples: the model at drifter positions and at fixed stations (csrc/points.hip) ---------------------------
 * No counterpart in the reference snapshot.  What did the buoy see along its track, what passed over this mooring?  Everything a sample needs
 * is on the device at the end of every step and local to the point's own element.
 *
 * nsdg_points_sample: ONE launch on the context's stream, one lane per point, no atomics, no LDS.  x, y: device arrays of n GLOBAL coordinates
 * in metres (the domain of "drifters"; planes 0 and 1 of a drifter array d[3][n] can be passed as they are).  fields: nfields ids of
 * NSDG_HIST_* (the names of nsdg_history_field_name); src: the struct the history calls take, with H, A, D the DG fields of `order` p
 * (1 / 3 / 6 coefficient planes f[c N + e], N = nx ny of the local array) and every plane read.  The result is
 *     out[k * out_stride + p]   for field k and point p;  no other slot of out is written.
 * For every point (x, y), in THIS order:
 *   1. element     ix = min(nx - 1, (int)floor(x / hx)),  iyg = min(ny_global - 1, (int)floor(y / hy))  -- IEEE divisions, never a reciprocal:
 *                  who owns a point must be the same decision on every rank; the local row is iy = iyg - row0.  (An index is also never
 *                  below 0: a coordinate below 0 or a NaN, which the hosts refuse, never becomes an address.)
 *   2. ownership   iy outside [j0, j1): the point is not this launch's -- every one of its nfields slots gets -inf.  Every other case writes
 *                  all of them, so the elementwise maximum over the launches of a decomposition is the whole table, as for the drifters.
 *   3. local       xi = x / hx - ix - 1/2,  eta = y / hy - iyg - 1/2, the quotient rounded once and both subtractions exact.  A point on the
 *                  domain's upper edge has xi = +1/2 (eta = +1/2) in the last element.
 *   4. samples     taken AT THE POINT, not at the cell centre:
 *      hice, cice, damage   the DG field with the basis of DESIGN.md section 3,
 *                               c0 + c1 xi + c2 eta + c3 (xi^2 - 1/12) + c4 (eta^2 - 1/12) + c5 xi eta     (order 0: c0; order 1: the first three),
 *                           summed in this order, unclamped.
 *      hsnow, tice          the element's value of their one plane.
 *      u, v                 V(x, y) exactly as rule 5 of nsdg_drifters_advance states it: the weights L-, L0, L+ of the nodes at -1/2, 0, +1/2,
 *                           the rows bottom to top, a row west to east.  speed = sqrt(u u + v v).
 *      divergence, shear    from the derivatives of the same biquadratic at the point, with L-'(t) = 4 t - 1, L0'(t) = -8 t, L+'(t) = 4 t + 1:
 *                               e11 = (1/hx) sum_r L_r(eta) sum_c L_c'(xi) u_rc,     e22 = (1/hy) sum_r L_r'(eta) sum_c L_c(xi) v_rc,
 *                               g   = (1/hy) sum_r L_r'(eta) sum_c L_c(xi) u_rc  +  (1/hx) sum_r L_r(eta) sum_c L_c'(xi) v_rc
 *                           (the sums formed first, then ONE IEEE division by hx or hy each);
 *                               divergence = e11 + e22,   shear = sqrt((e11 - e22)^2 + g g)      [1/s].
 *                           At an element centre these are the samples of the history output.
 *      sigma_n, sigma_s     the three stress components evaluated at the point with all EIGHT basis functions -- the six above, then
 *                           eta (xi^2 - 1/12) and xi (eta^2 - 1/12) -- read from the tiled arrays, a[T + (c/2) 128 + 2 l + c%2] in "Data layout";
 *                           then (s11 + s22) / 2 and sqrt((s11 - s22)^2 / 4 + s12^2).  The unit is whatever the rheology stores, as for the history.
 *      Every operation is one fp64 operation (IEEE add, multiply, divide; the device's square root); the device may contract a product and
 *      a sum into an FMA.  A NaN source gives a NaN sample of the fields that read it, at the points of its element and nowhere else.
 *   5. Every source value is loaded at most once per point, whatever the list.
 * What is read: the point's own element only -- for the velocity the node rows 2 iy .. 2 iy + 2 of OWNED rows.  The top node row of the last
 *   owned row is the one ghost node row a single-iteration sub-cycle does receive, so no ghost row has to be valid and
 *   no exchange of complete node rows (nsdg_rb_bbm_desc.complete_nodes, the drifters' own) is needed for a sample.
 * Checks, as for the history calls: grid set (else NSDG_ERR_STATE); 0 <= j0 <= j1 <= ny; order in 0..2; n >= 0; 1 <= nfields <=
 *   NSDG_HISTORY_MAX_FIELDS; fields and src non-null; known ids, no id twice; a field whose source pointer is NULL is refused with a message
 *   that names the field and the source (sources no listed field reads may be NULL); whichever of s11, s12, s22 the list reads 16-byte
 *   aligned, as every tiled array ("Data layout": the coefficients are loaded in pairs; a component no listed field reads is not looked
 *   at); out_stride >= n; x, y, out non-null unless n == 0: NSDG_ERR_ARG.  n == 0 launches nothing (and x, y, out may then be NULL).  j0 == j1 is NOT nothing: an empty row range owns no point,
 *   so it writes -inf into all nfields slots of all n points.  The call belongs to no phase of the phase table: the hosts make it after
 *   their NSDG_PHASE_END mark or, for the drifters, where they advance them. */
int nsdg_points_sample(nsdg_ctx* ctx, int32_t j0, int32_t j1, int32_t order, int64_t n, const double* x, const double* y, int32_t nfields,
    const int32_t* fields, const nsdg_history_sources* src, int64_t out_stride, double* out);

/* ---- row-block decomposition: ghost-row exchange (SURVEY.md section 8(b) "nsdg_halo_exchange", 8(e)) ----------
 * The reference is a single-process, single-thread program; these entry points have no
 * counterpart in it.  They sit behind the same seam as everything else, the batched model step
 * IModelStep::iterate (core/src/include/IModelStep.hpp:16-34): a multi-rank step owns one context per GPU and
 * exchanges ghost rows with its <= 2 neighbours between kernel launches.  No collective is involved.
 *
 * Communicator: one per context.  nsdg_comm_init is the RCCL transport (one process per GPU; `id` is the
 * NSDG_COMM_ID_BYTES-byte ncclUniqueId obtained by rank 0 from nsdg_comm_unique_id and distributed by the caller --
 * torch.distributed in the Python driver, a TCP rendezvous in the C++ host); collective over the ranks.
 * librccl.so.1 is loaded on first use.  nsdg_comm_init_local is the in-process transport: the ranks of `group`
 * are contexts of ONE process driven by one host thread each (device-to-device copies, host hand-shake); used
 * by the one-GPU tests of the multi-rank driver and usable as a single-process multi-GPU mode. */
#define NSDG_COMM_ID_BYTES 128
int nsdg_comm_unique_id(void* id);
int nsdg_comm_init(nsdg_ctx* ctx, int32_t rank, int32_t world, const void* id);
int nsdg_comm_init_local(nsdg_ctx* ctx, int64_t group, int32_t rank, int32_t world);
int nsdg_comm_finalize(nsdg_ctx* ctx);
int nsdg_comm_rank(nsdg_ctx* ctx, int32_t* rank, int32_t* world);
/* Upper bound in seconds on any wait for a neighbour: the host-side hand-shake of the local transport and the drain in
 * nsdg_ctx_synchronize (RCCL: a dead peer never answers).  0 = wait for ever.  Default: the environment variable
 * NSDG_COMM_TIMEOUT_S, else 300.  May be called before or after nsdg_comm_init*. */
int nsdg_comm_deadline_set(nsdg_ctx* ctx, double seconds);
/* Replaces *value in place with its maximum over the ranks of the context's communicator (a NaN on any rank gives NaN); without a
 * communicator, or with a world of one, it is left as it is.  Collective: every rank calls it, in the same order relative to its other
 * collective calls.  RCCL: ncclAllReduce(ncclMax) on a device scalar on the communication stream, the wait bounded by the deadline; local
 * transport: on the host, under the same deadline.  NSDG_ERR_COMM when a rank does not arrive in time. */
int nsdg_comm_max_f64(nsdg_ctx* ctx, double* value);
/* The elementwise maximum, in place, of the DEVICE array dev[0 .. n) over the ranks of the context's communicator (the NaN rule of
 * nsdg_comm_max_f64); without a communicator, with a world of one or with n == 0 nothing happens.  Collective, every rank with the same n.
 * After nsdg_drifters_advance exactly one rank holds a finite triple per drifter and the others -inf: this merge gives every rank the whole
 * list.  RCCL: ncclAllReduce(ncclMax) in place on the communication stream, ordered behind the context's stream by an event, and the
 * context's stream waits for it; the host does not wait (a dead peer shows at the next bounded wait).  This path has never run: no machine
 * with two GPUs was at hand, as for every RCCL path of this library.  Local transport: staged on the host under the group's mutex, as
 * nsdg_comm_max_f64 with a vector in place of the scalar -- this transport SYNCHRONISES the context's streams (within the deadline) on
 * every rank; NSDG_ERR_COMM when a rank does not arrive in time or brings another n. */
int nsdg_comm_max_f64_array(nsdg_ctx* ctx, double* dev, int64_t n);

/* Rehearsal aid for a box with ONE GPU (tools/rank_share_timing.py, bench.py's loopback rehearsal): a loopback exchange
 * has no wire time, so a kernel that spins for delay_us + bytes of the larger direction / gbs (GB/s per direction) is put on
 * the communication stream between pack and transport of every exchange.  0, 0 = off (the default unless the environment
 * variables NSDG_HALO_DELAY_US / NSDG_HALO_SIM_GBS are set when the communicator is created: they are read once, there). */
int nsdg_comm_simulate_wire(nsdg_ctx* ctx, double delay_us, double gbs);

/* A plan fixes what ONE kind of exchange moves: for each of the four directions a list of contiguous blocks of
 * doubles in the caller's arrays (row blocks: ghost rows are contiguous in every layout of this ABI).  up_send
 * travels to rank_above and is received there as from_below, down_send travels to rank_below and arrives as
 * from_above; the packed sizes of matching directions must agree between neighbours.  rank_* = -1: physical
 * boundary, no traffic.  rank_below == rank_above == own rank: loopback (what goes up arrives from below), the
 * one-GPU rehearsal of an interior block.  Every rank of a communicator creates its plans in the same order. */
typedef struct nsdg_halo nsdg_halo;
typedef struct {
    double* ptr;
    int64_t count;
} nsdg_halo_seg;
int nsdg_halo_plan_create(nsdg_ctx* ctx, int32_t rank_below, int32_t rank_above, int32_t n_up, const nsdg_halo_seg* up_send,
    int32_t n_down, const nsdg_halo_seg* down_send, int32_t n_above, const nsdg_halo_seg* from_above, int32_t n_below,
    const nsdg_halo_seg* from_below, nsdg_halo** out);
int nsdg_halo_plan_destroy(nsdg_halo* plan);
/* packed doubles per direction (segments are padded to 16 bytes) */
int nsdg_halo_counts(const nsdg_halo* plan, int64_t* up, int64_t* down, int64_t* above, int64_t* below);

/* One exchange.  start: everything enqueued on the context's stream so far is visible to the exchange; the send
 * blocks are packed (one launch) and the transport is posted on the context's communication stream.  finish: the
 * received blocks are scattered into the ghost rows (one launch) and the context's stream waits for that.  Neither
 * call blocks the host (the local transport blocks until the neighbour thread has posted).  Kernels launched between
 * the two calls overlap with the exchange; they must not write the send blocks nor touch the receive blocks. */
int nsdg_halo_start(nsdg_ctx* ctx, nsdg_halo* plan);
int nsdg_halo_finish(nsdg_ctx* ctx, nsdg_halo* plan);

/* What the exchanges of a plan (or of all plans of a row-block driver) cost, measured with events on the communication
 * stream: `ms` is the time from "the data to send is ready" (the compute stream has reached nsdg_halo_start) to "the
 * ghost rows are written" (the unpack kernel has finished), summed over `exchanges` exchanges -- it contains the pack
 * and unpack kernels, the transfer and any wait for a neighbour that is late, and it overlaps with whatever the
 * compute stream does between start and finish.  `untimed` exchanges could not be timed (events recycled before they
 * completed).  The call waits for the last exchange of the plan(s) to finish; reset != 0 zeroes the counters. */
typedef struct {
    int64_t exchanges, untimed;
    double ms;
    int64_t bytes_sent, bytes_received; /* per exchange */
} nsdg_halo_stats;
int nsdg_halo_stats_get(nsdg_ctx* ctx, nsdg_halo* plan, nsdg_halo_stats* out, int32_t reset);

/* ---- row-block drivers: one call per model step for the sub-cycle and for the transport of a rank's block ------
 * The sequence of kernel passes and ghost exchanges that a multi-rank model step (IModelStep::iterate,
 * core/src/include/IModelStep.hpp:16-34) issues, built once from the block geometry and the device arrays:
 *   local array nx x ny (ghost rows included), owned element rows [j0, j1), nominal ghost depths
 *   (depth_below, depth_above) -- the same on every rank -- and the neighbour ranks (-1 = physical boundary; a
 *   rank keeps ghost rows only towards existing neighbours: j0 = depth_below or 0, j1 = ny - depth_above or ny).
 * Kernels with v = 4 / 3 / 2 sub-iterations per pass (nsdg_mevp_variant_set) are used when the depths are (v k, v k - 1)
 * -- k passes run between two exchanges, the ghost rows are advanced redundantly -- or when the block has no
 * neighbours; otherwise one sub-iteration per pass with (1, 1).  Both calls are asynchronous on the context's
 * stream.  Blocks with neighbours need a communicator (nsdg_comm_init*) before the plan is created. */
typedef struct nsdg_rb_mevp nsdg_rb_mevp;
typedef struct {
    int32_t nx, ny, j0, j1;
    int32_t depth_below, depth_above;
    int32_t rank_below, rank_above;
    int32_t nsub; /* sub-iterations per model step */
    int32_t overlap; /* launch the rows whose results travel first, post the exchange, then the interior */
    int32_t use_graph; /* replay the launches between two exchanges as one hipGraph */
    int32_t reserved;
    double *s11[2], *s12[2], *s22[2]; /* ping-pong: tiled stress */
    double *u[2], *v[2]; /* ping-pong: CG2 velocity */
    const double* packed; /* nsdg_mevp_prepare / nsdg_mevp_pack_nodal output of this step */
    const double* pg; /* nsdg_ice_strength output of this step */
} nsdg_rb_mevp_desc;
int nsdg_rb_mevp_create(nsdg_ctx* ctx, const nsdg_rb_mevp_desc* desc, nsdg_rb_mevp** out);
int nsdg_rb_mevp_destroy(nsdg_rb_mevp* plan);
/* sub-iterations per kernel pass and passes between two exchanges the plan settled on */
int nsdg_rb_mevp_info(const nsdg_rb_mevp* plan, int32_t* per_pass, int32_t* group_passes);
/* nsub sub-iterations; `parity` = which of the ping-pong buffers holds the current iterate (ghost rows valid),
 * *parity_out = which one holds the result (ghost rows refreshed) */
int nsdg_rb_mevp_run(nsdg_ctx* ctx, nsdg_rb_mevp* plan, int32_t parity, int32_t* parity_out);
/* exchange statistics summed over the plan's ghost exchanges (bytes: of its largest exchange) */
int nsdg_rb_mevp_stats(nsdg_ctx* ctx, nsdg_rb_mevp* plan, nsdg_halo_stats* out, int32_t reset);

/* The brittle sub-cycle of a row block ("brittle rheology" above; csrc/rowblock.hip): nsub sub-iterations of nsdg_bbm_iterate with the
 * exchanges of the single-sub-iteration branch of nsdg_rb_mevp_run -- unsplit: one launch from k0 = max(j0 - 1, 0), then one velocity
 * node row down and two up; with `overlap` and at least 4 owned rows: the top row, the bottom row, the exchange posted, the interior, the
 * exchange finished.  No multi-iteration passes and no hipGraph replay.  A block with neighbours must have the ghost depth (1, 1)
 * (NSDG_ERR_ARG otherwise) and a communicator (NSDG_ERR_STATE otherwise).
 * The damage.  The transport plan holds fixed buffers phi[k] / t1[k] of D and alternates between them by its own parity; the sub-cycle
 * ping-pongs D nsub times.  So the plan takes both transport buffers, D[0] = phi and D[1] = t1 of that field, and a work buffer of the
 * same size (the transport's t2 of D is free between two transport steps).  nsdg_rb_bbm_run's damage_parity says which of D[] is current
 * (the transport plan's parity): the sub-iterations alternate between D[damage_parity] and D_work, after an odd nsub nsdg_copy_f64 of all
 * local rows puts the result back, and one exchange of the 6 coefficient planes hands the transport its ghost rows: D ends in
 * D[damage_parity] for every nsub > 0.  nsub == 0 launches nothing, exchanges nothing and returns the parity it was given.
 * complete_nodes != 0: the call ends (nsub > 0) with one more exchange of the final velocity with 2 depth_above + 1 node rows downwards, so
 * that every ghost node row is current (the drifters' predictor may sit in the ghost row above).
 * Before the call: nsdg_bbm_prepare into hg, eg, pm and nsdg_mevp_prepare(dt / nsub, ..., u0 = v0 = zeros) into packed. */
typedef struct nsdg_rb_bbm nsdg_rb_bbm;
typedef struct {
    int32_t nx, ny, j0, j1;
    int32_t depth_below, depth_above;
    int32_t rank_below, rank_above;
    int32_t nsub; /* sub-iterations per call */
    int32_t overlap; /* launch the rows whose results travel first, post the exchange, then the interior */
    int32_t complete_nodes; /* end with an exchange of every ghost node row of the final velocity */
    int32_t reserved;
    double *s11[2], *s12[2], *s22[2]; /* ping-pong: tiled stress */
    double *u[2], *v[2]; /* ping-pong: CG2 velocity */
    const double* packed; /* nsdg_mevp_prepare output of this step (dt / nsub, u0 = v0 = 0) */
    const double *hg, *eg, *pm; /* nsdg_bbm_prepare output of this step */
    double* D[2]; /* the transport's two buffers of the damage: [6][ny][nx] each */
    double* D_work; /* same size: the partner of the current buffer inside the call */
} nsdg_rb_bbm_desc;
int nsdg_rb_bbm_create(nsdg_ctx* ctx, const nsdg_rb_bbm_desc* desc, nsdg_rb_bbm** out);
int nsdg_rb_bbm_destroy(nsdg_rb_bbm* plan);
/* `parity`: which ping-pong set of stress and velocity is current, *parity_out: which one holds the result; damage_parity: above */
int nsdg_rb_bbm_run(nsdg_ctx* ctx, nsdg_rb_bbm* plan, int32_t parity, int32_t damage_parity, int32_t* parity_out);
int nsdg_rb_bbm_stats(nsdg_ctx* ctx, nsdg_rb_bbm* plan, nsdg_halo_stats* out, int32_t reset);

#define NSDG_RB_MAX_FIELDS 4
typedef struct nsdg_rb_transport nsdg_rb_transport;
typedef struct {
    int32_t nx, ny, j0, j1;
    int32_t depth_below, depth_above;
    int32_t rank_below, rank_above;
    int32_t order; /* 2 */
    int32_t nfields;
    double* phi[NSDG_RB_MAX_FIELDS]; /* DG2 coefficient planes [6][ny][nx] of each advected field */
    double* t1[NSDG_RB_MAX_FIELDS]; /* same size: stage buffer; receives the new state */
    double* t2[NSDG_RB_MAX_FIELDS]; /* same size: stage buffer */
    const double *vx_dg, *vy_dg, *un_x, *un_y; /* nsdg_prepare_advection output of this step */
    /* closure of the step (nsdg_field_bounds below "INPUT DOMAIN AND CLOSURE").  own_bounds = 0: whatever nsdg_transport_bounds_set has
     * stated on the context when the plan RUNS (ABI 5); own_bounds != 0: the plan's own -- nbounds of them (0 = none, or nfields) --
     * whatever the context says: a context that also steps other fields (a snow layer, a damage field) does not leak its bounds into
     * this plan, nor this plan's into those calls. */
    int32_t own_bounds, nbounds;
    nsdg_field_bounds bounds[NSDG_RB_MAX_FIELDS];
} nsdg_rb_transport_desc;
int nsdg_rb_transport_create(nsdg_ctx* ctx, const nsdg_rb_transport_desc* desc, nsdg_rb_transport** out);
int nsdg_rb_transport_destroy(nsdg_rb_transport* plan);
/* one SSP-RK3 step.  parity 0: the state is in phi[], the new state (ghost rows refreshed) is written to t1[];
 * parity 1: the other way round; *parity_out = 1 - parity */
int nsdg_rb_transport_run(nsdg_ctx* ctx, nsdg_rb_transport* plan, double dt, int32_t parity, int32_t* parity_out);
int nsdg_rb_transport_stats(nsdg_ctx* ctx, nsdg_rb_transport* plan, nsdg_halo_stats* out, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* NSDG_H */

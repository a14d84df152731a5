"""ctypes binding of the C ABI in include/nsdg.h (libnsdg.so) for Python callers (tests, bench,
multi-rank driver).  PyTorch is used only as the owner of device memory and streams: every call
below passes raw device pointers through the extern "C" boundary.

There is deliberately NO fallback: if the HIP library is missing or fails to load, importing the
handle raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GIVEN_UP_UNSEEN = 0  # waits of the mEVP pipeline that gave up on contexts that were closed without anybody asking (Context.close)
LIB_PATH = os.environ.get("NSDG_LIB", os.path.join(HERE, "lib", "libnsdg.so"))  # NSDG_LIB: A/B builds of the same ABI

c_double_p = C.POINTER(C.c_double)
NDIAG = 15
DIAG = ["rho", "qa", "qw", "qi", "cspec", "tau", "hi", "hs", "cnew", "qia", "qio", "subl", "dqdt", "hifroms", "qow"]
STATE = ["hice", "cice", "hsnow", "tice0"]
FORCING = ["sst", "sss", "tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall", "wind"]
ALBEDO = {"smu": 0, "smu2": 1, "ccsm": 2}
FREEZING = {"linear": 0, "unesco": 1}


class ColumnParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "drag_ocean_q", "drag_ocean_t", "drag_ice_t", "ocean_albedo", "i0", "min_conc", "min_thick",
        "ks", "h0", "phi_m", "ccsm_ice_albedo", "ccsm_snow_albedo")] + [
        ("flooding", C.c_int32), ("albedo_kind", C.c_int32), ("freezing_kind", C.c_int32), ("reserved", C.c_int32)]


class MevpParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "rho_ice", "rho_atm", "rho_ocean", "c_atm", "c_ocean", "pstar", "compaction", "delta_min", "fc",
        "alpha", "beta", "h_min", "min_conc", "min_thick", "aevp_c", "aevp_alpha_min")]


class BbmParams(C.Structure):
    """nsdg_bbm_params: the brittle rheology (include/nsdg.h "brittle rheology")"""
    _fields_ = [(n, C.c_double) for n in (
        "young", "nu", "p0", "lambda0", "tan_phi", "cohesion_lab", "compr_strength", "t_heal", "d_max")] + [
        ("relax_exponent", C.c_int32), ("reserved", C.c_int32)]


class BasalParams(C.Structure):
    """nsdg_basal_params: the grounding scheme of landfast ice (include/nsdg_basal.h)"""
    _fields_ = [(n, C.c_double) for n in ("k1", "k2", "alpha_b", "u0")]


class SlabParams(C.Structure):
    """nsdg_slab_params: the slab ocean of nsdg_column_step_ocean (include/nsdg_ocean.h)"""
    _fields_ = [(n, C.c_double) for n in ("relax_t", "relax_s", "ice_salinity")] + [("reserved", C.c_int32 * 2)]


SUBCYCLE_ADAPTIVE, SUBCYCLE_KEEP_ALPHA, SUBCYCLE_KEEP_DELTA_MIN, SUBCYCLE_ADAPTIVE_CONVERGED = 0, 1, 2, 3  # modes of nsdg_mevp_stable_params


class FieldBounds(C.Structure):
    """nsdg_field_bounds: closure of a transport step for one advected field"""
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("cap_mean", C.c_int32), ("reserved", C.c_int32)]


# the closure of the dynamics' two advected fields (include/nsdg.h "INPUT DOMAIN AND CLOSURE"): mean thickness H >= 0; concentration
# 0 <= A <= 1 with the cell mean capped at 1 (ridging: further convergence raises the true thickness H / A)
H_A_BOUNDS = ((0.0, float("inf"), False), (0.0, 1.0, True))


class HaloSeg(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("count", C.c_int64)]


class HaloStats(C.Structure):
    _fields_ = [("exchanges", C.c_int64), ("untimed", C.c_int64), ("ms", C.c_double), ("bytes_sent", C.c_int64), ("bytes_received", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# NSDG_PHASE_*: the phase ids both hosts share (include/nsdg.h "per-phase device timing"), in id order
PHASES = ("forcing", "column", "prepare", "sub-cycle", "transport", "reduction")
PHASE_MAX, PHASE_END, PHASE_RING = 16, -1, 256


class PhaseTable(C.Structure):
    """nsdg_phase_table"""
    _fields_ = [("ms", C.c_double * PHASE_MAX), ("count", C.c_int64 * PHASE_MAX), ("total_ms", C.c_double), ("spans", C.c_int64)]


# NSDG_HIST_*: the history fields in id order (include/nsdg.h "history output"); the library answers the same names (nsdg_history_field_name)
HISTORY_FIELDS = ("hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s", "hsnow", "tice", "damage")
HISTORY_SOURCES = ("H", "A", "u", "v", "s11", "s12", "s22", "hsnow", "tice", "D")
# NSDG_STAT_* and NSDG_SERIES_*, in id order; SERIES_SOURCES: what a quantity of nsdg_history_row_totals reads
HISTORY_STATS = ("mean", "ice_mean", "min", "max")
SERIES_QUANTITIES = ("area", "extent", "volume", "snow_volume", "drift", "speed_max", "hice_max")
SERIES_SOURCES = {"area": ("A",), "extent": ("A",), "volume": ("H",), "snow_volume": ("hsnow",), "drift": ("A", "u", "v"),
                  "speed_max": ("u", "v"), "hice_max": ("H",)}


class HistorySources(C.Structure):
    """nsdg_history_sources: the device arrays a sample is taken from (a field no listed field reads may stay NULL)"""
    _fields_ = [(n, C.c_void_p) for n in HISTORY_SOURCES]


# drifters (include/nsdg.h "drifters"): the status values of plane 2, and the lanes per workgroup of the launch (csrc/drifters.hip)
DRIFTER_ACTIVE, DRIFTER_LEFT, DRIFTER_NO_ICE, DRIFTER_LAND = 0, 1, 2, 3
DRIFTERS_BLOCK = 256
# point samples (include/nsdg.h "point samples"): the lanes per workgroup of the launch (csrc/points.hip), and what a field reads
POINTS_BLOCK = 256
POINTS_SOURCES = {"hice": ("H",), "cice": ("A",), "u": ("u",), "v": ("v",), "speed": ("u", "v"), "divergence": ("u", "v"), "shear": ("u", "v"),
                  "sigma_n": ("s11", "s22"), "sigma_s": ("s11", "s12", "s22"), "hsnow": ("hsnow",), "tice": ("tice",), "damage": ("D",)}

COMM_ID_BYTES = 128
RB_MAX_FIELDS = 4
TRACERS_MAX = 4  # NSDG_TRACERS_MAX (include/nsdg.h "ice tracers")
TRACER_PASSIVE, TRACER_AGE = 0, 1  # NSDG_TRACER_*


class RbMevpDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nx", "ny", "j0", "j1", "depth_below", "depth_above", "rank_below", "rank_above", "nsub",
                                          "overlap", "use_graph", "reserved")] + [
        (n, C.c_void_p * 2) for n in ("s11", "s12", "s22", "u", "v")] + [("packed", C.c_void_p), ("pg", C.c_void_p)]


class RbBbmDesc(C.Structure):
    """nsdg_rb_bbm_desc"""
    _fields_ = [(n, C.c_int32) for n in ("nx", "ny", "j0", "j1", "depth_below", "depth_above", "rank_below", "rank_above", "nsub",
                                          "overlap", "complete_nodes", "reserved")] + [
        (n, C.c_void_p * 2) for n in ("s11", "s12", "s22", "u", "v")] + [(n, C.c_void_p) for n in ("packed", "hg", "eg", "pm")] + [
        ("D", C.c_void_p * 2), ("D_work", C.c_void_p)]


class RbTransportDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nx", "ny", "j0", "j1", "depth_below", "depth_above", "rank_below", "rank_above", "order",
                                          "nfields")] + [
        (n, C.c_void_p * RB_MAX_FIELDS) for n in ("phi", "t1", "t2")] + [(n, C.c_void_p) for n in ("vx_dg", "vy_dg", "un_x", "un_y")] + [
        ("own_bounds", C.c_int32), ("nbounds", C.c_int32), ("bounds", FieldBounds * RB_MAX_FIELDS)]


class NsdgError(RuntimeError):
    pass


# name -> (restype, argtypes); kept in one table so tests can check every declared symbol exists
VP = C.c_void_p
I32, I64, D = C.c_int32, C.c_int64, C.c_double
DEFAULT_TRANSPORT_VARIANT = 2  # nsdg_ctx_create's default transport stage kernel (csrc/nsdg_ctx.hip)
DEFAULT_MEVP_VARIANT = 4  # nsdg_ctx_create's default (NSDG_MEVP_DEFAULT_VARIANT): four sub-iterations per kernel pass (csrc/mevp_fused4.hip)

SYMBOLS = {
    "nsdg_abi_version": (C.c_int, []),
    "nsdg_last_error": (C.c_char_p, []),
    "nsdg_ctx_create": (C.c_int, [C.c_int, VP, C.POINTER(VP)]),
    "nsdg_ctx_destroy": (C.c_int, [VP]),
    "nsdg_ctx_synchronize": (C.c_int, [VP]),
    "nsdg_copy_f64": (C.c_int, [VP, VP, VP, I64]),
    "nsdg_phase_timing_set": (C.c_int, [VP, I32]),
    "nsdg_phase_mark": (C.c_int, [VP, I32]),
    "nsdg_phase_times": (C.c_int, [VP, C.POINTER(PhaseTable), I32]),
    "nsdg_column_default_params": (None, [C.POINTER(ColumnParams)]),
    "nsdg_column_params_set": (C.c_int, [VP, C.POINTER(ColumnParams)]),
    "nsdg_column_step": (C.c_int, [VP, I64, D] + [VP] * 16),
    "nsdg_mevp_default_params": (None, [C.POINTER(MevpParams)]),
    "nsdg_mevp_params_set": (C.c_int, [VP, C.POINTER(MevpParams)]),
    "nsdg_mevp_stable_params": (C.c_int, [C.POINTER(MevpParams), I32, D, D]),
    "nsdg_mevp_creep_percent_per_day": (C.c_double, [C.POINTER(MevpParams)]),
    "nsdg_concentration_max": (C.c_int, [VP, I32, I32, VP, VP, C.POINTER(D)]),
    "nsdg_substep_count": (C.c_int, [C.POINTER(MevpParams), D, D, D, D, I32, C.POINTER(I32), C.POINTER(D)]),
    "nsdg_tiled_len": (C.c_int64, [I32, I32, I32]),
    "nsdg_grid_set": (C.c_int, [VP, I32, I32, D, D]),
    "nsdg_land_mask_set": (C.c_int, [VP, VP]),
    "nsdg_land_clear": (C.c_int, [VP, I32, I32, I32, VP]),
    "nsdg_land_clear_nodes": (C.c_int, [VP, VP, VP]),
    "nsdg_bbm_default_params": (None, [C.POINTER(BbmParams)]),
    "nsdg_bbm_params_set": (C.c_int, [VP, C.POINTER(BbmParams)]),
    "nsdg_bbm_params_check": (C.c_int, [C.POINTER(BbmParams)]),
    "nsdg_bbm_prepare": (C.c_int, [VP, I32, I32] + [VP] * 5),
    "nsdg_bbm_iterate": (C.c_int, [VP, I32, I32, I32] + [VP] * 16),
    "nsdg_bbm_substep_count": (C.c_int, [C.POINTER(BbmParams), D, D, D, D, I32, C.POINTER(I32)]),
    "nsdg_mevp_variant_set": (C.c_int, [VP, I32]),
    "nsdg_prepare_advection": (C.c_int, [VP, I32] + [VP] * 6),
    "nsdg_transport_variant_set": (C.c_int, [VP, I32, I32]),
    "nsdg_transport_stage": (C.c_int, [VP, I32, I32, I32, D, D, D, I32, C.POINTER(VP), C.POINTER(VP), C.POINTER(VP)] + [VP] * 4),
    "nsdg_transport_step": (C.c_int, [VP, I32, D, I32, C.POINTER(VP)] + [VP] * 5),
    "nsdg_transport_step_oop": (C.c_int, [VP, I32, D, I32, C.POINTER(VP), C.POINTER(VP)] + [VP] * 4),
    "nsdg_transport_step_oop_rows": (C.c_int, [VP, I32, I32, I32, D, I32, C.POINTER(VP), C.POINTER(VP)] + [VP] * 4),
    "nsdg_transport_bounds_set": (C.c_int, [VP, I32, C.POINTER(FieldBounds)]),
    "nsdg_transport_limit": (C.c_int, [VP, I32, I32, I32, I32, C.POINTER(VP)]),
    "nsdg_dg_to_cg": (C.c_int, [VP, I32, VP, VP]),
    "nsdg_ice_strength": (C.c_int, [VP, I32, I32, VP, VP, VP]),
    "nsdg_tracer_weight": (C.c_int, [VP, I32, I32, I32, VP, VP, VP]),
    "nsdg_tracer_recover": (C.c_int, [VP, I32, I32, I32, VP, VP, VP, D, D, VP]),
    "nsdg_history_accumulate": (C.c_int, [VP, I32, I32, I32, C.POINTER(I32), C.POINTER(HistorySources), I32, I32, I64, VP]),
    "nsdg_history_field_name": (C.c_char_p, [I32]),
    "nsdg_history_field_id": (C.c_int, [C.c_char_p]),
    "nsdg_history_accumulate_stats": (C.c_int, [VP, I32, I32, I32, C.POINTER(I32), C.POINTER(I32), C.POINTER(HistorySources), I32, I32, I64, VP, VP]),
    "nsdg_history_row_totals": (C.c_int, [VP, I32, I32, I32, C.POINTER(I32), C.POINTER(HistorySources), D, I32, I64, VP]),
    "nsdg_history_stat_name": (C.c_char_p, [I32]),
    "nsdg_history_stat_id": (C.c_int, [C.c_char_p]),
    "nsdg_history_series_name": (C.c_char_p, [I32]),
    "nsdg_history_series_id": (C.c_int, [C.c_char_p]),
    "nsdg_drifters_advance": (C.c_int, [VP, I32, I32, D, D, I64] + [VP] * 5),
    "nsdg_points_sample": (C.c_int, [VP, I32, I32, I32, I64, VP, VP, I32, C.POINTER(I32), C.POINTER(HistorySources), I64, VP]),
    "nsdg_boxtest_forcing": (C.c_int, [VP, D, D, VP, VP, VP, VP]),
    "nsdg_block_set": (C.c_int, [VP, I32, I32]),
    "nsdg_column_forcing": (C.c_int, [VP, I32, D] + [VP] * 7),
    "nsdg_column_wind": (C.c_int, [VP, VP, VP, VP]),
    "nsdg_forcing_sample": (C.c_int, [VP, I32, I32, I32, I32, C.POINTER(VP), C.POINTER(VP), D, C.POINTER(VP)]),
    "nsdg_wind_stress": (C.c_int, [VP, I64, VP, VP, VP, VP]),
    "nsdg_mevp_stress": (C.c_int, [VP, I32, I32] + [VP] * 6),
    "nsdg_mevp_pack_nodal": (C.c_int, [VP, D] + [VP] * 9),
    "nsdg_mevp_prepare": (C.c_int, [VP, D] + [VP] * 9),
    "nsdg_mevp_velocity": (C.c_int, [VP, I32, I32] + [VP] * 8),
    "nsdg_mevp_iterate": (C.c_int, [VP, I32, I32, I32] + [VP] * 12),
    "nsdg_mevp_iterate2": (C.c_int, [VP, I32, I32] + [VP] * 12),
    "nsdg_mevp_iterate3": (C.c_int, [VP, I32, I32] + [VP] * 12),
    "nsdg_mevp_iterate3_pair": (C.c_int, [VP, I32, I32, I32, I32] + [VP] * 12),
    "nsdg_mevp_iterate4": (C.c_int, [VP, I32, I32] + [VP] * 12),
    "nsdg_mevp_iterate4_pair": (C.c_int, [VP, I32, I32, I32, I32] + [VP] * 12),
    "nsdg_mevp_pipeline_health": (C.c_int, [VP, C.POINTER(C.c_uint32)]),
    "nsdg_mevp_strip_rows_set": (C.c_int, [VP, I32]),
    "nsdg_mevp_occupancy_set": (C.c_int, [VP, I32]),
    "nsdg_mevp_subcycle": (C.c_int, [VP, D, I32] + [VP] * 15),
    "nsdg_comm_unique_id": (C.c_int, [VP]),
    "nsdg_comm_init": (C.c_int, [VP, I32, I32, VP]),
    "nsdg_comm_init_local": (C.c_int, [VP, I64, I32, I32]),
    "nsdg_comm_finalize": (C.c_int, [VP]),
    "nsdg_comm_rank": (C.c_int, [VP, C.POINTER(I32), C.POINTER(I32)]),
    "nsdg_comm_deadline_set": (C.c_int, [VP, D]),
    "nsdg_comm_max_f64": (C.c_int, [VP, C.POINTER(D)]),
    "nsdg_comm_max_f64_array": (C.c_int, [VP, VP, I64]),
    "nsdg_comm_simulate_wire": (C.c_int, [VP, D, D]),
    "nsdg_halo_plan_create": (C.c_int, [VP, I32, I32, I32, C.POINTER(HaloSeg), I32, C.POINTER(HaloSeg), I32, C.POINTER(HaloSeg), I32,
                                        C.POINTER(HaloSeg), C.POINTER(VP)]),
    "nsdg_halo_plan_destroy": (C.c_int, [VP]),
    "nsdg_halo_counts": (C.c_int, [VP] + [C.POINTER(I64)] * 4),
    "nsdg_halo_start": (C.c_int, [VP, VP]),
    "nsdg_halo_finish": (C.c_int, [VP, VP]),
    "nsdg_halo_stats_get": (C.c_int, [VP, VP, C.POINTER(HaloStats), I32]),
    "nsdg_rb_mevp_create": (C.c_int, [VP, C.POINTER(RbMevpDesc), C.POINTER(VP)]),
    "nsdg_rb_mevp_destroy": (C.c_int, [VP]),
    "nsdg_rb_mevp_info": (C.c_int, [VP, C.POINTER(I32), C.POINTER(I32)]),
    "nsdg_rb_mevp_run": (C.c_int, [VP, VP, I32, C.POINTER(I32)]),
    "nsdg_rb_mevp_stats": (C.c_int, [VP, VP, C.POINTER(HaloStats), I32]),
    "nsdg_rb_bbm_create": (C.c_int, [VP, C.POINTER(RbBbmDesc), C.POINTER(VP)]),
    "nsdg_rb_bbm_destroy": (C.c_int, [VP]),
    "nsdg_rb_bbm_run": (C.c_int, [VP, VP, I32, I32, C.POINTER(I32)]),
    "nsdg_rb_bbm_stats": (C.c_int, [VP, VP, C.POINTER(HaloStats), I32]),
    "nsdg_rb_transport_create": (C.c_int, [VP, C.POINTER(RbTransportDesc), C.POINTER(VP)]),
    "nsdg_rb_transport_destroy": (C.c_int, [VP]),
    "nsdg_rb_transport_run": (C.c_int, [VP, VP, D, I32, C.POINTER(I32)]),
    "nsdg_rb_transport_stats": (C.c_int, [VP, VP, C.POINTER(HaloStats), I32]),
}

# the functions of include/nsdg_tracers.h (the "ice tracers" section, a header of its own that nsdg.h includes), bound like SYMBOLS
TRACER_SYMBOLS = {
    "nsdg_tracers_weight": (C.c_int, [VP, I32, I32, I32, VP, I32, C.POINTER(VP), C.POINTER(VP)]),
    "nsdg_tracers_recover": (C.c_int, [VP, I32, I32, I32, VP, VP, I32, C.POINTER(VP), C.POINTER(I32), D, D, D, C.POINTER(VP)]),
    "nsdg_tracers_dilute": (C.c_int, [VP, I32, I32, VP, VP, I32, C.POINTER(VP)]),
}

# the functions of include/nsdg_basal.h (the "landfast ice" section, a header of its own that nsdg.h includes), bound like SYMBOLS
BASAL_SYMBOLS = {
    "nsdg_basal_default_params": (None, [C.POINTER(BasalParams)]),
    "nsdg_basal_params_set": (C.c_int, [VP, C.POINTER(BasalParams)]),
    "nsdg_basal_depth_set": (C.c_int, [VP, VP]),
    "nsdg_basal_critical": (C.c_int, [VP, VP, VP, VP]),
}

# the functions of include/nsdg_ocean.h (the "slab ocean" section, a header of its own that nsdg.h includes), bound like SYMBOLS
OCEAN_SYMBOLS = {
    "nsdg_slab_default_params": (None, [C.POINTER(SlabParams)]),
    "nsdg_slab_params_set": (C.c_int, [VP, C.POINTER(SlabParams)]),
    "nsdg_column_step_ocean": (C.c_int, [VP, I64, D] + [VP] * 18),
}

# the functions of include/nsdg_snow.h (the "snow load" section, a header of its own that nsdg.h includes), bound like SYMBOLS
SNOW_SYMBOLS = {
    "nsdg_snow_load_set": (C.c_int, [VP, VP, I32, C.c_double]),
    "nsdg_snow_load_nodal": (C.c_int, [VP, VP, VP, VP]),
}
SNOW_DENSITY = 330.0  # NSDG_SNOW_DENSITY: the column step's rho_s

# the functions of include/nsdg_tilt.h (the "sea-surface tilt" section, a header of its own that nsdg.h includes), bound like SYMBOLS
TILT_SYMBOLS = {
    "nsdg_tilt_set": (C.c_int, [VP, VP, C.c_double]),
    "nsdg_tilt_nodal": (C.c_int, [VP, VP, VP]),
    "nsdg_boxtest_ssh": (C.c_int, [VP, C.c_double, C.c_double, C.c_double, VP]),
}
GRAVITY = 9.81  # NSDG_GRAVITY


class BudgetOut(C.Structure):
    """nsdg_budget_out: the sixteen nodal planes (NULL: not stored) and the row totals of nsdg_momentum_budget (include/nsdg_budget.h)"""
    _fields_ = [(t + "_" + c, C.c_void_p) for t in ("wind", "water", "coriolis", "tilt", "internal", "basal", "inertia", "residual") for c in "xy"] + [
        ("power", C.c_void_p), ("power_stride", C.c_int64), ("row0", C.c_int32)]


# the functions of include/nsdg_budget.h (the "momentum budget" section, a header of its own that nsdg.h includes), bound like SYMBOLS
BUDGET_SYMBOLS = {
    "nsdg_momentum_budget": (C.c_int, [VP, I32, I32] + [VP] * 10 + [C.POINTER(BudgetOut)]),
    "nsdg_budget_term_id": (C.c_int, [C.c_char_p]),
}
BUDGET_TERMS = ("wind", "water", "coriolis", "tilt", "internal", "basal", "inertia", "residual")  # in id order: nsdg_budget_term_id
BUDGET_KE, BUDGET_QUANTITIES = 8, 9  # NSDG_BUDGET_KE, NSDG_BUDGET_QUANTITIES

_lib = None


def load_library(path=LIB_PATH):
    """dlopen libnsdg.so and declare every entry point of include/nsdg.h.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    # Device pointers and streams come from PyTorch, so the kernels must be launched through the
    # SAME HIP runtime instance torch uses: import torch first so that its libamdhip64 is the one
    # already mapped when libnsdg.so's dependency on that soname is resolved.
    import torch  # noqa: F401

    if not os.path.exists(path):
        raise NsdgError("HIP library %s is missing: build it with `python -m nextsimdg_amd.build` "
                        "(there is no CPU fallback)" % path)
    lib = C.CDLL(path)
    for name, (res, args) in list(SYMBOLS.items()) + list(TRACER_SYMBOLS.items()) + list(BASAL_SYMBOLS.items()) + list(OCEAN_SYMBOLS.items()) + list(SNOW_SYMBOLS.items()) + list(TILT_SYMBOLS.items()) + list(BUDGET_SYMBOLS.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


TILE = 64


def stable_mevp_params(p, mode, h, dt):
    """nsdg_mevp_stable_params: the sub-cycle's stability rule (one copy, in the library) applied to the MevpParams `p` in place for cells
    of size h and a model time step dt; mode = SUBCYCLE_ADAPTIVE / SUBCYCLE_ADAPTIVE_CONVERGED / SUBCYCLE_KEEP_ALPHA / SUBCYCLE_KEEP_DELTA_MIN"""
    rc = load_library().nsdg_mevp_stable_params(C.byref(p), int(mode), float(h), float(dt))
    if rc != 0:
        raise NsdgError("nsdg error %d: %s" % (rc, load_library().nsdg_last_error().decode()))
    return p


AT_NODES, AT_ELEMENTS = 0, 1  # NSDG_AT_NODES / NSDG_AT_ELEMENTS: the targets of nsdg_forcing_sample
FORCING_MAX_FIELDS = 8  # NSDG_FORCING_MAX_FIELDS

SUBSTEP_COURANT = 1.5  # NSDG_SUBSTEP_COURANT: the default of the sub-stepping rule (include/nsdg.h "sub-stepping")


def substep_count(p, amax, h, dt, courant=SUBSTEP_COURANT, max_substeps=16):
    """nsdg_substep_count: (n, c) -- the number of sub-steps of dt that keeps the strength wave of a state with largest concentration amax
    within `courant` cells of size h per sub-step, and that wave speed c [m/s]; NsdgError (with the needed n) if n > max_substeps"""
    lib = load_library()
    n, c = I32(0), D(0.0)
    rc = lib.nsdg_substep_count(C.byref(p), float(amax), float(h), float(dt), float(courant), int(max_substeps), C.byref(n), C.byref(c))
    if rc != 0:
        raise NsdgError("nsdg error %d: %s" % (rc, lib.nsdg_last_error().decode()))
    return int(n.value), float(c.value)


BBM_COURANT = 0.25  # NSDG_BBM_COURANT: the default of the elastic-wave rule (include/nsdg.h "brittle rheology"; profiles/r09_bbm.md)


def bbm_default_params(**kw):
    """nsdg_bbm_default_params with members replaced by keyword (host only)"""
    p = BbmParams()
    load_library().nsdg_bbm_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise NsdgError("unknown BBM parameter " + k)
        setattr(p, k, v)
    return p


def basal_default_params(**kw):
    """nsdg_basal_default_params with members replaced by keyword (host only)"""
    p = BasalParams()
    load_library().nsdg_basal_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise NsdgError("unknown basal parameter " + k)
        setattr(p, k, v)
    return p


def slab_default_params(**kw):
    """nsdg_slab_default_params with members replaced by keyword (host only)"""
    p = SlabParams()
    load_library().nsdg_slab_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "reserved" or not hasattr(p, k):
            raise NsdgError("unknown slab-ocean parameter " + k)
        setattr(p, k, v)
    return p


def bbm_substep_count(p, rho_ice, h, dt, courant=BBM_COURANT, max_nsub=100000):
    """nsdg_bbm_substep_count: the number of sub-iterations of a model step dt that keeps the elastic wave of the undamaged ice within
    `courant` cells of size h per sub-iteration; NsdgError (with the needed number) if it exceeds max_nsub"""
    lib = load_library()
    n = I32(0)
    rc = lib.nsdg_bbm_substep_count(C.byref(p), float(rho_ice), float(h), float(dt), float(courant), int(max_nsub), C.byref(n))
    if rc != 0:
        raise NsdgError("nsdg error %d: %s" % (rc, lib.nsdg_last_error().decode()))
    return int(n.value)


def creep_percent_per_day(p):
    """strain rate below which the ice creeps instead of staying rigid (= delta_min), in percent per day"""
    return float(load_library().nsdg_mevp_creep_percent_per_day(C.byref(p)))


def tile(a):
    """[nc, ny, nx] coefficient planes -> the tiled layout of include/nsdg.h (stress coefficients and Gauss-point
    ice strength), returned as [ny, ceil(nx/64), nc*64]: per tile of 64 elements the coefficients in pairs
    interleaved by element, (c/2)*128 + 2*l + c%2, an odd last coefficient at (nc/2)*128 + l; padding elements
    are zero"""
    import torch

    nc, ny, nx = a.shape
    ntx = (nx + TILE - 1) // TILE
    b = torch.nn.functional.pad(a, (0, ntx * TILE - nx)).reshape(nc, ny, ntx, TILE)
    npair = nc // 2
    parts = [b[:2 * npair].reshape(npair, 2, ny, ntx, TILE).permute(2, 3, 0, 4, 1).reshape(ny, ntx, npair * 2 * TILE)]
    if nc % 2:
        parts.append(b[nc - 1].reshape(ny, ntx, TILE))
    return torch.cat(parts, dim=2).contiguous()


def untile(t, nx):
    """inverse of tile(): [ny, ntx, nc*64] -> [nc, ny, nx]"""
    import torch

    ny, ntx, w = t.shape
    nc = w // TILE
    npair = nc // 2
    pairs = t[:, :, :npair * 2 * TILE].reshape(ny, ntx, npair, TILE, 2).permute(2, 4, 0, 1, 3).reshape(2 * npair, ny, ntx * TILE)
    planes = [pairs]
    if nc % 2:
        planes.append(t[:, :, npair * 2 * TILE:].reshape(1, ny, ntx * TILE))
    return torch.cat(planes, dim=0)[:, :, :nx].contiguous()


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def _check_f64(*tensors):
    import torch

    for t in tensors:
        if t is None:
            continue
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
            raise NsdgError("expected contiguous float64 CUDA tensors")


def _ptr_array(tensors):
    arr = (VP * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


class HaloPlanHandle:
    """an nsdg_halo plan; start() / finish() are pre-bound zero-argument calls"""

    def __init__(self, ctx, below, above, up_send, down_send, from_above, from_below):
        def pieces(v):  # a row block of a [nc, ny, nx] array is one contiguous block per coefficient plane
            return [v] if v.is_contiguous() else [p for sub in v.unbind(0) for p in pieces(sub)]

        lists = tuple([p for v in views for p in pieces(v)] for views in (up_send, down_send, from_above, from_below))
        for views in lists:
            _check_f64(*views)
        self.keep = [list(v) for v in lists]  # the tensors must outlive the plan
        arrs = []
        for views in lists:
            a = (HaloSeg * max(len(views), 1))()
            for i, v in enumerate(views):
                a[i].ptr, a[i].count = v.data_ptr(), v.numel()
            arrs.append(a)
        h = VP()
        nb = lambda r: -1 if r is None else int(r)
        ctx._call(ctx.lib.nsdg_halo_plan_create(ctx.h, nb(below), nb(above), len(lists[0]), arrs[0], len(lists[1]), arrs[1],
                                                len(lists[2]), arrs[2], len(lists[3]), arrs[3], C.byref(h)))
        self.ctx, self.h = ctx, h
        lib, ch = ctx.lib, ctx.h

        def start():
            rc = lib.nsdg_halo_start(ch, h)
            if rc != 0:
                ctx._call(rc)

        def finish():
            rc = lib.nsdg_halo_finish(ch, h)
            if rc != 0:
                ctx._call(rc)

        self.start, self.finish = start, finish

    def stats(self, reset=False):
        """what the exchanges of this plan cost so far (nsdg_halo_stats_get)"""
        st = HaloStats()
        self.ctx._call(self.ctx.lib.nsdg_halo_stats_get(self.ctx.h, self.h, C.byref(st), int(reset)))
        return st.as_dict()

    def counts(self):
        c = [I64() for _ in range(4)]
        self.ctx._call(self.ctx.lib.nsdg_halo_counts(self.h, *[C.byref(x) for x in c]))
        return tuple(x.value for x in c)

    def close(self):
        if self.h:
            self.ctx.lib.nsdg_halo_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.ctx.h:  # plans die with their context's communicator otherwise
                self.close()
        except Exception:
            pass


class Context:
    """One nsdg_ctx bound to a torch device and (by default) torch's current stream on it, so that
    torch.cuda.Event timing and torch.distributed collectives order correctly with the kernels."""

    def __init__(self, device=None, stream=None):
        import torch

        self.lib = load_library()
        if not torch.cuda.is_available():
            raise NsdgError("no HIP device visible: the nextsimdg_amd kernels need a GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream() if stream is None else stream
        h = VP()
        self._call(self.lib.nsdg_ctx_create(self.device.index or 0, VP(self.stream.cuda_stream), C.byref(h)))
        self.h = h
        self.nx = self.ny = 0
        self.mevp_variant = DEFAULT_MEVP_VARIANT  # the library default (four sub-iterations per pass)
        self.land_mask = None  # the tensor behind nsdg_land_mask_set (set_land_mask keeps it alive)
        self.basal_depth = None  # the tensor behind nsdg_basal_depth_set (set_basal_depth keeps it alive)
        self.snow_load = None  # the tensor behind nsdg_snow_load_set (set_snow_load keeps it alive)
        self.ssh = None  # the tensor behind nsdg_tilt_set (set_tilt keeps it alive)

    def _call(self, rc):
        if rc != 0:
            raise NsdgError("nsdg error %d: %s" % (rc, self.lib.nsdg_last_error().decode()))

    def close(self):
        """destroys the context; a wait of the mEVP pipeline that gave up on it and was never taken (pipeline_waits_given_up) is
        added to the process-wide tally abi.GIVEN_UP_UNSEEN first: a session that ignored wrong results can still be told"""
        global GIVEN_UP_UNSEEN
        if getattr(self, "h", None):
            try:
                GIVEN_UP_UNSEEN += self.pipeline_waits_given_up()
            except Exception:
                pass
            self.lib.nsdg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        """drains the context's streams; with a communicator the wait is bounded by its deadline (NsdgError on expiry)"""
        self._call(self.lib.nsdg_ctx_synchronize(self.h))

    def copy_f64(self, dst, src):
        """streaming device copy, 16 bytes per lane (the measured copy ceiling of the roofline)"""
        _check_f64(dst, src)
        if dst.numel() != src.numel():
            raise NsdgError("copy_f64: sizes differ")
        self._call(self.lib.nsdg_copy_f64(self.h, dst.data_ptr(), src.data_ptr(), src.numel()))

    def phase_timing(self, enable):
        """per-phase device timing on / off (nsdg_phase_timing_set); off discards what was pending"""
        self._call(self.lib.nsdg_phase_timing_set(self.h, int(bool(enable))))

    def phase_mark(self, phase):
        """one timing event on the context's stream: closes the running phase and opens `phase` (an id below PHASE_MAX, or PHASE_END);
        does nothing while timing is off"""
        self._call(self.lib.nsdg_phase_mark(self.h, int(phase)))

    def phase_times(self, reset=False):
        """waits for the last mark; ({phase id: (ms, count)} for the ids that closed an interval, (total_ms, spans)) (nsdg_phase_times)"""
        t = PhaseTable()
        self._call(self.lib.nsdg_phase_times(self.h, C.byref(t), int(bool(reset))))
        return {k: (float(t.ms[k]), int(t.count[k])) for k in range(PHASE_MAX) if t.count[k]}, (float(t.total_ms), int(t.spans))

    def comm_deadline(self, seconds):
        """upper bound on any wait for a neighbour rank (0 = for ever)"""
        self._call(self.lib.nsdg_comm_deadline_set(self.h, float(seconds)))

    def comm_simulate_wire(self, delay_us=0.0, gbs=0.0):
        """rehearsal aid: every exchange spins for delay_us + bytes / gbs on the communication stream (0, 0 = off)"""
        self._call(self.lib.nsdg_comm_simulate_wire(self.h, float(delay_us), float(gbs)))

    def num_cus(self):
        import torch

        return torch.cuda.get_device_properties(self.device).multi_processor_count

    # ---- row-block communicator and ghost-row exchange plans (csrc/halo.hip)
    def comm_init_rccl(self, rank, world, group=None):
        """RCCL communicator of this context; the ncclUniqueId of rank 0 travels through torch.distributed
        (any backend: it is 128 bytes, once)"""
        import torch.distributed as dist

        buf = C.create_string_buffer(COMM_ID_BYTES)
        if rank == 0:
            self._call(self.lib.nsdg_comm_unique_id(buf))
        if world > 1:
            box = [buf.raw if rank == 0 else None]
            dist.broadcast_object_list(box, src=0, group=group)
            buf = C.create_string_buffer(box[0], COMM_ID_BYTES)
        self._call(self.lib.nsdg_comm_init(self.h, rank, world, buf))

    def comm_init_local(self, group_id, rank, world):
        """in-process communicator: the ranks of `group_id` are contexts driven by one thread each"""
        self._call(self.lib.nsdg_comm_init_local(self.h, int(group_id), rank, world))

    def comm_finalize(self):
        self._call(self.lib.nsdg_comm_finalize(self.h))

    def halo_plan(self, below, above, up_send, down_send, from_above, from_below):
        """plan of one kind of exchange; the arguments are lists of CONTIGUOUS tensor views (row blocks)"""
        return HaloPlanHandle(self, below, above, up_send, down_send, from_above, from_below)

    # ---- row-block drivers (csrc/rowblock.hip): one call per model step
    def _geometry(self, desc, blk, peers):
        desc.nx, desc.ny, desc.j0, desc.j1 = blk.nx, blk.ny, blk.j0, blk.j1
        desc.depth_below, desc.depth_above = blk.depth_below, blk.depth_above
        desc.rank_below = -1 if peers[0] is None else peers[0]
        desc.rank_above = -1 if peers[1] is None else peers[1]

    def rb_mevp(self, blk, peers, nsub, overlap, use_graph, s2, uv2, packed, pg):
        """native sub-cycle driver of a row block; s2 = (s, sb): two lists of three tiled stress arrays, uv2 =
        ((u, v), (ub, vb)).  Returns run(parity) -> parity of the result and the plan's (per_pass, group_passes)."""
        d = RbMevpDesc()
        self._geometry(d, blk, peers)
        d.nsub, d.overlap, d.use_graph = nsub, int(bool(overlap)), int(bool(use_graph))
        ts = list(s2[0]) + list(s2[1]) + list(uv2[0]) + list(uv2[1]) + [packed, pg]
        _check_f64(*ts)
        for k in range(2):
            d.s11[k], d.s12[k], d.s22[k] = (s2[k][i].data_ptr() for i in range(3))
            d.u[k], d.v[k] = uv2[k][0].data_ptr(), uv2[k][1].data_ptr()
        d.packed, d.pg = packed.data_ptr(), pg.data_ptr()
        h = VP()
        self._call(self.lib.nsdg_rb_mevp_create(self.h, C.byref(d), C.byref(h)))
        per_pass, group = I32(), I32()
        self._call(self.lib.nsdg_rb_mevp_info(h, C.byref(per_pass), C.byref(group)))
        out, fn, ch = I32(), self.lib.nsdg_rb_mevp_run, self.h

        def run(parity):
            rc = fn(ch, h, parity, C.byref(out))
            if rc != 0:
                self._call(rc)
            return out.value

        def stats(reset=False):
            st = HaloStats()
            self._call(self.lib.nsdg_rb_mevp_stats(ch, h, C.byref(st), int(reset)))
            return st.as_dict()

        def close():  # destroys the plan (its halo plans, packed buffers and events); idempotent, before the context goes
            if run.handle is not None and self.h:
                self.lib.nsdg_rb_mevp_destroy(run.handle)
            run.handle = None

        run.keep = ts
        run.handle = h
        run.stats = stats
        run.close = close
        return run, per_pass.value, group.value

    def rb_bbm(self, blk, peers, nsub, overlap, s2, uv2, packed, gauss, damage, damage_work, complete_nodes=False):
        """native brittle sub-cycle driver of a row block (nsdg_rb_bbm_*); s2, uv2: as rb_mevp; gauss = (hg, eg, pm) of bbm_prepare;
        damage = the transport's two buffers of D (phi, t1), damage_work: the partner inside the call.  Returns
        run(parity, damage_parity) -> parity of the result; D ends in damage[damage_parity]"""
        d = RbBbmDesc()
        self._geometry(d, blk, peers)
        d.nsub, d.overlap, d.complete_nodes = nsub, int(bool(overlap)), int(bool(complete_nodes))
        ts = list(s2[0]) + list(s2[1]) + list(uv2[0]) + list(uv2[1]) + [packed] + list(gauss) + list(damage) + [damage_work]
        _check_f64(*ts)
        for k in range(2):
            d.s11[k], d.s12[k], d.s22[k] = (s2[k][i].data_ptr() for i in range(3))
            d.u[k], d.v[k] = uv2[k][0].data_ptr(), uv2[k][1].data_ptr()
            d.D[k] = damage[k].data_ptr()
        d.packed, d.D_work = packed.data_ptr(), damage_work.data_ptr()
        d.hg, d.eg, d.pm = (t.data_ptr() for t in gauss)
        h = VP()
        self._call(self.lib.nsdg_rb_bbm_create(self.h, C.byref(d), C.byref(h)))
        out, fn, ch = I32(), self.lib.nsdg_rb_bbm_run, self.h

        def run(parity, damage_parity):
            rc = fn(ch, h, parity, damage_parity, C.byref(out))
            if rc != 0:
                self._call(rc)
            return out.value

        def stats(reset=False):
            st = HaloStats()
            self._call(self.lib.nsdg_rb_bbm_stats(ch, h, C.byref(st), int(reset)))
            return st.as_dict()

        def close():
            if run.handle is not None and self.h:
                self.lib.nsdg_rb_bbm_destroy(run.handle)
            run.handle = None

        run.keep = ts
        run.handle = h
        run.stats = stats
        run.close = close
        return run

    def rb_transport(self, blk, peers, phi, t1, t2, adv, bounds=None):
        """native SSP-RK3 transport driver of a row block; returns run(dt, parity) -> parity of the new state.  bounds: the closure of the
        step as the plan's OWN (one (lo, hi, cap_mean) per field, () = none), whatever set_transport_bounds says on the context; None:
        the context's bounds of the moment the plan runs"""
        d = RbTransportDesc()
        self._geometry(d, blk, peers)
        d.order, d.nfields = 2, len(phi)
        if bounds is not None:
            d.own_bounds, d.nbounds = 1, len(bounds)
            for k, (lo, hi, cap) in enumerate(bounds):
                d.bounds[k].lo, d.bounds[k].hi, d.bounds[k].cap_mean = float(lo), float(hi), int(bool(cap))
        ts = list(phi) + list(t1) + list(t2) + list(adv)
        _check_f64(*ts)
        for i in range(len(phi)):
            d.phi[i], d.t1[i], d.t2[i] = phi[i].data_ptr(), t1[i].data_ptr(), t2[i].data_ptr()
        d.vx_dg, d.vy_dg, d.un_x, d.un_y = (a.data_ptr() for a in adv)
        h = VP()
        self._call(self.lib.nsdg_rb_transport_create(self.h, C.byref(d), C.byref(h)))
        out, fn, ch = I32(), self.lib.nsdg_rb_transport_run, self.h

        def run(dt, parity):
            rc = fn(ch, h, float(dt), parity, C.byref(out))
            if rc != 0:
                self._call(rc)
            return out.value

        def stats(reset=False):
            st = HaloStats()
            self._call(self.lib.nsdg_rb_transport_stats(ch, h, C.byref(st), int(reset)))
            return st.as_dict()

        def close():
            if run.handle is not None and self.h:
                self.lib.nsdg_rb_transport_destroy(run.handle)
            run.handle = None

        run.keep = ts
        run.handle = h
        run.stats = stats
        run.close = close
        return run

    # ---- arrays private to the mEVP sub-cycle (stress, ice strength) live in the tiled layout
    def private_zeros(self, nc, ny, nx, device):
        import torch

        return torch.zeros(ny, (nx + TILE - 1) // TILE, nc * TILE, dtype=torch.float64, device=device)

    @staticmethod
    def private_rows(f, j0, j1):
        return f[j0:j1]

    @staticmethod
    def private_to_planes(f, nx):
        """tiled private array -> coefficient planes [nc, ny, nx] (checkpoints, gathers)"""
        return untile(f, nx)

    @staticmethod
    def planes_to_private(a):
        return tile(a)

    # ---- column physics
    def column_default_params(self, **kw):
        p = ColumnParams()
        self.lib.nsdg_column_default_params(C.byref(p))
        for k, v in kw.items():
            if k == "albedo":
                p.albedo_kind = ALBEDO[v]
            elif k == "freezing":
                p.freezing_kind = FREEZING[v]
            else:
                if not hasattr(p, k):
                    raise NsdgError("unknown column parameter " + k)
                setattr(p, k, v)
        return p

    def set_column_params(self, p):
        self._call(self.lib.nsdg_column_params_set(self.h, C.byref(p)))

    def column_step(self, dt, state, forcing, newice, diag=None):
        ts = [state[k] for k in STATE] + [forcing[k] for k in FORCING] + [newice]
        _check_f64(*ts, diag)
        n = ts[0].numel()
        # the ABI takes bare pointers and one n: a shorter plane would be read and written past its end on the device
        for name, t in zip(STATE + FORCING + ["newice"], ts):
            if t.numel() != n:
                raise NsdgError("column_step: %s has %d elements, hice has %d" % (name, t.numel(), n))
        if diag is not None and diag.numel() != NDIAG * n:
            raise NsdgError("column_step: diag has %d elements, expected NDIAG * n = %d" % (diag.numel(), NDIAG * n))
        self._call(self.lib.nsdg_column_step(self.h, n, float(dt), *[_ptr(t) for t in ts], _ptr(diag)))

    # ---- slab ocean (include/nsdg_ocean.h): the column step that also advances the mixed layer's sst and sss
    def slab_default_params(self, **kw):
        return slab_default_params(**kw)

    def set_slab_params(self, p):
        """nsdg_slab_params_set: acts on the next column_step_ocean"""
        self._call(self.lib.nsdg_slab_params_set(self.h, C.byref(p)))

    def column_step_ocean(self, dt, state, forcing, newice, ext=None, skip=None):
        """nsdg_column_step_ocean: column_step that writes forcing["sst"], forcing["sss"] too.  ext: {"sst": , "sss": } relaxation targets
        (read only under their relaxation time; either may be absent otherwise); skip: a uint8 tensor of n bytes or None"""
        import torch

        ts = [state[k] for k in STATE] + [forcing[k] for k in FORCING] + [newice]
        ex = [(ext or {}).get(k) for k in ("sst", "sss")]
        _check_f64(*ts, *ex)
        n = ts[0].numel()
        for name, t in zip(STATE + FORCING + ["newice", "sst_ext", "sss_ext"], ts + ex):
            if t is not None and t.numel() != n:
                raise NsdgError("column_step_ocean: %s has %d elements, hice has %d" % (name, t.numel(), n))
        if skip is not None and (skip.dtype != torch.uint8 or not skip.is_contiguous() or not skip.is_cuda or skip.numel() != n):
            raise NsdgError("column_step_ocean: skip must be a contiguous uint8 CUDA tensor of %d bytes" % n)
        self._call(self.lib.nsdg_column_step_ocean(self.h, n, float(dt), *[_ptr(t) for t in ts], _ptr(ex[0]), _ptr(ex[1]), _ptr(skip)))

    # ---- dynamics
    def mevp_default_params(self, **kw):
        p = MevpParams()
        self.lib.nsdg_mevp_default_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise NsdgError("unknown mEVP parameter " + k)
            setattr(p, k, v)
        return p

    def set_mevp_params(self, p):
        self._call(self.lib.nsdg_mevp_params_set(self.h, C.byref(p)))

    def set_grid(self, nx, ny, hx, hy):
        self._call(self.lib.nsdg_grid_set(self.h, nx, ny, float(hx), float(hy)))
        if (nx, ny) != (self.nx, self.ny):
            self.land_mask = self.basal_depth = self.snow_load = None  # the library dropped a mask, a depth array and a snow field of the old shape
            self.ssh = None  # and a sea-surface height
        self.nx, self.ny = nx, ny

    # ---- land mask (include/nsdg.h "land mask"): coastlines as fixed nodes of the sub-cycle
    def set_land_mask(self, land):
        """nsdg_land_mask_set: `land` = a contiguous uint8 or bool CUDA tensor [ny, nx] of the local array (1 = land), kept alive by this
        object while it is set; None clears the mask.  Acts from the next coefficient packing on"""
        import torch

        if land is not None:
            if land.dtype not in (torch.uint8, torch.bool) or not land.is_contiguous() or not land.is_cuda:
                raise NsdgError("expected a contiguous uint8 or bool CUDA tensor")
            if tuple(land.shape) != (self.ny, self.nx):
                raise NsdgError("the land mask has shape %s, the local array is [%d, %d]" % (tuple(land.shape), self.ny, self.nx))
        self._call(self.lib.nsdg_land_mask_set(self.h, _ptr(land)))
        self.land_mask = land

    def land_clear(self, f, j0=0, j1=None):
        """nsdg_land_clear: 0 in every coefficient plane of f ([nc, ny, nx] or one plane [ny, nx]) at the land elements of rows [j0, j1)"""
        _check_f64(f)
        nplanes = f.shape[0] if f.dim() == 3 else 1
        if f.numel() != nplanes * self.nx * self.ny:
            raise NsdgError("land_clear: %d values, the planes of the grid need %d" % (f.numel(), nplanes * self.nx * self.ny))
        self._call(self.lib.nsdg_land_clear(self.h, j0, self.ny if j1 is None else j1, nplanes, _ptr(f)))

    def land_clear_nodes(self, u, v):
        """nsdg_land_clear_nodes: u = v = 0 at the land nodes of the CG2 lattice"""
        _check_f64(u, v)
        n = (2 * self.nx + 1) * (2 * self.ny + 1)
        if u.numel() != n or v.numel() != n:
            raise NsdgError("land_clear_nodes: the nodal arrays of the grid hold %d values" % n)
        self._call(self.lib.nsdg_land_clear_nodes(self.h, _ptr(u), _ptr(v)))

    # ---- landfast ice (include/nsdg_basal.h): grounding on shoals as a basal stress in the momentum update
    def basal_default_params(self, **kw):
        return basal_default_params(**kw)

    def set_basal_params(self, p):
        """nsdg_basal_params_set: acts from the next coefficient packing on"""
        self._call(self.lib.nsdg_basal_params_set(self.h, C.byref(p)))

    def set_basal_depth(self, depth):
        """nsdg_basal_depth_set: `depth` = a contiguous float64 CUDA tensor [ny, nx] of the local array (metres, >= 0), kept alive by this
        object while it is set; None clears it.  Acts from the next coefficient packing on"""
        if depth is not None:
            _check_f64(depth)
            if tuple(depth.shape) != (self.ny, self.nx):
                raise NsdgError("the depth array has shape %s, the local array is [%d, %d]" % (tuple(depth.shape), self.ny, self.nx))
        self._call(self.lib.nsdg_basal_depth_set(self.h, _ptr(depth)))
        self.basal_depth = depth

    def basal_critical(self, cgh, cga, tb):
        """nsdg_basal_critical: tb = the critical stress T_b at every node of the CG2 lattice, what the next packing would store"""
        _check_f64(cgh, cga, tb)
        n = (2 * self.nx + 1) * (2 * self.ny + 1)
        if cgh.numel() != n or cga.numel() != n or tb.numel() != n:
            raise NsdgError("basal_critical: the nodal arrays of the grid hold %d values" % n)
        self._call(self.lib.nsdg_basal_critical(self.h, _ptr(cgh), _ptr(cga), _ptr(tb)))

    # ---- snow load (include/nsdg_snow.h): the momentum equation feels the snow's weight
    def set_snow_load(self, snow, rho_snow=SNOW_DENSITY):
        """nsdg_snow_load_set: `snow` = a contiguous float64 CUDA tensor of the local array, [ny, nx] (the column plane hsnow) or
        [nc, ny, nx] with nc = 1, 3 or 6 (the DG field S), kept alive by this object while it is set; None clears it.  Read by the next
        coefficient packing"""
        ncoef = 0
        if snow is not None:
            _check_f64(snow)
            if snow.dim() not in (2, 3) or tuple(snow.shape[-2:]) != (self.ny, self.nx):
                raise NsdgError("the snow field has shape %s, the local array is [%d, %d]" % (tuple(snow.shape), self.ny, self.nx))
            ncoef = 1 if snow.dim() == 2 else snow.shape[0]
        self._call(self.lib.nsdg_snow_load_set(self.h, _ptr(snow), ncoef, float(rho_snow)))
        self.snow_load = snow

    def snow_load_nodal(self, cgh, cga, out):
        """nsdg_snow_load_nodal: out = the thickness h' behind the nodal mass at every node of the CG2 lattice, what the next packing
        would store as its first coefficient before the ice-free scaling"""
        _check_f64(cgh, cga, out)
        n = (2 * self.nx + 1) * (2 * self.ny + 1)
        if cgh.numel() != n or cga.numel() != n or out.numel() != n:
            raise NsdgError("snow_load_nodal: the nodal arrays of the grid hold %d values" % n)
        self._call(self.lib.nsdg_snow_load_nodal(self.h, _ptr(cgh), _ptr(cga), _ptr(out)))

    # ---- sea-surface tilt (include/nsdg_tilt.h): the tilt force from the gradient of a sea-surface height
    def set_tilt(self, ssh, gravity=GRAVITY):
        """nsdg_tilt_set: `ssh` = a contiguous float64 CUDA tensor of the local CG2 lattice, [2 ny + 1, 2 nx + 1] metres, kept alive by this
        object while it is set; None clears it.  Read by the next coefficient packing"""
        if ssh is not None:
            _check_f64(ssh)
            if ssh.numel() != (2 * self.nx + 1) * (2 * self.ny + 1):
                raise NsdgError("the sea-surface height has shape %s, the local lattice is [%d, %d]" % (tuple(ssh.shape), 2 * self.ny + 1, 2 * self.nx + 1))
        self._call(self.lib.nsdg_tilt_set(self.h, _ptr(ssh), float(gravity)))
        self.ssh = ssh

    def tilt_nodal(self, sx, sy):
        """nsdg_tilt_nodal: sx, sy = the gradient of the sea-surface height the next packing would use, at every node of the CG2 lattice"""
        _check_f64(sx, sy)
        n = (2 * self.nx + 1) * (2 * self.ny + 1)
        if sx.numel() != n or sy.numel() != n:
            raise NsdgError("tilt_nodal: the nodal arrays of the grid hold %d values" % n)
        self._call(self.lib.nsdg_tilt_nodal(self.h, _ptr(sx), _ptr(sy)))

    def boxtest_ssh(self, domain_size, fc, gravity, ssh):
        """nsdg_boxtest_ssh: ssh = the sea-surface height whose geostrophic current is the box test's gyre (boxtest_forcing: ocean)"""
        _check_f64(ssh)
        if ssh.numel() != (2 * self.nx + 1) * (2 * self.ny + 1):
            raise NsdgError("boxtest_ssh: the nodal arrays of the grid hold %d values" % ((2 * self.nx + 1) * (2 * self.ny + 1)))
        self._call(self.lib.nsdg_boxtest_ssh(self.h, float(domain_size), float(fc), float(gravity), _ptr(ssh)))

    # ---- momentum balance diagnostics (include/nsdg_budget.h): the nodal forces of the momentum equation and their power
    def momentum_budget(self, j0, j1, H, A, wind, s, uv, packed, planes=None, power=None, row0=0):
        """nsdg_momentum_budget on the element rows [j0, j1): `planes` = {"<term>_x" / "<term>_y": a float64 CUDA tensor of the local CG2
        lattice} -- only these are written --, `power` = a [9, rows] tensor of the row totals (term ids 0..7, then the kinetic energy), row
        iy at column iy - row0; the state (uv, s) and `packed` are those the sub-cycle left"""
        planes = dict(planes or {})
        ts = [H, A, wind[0], wind[1], s[0], s[1], s[2], uv[0], uv[1], packed] + list(planes.values())
        _check_f64(*ts)
        n = (2 * self.nx + 1) * (2 * self.ny + 1)
        out = BudgetOut()
        names = [f[0] for f in BudgetOut._fields_[:16]]
        for k, t in planes.items():
            if k not in names:
                raise NsdgError("momentum_budget: unknown plane %r" % (k,))
            if t.numel() != n:
                raise NsdgError("momentum_budget: plane %s holds %d values, the nodal arrays of the grid hold %d" % (k, t.numel(), n))
            setattr(out, k, t.data_ptr())
        if power is not None:
            _check_f64(power)
            if power.dim() != 2 or power.shape[0] != BUDGET_QUANTITIES:
                raise NsdgError("momentum_budget: power must be [%d, rows]" % BUDGET_QUANTITIES)
            out.power, out.power_stride, out.row0 = power.data_ptr(), power.shape[1], row0
        self._call(self.lib.nsdg_momentum_budget(self.h, j0, j1, *[_ptr(t) for t in ts[:10]], C.byref(out)))

    def set_mevp_variant(self, variant):
        self._call(self.lib.nsdg_mevp_variant_set(self.h, variant))
        self.mevp_variant = variant

    def set_mevp_strip_rows(self, rows):
        self._call(self.lib.nsdg_mevp_strip_rows_set(self.h, rows))

    def set_mevp_occupancy(self, waves_per_simd):
        self._call(self.lib.nsdg_mevp_occupancy_set(self.h, waves_per_simd))

    def set_transport_variant(self, variant, strip_rows=0):
        self._call(self.lib.nsdg_transport_variant_set(self.h, variant, strip_rows))

    def prepare_advection(self, order, u, v, vx, vy, unx, uny):
        _check_f64(u, v, vx, vy, unx, uny)
        self._call(self.lib.nsdg_prepare_advection(self.h, order, *[_ptr(t) for t in (u, v, vx, vy, unx, uny)]))

    def transport_stage(self, order, j0, j1, dt, a, b, phi0, phis, out, adv):
        _check_f64(*phi0, *phis, *out, *adv)
        self._call(self.lib.nsdg_transport_stage(self.h, order, j0, j1, float(dt), float(a), float(b), len(phis),
                                                 _ptr_array(phi0), _ptr_array(phis), _ptr_array(out),
                                                 *[_ptr(t) for t in adv]))

    def transport_step(self, order, dt, fields, adv, scratch):
        _check_f64(*fields, *adv, scratch)
        need = 2 * sum(f.numel() for f in fields)
        if scratch.numel() < need:
            raise NsdgError("transport scratch too small: need %d doubles" % need)
        self._call(self.lib.nsdg_transport_step(self.h, order, float(dt), len(fields), _ptr_array(fields),
                                                *[_ptr(t) for t in adv], _ptr(scratch)))

    def transport_step_oop(self, order, dt, fields_in, fields_out, adv):
        """one SSP-RK step of every field, out of place, all stages in ONE launch (fields_out must not alias fields_in)"""
        _check_f64(*fields_in, *fields_out, *adv)
        self._call(self.lib.nsdg_transport_step_oop(self.h, order, float(dt), len(fields_in), _ptr_array(fields_in), _ptr_array(fields_out),
                                                    *[_ptr(t) for t in adv]))

    def transport_step_oop_rows(self, order, j0, j1, dt, fields_in, fields_out, adv):
        """the fused step on the rows [j0, j1) only (a row block's own rows; fields_in valid order + 2 rows around them)"""
        _check_f64(*fields_in, *fields_out, *adv)
        self._call(self.lib.nsdg_transport_step_oop_rows(self.h, order, j0, j1, float(dt), len(fields_in), _ptr_array(fields_in),
                                                         _ptr_array(fields_out), *[_ptr(t) for t in adv]))

    def pipeline_waits_given_up(self):
        """waits of the point-to-point mEVP pipelines (csrc/mevp_p2p.h) on THIS context that gave up since the last call: 0 in a correct
        program (a non-zero count means wrong results of the launches in between, and synchronize / mevp_subcycle / the row-block
        run raise NsdgError until this call has taken the events); waits for the context's stream"""
        n = C.c_uint32(0)
        self._call(self.lib.nsdg_mevp_pipeline_health(self.h, C.byref(n)))
        return int(n.value)

    def set_transport_bounds(self, bounds):
        """closure of a transport step: one (lo, hi, cap_mean) per advected field, in the order of the step calls' field lists;
        () or None = none.  abi.H_A_BOUNDS: the dynamics' H and A"""
        bounds = tuple(bounds or ())
        arr = (FieldBounds * max(len(bounds), 1))()
        for k, (lo, hi, cap) in enumerate(bounds):
            arr[k].lo, arr[k].hi, arr[k].cap_mean = float(lo), float(hi), int(bool(cap))
        self._call(self.lib.nsdg_transport_bounds_set(self.h, len(bounds), arr))
        self.transport_bounds = bounds

    def transport_limit(self, order, j0, j1, fields):
        """cap + scaling limiter in place on the rows [j0, j1) (what the step entry points apply themselves)"""
        _check_f64(*fields)
        self._call(self.lib.nsdg_transport_limit(self.h, order, j0, j1, len(fields), _ptr_array(fields)))

    def dg_to_cg(self, f_dg, f_cg):
        _check_f64(f_dg, f_cg)
        if f_dg.dim() != 3:
            raise NsdgError("dg_to_cg expects coefficient planes [nc, ny, nx]")
        self._call(self.lib.nsdg_dg_to_cg(self.h, f_dg.shape[0], _ptr(f_dg), _ptr(f_cg)))

    def ice_strength(self, H, A, pg, j0=0, j1=None):
        _check_f64(H, A, pg)
        self._call(self.lib.nsdg_ice_strength(self.h, j0, self.ny if j1 is None else j1, _ptr(H), _ptr(A), _ptr(pg)))

    # ---- column state transport (include/nsdg.h): tice0 rides on the ice as Q = H T
    def tracer_weight(self, order, j0, j1, H, T, Q):
        """nsdg_tracer_weight: Q[c] = T * H[c] for every coefficient plane c of the elements of rows [j0, j1)"""
        _check_f64(H, T, Q)
        self._call(self.lib.nsdg_tracer_weight(self.h, order, j0, j1, _ptr(H), _ptr(T), _ptr(Q)))

    def tracer_recover(self, order, j0, j1, H, A, Q, min_conc, min_thick, T):
        """nsdg_tracer_recover: T = Q[0] / H[0] where the element of rows [j0, j1) holds ice (H[0] > 0, A[0] >= min_conc,
        H[0] >= min_thick A[0]); T keeps its value elsewhere"""
        _check_f64(H, A, Q, T)
        self._call(self.lib.nsdg_tracer_recover(self.h, order, j0, j1, _ptr(H), _ptr(A), _ptr(Q), float(min_conc), float(min_thick), _ptr(T)))

    # ---- ice tracers (include/nsdg.h "ice tracers"; csrc/tracers.hip): up to TRACERS_MAX intensive planes per call
    @staticmethod
    def _tracer_planes(call, *lists):
        n = len(lists[0])
        if not 1 <= n <= TRACERS_MAX or any(len(x) != n for x in lists):
            raise NsdgError("%s: 1 .. %d tracers, one entry per tracer in every list" % (call, TRACERS_MAX))
        return n

    def tracers_weight(self, order, j0, j1, H, T, Q):
        """nsdg_tracers_weight: Q[k][c] = T[k] * H[c] for every tracer k and coefficient plane c of the elements of rows [j0, j1)"""
        n = self._tracer_planes("tracers_weight", T, Q)
        _check_f64(H, *T, *Q)
        self._call(self.lib.nsdg_tracers_weight(self.h, order, j0, j1, _ptr(H), n, _ptr_array(T), _ptr_array(Q)))

    def tracers_recover(self, order, j0, j1, H, A, Q, kinds, dt, min_conc, min_thick, T):
        """nsdg_tracers_recover: where the element of rows [j0, j1) holds ice T[k] = Q[k][0] / H[0], plus dt for kinds[k] == TRACER_AGE;
        T[k] = 0 where it does not"""
        n = self._tracer_planes("tracers_recover", Q, kinds, T)
        _check_f64(H, A, *Q, *T)
        self._call(self.lib.nsdg_tracers_recover(self.h, order, j0, j1, _ptr(H), _ptr(A), n, _ptr_array(Q), (I32 * n)(*[int(k) for k in kinds]),
                                                 float(dt), float(min_conc), float(min_thick), _ptr_array(T)))

    def tracers_dilute(self, j0, j1, h_before, h_after, T):
        """nsdg_tracers_dilute: growth of the mean thickness from max(h_before, 0) to h_after mixes every T[k] with ice of the value 0"""
        n = self._tracer_planes("tracers_dilute", T)
        _check_f64(h_before, h_after, *T)
        self._call(self.lib.nsdg_tracers_dilute(self.h, j0, j1, _ptr(h_before), _ptr(h_after), n, _ptr_array(T)))

    # ---- history output (include/nsdg.h "history output"; csrc/history.hip)
    def history_accumulate(self, j0, j1, fields, sources, store, row0, acc):
        """nsdg_history_accumulate: one sample of every field of `fields` (names of HISTORY_FIELDS) at the elements of the local rows
        [j0, j1), stored into (store) or added to acc[k, iy - row0, ix]; acc: [len(fields), rows, nx] with rows >= j1 - row0.  sources:
        name -> tensor for the names of HISTORY_SOURCES the fields read (H, A, D: DG planes [nc, ny, nx], plane 0 is read; u, v: the CG2
        lattice; s11, s12, s22: tiled; hsnow, tice: one plane)"""
        ids = self._history_ids(fields, HISTORY_FIELDS, "history field")
        src = self._history_sources("history_accumulate", sources, acc)
        self._history_check_acc("history_accumulate", acc, len(fields), j1, row0)
        self._call(self.lib.nsdg_history_accumulate(self.h, j0, j1, len(fields), ids, C.byref(src), int(bool(store)), row0,
                                                    acc.shape[1] * acc.shape[2], _ptr(acc)))

    def history_accumulate_stats(self, j0, j1, pairs, sources, store, row0, acc, wacc=None):
        """nsdg_history_accumulate_stats: history_accumulate with a statistic per plane.  pairs: (field, stat) with stat a name of
        HISTORY_STATS; wacc: the weight plane [rows, nx] of the "ice_mean" pairs (None when there is none)"""
        pairs = [tuple(p) for p in pairs]
        ids = self._history_ids([f for f, _ in pairs], HISTORY_FIELDS, "history field")
        stats = self._history_ids([s for _, s in pairs], HISTORY_STATS, "history statistic")
        src = self._history_sources("history_accumulate_stats", sources, acc, wacc)
        self._history_check_acc("history_accumulate_stats", acc, len(pairs), j1, row0)
        if wacc is not None and tuple(wacc.shape) != tuple(acc.shape[1:]):
            raise NsdgError("history_accumulate_stats: wacc has shape %s, expected %s" % (tuple(wacc.shape), tuple(acc.shape[1:])))
        self._call(self.lib.nsdg_history_accumulate_stats(self.h, j0, j1, len(pairs), ids, stats, C.byref(src), int(bool(store)), row0,
                                                          acc.shape[1] * acc.shape[2], _ptr(acc), _ptr(wacc)))

    def history_row_totals(self, j0, j1, quantities, sources, extent_conc, row0, out):
        """nsdg_history_row_totals: out[k, iy - row0] = the total of quantity k (names of SERIES_QUANTITIES) over row iy, for the local rows
        [j0, j1); out: [len(quantities), rows] with rows >= j1 - row0 and unit stride along the rows (a slot of a larger buffer is fine)"""
        ids = self._history_ids(quantities, SERIES_QUANTITIES, "series quantity")
        import torch

        src = self._history_sources("history_row_totals", sources)
        if out.dtype != torch.float64 or not out.is_cuda:
            raise NsdgError("expected a float64 CUDA tensor")
        if out.dim() != 2 or out.shape[0] != len(quantities) or out.shape[1] < j1 - row0 or out.stride(1) != 1 or out.stride(0) < out.shape[1]:
            raise NsdgError("history_row_totals: out has shape %s and strides %s, expected [%d, >= %d] with unit stride along the rows"
                            % (tuple(out.shape), tuple(out.stride()), len(quantities), j1 - row0))
        self._call(self.lib.nsdg_history_row_totals(self.h, j0, j1, len(quantities), ids, C.byref(src), float(extent_conc), row0,
                                                    out.stride(0), out.data_ptr()))

    @staticmethod
    def _history_ids(names, known, what):
        ids = (I32 * max(len(names), 1))()
        for k, name in enumerate(names):
            if name not in known:
                raise NsdgError("unknown %s %r (known: %s)" % (what, name, " ".join(known)))
            ids[k] = known.index(name)
        return ids

    def _history_sources(self, call, sources, *outputs):
        ts = {n: sources.get(n) for n in HISTORY_SOURCES}
        _check_f64(*[t for t in outputs if t is not None], *ts.values())
        n_el, n_node = self.nx * self.ny, (2 * self.nx + 1) * (2 * self.ny + 1)
        need = {"H": n_el, "A": n_el, "D": n_el, "hsnow": n_el, "tice": n_el, "u": n_node, "v": n_node}
        need.update({n: (self.ny * ((self.nx + TILE - 1) // TILE) * 8 * TILE) for n in ("s11", "s12", "s22")})
        for n, t in ts.items():  # the ABI takes bare pointers: a shorter array would be read past its end on the device
            if t is not None and t.numel() < need[n]:
                raise NsdgError("%s: source %s has %d values, the grid needs %d" % (call, n, t.numel(), need[n]))
        return HistorySources(*[None if ts[n] is None else ts[n].data_ptr() for n in HISTORY_SOURCES])

    def _history_check_acc(self, call, acc, nplanes, j1, row0):
        if acc.dim() != 3 or acc.shape[0] != nplanes or acc.shape[2] != self.nx or acc.shape[1] < j1 - row0:
            raise NsdgError("%s: acc has shape %s, expected [%d, >= %d, %d]" % (call, tuple(acc.shape), nplanes, j1 - row0, self.nx))

    def concentration_max(self, H, A, j0=0, j1=None):
        """nsdg_concentration_max: largest clamped concentration at the Gauss points of rows [j0, j1) where there is ice (waits for the
        result; NsdgError on a non-finite H or A)"""
        _check_f64(H, A)
        out = D(0.0)
        self._call(self.lib.nsdg_concentration_max(self.h, j0, self.ny if j1 is None else j1, _ptr(H), _ptr(A), C.byref(out)))
        return float(out.value)

    def comm_max_f64(self, value):
        """nsdg_comm_max_f64: the maximum of `value` over the ranks of the context's communicator (collective)"""
        v = D(float(value))
        self._call(self.lib.nsdg_comm_max_f64(self.h, C.byref(v)))
        return float(v.value)

    def comm_max_f64_array(self, t):
        """nsdg_comm_max_f64_array: the elementwise maximum of the device tensor t over the ranks of the context's communicator, in place
        (collective; the local transport synchronises)"""
        _check_f64(t)
        self._call(self.lib.nsdg_comm_max_f64_array(self.h, _ptr(t), t.numel()))

    # ---- drifters (include/nsdg.h "drifters"; csrc/drifters.hip)
    def drifters_advance(self, j0, j1, dt, min_conc, u, v, A, d_in, d_out):
        """nsdg_drifters_advance: one Heun step of the drifters d_in ([3, n]: x, y, status) whose element lies in the local rows [j0, j1),
        written to d_out; every other drifter of d_out is -inf in all three planes.  u, v: the CG2 velocity; A: the concentration ([nc, ny,
        nx], plane 0 is read)"""
        _check_f64(u, v, A, d_in, d_out)
        if d_in.dim() != 2 or d_in.shape[0] != 3 or tuple(d_out.shape) != tuple(d_in.shape):
            raise NsdgError("drifters_advance: d_in and d_out must be [3, n] arrays of one shape, got %s and %s" % (tuple(d_in.shape), tuple(d_out.shape)))
        n_node = (2 * self.nx + 1) * (2 * self.ny + 1)
        if u.numel() != n_node or v.numel() != n_node:  # the ABI takes bare pointers
            raise NsdgError("drifters_advance: the nodal arrays of the grid hold %d values" % n_node)
        if A.numel() < self.nx * self.ny:
            raise NsdgError("drifters_advance: A has %d values, the grid needs %d" % (A.numel(), self.nx * self.ny))
        self._call(self.lib.nsdg_drifters_advance(self.h, j0, j1, float(dt), float(min_conc), d_in.shape[1], _ptr(u), _ptr(v), _ptr(A),
                                                  _ptr(d_in), _ptr(d_out)))

    # ---- point samples (include/nsdg.h "point samples"; csrc/points.hip)
    def points_sample(self, j0, j1, order, x, y, fields, sources, out):
        """nsdg_points_sample: out[k, p] = field k (names of HISTORY_FIELDS) at the point (x[p], y[p]) -- global coordinates in metres -- for
        the points whose element lies in the local rows [j0, j1), -inf for every other point.  x, y: [n] with unit stride (planes of a
        drifter array are fine); out: [len(fields), n] with unit stride along the points (a slot of a larger buffer is fine).  sources: as
        history_accumulate, but H, A, D hold all the coefficient planes of `order` (1 / 3 / 6) and every one is read"""
        import torch

        ids = self._history_ids(fields, HISTORY_FIELDS, "history field")
        src = self._history_sources("points_sample", sources, x, y)
        n, nc = x.numel(), (1, 3, 6)[order] if order in (0, 1, 2) else 1
        for name in ("H", "A", "D"):  # the ABI takes bare pointers
            t = sources.get(name)
            if t is not None and t.numel() < nc * self.nx * self.ny:
                raise NsdgError("points_sample: source %s has %d values, order %d needs %d" % (name, t.numel(), order, nc * self.nx * self.ny))
        if x.dim() != 1 or y.dim() != 1 or y.numel() != n or (n > 1 and (x.stride(0) != 1 or y.stride(0) != 1)):
            raise NsdgError("points_sample: x and y must be [n] arrays of one length with unit stride, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        if out.dtype != torch.float64 or not out.is_cuda:
            raise NsdgError("expected a float64 CUDA tensor")
        if out.dim() != 2 or tuple(out.shape) != (len(fields), n) or (n > 1 and out.stride(1) != 1) or (len(fields) > 1 and out.stride(0) < n):
            raise NsdgError("points_sample: out has shape %s and strides %s, expected [%d, %d] with unit stride along the points"
                            % (tuple(out.shape), tuple(out.stride()), len(fields), n))
        self._call(self.lib.nsdg_points_sample(self.h, j0, j1, order, n, x.data_ptr(), y.data_ptr(), len(fields), ids, C.byref(src),
                                               max(out.stride(0), n) if len(fields) > 1 else n, out.data_ptr()))

    def boxtest_forcing(self, domain_size, t, wind=None, ocean=None):
        ts = list(wind or (None, None)) + list(ocean or (None, None))
        _check_f64(*ts)
        self._call(self.lib.nsdg_boxtest_forcing(self.h, float(domain_size), float(t), *[_ptr(x) for x in ts]))

    def set_block(self, row0, ny_global):
        """placement of the local array in the global domain (analytic forcing providers)"""
        self._call(self.lib.nsdg_block_set(self.h, int(row0), int(ny_global)))

    def column_forcing(self, kind, t, forcing):
        """thermodynamic forcing planes at model time t; kind: "dummy" (the reference's constants) or "winter" """
        ts = [forcing[k] for k in ("tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall")]
        _check_f64(*ts)
        self._call(self.lib.nsdg_column_forcing(self.h, {"dummy": 0, "winter": 1}[kind], float(t), *[_ptr(x) for x in ts]))

    def column_wind(self, ua, va, wind):
        _check_f64(ua, va, wind)
        self._call(self.lib.nsdg_column_wind(self.h, _ptr(ua), _ptr(va), _ptr(wind)))

    def forcing_sample(self, where, rec0, rec1, w, out):
        """nsdg_forcing_sample: out[k] = the records rec0[k], rec1[k] ([nyr, nxr] tensors on one lattice) sampled bilinearly onto the
        local array's CG2 nodes (where = "nodes") or element centres (where = "elements") and interpolated in time with weight w in
        [0, 1] (include/nsdg.h "forcing from a file")"""
        rec0, rec1, out = list(rec0), list(rec1), list(out)
        if not (len(rec0) == len(rec1) == len(out)) or not rec0:
            raise NsdgError("forcing_sample: rec0, rec1 and out need the same number (>= 1) of fields")
        _check_f64(*(rec0 + rec1 + out))
        nyr, nxr = rec0[0].shape
        for r in rec0 + rec1:
            if tuple(r.shape) != (nyr, nxr):
                raise NsdgError("forcing_sample: every record plane must be [nyr, nxr] = [%d, %d]" % (nyr, nxr))
        n = (2 * self.nx + 1) * (2 * self.ny + 1) if where == "nodes" else self.nx * self.ny
        for o in out:  # the kernel writes n values into every output plane
            if o.numel() != n:
                raise NsdgError("forcing_sample: an output plane of %d values, the %s of the grid need %d" % (o.numel(), where, n))
        self._call(self.lib.nsdg_forcing_sample(self.h, {"nodes": AT_NODES, "elements": AT_ELEMENTS}[where], nxr, nyr, len(out),
                                                _ptr_array(rec0), _ptr_array(rec1), float(w), _ptr_array(out)))

    def wind_stress(self, ua, va, tax, tay):
        _check_f64(ua, va, tax, tay)
        self._call(self.lib.nsdg_wind_stress(self.h, ua.numel(), _ptr(ua), _ptr(va), _ptr(tax), _ptr(tay)))

    def mevp_stress(self, k0, k1, u, v, pg, s11, s12, s22):
        _check_f64(u, v, pg, s11, s12, s22)
        self._call(self.lib.nsdg_mevp_stress(self.h, k0, k1, *[_ptr(t) for t in (u, v, pg, s11, s12, s22)]))

    def mevp_pack_nodal(self, dt, u0v0, tau, ocean, cgh, cga, packed):
        ts = [u0v0[0], u0v0[1], tau[0], tau[1], ocean[0], ocean[1], cgh, cga, packed]
        _check_f64(*ts)
        if packed.numel() < 8 * cgh.numel():
            raise NsdgError("packed nodal buffer too small: need %d doubles" % (8 * cgh.numel()))
        self._call(self.lib.nsdg_mevp_pack_nodal(self.h, float(dt), *[_ptr(t) for t in ts]))

    def mevp_prepare(self, dt, H, A, wind, ocean, u0v0, packed):
        """nodal means of H and A + wind stress + coefficient packing in one launch"""
        ts = [H, A, wind[0], wind[1], ocean[0], ocean[1], u0v0[0], u0v0[1], packed]
        _check_f64(*ts)
        self._call(self.lib.nsdg_mevp_prepare(self.h, float(dt), *[_ptr(t) for t in ts]))

    def mevp_velocity(self, j0, j1, s, uv_old, uv_new, packed):
        ts = [s[0], s[1], s[2], uv_old[0], uv_old[1], uv_new[0], uv_new[1], packed]
        _check_f64(*ts)
        self._call(self.lib.nsdg_mevp_velocity(self.h, j0, j1, *[_ptr(t) for t in ts]))

    def _bind_mevp_pass(self, fn, rows, s_in, s_out, uv_old, uv_new, packed, pg):
        """Checks and marshals the arguments of the nsdg_mevp_iterate* entry point `fn` (row arguments `rows`) once and returns
        a zero-argument callable that makes the call.  (Argument checking and ctypes marshalling cost ~20 us per call in
        Python -- comparable to a sub-iteration of a 256-row block -- so the 120-iteration sub-cycle binds its calls once.)"""
        ts = [s_in[0], s_in[1], s_in[2], s_out[0], s_out[1], s_out[2], uv_old[0], uv_old[1], uv_new[0], uv_new[1], packed, pg]
        _check_f64(*ts)
        args = (self.h,) + tuple(I32(r) for r in rows) + tuple(_ptr(t) for t in ts)

        def call():
            rc = fn(*args)
            if rc != 0:
                self._call(rc)
            return ts is None  # the tensors must outlive the binding

        return call

    def mevp_iterate(self, k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        self.bind_mevp_iterate(k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg)()

    def bind_mevp_iterate(self, k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        """pre-validated, pre-marshalled form of mevp_iterate for inner loops (_bind_mevp_pass)"""
        return self._bind_mevp_pass(self.lib.nsdg_mevp_iterate, (k0, j0, j1), s_in, s_out, uv_old, uv_new, packed, pg)

    # ---- brittle rheology (include/nsdg.h "brittle rheology"; csrc/bbm.hip)
    def bbm_default_params(self, **kw):
        return bbm_default_params(**kw)

    def set_bbm_params(self, p):
        self._call(self.lib.nsdg_bbm_params_set(self.h, C.byref(p)))

    def bbm_prepare(self, H, A, hg, eg, pm, j0=0, j1=None):
        """nsdg_bbm_prepare: hg = max(H, 0), eg = exp(-C (1 - clamp(A))), pm = p0 hg^(3/2) eg at the Gauss points of rows [j0, j1) (tiled)"""
        _check_f64(H, A, hg, eg, pm)
        self._call(self.lib.nsdg_bbm_prepare(self.h, j0, self.ny if j1 is None else j1, *[_ptr(t) for t in (H, A, hg, eg, pm)]))

    def bbm_iterate(self, k0, j0, j1, s_in, s_out, d_in, d_out, uv_old, uv_new, packed, gauss):
        """one BBM sub-iteration: stress and damage on rows [k0, j1) (out of place), velocity of the nodes owned by rows [j0, j1);
        gauss = (hg, eg, pm) of bbm_prepare"""
        self.bind_bbm_iterate(k0, j0, j1, s_in, s_out, d_in, d_out, uv_old, uv_new, packed, gauss)()

    def bind_bbm_iterate(self, k0, j0, j1, s_in, s_out, d_in, d_out, uv_old, uv_new, packed, gauss):
        """pre-validated, pre-marshalled form of bbm_iterate for inner loops (as bind_mevp_iterate)"""
        ts = [s_in[0], s_in[1], s_in[2], s_out[0], s_out[1], s_out[2], d_in, d_out, uv_old[0], uv_old[1], uv_new[0], uv_new[1], packed,
              gauss[0], gauss[1], gauss[2]]
        _check_f64(*ts)
        fn = self.lib.nsdg_bbm_iterate
        args = (self.h, I32(k0), I32(j0), I32(j1)) + tuple(_ptr(t) for t in ts)

        def call():
            rc = fn(*args)
            if rc != 0:
                self._call(rc)
            return ts is None  # the tensors must outlive the binding

        return call

    def mevp_iterate2(self, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        """two sub-iterations in one pass on the owned rows [j0, j1) (variant 2)"""
        self.bind_mevp_iterate2(j0, j1, s_in, s_out, uv_old, uv_new, packed, pg)()

    def bind_mevp_iterate2(self, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        return self._bind_mevp_pass(self.lib.nsdg_mevp_iterate2, (j0, j1), s_in, s_out, uv_old, uv_new, packed, pg)

    def mevp_iterate3(self, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        """three sub-iterations in one pass on the owned rows [j0, j1) (variant 3)"""
        self.bind_mevp_iterate3(j0, j1, s_in, s_out, uv_old, uv_new, packed, pg)()

    def bind_mevp_iterate3(self, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        return self._bind_mevp_pass(self.lib.nsdg_mevp_iterate3, (j0, j1), s_in, s_out, uv_old, uv_new, packed, pg)

    def mevp_iterate3_pair(self, ra, rb, s_in, s_out, uv_old, uv_new, packed, pg):
        """three sub-iterations on two disjoint row ranges ra = (j0, j1), rb = (j0, j1) in one launch"""
        self._bind_mevp_pass(self.lib.nsdg_mevp_iterate3_pair, (ra[0], ra[1], rb[0], rb[1]), s_in, s_out, uv_old, uv_new, packed, pg)()

    def mevp_iterate4(self, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        """four sub-iterations in one pass on the owned rows [j0, j1) (variant 4: one pipeline stage per wave)"""
        self.bind_mevp_iterate4(j0, j1, s_in, s_out, uv_old, uv_new, packed, pg)()

    def bind_mevp_iterate4(self, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        return self._bind_mevp_pass(self.lib.nsdg_mevp_iterate4, (j0, j1), s_in, s_out, uv_old, uv_new, packed, pg)

    def mevp_iterate4_pair(self, ra, rb, s_in, s_out, uv_old, uv_new, packed, pg):
        """four sub-iterations on two disjoint row ranges ra = (j0, j1), rb = (j0, j1) in one launch"""
        self._bind_mevp_pass(self.lib.nsdg_mevp_iterate4_pair, (ra[0], ra[1], rb[0], rb[1]), s_in, s_out, uv_old, uv_new, packed, pg)()

    def mevp_subcycle(self, dt, nsub, s, u, v, u0, v0, tax, tay, uo, vo, cgh, cga, pg, scratch):
        ts = [s[0], s[1], s[2], u, v, u0, v0, tax, tay, uo, vo, cgh, cga, pg, scratch]
        _check_f64(*ts)
        need = 10 * u.numel() + 3 * s[0].numel()  # s[k] are tiled arrays: numel() == nsdg_tiled_len(nx, ny, 8)
        if scratch.numel() < need:
            raise NsdgError("mEVP scratch too small: need %d doubles" % need)
        self._call(self.lib.nsdg_mevp_subcycle(self.h, float(dt), int(nsub), *[_ptr(t) for t in ts]))

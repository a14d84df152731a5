"""The inputs of one mEVP sub-iteration that reach what the rest of the suite stays clear of, TEST INFRASTRUCTURE shared by
tests/test_mevp_regimes_cpu.py (the condition every case must hold, on the reference alone) and tests/test_gpu_mevp_regimes.py (the
device).  numpy, tests/mevp_ref.py and the island of tests/bbm_cases.py only: nothing here needs a GPU.

build(nx, ny, seed, kind, land=None) draws random fields -- H cell means in [0.35, 1.9], A in [0.72, 0.98], a stress of 1e3 Pa in all 8
coefficients, wind of +- 10 m/s, ocean of +- 0.05 m/s, nodal velocities of +- amp with u0 = 0.9 u + 0.05 amp noise -- and changes what
the kind says (hx = hy = 1000 m, dt = 120 s, alpha = 300, beta = 450 unless stated):

  plastic     amp = 0.05 m/s: Delta >> delta_min, the inputs of the older tests, but alpha != beta
  transition  amp = 1.5e-6 m/s: Delta of the order of delta_min
  viscous     amp = 2e-9 m/s: Delta = delta_min to 1e-3, zeta = P / 2 delta_min
  rest        u = v = u0 = v0 = 0 exactly and an ocean at rest on REST_PATCH (across column 63, on the bottom row): |v_o - v| == 0 exactly
  params      plastic with every physical parameter, alpha, beta and hy off its default (PARAMS) and a patch with a nodal thickness between
              the default h_min and the case's, without which h_min would not enter
  clamps      A above 1 and below 0 and H below 0 at Gauss points and nodes, nodal H under the mass floor; ice-free rule off
  icefree     five patches, one or two triggers of the ice-free rule each (PATCHES): across columns 57 and 63, on the first and last row
  ad_floor    adaptive, amp of viscous, A in [0.2, 0.4]: ice so weak that the stability bound stays under alpha_min
  ad_spread   adaptive with aevp_c = 40, alpha_min = 8, amp = 5e-4 m/s: alpha_e spread over more than a factor 2
  ad_icefree  ad_spread on the icefree fields, plus a patch of light ice (H = 0.02, not ice-free) beside strong elements
  drift       u = 0.1, v = 0.05 m/s everywhere (the array edge too) plus noise of 1e-7 m/s: rigid ice that moves.  The strain rate is a
              difference of nearly equal velocities, so this kind is compared under a bound of its own (DRIFT_BOUNDS)"""
import functools
import json
import os

import numpy as np

import mevp_ref as R
from bbm_cases import island

HX = HY = 1000.0
DT = 120.0
KINDS = ("plastic", "transition", "viscous", "rest", "params", "clamps", "icefree", "ad_floor", "ad_spread", "ad_icefree", "drift")
AB = dict(alpha=300.0, beta=450.0)
AD = dict(aevp_c=40.0, aevp_alpha_min=8.0)
PARAMS = dict(rho_ice=917.0, rho_ocean=1020.0, rho_atm=1.2, c_atm=2e-3, c_ocean=4e-3, pstar=2e4, compaction=15.0, delta_min=5e-9, fc=-1.2e-4,
              h_min=1e-3, alpha=250.0, beta=400.0)
# kind: (parameter overrides, velocity amplitude in m/s, hx, hy)
RECIPES = {
    "plastic": (AB, 0.05, HX, HY),
    "transition": (AB, 1.5e-6, HX, HY),
    "viscous": (AB, 2e-9, HX, HY),
    "rest": (AB, 0.0, HX, HY),
    "params": (PARAMS, 0.05, 1000.0, 700.0),
    "clamps": (dict(AB, min_conc=0.0, min_thick=0.0), 0.05, HX, HY),
    "icefree": (AB, 0.05, HX, HY),
    "ad_floor": (dict(aevp_c=(2.4 * np.pi) ** 2), 2e-9, HX, HY),
    "ad_spread": (AD, 5e-4, HX, HY),
    "ad_icefree": (AD, 5e-4, HX, HY),
    "drift": (AB, 1e-7, HX, HY),
}
ADAPTIVE_KINDS = tuple(k for k in KINDS if "aevp_c" in RECIPES[k][0])
UNIFORM_KINDS = tuple(k for k in KINDS if k not in ADAPTIVE_KINDS)
# (element rows, element columns).  A wave of mevp_fused_kernel owns 63 columns, a workgroup of mevp_fused4_kernel 57
REST_PATCH = (slice(0, 4), slice(58, 70))
PATCHES = {
    "free": (slice(1, 5), slice(60, 67)),  # H = A = 0: concentration and floor triggers
    "negative": (slice(5, 9), slice(5, 15)),  # H = -0.1: thickness and floor triggers, on the last row
    "thin": (slice(0, 3), slice(52, 60)),  # H = 0.004, H / A < min_thick = 0.01, above h_min: the thickness trigger alone, on the first row
    "floor": (slice(6, 9), slice(54, 66)),  # H = 5e-5 <= h_min, A = 0.003, H / A > min_thick: the floor trigger alone, on the last row
    "lowconc": (slice(0, 2), slice(20, 28)),  # A = 0 under ice of ordinary thickness: the concentration trigger alone, on the first row
}
LIGHT_PATCH = (slice(3, 6), slice(30, 40))  # ad_icefree: H = 0.02, A unchanged: H / A > min_thick, not ice-free, a fiftieth of its neighbours' mass
FLOOR_PATCH_PARAMS = (slice(3, 6), slice(61, 66))  # params: H = 5e-4, between the default h_min = 1e-4 and the case's 1e-3


def dg2(rng, lo, hi, ny, nx, wiggle):
    """a DG2 field with cell means in [lo, hi] and higher coefficients of +- wiggle"""
    f = wiggle * rng.uniform(-1.0, 1.0, (6, ny, nx))
    f[0] = rng.uniform(lo, hi, (ny, nx))
    return f


def fields(nx, ny, seed, amp, land=None):
    rng = np.random.default_rng(seed)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v, n0, n1 = rng.uniform(-1.0, 1.0, (4,) + shape)
    u, v = amp * u, amp * v
    u0, v0 = 0.9 * u + 0.05 * amp * n0, 0.9 * v + 0.05 * amp * n1
    for a in (u, v, u0, v0):
        a[0] = a[-1] = 0.0
        a[:, 0] = a[:, -1] = 0.0
    c = dict(nx=nx, ny=ny, S=[1e3 * rng.standard_normal((8, ny, nx)) for _ in range(3)], u=u, v=v, u0=u0, v0=v0, H=dg2(rng, 0.35, 1.9, ny, nx, 0.01),
             A=dg2(rng, 0.72, 0.98, ny, nx, 0.004), ua=rng.uniform(-10.0, 10.0, shape), va=rng.uniform(-10.0, 10.0, shape),
             uo=rng.uniform(-0.05, 0.05, shape), vo=rng.uniform(-0.05, 0.05, shape), land=land)
    c["rng"] = rng
    return c


def set_patch(f, patch, mean):
    f[(slice(None),) + patch] = 0.0
    f[(0,) + patch] = mean


def icefree_patches(c):
    H, A = c["H"], c["A"]
    set_patch(H, PATCHES["free"], 0.0)
    set_patch(A, PATCHES["free"], 0.0)
    H[(0,) + PATCHES["negative"]] = -0.1
    set_patch(H, PATCHES["thin"], 0.004)
    set_patch(H, PATCHES["floor"], 5e-5)
    set_patch(A, PATCHES["floor"], 0.003)
    set_patch(A, PATCHES["lowconc"], 0.0)


def build(nx, ny, seed, kind, land=None):
    """dict(c = the fields, par = parameter overrides, dt, hx, hy, kind)"""
    over, amp, hx, hy = RECIPES[kind]
    c = fields(nx, ny, seed, amp, land)
    rng = c.pop("rng")
    if kind in ("rest", "params", "icefree", "ad_icefree"):
        assert nx >= 70 and ny >= 9 and land is None
    if kind == "rest":
        c["uo"][2 * REST_PATCH[0].start:2 * REST_PATCH[0].stop + 1, 2 * REST_PATCH[1].start:2 * REST_PATCH[1].stop + 1] = 0.0
        c["vo"][2 * REST_PATCH[0].start:2 * REST_PATCH[0].stop + 1, 2 * REST_PATCH[1].start:2 * REST_PATCH[1].stop + 1] = 0.0
    elif kind == "params":
        set_patch(c["H"], FLOOR_PATCH_PARAMS, 5e-4)
    elif kind == "clamps":
        c["H"] = dg2(rng, -0.05, 0.6, ny, nx, 0.05)
        c["A"] = dg2(rng, -0.1, 1.15, ny, nx, 0.06)
    elif kind in ("icefree", "ad_icefree"):
        icefree_patches(c)
        if kind == "ad_icefree":
            set_patch(c["H"], LIGHT_PATCH, 0.02)
    elif kind == "ad_floor":
        c["A"] = dg2(rng, 0.2, 0.4, ny, nx, 0.004)
    elif kind == "drift":
        c["u"] = 0.1 + amp * rng.uniform(-1.0, 1.0, c["u"].shape)
        c["v"] = 0.05 + amp * rng.uniform(-1.0, 1.0, c["v"].shape)
        c["u0"], c["v0"] = c["u"].copy(), c["v"].copy()
    if land is not None:  # no ice, no stress, no motion on land -- and a wind that must never enter
        for f in [c["H"], c["A"]] + c["S"]:
            f[:, land] = 0.0
        ln = R.land_nodes(land)
        for k in ("u", "v", "u0", "v0"):
            c[k][ln] = 0.0
        c["ua"][ln] = c["va"][ln] = np.nan
    return dict(c=c, par=dict(over), dt=DT, hx=hx, hy=hy, kind=kind)


def params_of(case):
    return R.par(**case["par"])


def land_of(case):
    land = case["c"].get("land")
    return None if land is None else R.land_nodes(land)


def reference(case, dtype=None, k0=0, j0=0, j1=None, par=None, hx=None, hy=None):
    """one sub-iteration of tests/mevp_ref.py on the case.  dtype: every input array is cast to it first (np.longdouble: the probe of the
    case's conditioning).  par, hx, hy: in place of the case's (the one-parameter-reset probe of the params kind)"""
    c, p, diag = case["c"], par or params_of(case), {}
    if dtype is not None:
        c = dict(c, S=[np.asarray(x, dtype=dtype) for x in c["S"]], **{k: np.asarray(c[k], dtype=dtype) for k in ("u", "v", "u0", "v0", "H", "A", "ua", "va", "uo", "vo")})
    ln = land_of(case)
    prep = R.prepare(p, c["H"], c["A"], c["ua"], c["va"], c["uo"], c["vo"], diag)
    if ln is not None:  # land nodes are packed with constants: a NaN forcing there never enters
        prep["tax"], prep["tay"] = np.where(ln, 0.0, prep["tax"]), np.where(ln, 0.0, prep["tay"])
    S, u, v = R.iterate(p, hx or case["hx"], hy or case["hy"], case["dt"], c["S"], c["u"], c["v"], c["u0"], c["v0"], prep, k0, j0, j1, ln, diag)
    return dict(S=S, u=u, v=v, prep=prep, diag=diag)


# ---- the cases of the device tests: (kind, nx, ny, seed, mask) ---------------------------------------------------------------------------
# The seeds 11, 12 and 13 all keep every condition; conditioning does not tell them apart (worst float64 - longdouble distance 0.0018,
# 0.0015, 0.0022 of the bound, drift aside).  12 keeps the widest smallest margin over all 43 cases (2.6e-5 against 1.0e-5 and 1.4e-5), so
# it is the one, and no shape needs a seed of its own
SEED = 12
KIND_CASES = [(k, 70, 9, SEED, None) for k in KINDS]
ISLAND_CASES = [(k, 70, 9, SEED, "island") for k in ("plastic", "ad_spread")]
SHAPES = [(1, 1), (1, 5), (56, 3), (57, 3), (58, 3), (63, 3), (64, 3), (65, 3), (114, 2), (115, 2), (127, 3), (130, 5), (190, 2), (130, 1), (3, 70)]
SHAPE_SEEDS = {}
SHAPE_CASES = [(k, nx, ny, SHAPE_SEEDS.get((nx, ny), SEED), None) for k in ("plastic", "ad_spread") for nx, ny in SHAPES]
PIPELINE_SHAPES = [(57, 3), (58, 3), (65, 3), (115, 2), (130, 5)]
PIPELINE_CASES = KIND_CASES + [k for k in SHAPE_CASES if (k[1], k[2]) in PIPELINE_SHAPES]
ALL_CASES = KIND_CASES + ISLAND_CASES + SHAPE_CASES


def case_id(key):
    return "%s-%dx%d%s" % (key[0], key[1], key[2], "-" + key[4] if key[4] else "")


def shape_case(kind, nx, ny):
    return next(k for k in SHAPE_CASES if k[:3] == (kind, nx, ny))


@functools.lru_cache(maxsize=None)
def built(key):
    """(case, reference) of a key of ALL_CASES, computed once per process and shared: nobody changes them"""
    kind, nx, ny, seed, mask = key
    case = build(nx, ny, seed, kind, island() if mask == "island" else None)
    return case, reference(case)


@functools.lru_cache(maxsize=None)
def built_wide(key):
    """the longdouble evaluation of the case of a key: what the drift kind is compared with, rounded to float64"""
    return reference(built(key)[0], np.longdouble)


def reference_steps(case, n):
    """n successive whole-array sub-iterations of the reference: dict(S, u, v)"""
    cur = case
    for _ in range(n):
        r = reference(cur)
        cur = dict(cur, c=dict(cur["c"], S=r["S"], u=r["u"], v=r["v"]))
    return dict(S=r["S"], u=r["u"], v=r["v"])


# ---- the comparison bound: that of tests/test_gpu_parity.py::test_mevp_single_iteration_matches_oracle --------------------------------
STRESS_TOL, VELOCITY_TOL = (1e-12, 1e-12), (1e-11, 1e-13)  # (relative, share of the largest reference value of the array)
OUTPUTS = ("s11", "s12", "s22", "u", "v")


def outputs(res):
    """the five output arrays of a result dict(S, u, v) by name"""
    return dict(s11=res["S"][0], s12=res["S"][1], s22=res["S"][2], u=res["u"], v=res["v"])


def tolerance(name, want, floor_from=None):
    rel, floor = VELOCITY_TOL if name in ("u", "v") else STRESS_TOL
    return rel * np.abs(want) + floor * np.max(np.abs(want if floor_from is None else floor_from))


DRIFT_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mevp_drift_bounds.json")
DRIFT_FACTOR = 4.0  # the kernel's other order of operations and its reciprocal square roots of 1 to 2 ulp


def drift_distances(ref, wide):
    """per output array: the largest distance of the float64 reference from its longdouble evaluation rounded to float64"""
    a, b = outputs(ref), outputs(wide)
    return {k: float(np.max(np.abs(a[k] - b[k].astype(np.float64)))) for k in OUTPUTS}


def drift_bounds():
    """the absolute bound per output array of the drift kind: DRIFT_FACTOR times the distance recorded by tests/test_mevp_regimes_cpu.py"""
    rec = json.load(open(DRIFT_JSON))
    assert rec["case"] == case_id(KIND_CASES[KINDS.index("drift")]) and rec["seed"] == SEED and rec["factor"] == DRIFT_FACTOR
    return {k: DRIFT_FACTOR * rec["distance"][k] for k in OUTPUTS}


# ---- what a case reaches, from the reference's diag --------------------------------------------------------------------------------------
def sea_elements(case):
    land = case["c"].get("land")
    return np.ones((case["c"]["ny"], case["c"]["nx"]), dtype=bool) if land is None else ~land


def sea_nodes(case):
    ln = land_of(case)
    return np.ones(case["c"]["u"].shape, dtype=bool) if ln is None else ~ln


def interior(case):
    m = np.zeros(case["c"]["u"].shape, dtype=bool)
    m[1:-1, 1:-1] = True
    return m & sea_nodes(case)


def ice_free_nodes(case, ref):
    return ref["diag"]["free"] & sea_nodes(case)


def _away(x, threshold, scale):
    """the smallest |x - threshold| / scale over the entries that are not exactly ON the threshold (an exact 0 of a patch of zeros is
    the same 0 in every arithmetic); inf where there are none"""
    d = np.abs(np.asarray(x, dtype=np.float64) - threshold)
    d = d[np.isfinite(d) & (d > 0.0)]
    return float(d.min() / scale) if d.size else float("inf")


def margins(case, ref):
    """the relative distance of every threshold decision of the sub-iteration from its threshold, smallest over the array"""
    p, d, sea, nodes = params_of(case), ref["diag"], sea_elements(case), sea_nodes(case)
    h, a = d["h_gauss"][:, sea], d["a_gauss"][:, sea]
    m = dict(h_gauss_0=_away(h, 0.0, max(1.0, float(np.max(np.abs(h))))), a_gauss_0=_away(a, 0.0, 1.0), a_gauss_1=_away(a, 1.0, 1.0),
             a_node_0=_away(d["a_node"][nodes], 0.0, 1.0), a_node_1=_away(d["a_node"][nodes], 1.0, 1.0),
             h_node_floor=_away(d["h_node"][nodes], p["h_min"], p["h_min"]))
    if p["min_conc"] > 0.0 or p["min_thick"] > 0.0:
        m.update(trig_conc=_away(d["trig_conc"][nodes], p["min_conc"], p["min_conc"]), trig_thick=_away(d["trig_thick"][nodes], p["min_thick"], p["min_thick"]),
                 trig_floor=_away(d["trig_floor"][nodes], p["h_min"], p["h_min"]))
    if R.adaptive(p):
        live = sea & ~d["free_centre"]
        m["alpha_min"] = _away(d["alpha_bound"][live] / p["aevp_alpha_min"], 1.0, 1.0)
        pick = nodes & ~d["free"] & ~d["fixed"]
        best = np.maximum(d["offer"], d["offer_floor"])[pick]
        other = np.where(d["offer"] > d["offer_floor"], np.maximum(d["offer_second"], d["offer_floor"]), d["offer"])[pick]
        m["beta_offer"] = _away(other / best, 1.0, 1.0)
    return m


MARGIN = 1e-6


def assert_margins(case, ref, what=""):
    m = margins(case, ref)
    print("%s margins: %s" % (what, ", ".join("%s %.3g" % kv for kv in m.items())))
    assert min(m.values()) >= MARGIN, (what, m)
    return m


def triggers(case, ref):
    """(conc, thick, floor): bool arrays of the nodes where each trigger of the ice-free rule holds"""
    p, d = params_of(case), ref["diag"]
    with np.errstate(invalid="ignore"):
        return d["trig_conc"] < p["min_conc"], d["trig_thick"] < p["min_thick"], d["trig_floor"] <= p["h_min"]


def adjacent_max(alpha_e, shape):
    """per node the largest alpha_e of the elements it belongs to"""
    ny, nx = alpha_e.shape
    out = np.zeros(shape)
    for b in range(9):
        by, bx = divmod(b, 3)
        blk = out[by:by + 2 * ny:2, bx:bx + 2 * nx:2]
        blk[...] = np.maximum(blk, alpha_e)
    return out


def seam_sides(mask, col):
    """does a bool array over the nodes hold entries on both sides of the element seam after element column col"""
    return bool(mask[:, 2 * col - 1:2 * col + 2].any() and mask[:, 2 * col + 3:2 * col + 6].any())


def shares(case, ref):
    """the shares the table of conditions is stated on, from the reference alone"""
    p, d, c = params_of(case), ref["diag"], case["c"]
    sea = np.broadcast_to(sea_elements(case), d["delta"].shape)
    r = (d["delta"] / p["delta_min"])[sea]
    inner = interior(case)
    mean = lambda x: float(np.mean(x))
    s = dict(plastic=mean(r >= 100.0), transition=mean((r >= 1.1) & (r <= 10.0)), viscous=mean(r <= 1.001), ratio_max=float(r.max()),
             rest=mean(d["speed"][inner[slice(*d["node_rows"])]] == 0.0), ice_free=mean(ice_free_nodes(case, ref)[inner]))
    h, a = d["h_gauss"][:, sea_elements(case)], d["a_gauss"][:, sea_elements(case)]
    s.update(h_gauss_below_0=mean(h < 0.0), a_gauss_below_0=mean(a < 0.0), a_gauss_above_1=mean(a > 1.0), a_node_below_0=mean(d["a_node"][inner] < 0.0),
             a_node_above_1=mean(d["a_node"][inner] > 1.0), h_node_under_floor=mean(d["h_node"][inner] < p["h_min"]))
    if R.adaptive(p):
        e = sea_elements(case)
        s.update(alpha_spread=float(d["alpha_e"][e].max() / d["alpha_e"][e].min()), alpha_above_min=mean(d["alpha_e"][e] > p["aevp_alpha_min"]),
                 beta_from_offer=mean(d["beta_from_offer"][inner]))
    return s


def check_condition(case, ref):
    """asserts the condition of the kind's row in the table of tests/test_mevp_regimes_cpu.py; returns the shares"""
    kind, p, d, s = case["kind"], params_of(case), ref["diag"], shares(case, ref)
    inner = interior(case)
    if kind in ("plastic", "params"):
        assert s["plastic"] >= 0.9, s
    if kind == "plastic":
        assert p["alpha"] != p["beta"]
    elif kind == "transition":
        assert s["transition"] >= 0.5, s
    elif kind == "viscous":
        assert s["viscous"] == 1.0, s
    elif kind == "rest":
        c = case["c"]
        assert not any(c[k].any() for k in ("u", "v", "u0", "v0")) and all(x.any() for x in c["S"])
        assert 0.05 <= s["rest"] < 0.5 and s["viscous"] == 1.0, s
    elif kind == "params":
        base = R.par()
        assert all(p[k] != base[k] for k in PARAMS) and case["hx"] != case["hy"]
    elif kind == "clamps":
        assert p["min_conc"] == 0.0 and p["min_thick"] == 0.0 and s["ice_free"] == 0.0
        for k in ("h_gauss_below_0", "a_gauss_below_0", "a_gauss_above_1", "a_node_below_0", "a_node_above_1", "h_node_under_floor"):
            assert s[k] > 0.0, (k, s)
    elif kind in ("icefree", "ad_icefree"):
        conc, thick, floor = triggers(case, ref)
        alone = dict(conc=conc & ~thick & ~floor, thick=thick & ~conc & ~floor, floor=floor & ~conc & ~thick)
        for k, m in alone.items():
            s["alone_" + k] = int(np.sum(m & inner))
            assert s["alone_" + k] >= 1, k
        free = d["free"] & inner
        assert np.array_equal(d["free"], conc | thick | floor)
        for col in (57, 63):
            assert seam_sides(free, col), col
        assert free[1].any() and free[-2].any()  # the first and the last node row that moves
        if kind == "ad_icefree":
            amin = p["aevp_alpha_min"]
            assert d["free_centre"].any() and np.all(d["alpha_e"][d["free_centre"]] == amin)
            assert np.all(d["beta_n"][d["free"]] == amin)
            light = ~d["free"] & inner & (d["beta_n"] > 5.0 * amin) & (d["beta_n"] > 1.5 * adjacent_max(d["alpha_e"], d["free"].shape))
            s["light_beside_strong"] = int(np.sum(light))
            assert s["light_beside_strong"] >= 1
    elif kind == "ad_floor":
        assert np.all(d["alpha_e"] == p["aevp_alpha_min"]) and s["alpha_spread"] == 1.0
    elif kind == "ad_spread":
        assert s["alpha_spread"] > 2.0 and s["alpha_above_min"] >= 0.3 and s["beta_from_offer"] >= 0.1, s
    elif kind == "drift":
        assert s["ratio_max"] <= 3.0 and np.min(np.abs(case["c"]["u"])) > 0.09, s
    return s

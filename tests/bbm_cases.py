"""The inputs of one brittle Bingham-Maxwell sub-iteration, TEST INFRASTRUCTURE shared by tests/test_bbm_cpu.py (the conditions a case
must hold, on the reference alone) and the device tests (tests/test_gpu_bbm.py, tests/test_gpu_bbm_branches.py).  numpy and
tests/bbm_ref.py only: nothing here needs a GPU.

random_case is the input of tests/test_gpu_bbm.py: it stays clear of the compressive branch, of r = 1, of damage outside [0, d_max] and of
ice-free nodes.  build(nx, ny, seed, kind) makes the inputs that reach them, one kind per set of parameters:

  branches   damage cell means in [-0.2, 1.2], a tenth of the cells at 1e-5 (below dt_s / t_heal = 4e-5: healing ends at exactly 0);
             compr_strength = 1.5e4 Pa inside the range of |sigma_n| (compressive failure); dt_s = 4 s (r = min(1, .) reaches 1)
  dmax       branches with t_heal = 1e30 and dt_s = 1 s: damage clamped to d_max stays there and the output clamp min(d_max, .) acts
  exponent1  branches with relax_exponent = 1 (no trip of the lambda loop), lambda0 = 50 s, hx = 1000 m, hy = 700 m
  exponent2  branches with relax_exponent = 2 (one trip), lambda0 = 1e3 s, hx = 600 m, hy = 1000 m
  params     branches with rho_ice = 917, fc = -1.2e-4, c_ocean = 4e-3, compaction = 15
  icefree    random_case with a patch of H = A = 0, a patch of negative thickness and a patch of thin ice (H / A < min_thick): ice-free
             nodes and Gauss points with hg = 0.  Its floor-mass nodes are the fastest of the array (1.4 m/s against 0.36 m/s where there
             is ice), so it is a kind of its own and its nodes with ice are compared once more under the floor of their own maximum."""
import functools

import numpy as np

import bbm_ref as R

HX = HY = 1000.0
DTS = 1.0
KINDS = ("branches", "dmax", "exponent1", "exponent2", "params", "icefree")
BRANCHES = dict(compr_strength=1.5e4)
# kind: (BBM parameter overrides, mEVP parameter overrides, dt_s, hx, hy)
RECIPES = {
    "branches": (BRANCHES, {}, 4.0, HX, HY),
    "dmax": (dict(BRANCHES, t_heal=1e30), {}, 1.0, HX, HY),
    "exponent1": (dict(BRANCHES, relax_exponent=1, lambda0=50.0), {}, 4.0, 1000.0, 700.0),
    "exponent2": (dict(BRANCHES, relax_exponent=2, lambda0=1e3), {}, 4.0, 600.0, 1000.0),
    "params": (BRANCHES, dict(rho_ice=917.0, fc=-1.2e-4, c_ocean=4e-3, compaction=15.0), 4.0, HX, HY),
    "icefree": ({}, {}, DTS, HX, HY),
}
TINY_DAMAGE = 1e-5  # < dt_s / t_heal = 4e-5 of the branches recipe


def dg2(rng, lo, hi, ny, nx, wiggle):
    """a DG2 field with cell means in [lo, hi] and small higher coefficients"""
    f = wiggle * rng.uniform(-1.0, 1.0, (6, ny, nx))
    f[0] = rng.uniform(lo, hi, (ny, nx))
    return f


def random_case(nx, ny, seed=11, land=None):
    """the inputs of one sub-iteration: |sigma_n| in [1.5e3, 3e4] Pa with both signs (+- 350 Pa from the higher coefficients), the
    deviatoric part +- 2e4 Pa, nodal velocities of +- 5e-5 m/s on 500 m node spacing, H in [0.3, 2], A in [0.7, 1], D in [0, 0.9]"""
    rng = np.random.default_rng(seed)
    sn = rng.uniform(1.5e3, 3.0e4, (ny, nx)) * rng.choice([-1.0, 1.0], (ny, nx))
    d1, d2 = rng.uniform(-2e4, 2e4, (2, ny, nx))
    S = [50.0 * rng.uniform(-1.0, 1.0, (8, ny, nx)) for _ in range(3)]
    S[0][0], S[1][0], S[2][0] = sn + d1, d2, sn - d1
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = 5e-5 * rng.uniform(-1.0, 1.0, (2,) + shape)
    for a in (u, v):
        a[0] = a[-1] = 0.0
        a[:, 0] = a[:, -1] = 0.0
    c = dict(nx=nx, ny=ny, S=S, u=u, v=v, H=dg2(rng, 0.35, 1.9, ny, nx, 0.01), A=dg2(rng, 0.72, 0.98, ny, nx, 0.004), D=dg2(rng, 0.05, 0.85, ny, nx, 0.01),
             ua=rng.uniform(-10.0, 10.0, shape), va=rng.uniform(-10.0, 10.0, shape), uo=rng.uniform(-0.05, 0.05, shape),
             vo=rng.uniform(-0.05, 0.05, shape), land=land)
    if land is not None:  # no ice, no stress, no motion on land -- and a wind that must never enter
        for f in [c["H"], c["A"], c["D"]] + S:
            f[:, land] = 0.0
        ln = R.land_nodes(land)
        u[ln] = v[ln] = 0.0
        c["ua"][ln] = c["va"][ln] = np.nan
    return c


def island():
    """the mask of tests/test_gpu_bbm.py::test_land_stays_at_zero_and_the_ocean_finite: an island across the wave seam, and a rock"""
    land = np.zeros((9, 70), dtype=bool)
    land[2:6, 60:67] = True
    land[7, 3] = True
    return land


def branch_damage(nx, ny, seed, land=None):
    """damage of the branches recipe: cell means uniform in [-0.2, 1.2] (a seventh below 0, a seventh above d_max), higher coefficients
    of +- 0.01; a tenth of the cells hold the constant 1e-5"""
    rng = np.random.default_rng([seed, 7])  # a stream of its own: random_case keeps its draws
    D = dg2(rng, -0.2, 1.2, ny, nx, 0.01)
    tiny = rng.random((ny, nx)) < 0.1
    D[:, tiny] = 0.0
    D[0, tiny] = TINY_DAMAGE
    if land is not None:
        D[:, land] = 0.0
    return D


# the patches of the icefree kind, (element rows, element columns): across the wave seam at column 63, on the top and on the bottom row
FREE_PATCH, NEGATIVE_PATCH, THIN_PATCH = (slice(1, 5), slice(56, 68)), (slice(5, 9), slice(5, 15)), (slice(0, 3), slice(30, 40))


def recipe(kind, c=None):
    """dict(c = the fields, bbm, mevp = parameter overrides, dts, hx, hy, kind)"""
    bbm, mevp, dts, hx, hy = RECIPES[kind]
    return dict(c=c, bbm=dict(bbm), mevp=dict(mevp), dts=dts, hx=hx, hy=hy, kind=kind)


def build(nx, ny, seed, kind, land=None):
    """the case (nx, ny, seed, kind): recipe(kind) around the fields, which have the form random_case returns"""
    c = random_case(nx, ny, seed, land)
    if kind == "icefree":
        assert nx >= 68 and ny >= 9 and land is None
        H, A = c["H"], c["A"]
        H[(slice(None),) + FREE_PATCH] = 0.0
        A[(slice(None),) + FREE_PATCH] = 0.0
        H[(0,) + NEGATIVE_PATCH] = -0.1
        H[(slice(None),) + THIN_PATCH] = 0.0
        H[(0,) + THIN_PATCH] = 0.004  # H / A ~ 0.005 < min_thick = 0.01, above h_min = 1e-4: the thin-ice rule alone decides
    else:
        c["D"] = branch_damage(nx, ny, seed, land)
    return recipe(kind, c)


def reference(c, bp=None, dts=DTS, hx=HX, hy=HY, mpar=None, dtype=None):
    """one sub-iteration of tests/bbm_ref.py on the fields c.  dtype: every input array is cast to it first (np.longdouble: the probe of
    the case's conditioning -- bbm_ref runs unchanged in that type)"""
    mpar, bp, diag = mpar or R.mevp_par(), bp or R.bbm_par(), {}
    if dtype is not None:
        cast = lambda a: np.asarray(a, dtype=dtype)
        c = dict(c, S=[cast(x) for x in c["S"]], **{k: cast(c[k]) for k in ("u", "v", "H", "A", "D", "ua", "va", "uo", "vo")})
    gauss = R.prepare(mpar, bp, c["H"], c["A"])
    nod = R.nodal_fields(mpar, c["H"], c["A"], c["ua"], c["va"], c["uo"], c["vo"])
    ln = R.land_nodes(c["land"]) if c.get("land") is not None else None
    So, Do, un, vn = R.iterate(mpar, bp, hx, hy, dts, c["S"], c["D"], c["u"], c["v"], gauss, nod, land=ln, diag=diag)
    return dict(S=So, D=Do, u=un, v=vn, gauss=gauss, diag=diag, nod=nod)


def case_reference(case, dtype=None):
    return reference(case["c"], R.bbm_par(**case["bbm"]), case["dts"], case["hx"], case["hy"], R.mevp_par(**case["mevp"]), dtype)


# ---- the cases of tests/test_gpu_bbm_branches.py: (kind, nx, ny, seed, mask) ------------------------------------------------------------
SEED = 12  # of 11, 12, 13 the one whose float64 reference lies closest to its longdouble evaluation in every case (worst 0.11 of the tolerance)
KIND_CASES = [(k, 70, 9, SEED, None) for k in KINDS]
ISLAND_CASE = ("branches", 70, 9, SEED, "island")  # the all-ocean mask runs KIND_CASES[0] itself
SHAPES = [(1, 1), (1, 5), (63, 3), (64, 3), (65, 3), (127, 3), (130, 5), (190, 2), (130, 1), (3, 70)]
# 1 x 1 has nine Gauss points and seed 12 damages its element so far that the stress relaxes to 0.03 Pa; with seed 5 it carries
# 1.8e4 Pa and all nine points fail in compression
SHAPE_SEEDS = {(1, 1): 5}
SHAPE_CASES = [("branches", nx, ny, SHAPE_SEEDS.get((nx, ny), SEED), None) for nx, ny in SHAPES]
ALL_CASES = KIND_CASES + [ISLAND_CASE] + SHAPE_CASES


def case_id(key):
    return "%s-%dx%d%s" % (key[0], key[1], key[2], "-" + key[4] if key[4] else "")


@functools.lru_cache(maxsize=None)
def built(key):
    """(case, reference) of a key of ALL_CASES, computed once per process and shared: nobody changes them"""
    kind, nx, ny, seed, mask = key
    case = build(nx, ny, seed, kind, island() if mask == "island" else None)
    return case, case_reference(case)


# ---- what a case reaches, from the reference's diag -------------------------------------------------------------------------------------
def ocean_points(case):
    """the Gauss points [9, ny, nx] the margins are stated on: all of them, but for land elements (stress exactly 0 on both sides)"""
    land = case["c"].get("land")
    shape = (9, case["c"]["ny"], case["c"]["nx"])
    return np.ones(shape, dtype=bool) if land is None else np.broadcast_to(~land, shape)


def margins(case, ref):
    """(min |sigma_n old| in Pa, min |sigma_n new + N| / N): the distances from the scheme's two discontinuities"""
    N, sea, d = R.bbm_par(**case["bbm"])["compr_strength"], ocean_points(case), ref["diag"]
    return float(np.min(np.abs(d["sn_old"][sea]))), float(np.min(np.abs(d["sn_new"][sea] + N))) / N


def assert_margins(case, ref, what=""):
    sn_old, sn_new = margins(case, ref)
    print("%s min |sn_old| %.4g Pa, min |sn_new + N| / N %.3g" % (what, sn_old, sn_new))
    assert sn_old >= 1e3 and sn_new >= 1e-6, what


def shares(case, ref):
    """the share of the Gauss points (of the nodes, for ice_free) in each branch of steps 1-7, from the reference alone"""
    bp, mp, c, d = R.bbm_par(**case["bbm"]), R.mevp_par(**case["mevp"]), case["c"], ref["diag"]
    N, d_in = bp["compr_strength"], R.apply(R.PSI_Q[:, :6], c["D"])
    compressive = d["sn_new"] < -N
    with np.errstate(divide="ignore", invalid="ignore"):
        pt_clamped = (d["sn_old"] < 0.0) & (-ref["gauss"][2] / d["sn_old"] >= 1.0)
    m = lambda x: float(np.mean(x))
    return dict(compressive=m(compressive), envelope=m(~compressive & d["failing"]), intact=m(d["d_c"] == 1.0), r_is_1=m(d["r"] == 1.0),
                d_below_0=m(d_in < 0.0), d_above_dmax=m(d_in > bp["d_max"]), healed_to_0=m((d_in > 0.0) & (d["d_healed"] == 0.0)),
                out_at_dmax=m(d["d"] == bp["d_max"]), pt_clamped=m(pt_clamped), pt_zero=m(d["sn_old"] >= 0.0),
                ice_free=m(ice_free_nodes(case, ref)), hg_zero=m(ref["gauss"][0] == 0.0))


def ice_free_nodes(case, ref):
    """the nodes the ice-free rule (not a land mask) sets drifting freely"""
    free = R.ice_free(R.mevp_par(**case["mevp"]), ref["nod"]["cgh"], ref["nod"]["cga"])
    land = case["c"].get("land")
    return free if land is None else free & ~R.land_nodes(land)


def tolerance(want, floor_from=None):
    """the limit of tests/test_gpu_bbm.py::check_against_reference, restated for the conditioning probe: 1e-11 relative plus 1e-13 of the
    largest reference value (of floor_from, where the floor comes from a subset)"""
    return 1e-11 * np.abs(want) + 1e-13 * np.max(np.abs(want if floor_from is None else floor_from))


# ---- slabs of whole rows: the reference of an array too large for numpy -----------------------------------------------------------------
def slab(c, r0, r1):
    """the element rows [r0, r1) of the fields c as a local array of its own"""
    n0, n1 = 2 * r0, 2 * r1 + 1
    out = dict(nx=c["nx"], ny=r1 - r0, S=[x[:, r0:r1] for x in c["S"]], land=None)
    out.update({k: c[k][:, r0:r1] for k in ("H", "A", "D")})
    out.update({k: c[k][n0:n1] for k in ("u", "v", "ua", "va", "uo", "vo")})
    return out


def slab_interior(r0, r1, ny):
    """(e0, e1, n0, n1): the local element rows [e0, e1) and node rows [n0, n1) of the slab [r0, r1) of an array of ny rows that a slab
    evaluation gets right: one margin element row is dropped on every side that is not the physical boundary, and with it the node rows
    that only it touches and the slab's own edge row (the slab evaluation holds that one at 0 and averages H and A over one side only)"""
    lo, hi = int(r0 > 0), int(r1 < ny)
    rows = r1 - r0
    return lo, rows - hi, 2 * lo, 2 * (rows - hi) + 1

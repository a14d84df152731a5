"""The maps of tests/symmetry_maps.py and the cases of tests/symmetry_cases.py, checked without a GPU: the maps are involutions, Y equals
T o X o T bit for bit, and the CPU references (the oracle, land_ref, bbm_ref, history_ref) are equivariant under T, X and Y at round-off
on every case the device test runs.  The device test (tests/test_gpu_symmetry.py) then compares device with mapped device; what it
needs of its inputs -- decision masks that map exactly, thresholds kept at a distance, alpha_e that spread -- is asserted here.

Bound: 1e-13 max|array| for single applications, 1e-12 max|array| for 25 sub-iterations and three transport steps.  Sensitivity: a map
that is wrong in one ingredient (fc sign, coefficient permutation, s12 sign) misses by more than 1e-6."""
import functools

import numpy as np
import pytest

import bbm_ref as R
import history_ref
import land_ref
import oracle_lib as O
import symmetry_cases as SC
import symmetry_maps as SM

MAPS = [SM.T, SM.X, SM.Y]
ONCE, MANY = 1e-13, 1e-12
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\noracle equivariance, %s: largest mismatch %.3g of max|array|" % (k, WORST[k]))


def mismatch(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(float(np.max(np.abs(a))), float(np.max(np.abs(b))))
    return float(np.max(np.abs(a - b))) / scale if scale > 0 else 0.0


def check(what, pairs, bound):
    worst = max(mismatch(a, b) for a, b in pairs)
    WORST[what] = max(WORST.get(what, 0.0), worst)
    assert worst <= bound, "%s: mismatch %.3g of max|array|, bound %.3g" % (what, worst, bound)
    return worst


# ------------------------------------------------------------------------------------------------ the maps themselves
def _arrays(rng, nx=7, ny=5):
    return dict(node=rng.standard_normal((2 * ny + 1, 2 * nx + 1)), elem=rng.standard_normal((ny, nx)), gauss=rng.standard_normal((9, ny, nx)),
                dg8=rng.standard_normal((8, ny, nx)), dg6=rng.standard_normal((6, ny, nx)), dg3=rng.standard_normal((3, ny, nx)),
                dg1=rng.standard_normal((1, ny, nx)), unx=rng.standard_normal((3, ny, nx + 1)), uny=rng.standard_normal((3, ny + 1, nx)))


def _apply_all(M, a):
    """every array kind through M: a flat list of arrays"""
    out = [M.node(a["node"]), M.elem(a["elem"]), M.elem(a["elem"] > 0), M.gauss(a["gauss"])]
    out += [M.dg(a[k]) for k in ("dg8", "dg6", "dg3", "dg1")]
    out += list(M.vec(a["node"], 2.0 * a["node"])) + list(M.dgvec(a["dg6"], 3.0 * a["dg6"])) + list(M.stress(a["dg8"], 2.0 * a["dg8"], 3.0 * a["dg8"]))
    out += list(M.edges(a["unx"], a["uny"]))
    return out


def _twice(M, N, a):
    """N o M on every array kind"""
    n, e, g = N.node(M.node(a["node"])), N.elem(M.elem(a["elem"])), N.gauss(M.gauss(a["gauss"]))
    out = [n, e, N.elem(M.elem(a["elem"] > 0)), g] + [N.dg(M.dg(a[k])) for k in ("dg8", "dg6", "dg3", "dg1")]
    out += list(N.vec(*M.vec(a["node"], 2.0 * a["node"]))) + list(N.dgvec(*M.dgvec(a["dg6"], 3.0 * a["dg6"])))
    out += list(N.stress(*M.stress(a["dg8"], 2.0 * a["dg8"], 3.0 * a["dg8"]))) + list(N.edges(*M.edges(a["unx"], a["uny"])))
    return out


IDENTITY = type("I", (), {k: staticmethod(lambda *a: a[0] if len(a) == 1 else a) for k in ("node", "elem", "gauss", "dg", "vec", "dgvec", "stress", "edges")})


@pytest.mark.parametrize("M", MAPS, ids=repr)
def test_every_map_is_an_involution(M):
    a = _arrays(np.random.default_rng(1))
    for got, want in zip(_twice(M, M, a), _apply_all(IDENTITY, a)):
        assert got.shape == want.shape and np.array_equal(got, want)
    assert M.params(M.params(dict(fc=1e-4, hx=3.0, hy=5.0, alpha=7.0))) == dict(fc=1e-4, hx=3.0, hy=5.0, alpha=7.0)
    assert M.grid(*M.grid(7, 5, 3.0, 4.0)) == (7, 5, 3.0, 4.0)


def test_y_equals_t_x_t_bit_for_bit():
    a = _arrays(np.random.default_rng(2))
    tx = _twice(SM.T, SM.X, a)  # X o T of every kind, as a flat list in the order of _apply_all: map it once more by T, kind by kind
    keys = ["node", "elem", "mask", "gauss", "dg8", "dg6", "dg3", "dg1"]
    b = dict(zip(keys, tx[:8]))
    txt = [SM.T.node(b["node"]), SM.T.elem(b["elem"]), SM.T.elem(b["mask"]), SM.T.gauss(b["gauss"])] + [SM.T.dg(b[k]) for k in keys[4:]]
    txt += list(SM.T.vec(*tx[8:10])) + list(SM.T.dgvec(*tx[10:12])) + list(SM.T.stress(*tx[12:15])) + list(SM.T.edges(*tx[15:17]))
    want = _apply_all(SM.Y, a)
    assert len(txt) == len(want) == 17
    for got, w in zip(txt, want):
        assert got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w)
    p = dict(fc=1e-4, hx=3.0, hy=5.0)
    assert SM.T.params(SM.X.params(SM.T.params(p))) == SM.Y.params(p)


def test_the_land_mask_has_no_symmetry_and_all_its_parts():
    for nx, ny in SC.MEVP_GRIDS + ((64, 48),):
        m = SC.land_mask(nx, ny)
        assert m.any() and not m.all()
        assert m[:, 0].any() and m[0, :].any() and m[-1, :].any() and not m[:, -1].any()  # two adjacent sides, and the channel's block on a third
        for img in (m[:, ::-1], m[::-1], m[::-1, ::-1]):
            assert not np.array_equal(img, m)
        if nx == ny:
            assert not np.array_equal(m.T, m)
        top = m[-1]
        assert np.any(~top[1:-1] & top[:-2] & top[2:])  # the one-element channel


# ------------------------------------------------------------------------------------------------ helpers of the oracle
def derived(c):
    """what the oracle's helpers make of a case: (params, pg, cgh, cga, tax, tay)"""
    p = O.mevp_params(**c["params"])
    nx, ny = c["nx"], c["ny"]
    tax, tay = O.wind_stress(p, np.ascontiguousarray(c["ua"]), np.ascontiguousarray(c["va"]))
    return p, O.ice_strength(nx, ny, p, c["H"], c["A"]), O.dg_to_cg(nx, ny, c["H"]), O.dg_to_cg(nx, ny, c["A"]), tax, tay


def free_nodes(p, cgh, cga):
    """the ice-free-node rule's decision and the smallest relative distance of any node from its three thresholds"""
    free = (cga < p.min_conc) | (cgh < p.min_thick * cga) | (cgh <= p.h_min)
    with np.errstate(invalid="ignore"):  # (0 / 0 on land, where nobody asks for the margin)
        margin = min(float(np.min(np.abs(cga - p.min_conc))) / p.min_conc, float(np.min(np.abs(cgh - p.h_min))) / p.h_min,
                     float(np.min(np.abs(cgh - p.min_thick * cga) / np.maximum(cgh, p.min_thick * cga))))
    return free, margin


@pytest.mark.parametrize("M", MAPS, ids=repr)
@pytest.mark.parametrize("nx,ny", SC.MEVP_GRIDS)
def test_oracle_helpers_are_equivariant(nx, ny, M):
    c = SC.mevp_case(nx, ny, "uniform")
    ci = SC.image(c, M)
    p, pg, cgh, cga, tax, tay = derived(c)
    pi, pgi, cghi, cgai, taxi, tayi = derived(ci)
    check("dg_to_cg", [(M.node(cgh), cghi), (M.node(cga), cgai)], ONCE)
    check("ice_strength", [(M.gauss(pg), pgi)], ONCE)
    check("wind_stress", zip(M.vec(tax, tay), (taxi, tayi)), ONCE)
    if ny >= 5:  # a row range: the same rows under X, the mirrored rows under Y, every row of the image under T (its rows are columns here)
        j0, j1 = 1, ny - 2
        part = O.ice_strength(nx, ny, p, c["H"], c["A"], j0, j1)
        r = {"T": (0, ci["ny"]), "X": (j0, j1), "Y": (ny - j1, ny - j0)}[M.kind]
        back = M.gauss(O.ice_strength(ci["nx"], ci["ny"], pi, ci["H"], ci["A"], *r))
        check("ice_strength on a row range", [(back[:, j0:j1], part[:, j0:j1])], ONCE)
        assert np.all(part[:, :j0] == 0) and np.all(part[:, j1:] == 0)
    free, margin = free_nodes(p, cgh, cga)
    freei, margini = free_nodes(pi, cghi, cgai)
    assert free.any() and np.array_equal(M.node(free), freei) and min(margin, margini) >= 1e-6, (margin, margini)


@pytest.mark.parametrize("M", MAPS, ids=repr)
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("nx,ny", SC.TRANSPORT_GRIDS)
def test_oracle_prepare_advection_is_equivariant(nx, ny, order, M):
    c = SC.transport_case(nx, ny, order)
    ci = SC.image(c, M)
    vx, vy, unx, uny = O.prepare_advection(nx, ny, order, c["u"], c["v"])
    got = O.prepare_advection(ci["nx"], ci["ny"], order, ci["u"], ci["v"])
    check("prepare_advection", zip(M.dgvec(vx, vy) + M.edges(unx, uny), got), ONCE)


@pytest.mark.parametrize("order", [1, 2])
def test_the_oracle_decides_the_gauss_index_of_the_edge_velocities_under_x(order):
    """un_x lives on vertical edges with its Gauss points along y, which X leaves alone: it is reversed in ix and negated, its Gauss
    index stays; un_y (Gauss points along x) is reversed in ix and in its Gauss index.  The other candidate -- un_x reversed in its
    Gauss index as well -- is not what the oracle computes"""
    c = SC.transport_case(13, 9, order)
    ci = SC.image(c, SM.X)
    _, _, unx, uny = O.prepare_advection(13, 9, order, c["u"], c["v"])
    _, _, unxi, unyi = O.prepare_advection(13, 9, order, ci["u"], ci["v"])
    assert mismatch(SM.X.edges(unx, uny)[0], unxi) <= ONCE and mismatch(SM.X.edges(unx, uny)[1], unyi) <= ONCE
    assert mismatch(np.ascontiguousarray(-unx[::-1, :, ::-1]), unxi) > 1e-6 and mismatch(np.ascontiguousarray(uny[:, :, ::-1]), unyi) > 1e-6


# ------------------------------------------------------------------------------------------------ mEVP sub-iterations
@functools.lru_cache(maxsize=None)
def mevp_run(nx, ny, form, land, nsub, kind=None, **wrong):
    """nsub sub-iterations of the oracle (land_ref.subcycle with a mask) on the case, or on its image under the map `kind` (built with
    the keyword arguments `wrong`: a deliberately wrong map): (M, u, v, s, alpha_e of the input state, free nodes)"""
    c = SC.mevp_case(nx, ny, form, land)
    M = SM.Map(kind, **wrong) if kind else None
    if M:
        c = SC.image(c, M)
    p, pg, cgh, cga, tax, tay = derived(c)
    u, v, s = c["u"].copy(), c["v"].copy(), [x.copy() for x in c["s"]]
    al = np.zeros((c["ny"], c["nx"]))
    if form == "adaptive":
        O.mevp_stress(c["nx"], c["ny"], 0, c["ny"], c["hx"], c["hy"], p, u, v, pg, *[x.copy() for x in s], dt=c["dt"], cgh=cgh, cga=cga, alpha_e=al)
    args = (c["u0"], c["v0"], tax, tay, np.ascontiguousarray(c["uo"]), np.ascontiguousarray(c["vo"]), cgh, cga, pg)
    if land:
        land_ref.subcycle(c["nx"], c["ny"], c["hx"], c["hy"], c["dt"], nsub, p, c["land"], s, u, v, *args)
    else:
        O.mevp_subcycle(c["nx"], c["ny"], c["hx"], c["hy"], c["dt"], nsub, p, s, u, v, *args)
    return M, u, v, s, al, free_nodes(p, cgh, cga)[0]


def mevp_pairs(M, a, b):
    """(mapped original, image) pairs of u, v and the stress triple"""
    return list(zip(M.vec(a[1], a[2]) + M.stress(*a[3]), (b[1], b[2]) + tuple(b[3])))


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("nsub", [1, 25])
@pytest.mark.parametrize("land", [False, True], ids=["ocean", "land"])
@pytest.mark.parametrize("form", ["uniform", "adaptive"])
@pytest.mark.parametrize("nx,ny", SC.MEVP_GRIDS)
def test_oracle_mevp_is_equivariant(nx, ny, form, land, nsub, kind):
    a, b = mevp_run(nx, ny, form, land, nsub), mevp_run(nx, ny, form, land, nsub, kind)
    M = b[0]
    assert np.max(np.abs(a[1])) > 0 and np.all(np.isfinite(a[1]))
    check("mEVP, %d sub-iteration(s), %s" % (nsub, form), mevp_pairs(M, a, b), ONCE if nsub == 1 else MANY)
    assert np.array_equal(M.node(a[5]), b[5]) and a[5].any()
    if form == "adaptive":
        check("alpha_e", [(M.elem(a[4]), b[4])], ONCE)
        assert float(a[4].max()) > 2 * float(a[4].min()), (a[4].min(), a[4].max())  # the alphas spread: not the uniform form in disguise


@pytest.mark.parametrize("kind,wrong", [("T", "fc_sign"), ("X", "fc_sign"), ("T", "permute8"), ("X", "s12_sign")])
def test_a_map_wrong_in_one_ingredient_is_exposed(kind, wrong):
    """the same comparison with a map that lacks the fc sign, the 8-coefficient permutation or the s12 sign: far outside round-off"""
    for form in ("uniform", "adaptive"):
        a, b = mevp_run(58, 13, form, False, 1), mevp_run(58, 13, form, False, 1, kind, **{wrong: False})
        worst = max(mismatch(x, y) for x, y in mevp_pairs(b[0], a, b))
        print("%s without %s, %s: mismatch %.3g" % (kind, wrong, form, worst))
        assert worst > 1e-6


# ------------------------------------------------------------------------------------------------ transport
@functools.lru_cache(maxsize=None)
def transport_run(nx, ny, order, kind=None):
    """three steps of the oracle's transport with cap and limiter after each: (fields, [per step, per field (capped, limited)], margin)"""
    c = SC.transport_case(nx, ny, order, nfields=4)
    if kind:
        c = SC.image(c, SM.MAPS[kind])
    adv = O.prepare_advection(c["nx"], c["ny"], order, c["u"], c["v"])
    fields = [f.copy() for f in c["fields"]]
    masks, margin = [], np.inf
    for _ in range(3):
        for f, (lo, hi, cap) in zip(fields, c["bounds"]):
            O.transport_step(c["nx"], c["ny"], c["hx"], c["hy"], order, c["dt"], f, adv)
            capped, limited, m = SC.closure_decisions(f, order, lo, hi, cap)
            masks.append((capped, limited))
            margin = min(margin, m)
            O.transport_limit(c["nx"], c["ny"], order, f, lo, hi, cap)
    return fields, masks, margin, c["fields"]


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("nx,ny", SC.TRANSPORT_GRIDS)
def test_oracle_transport_is_equivariant(nx, ny, order, kind):
    M = SM.MAPS[kind]
    a, b = transport_run(nx, ny, order), transport_run(nx, ny, order, kind)
    check("transport, three steps, order %d" % order, [(M.dg(x), y) for x, y in zip(a[0], b[0])], MANY)
    assert float(np.abs(a[0][1] - a[3][1]).max()) > 1e-3  # the fields moved
    for (ca, la), (cb, lb) in zip(a[1], b[1]):
        assert np.array_equal(M.elem(ca), cb) and np.array_equal(M.elem(la), lb)
    assert min(a[2], b[2]) >= 1e-6, (a[2], b[2])
    if nx * ny >= 35:  # cap and limiter both act on the bounded field, and leave elements alone
        capped, limited = a[1][1]
        assert capped.any() and not capped.all() and (order == 0 or (limited.any() and not limited.all()))


# ------------------------------------------------------------------------------------------------ brittle rheology, history
@functools.lru_cache(maxsize=None)
def bbm_run(nx, ny, kind=None):
    c = SC.bbm_case(nx, ny)
    if kind:
        c = SC.image(c, SM.MAPS[kind])
    mp, bp, diag = R.mevp_par(**c["params"]), R.bbm_par(), {}
    gauss = R.prepare(mp, bp, c["H"], c["A"])
    nod = R.nodal_fields(mp, c["H"], c["A"], c["ua"], c["va"], c["uo"], c["vo"])
    S, D, u, v = R.iterate(mp, bp, c["hx"], c["hy"], c["dts"], c["s"], c["D"], c["u"], c["v"], gauss, nod, diag=diag)
    return S, D, u, v, gauss, diag


@pytest.mark.parametrize("kind", SM.KINDS)
def test_bbm_reference_is_equivariant(kind):
    M = SM.MAPS[kind]
    a, b = bbm_run(130, 23), bbm_run(130, 23, kind)
    check("bbm_prepare", [(M.gauss(x), y) for x, y in zip(a[4], b[4])], ONCE)
    check("bbm sub-iteration", list(zip(M.stress(*a[0]) + (M.dg(a[1]),) + M.vec(a[2], a[3]), tuple(b[0]) + (b[1], b[2], b[3]))), ONCE)
    N = R.bbm_par()["compr_strength"]
    for d in (a[5], b[5]):  # sigma_n = 0 and sigma_n = -N: every Gauss point at a distance
        assert np.min(np.abs(d["sn_old"])) >= 1e-6 * np.max(np.abs(d["sn_old"])) and np.min(np.abs(d["sn_new"] + N)) >= 1e-6 * N
    for k in ("Pt_used", "failing"):
        assert np.array_equal(M.gauss(a[5][k]), b[5][k]) and a[5][k].any() and not a[5][k].all()
    assert np.array_equal(M.gauss(a[5]["sn_new"] < -N), b[5]["sn_new"] < -N)
    assert 0.0 < np.min(R.apply(R.PSI_Q[:, :6], SC.bbm_case(130, 23)["D"])) and np.max(a[1][0]) < R.bbm_par()["d_max"]


INVARIANT = ("divergence", "shear", "sigma_n", "sigma_s", "speed", "hice", "cice", "damage", "hsnow", "tice")


def history_pairs(M, a, b):
    """samples [12, ny, nx] in the order of history_ref.FIELDS: the scalars are invariant, (u, v) is a vector"""
    f = history_ref.FIELDS
    pairs = [(M.elem(a[f.index(k)]), b[f.index(k)]) for k in INVARIANT]
    return pairs + list(zip(M.vec(a[f.index("u")], a[f.index("v")], scalar=M.elem), (b[f.index("u")], b[f.index("v")])))


@pytest.mark.parametrize("kind", SM.KINDS)
def test_history_samples_are_equivariant(kind):
    M = SM.MAPS[kind]
    out = []
    for c in (SC.history_case(130, 23), SC.image(SC.history_case(130, 23), M)):
        out.append(history_ref.samples(history_ref.FIELDS, c["hx"], c["hy"], H=c["H"], A=c["A"], u=c["u"], v=c["v"], s11=c["s"][0], s12=c["s"][1],
                                       s22=c["s"][2], hsnow=c["hsnow"], tice=c["tice"], D=c["D"]))
    check("history samples", history_pairs(M, *out), ONCE)

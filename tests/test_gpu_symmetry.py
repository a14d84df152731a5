"""Every neighbour-coupled kernel held to the scheme's own mirror and transpose symmetry, device against mapped device.

x runs along the 64 lanes of a wave and y along the march, so every coupling has two implementations: DPP moves / carries, hasL / hasB,
window seams / strip seams, ihx / ihy.  The discrete scheme has the full symmetry group of the square (tests/test_symmetry_cpu.py: the
CPU references are equivariant at round-off on exactly these cases).  Here each operation runs on a rough random case
(tests/symmetry_cases.py) and on its image under T (x <-> y), X (x -> L - x) or Y (y -> L - y) (tests/symmetry_maps.py): the transposed
run sends every window seam, tile seam and left / right boundary through the strip, carry and top / bottom code, the mirrored runs move
every seam onto other data.  abi.Context only: no oracle takes part in a comparison of this file.

Bound per array: the project's device-against-oracle tolerance for the same operation, NOT doubled --
    helpers, transport, history                rtol 1e-12, atol 1e-13 max|array|
    one mEVP sub-iteration                     stress rtol 1e-12, atol 1e-12 max; velocity rtol 1e-11, atol 1e-13 max
    one pass of four sub-iterations            four times the bound of one (four applications; round-off adds at most linearly)
    25 sub-iterations                          rtol 1e-9, atol 1e-10 max
    one BBM sub-iteration                      rtol 1e-11, atol 1e-13 max (tests/test_gpu_bbm.py)
    three coupled steps                        rtol 1e-9, atol 1e-11 max (test_gpu_parity.py::test_coupled_step_matches_oracle)
The largest observed ratios of distance to bound are in profiles/symmetry.md."""
import numpy as np
import pytest
import torch

import symmetry_cases as SC
import symmetry_maps as SM
from nextsimdg_amd import abi, rowblock

pytestmark = pytest.mark.gpu

HELPER = (1e-12, 1e-13)
STRESS1, VELOCITY1 = (1e-12, 1e-12), (1e-11, 1e-13)
MANY = (1e-9, 1e-10)
BBM = (1e-11, 1e-13)
COUPLED = (1e-9, 1e-11)
WORST = {}
GRID_IDS = ["%dx%d" % g for g in SC.MEVP_GRIDS]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()
    for k in sorted(WORST):
        print("\nsymmetry on the device, %s: largest distance / bound %.3g" % (k, WORST[k]))


@pytest.fixture(autouse=True)
def _defaults_after_each_test(ctx):
    yield
    if ctx.nx:
        ctx.set_land_mask(None)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_bbm_params(ctx.bbm_default_params())
    ctx.set_transport_variant(abi.DEFAULT_TRANSPORT_VARIANT, 0)
    ctx.set_transport_bounds(())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tdev(a):
    return abi.tile(dev(a))


def host(t):
    return t.cpu().numpy()


def thost(t, nx):
    return abi.untile(t, nx).cpu().numpy()


def nans(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def compare(what, test, pairs, tol, scale=1.0):
    """pairs of (device on the image, mapped device on the original): every entry within scale * (rtol |want| + atol max|want|)"""
    rtol, atol = tol
    for k, (got, want) in enumerate(pairs):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(want)), (what, k)
        top = float(np.max(np.abs(want)))
        lim = scale * (rtol * np.abs(want) + atol * top)
        err = np.abs(got - want)
        r = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))))
        WORST[test] = max(WORST.get(test, 0.0), r)
        print("%s [%d]: distance / bound %.3g (max|array| %.3g)" % (what, k, r, top))
        assert r <= 1.0, "%s [%d]: %.3g times the bound (rtol %g, atol %g max|array|)" % (what, k, r, scale * rtol, scale * atol)


# ------------------------------------------------------------------------------------------------ running a case on the device
def set_case(ctx, c):
    ctx.set_mevp_params(ctx.mevp_default_params(**c.get("params", {})))
    ctx.set_grid(c["nx"], c["ny"], c["hx"], c["hy"])
    land = c.get("land")
    ctx.set_land_mask(None if land is None else torch.from_numpy(np.ascontiguousarray(land).astype(np.uint8)).cuda())


def helpers(ctx, c, rows=None):
    """the device's nodal means, ice strength and wind stress of a case: device tensors (pg tiled)"""
    nx, ny = c["nx"], c["ny"]
    H, A = dev(c["H"]), dev(c["A"])
    cgh, cga = nans(2 * ny + 1, 2 * nx + 1), nans(2 * ny + 1, 2 * nx + 1)
    ctx.dg_to_cg(H, cgh)
    ctx.dg_to_cg(A, cga)
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(H, A, pg, *(rows or ()))
    tax, tay = nans(*cgh.shape), nans(*cgh.shape)
    ctx.wind_stress(dev(c["ua"]), dev(c["va"]), tax, tay)
    return dict(cgh=cgh, cga=cga, pg=pg, tax=tax, tay=tay)


def packed_of(ctx, c, h):
    packed = torch.zeros(8 * h["cgh"].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_pack_nodal(c["dt"], (dev(c["u0"]), dev(c["v0"])), (h["tax"], h["tay"]), (dev(c["uo"]), dev(c["vo"])), h["cgh"], h["cga"], packed)
    return packed


def run_pass(ctx, c, variant, passes=1, strip_rows=0):
    """one launch of nsdg_mevp_iterate (passes = 1) or nsdg_mevp_iterate4 (passes = 4) on the whole array: (u, v, [s11, s12, s22]) on the host"""
    nx, ny = c["nx"], c["ny"]
    set_case(ctx, c)
    ctx.set_mevp_variant(variant)
    ctx.set_mevp_strip_rows(strip_rows)
    h = helpers(ctx, c)
    packed = packed_of(ctx, c, h)
    s_in = [tdev(x) for x in c["s"]]
    s_out = [torch.zeros_like(x) for x in s_in]
    un, vn = nans(2 * ny + 1, 2 * nx + 1), nans(2 * ny + 1, 2 * nx + 1)
    if passes == 1:
        ctx.mevp_iterate(0, 0, ny, s_in, s_out, (dev(c["u"]), dev(c["v"])), (un, vn), packed, h["pg"])
    else:
        ctx.mevp_iterate4(0, ny, s_in, s_out, (dev(c["u"]), dev(c["v"])), (un, vn), packed, h["pg"])
    ctx.synchronize()
    return host(un), host(vn), [thost(x, nx) for x in s_out]


def run_subcycle(ctx, c, nsub):
    nx, ny = c["nx"], c["ny"]
    set_case(ctx, c)
    h = helpers(ctx, c)
    u, v, s = dev(c["u"]), dev(c["v"]), [tdev(x) for x in c["s"]]
    scratch = torch.zeros(10 * u.numel() + 3 * s[0].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_subcycle(c["dt"], nsub, s, u, v, dev(c["u0"]), dev(c["v0"]), h["tax"], h["tay"], dev(c["uo"]), dev(c["vo"]), h["cgh"], h["cga"], h["pg"], scratch)
    ctx.synchronize()
    return host(u), host(v), [thost(x, nx) for x in s]


def mevp_pairs(M, a, b):
    """(image run, mapped original run): velocity pairs and stress pairs"""
    return list(zip((b[0], b[1]), M.vec(a[0], a[1]))), list(zip(b[2], M.stress(*a[2])))


_CACHE = {}


def cached(key, make):
    """the original's run of a case, made once and shared by the maps it is compared under (nobody writes to it)"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ helpers
@pytest.mark.parametrize("kind", ["T", "X"])
def test_helpers(ctx, kind):
    """dg_to_cg, ice_strength (all rows and a row range), wind_stress, prepare_advection and bbm_prepare on 130 x 23"""
    M = SM.MAPS[kind]
    nx, ny = 130, 23
    c = SC.mevp_case(nx, ny, "uniform")
    ci = SC.image(c, M)
    j0, j1 = 3, ny - 4
    rows = {"T": None, "X": (j0, j1)}[kind]  # the image's rows under T are the original's columns: all of them
    out = []
    for case, r in ((c, (j0, j1)), (ci, rows)):
        set_case(ctx, case)
        ctx.set_bbm_params(ctx.bbm_default_params())
        n = case["nx"]
        h, part = helpers(ctx, case), helpers(ctx, case, r)["pg"]
        adv = (nans(6, case["ny"], n), nans(6, case["ny"], n), nans(3, case["ny"], n + 1), nans(3, case["ny"] + 1, n))
        ctx.prepare_advection(2, dev(case["u"]), dev(case["v"]), *adv)
        g = [ctx.private_zeros(9, case["ny"], n, "cuda") for _ in range(3)]
        ctx.bbm_prepare(dev(case["H"]), dev(case["A"]), *g)
        ctx.synchronize()
        out.append(dict(cgh=host(h["cgh"]), cga=host(h["cga"]), pg=thost(h["pg"], n), part=thost(part, n), tax=host(h["tax"]), tay=host(h["tay"]),
                        adv=[host(x) for x in adv], g=[thost(x, n) for x in g]))
    a, b = out
    t = "helpers"
    compare("dg_to_cg", t, [(b["cgh"], M.node(a["cgh"])), (b["cga"], M.node(a["cga"]))], HELPER)
    compare("ice_strength", t, [(b["pg"], M.gauss(a["pg"]))], HELPER)
    compare("ice_strength on the rows [%d, %d)" % (j0, j1), t, [(M.gauss(b["part"])[:, j0:j1], a["part"][:, j0:j1])], HELPER)
    assert np.all(a["part"][:, :j0] == 0) and np.all(a["part"][:, j1:] == 0)
    compare("wind_stress", t, zip((b["tax"], b["tay"]), M.vec(a["tax"], a["tay"])), HELPER)
    compare("prepare_advection", t, zip(b["adv"], M.dgvec(a["adv"][0], a["adv"][1]) + M.edges(a["adv"][2], a["adv"][3])), HELPER)
    compare("bbm_prepare", t, [(y, M.gauss(x)) for x, y in zip(a["g"], b["g"])], HELPER)


# ------------------------------------------------------------------------------------------------ mEVP
RUNS = [pytest.param(0, "uniform", id="variant0-uniform"), pytest.param(1, "uniform", id="variant1-uniform"), pytest.param(1, "adaptive", id="variant1-adaptive")]


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("land", [False, True], ids=["ocean", "land"])
@pytest.mark.parametrize("variant,form", RUNS)
@pytest.mark.parametrize("nx,ny", SC.MEVP_GRIDS, ids=GRID_IDS)
def test_one_sub_iteration(ctx, nx, ny, variant, form, land, kind):
    """nsdg_mevp_iterate on the rough state with ice-free nodes, with and without the land mask"""
    M = SM.MAPS[kind]
    c = SC.mevp_case(nx, ny, form, land)
    a = cached(("pass", nx, ny, variant, form, land), lambda: run_pass(ctx, c, variant))
    b = run_pass(ctx, SC.image(c, M), variant)
    assert np.max(np.abs(a[0])) > 0.1 * SC.SPEED[form]
    vel, stress = mevp_pairs(M, a, b)
    compare("velocity", "one sub-iteration", vel, VELOCITY1)
    compare("stress", "one sub-iteration", stress, STRESS1)


@pytest.mark.parametrize("kind", ["T", "X"])
@pytest.mark.parametrize("strip_rows", [5, 0])
@pytest.mark.parametrize("form", ["uniform", "adaptive"])
@pytest.mark.parametrize("nx,ny", SC.MEVP_GRIDS[:2], ids=GRID_IDS[:2])
def test_one_pass_of_four(ctx, nx, ny, form, strip_rows, kind):
    """nsdg_mevp_iterate4 (the stage-per-wave pipeline) with the land mask: four sub-iterations, four times the bound of one"""
    M = SM.MAPS[kind]
    c = SC.mevp_case(nx, ny, form, True)
    a = cached(("four", nx, ny, form, strip_rows), lambda: run_pass(ctx, c, 4, 4, strip_rows))
    b = run_pass(ctx, SC.image(c, M), 4, 4, strip_rows)
    vel, stress = mevp_pairs(M, a, b)
    compare("velocity", "one pass of four", vel, VELOCITY1, 4.0)
    compare("stress", "one pass of four", stress, STRESS1, 4.0)


@pytest.mark.parametrize("kind", ["T", "X"])
@pytest.mark.parametrize("form", ["uniform", "adaptive"])
def test_25_sub_iterations(ctx, form, kind):
    """nsdg_mevp_subcycle with the library's default variant from the rough state, land mask on, on 130 x 23"""
    M = SM.MAPS[kind]
    c = SC.mevp_case(130, 23, form, True)
    a = cached(("subcycle", form), lambda: run_subcycle(ctx, c, 25))
    b = run_subcycle(ctx, SC.image(c, M), 25)
    assert np.max(np.abs(a[0])) > 0.1 * SC.SPEED[form]
    vel, stress = mevp_pairs(M, a, b)
    compare("velocity", "25 sub-iterations", vel, MANY)
    compare("stress", "25 sub-iterations", stress, MANY)


# ------------------------------------------------------------------------------------------------ brittle rheology
def run_bbm(ctx, c):
    nx, ny = c["nx"], c["ny"]
    set_case(ctx, c)
    ctx.set_bbm_params(ctx.bbm_default_params())
    H, A, D = dev(c["H"]), dev(c["A"]), dev(c["D"])
    S, u, v = [tdev(x) for x in c["s"]], dev(c["u"]), dev(c["v"])
    gauss = [ctx.private_zeros(9, ny, nx, "cuda") for _ in range(3)]
    ctx.bbm_prepare(H, A, *gauss)
    packed = torch.zeros(8 * u.numel(), dtype=torch.float64, device="cuda")
    zero = torch.zeros_like(u)
    ctx.mevp_prepare(c["dts"], H, A, (dev(c["ua"]), dev(c["va"])), (dev(c["uo"]), dev(c["vo"])), (zero, zero), packed)
    So, Do = [torch.zeros_like(x) for x in S], nans(*D.shape)
    un, vn = nans(*u.shape), nans(*u.shape)
    ctx.bbm_iterate(0, 0, ny, S, So, D, Do, (u, v), (un, vn), packed, gauss)
    ctx.synchronize()
    return host(un), host(vn), [thost(x, nx) for x in So], host(Do)


@pytest.mark.parametrize("kind", ["T", "X"])
def test_one_bbm_sub_iteration(ctx, kind):
    """nsdg_bbm_iterate with damage inside (0, d_max) on 130 x 23"""
    M = SM.MAPS[kind]
    c = SC.bbm_case(130, 23)
    a = cached("bbm", lambda: run_bbm(ctx, c))
    b = run_bbm(ctx, SC.image(c, M))
    assert np.max(np.abs(a[0])) > 1e-5
    vel, stress = mevp_pairs(M, a, b)
    compare("velocity", "one BBM sub-iteration", vel, BBM)
    compare("stress", "one BBM sub-iteration", stress, BBM)
    compare("damage", "one BBM sub-iteration", [(b[3], M.dg(a[3]))], BBM)


# ------------------------------------------------------------------------------------------------ transport
def run_transport(ctx, c, staged=False):
    """three steps with the closure of the case's bounds: the march between ping-pong buffers, or the staged step (variant 0) in place"""
    nx, ny, order = c["nx"], c["ny"], c["order"]
    ctx.set_grid(nx, ny, c["hx"], c["hy"])
    nc, ng = SC.NCOEF[order], order + 1
    adv = (nans(nc, ny, nx), nans(nc, ny, nx), nans(ng, ny, nx + 1), nans(ng, ny + 1, nx))
    ctx.prepare_advection(order, dev(c["u"]), dev(c["v"]), *adv)
    ctx.set_transport_bounds(c["bounds"])
    a = [dev(f) for f in c["fields"]]
    if staged:
        ctx.set_transport_variant(0, 0)
        scratch = nans(2 * sum(f.numel() for f in a))
        for _ in range(3):
            ctx.transport_step(order, c["dt"], a, adv, scratch)
    else:
        b = [nans(*f.shape) for f in a]
        for _ in range(3):
            ctx.transport_step_oop(order, c["dt"], a, b, adv)
            a, b = b, a
    ctx.synchronize()
    return [host(f) for f in a]


TRANSPORT_RUNS = [pytest.param(0, 2, False, id="p0-2fields"), pytest.param(1, 2, False, id="p1-2fields"), pytest.param(2, 2, False, id="p2-2fields"),
                  pytest.param(2, 4, False, id="p2-4fields"), pytest.param(2, 2, True, id="p2-staged")]


@pytest.mark.parametrize("kind", SM.KINDS)
@pytest.mark.parametrize("order,nfields,staged", TRANSPORT_RUNS)
@pytest.mark.parametrize("nx,ny", SC.TRANSPORT_GRIDS, ids=["%dx%d" % g for g in SC.TRANSPORT_GRIDS])
def test_three_transport_steps(ctx, nx, ny, order, nfields, staged, kind):
    """nsdg_transport_step_oop (and nsdg_transport_step under variant 0) with the bounds ((0, inf, no cap), (0, 1, cap)) per pair of fields"""
    M = SM.MAPS[kind]
    c = SC.transport_case(nx, ny, order, nfields)
    a = cached(("transport", nx, ny, order, nfields, staged), lambda: run_transport(ctx, c, staged))
    b = run_transport(ctx, SC.image(c, M), staged)
    assert float(np.abs(a[1] - c["fields"][1]).max()) > 1e-3
    compare("fields", "three transport steps, order %d" % order, [(y, M.dg(x)) for x, y in zip(a, b)], HELPER)


# ------------------------------------------------------------------------------------------------ coupled model steps
def run_coupled(ctx, c, nsteps=3):
    ctx.set_mevp_params(ctx.mevp_default_params(**c["params"]))
    core = rowblock.DynamicsCore(ctx, rowblock.RowBlock(c["nx"], c["ny"]), c["hx"], c["hy"], c["dt"], c["nsub"], torch.device("cuda"), land=c["land"])
    core.load_global(c["H"], c["A"], c["uo"], c["vo"], c["ua"], c["va"])
    for _ in range(nsteps):
        core.step()
    torch.cuda.synchronize()
    out = dict(H=host(core.H), A=host(core.A), u=host(core.u), v=host(core.v), s=[thost(x, c["nx"]) for x in core.s])
    core.close()
    return out


def test_three_coupled_steps_under_transposition(ctx):
    """rowblock.DynamicsCore on one block, variant 4, closure on, land mask, adaptive alpha / beta: 64 x 48 against 48 x 64"""
    assert ctx.mevp_variant == 4
    M = SM.T
    c = SC.coupled_case(64, 48)
    a, b = run_coupled(ctx, c), run_coupled(ctx, SC.image(c, M))
    assert np.max(np.abs(a["u"])) > 1e-3 and float(np.abs(a["A"] - c["A"])[:, ~c["land"]].max()) > 1e-4
    t = "three coupled steps"
    compare("H, A", t, [(b["H"], M.dg(a["H"])), (b["A"], M.dg(a["A"]))], COUPLED)
    compare("u, v", t, zip((b["u"], b["v"]), M.vec(a["u"], a["v"])), COUPLED)
    compare("stress", t, zip(b["s"], M.stress(*a["s"])), COUPLED)


# ------------------------------------------------------------------------------------------------ history
INVARIANT = ("divergence", "shear", "sigma_n", "sigma_s", "speed", "hice", "cice", "damage", "hsnow", "tice")


def run_history(ctx, c):
    nx, ny = c["nx"], c["ny"]
    ctx.set_grid(nx, ny, c["hx"], c["hy"])
    src = dict(H=dev(c["H"]), A=dev(c["A"]), D=dev(c["D"]), u=dev(c["u"]), v=dev(c["v"]), hsnow=dev(c["hsnow"]), tice=dev(c["tice"]))
    src.update({k: tdev(x) for k, x in zip(("s11", "s12", "s22"), c["s"])})
    acc = nans(len(abi.HISTORY_FIELDS), ny, nx)
    ctx.history_accumulate(0, ny, abi.HISTORY_FIELDS, src, True, 0, acc)
    ctx.synchronize()
    return host(acc)


@pytest.mark.parametrize("kind", ["T", "X"])
def test_one_history_sample_of_every_field(ctx, kind):
    """nsdg_history_accumulate: the scalar samples are invariant, (u, v) swap under T and u changes sign under X"""
    M = SM.MAPS[kind]
    c = SC.history_case(130, 23)
    a = cached("history", lambda: run_history(ctx, c))
    b = run_history(ctx, SC.image(c, M))
    f = abi.HISTORY_FIELDS
    assert set(f) == set(INVARIANT) | {"u", "v"}
    pairs = [(b[f.index(k)], M.elem(a[f.index(k)])) for k in INVARIANT]
    pairs += list(zip((b[f.index("u")], b[f.index("v")]), M.vec(a[f.index("u")], a[f.index("v")], scalar=M.elem)))
    compare("samples", "history", pairs, HELPER)

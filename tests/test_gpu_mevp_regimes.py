"""The mEVP sub-iteration on the device -- csrc/mevp_fused.hip, csrc/mevp_fused4.hip, the element and node arithmetic of
csrc/mevp_common.h and the two-kernel form of csrc/mevp.hip -- against the numpy restatement tests/mevp_ref.py on the inputs of
tests/mevp_cases.py: alpha != beta, every physical parameter off its default, the viscous regime, the transition and ice at rest, the
clamps, every trigger of the ice-free rule across the column seams and on the first and last row, the adaptive form at its floor, spread
out and beside ice-free nodes, and rigid ice that moves; the array widths around the 63 owned columns of a wave, the 57 of a workgroup
of the four-stage pass and the 64-element tile; the passes of 2, 3 and 4 and the sub-cycle bit for bit on the same inputs; and nothing
written outside the rows of a launch.  The bound is that of test_gpu_parity.py::test_mevp_single_iteration_matches_oracle everywhere
(mevp_cases.STRESS_TOL, VELOCITY_TOL), but for the drift kind, whose bound is recorded by tests/test_mevp_regimes_cpu.py; that the cases
hold their conditions and margins and are well conditioned is asserted there, without a GPU."""
import numpy as np
import pytest
import torch

import mevp_cases as B
import mevp_ref as R
from nextsimdg_amd import abi
from test_gpu_parity import assert_close, dev, host, pack, tdev, thost

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults_after_each_test(ctx):
    yield
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_land_mask(None)
    ctx.set_mevp_params(ctx.mevp_default_params())


def held(got, want, rtol, atol, what):
    """assert_close, and the largest |difference| / bound for the record"""
    got, want = np.asarray(got), np.asarray(want)
    assert_close(got, want, rtol, atol, what)
    lim = atol + rtol * np.abs(want)
    err = np.abs(got - want)
    return float(np.max(np.where(err > 0.0, err / np.where(lim > 0.0, lim, 1.0), 0.0))) if got.size else 0.0


class Device:
    """the device arrays of a case -- parameters, grid and mask set on the context, ice strength and coefficient packing made by the
    calls a model step makes -- and launches of one sub-iteration or pass on them"""

    def __init__(self, ctx, case, land_mask=None):
        c = case["c"]
        nx, ny = c["nx"], c["ny"]
        self.ctx, self.case, self.nx, self.ny = ctx, case, nx, ny
        ctx.set_mevp_params(ctx.mevp_default_params(**case["par"]))
        ctx.set_grid(nx, ny, case["hx"], case["hy"])
        self.mask = None if land_mask is None else torch.from_numpy(np.ascontiguousarray(land_mask).astype(np.uint8)).cuda()
        ctx.set_land_mask(self.mask)
        for k in ("H", "A", "u", "v", "u0", "v0", "ua", "va", "uo", "vo"):
            setattr(self, k, dev(c[k]))
        self.S = [tdev(x) for x in c["S"]]
        self.pg = ctx.private_zeros(9, ny, nx, "cuda")
        ctx.ice_strength(self.H, self.A, self.pg)
        self.packed = torch.zeros(8 * self.u.numel(), dtype=torch.float64, device="cuda")
        ctx.mevp_prepare(case["dt"], self.H, self.A, (self.ua, self.va), (self.uo, self.vo), (self.u0, self.v0), self.packed)

    def outputs(self, fill):
        return [torch.full_like(x, fill) for x in self.S] + [torch.full_like(self.u, fill), torch.full_like(self.v, fill)]

    def launch(self, variant=1, rows=None, strip_rows=0, fill=3.0, state=None):
        """one nsdg_mevp_iterate on (k0, j0, j1) = rows from `state` (the case's own): the five output tensors"""
        ctx = self.ctx
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_strip_rows(strip_rows)
        cur = state or self.S + [self.u, self.v]
        out = self.outputs(fill)
        k0, j0, j1 = rows or (0, 0, self.ny)
        ctx.mevp_iterate(k0, j0, j1, cur[:3], out[:3], (cur[3], cur[4]), (out[3], out[4]), self.packed, self.pg)
        torch.cuda.synchronize()
        return out

    def result(self, out):
        return dict(S=[thost(x, self.nx) for x in out[:3]], u=host(out[3]), v=host(out[4]))

    def nodal_inputs(self):
        """cgH, cgA and the wind stress as arrays, for the calls that pack themselves"""
        z = lambda: torch.zeros_like(self.u)
        cgh, cga, tax, tay = z(), z(), z(), z()
        self.ctx.dg_to_cg(self.H, cgh)
        self.ctx.dg_to_cg(self.A, cga)
        self.ctx.wind_stress(self.ua, self.va, tax, tay)
        return cgh, cga, tax, tay


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_against_reference(key, got, ref=None, rows=None, what=""):
    """one sub-iteration against the restatement under the bound of test_mevp_single_iteration_matches_oracle: stress 1e-12 relative plus
    1e-12 of the array's largest reference value, velocity 1e-11 plus 1e-13.  The ice-free kinds: the nodes with ice once more under the
    floor of their own maximum (their free-drift nodes are the fastest of the array).  drift: against the longdouble evaluation rounded
    to float64, under 4 times the distance of the float64 reference from it (tests/golden/mevp_drift_bounds.json).  rows = (k0, j0,
    j1): only what that launch writes.  Returns the largest |difference| / bound"""
    case, full = B.built(key)
    ref = ref or full
    ny = case["c"]["ny"]
    k0, j0, j1 = rows or (0, 0, ny)
    g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == ny else 0)
    cut = lambda r: dict(s11=r["S"][0][:, k0:j1], s12=r["S"][1][:, k0:j1], s22=r["S"][2][:, k0:j1], u=r["u"][g0:g1], v=r["v"][g0:g1])
    g, w = cut(got), cut(ref)
    worst = 0.0
    if case["kind"] == "drift":
        bounds, w = B.drift_bounds(), {k: x.astype(np.float64) for k, x in cut(B.built_wide(key)).items()}
        for k in B.OUTPUTS:
            worst = max(worst, held(g[k], w[k], 0.0, bounds[k], "%s %s" % (what, k)))
    else:
        for k in B.OUTPUTS:
            rel, floor = B.VELOCITY_TOL if k in ("u", "v") else B.STRESS_TOL
            worst = max(worst, held(g[k], w[k], rel, floor * np.max(np.abs(w[k])), "%s %s" % (what, k)))
        if case["kind"] in ("icefree", "ad_icefree"):
            ice = ~B.ice_free_nodes(case, full)[g0:g1]
            assert np.max(np.abs(w["u"][~ice])) > 2.0 * np.max(np.abs(w["u"][ice])) > 0.0
            for k in ("u", "v"):
                worst = max(worst, held(g[k][ice], w[k][ice], B.VELOCITY_TOL[0], B.VELOCITY_TOL[1] * np.max(np.abs(w[k][ice])), "%s %s (ice)" % (what, k)))
    assert np.max(np.abs(w["u"])) > 1e-5  # something moves (1 x 1 has one node that does)
    print("%s %s: worst |difference| / bound %.4f" % (B.case_id(key), what, worst))
    return worst


def mask_of(key):
    return B.built(key)[0]["c"]["land"]


# ---- 1. the helpers and the coefficient packing on every kind and shape -------------------------------------------------------------------
def unpack(packed, shape):
    """[6, 2ny+1, 2nx+1] from the three pair planes of the packing (csrc/mevp_common.h: pair k of node n at packed[k plane + 2 n])"""
    n = shape[0] * shape[1]
    return host(packed)[:6 * n].reshape(3, n, 2).transpose(0, 2, 1).reshape(6, *shape)


@pytest.mark.parametrize("key", B.ALL_CASES, ids=B.case_id)
def test_helpers_and_packing_match_the_reference(ctx, key):
    """nsdg_ice_strength, nsdg_dg_to_cg and nsdg_wind_stress under the bounds of test_mevp_helpers_match_oracle; nsdg_mevp_prepare bit
    for bit what nsdg_dg_to_cg x 2 + nsdg_wind_stress + nsdg_mevp_pack_nodal give, under the case's mask too; and the packing against the
    coefficients the reference implies: the ice-free decision at every node (the 2^100 scaling), the flag and the constants of a land
    node exactly, u_o and v_o exactly, and h', a C_o rho_o, c2 and c3 -- sums of at most three products of inputs held to 1e-13 -- to
    1e-12 relative plus 1e-13 of the plane's largest value, with the scaling divided out"""
    case, ref = B.built(key)
    c, prep, p = case["c"], ref["prep"], B.params_of(case)
    d = Device(ctx, case, mask_of(key))
    nx, ny, shape = d.nx, d.ny, c["u"].shape
    worst = held(thost(d.pg, nx), prep["pg"], 1e-12, 1e-10, "ice strength")
    cgh, cga, tax, tay = d.nodal_inputs()
    sea = B.sea_nodes(case)  # the wind is NaN over land: it must not enter the packing, the wind stress there is nobody's
    worst = max(worst, held(host(cgh), prep["cgh"], 1e-13, 1e-14, "cgh"), held(host(cga), prep["cga"], 1e-13, 1e-14, "cga"))
    tx, ty = R.wind_stress(p, c["ua"], c["va"])
    worst = max(worst, held(host(tax)[sea], tx[sea], 1e-13, 1e-16, "tax"), held(host(tay)[sea], ty[sea], 1e-13, 1e-16, "tay"))
    assert torch.equal(pack(ctx, case["dt"], c["u0"], c["v0"], host(tax), host(tay), c["uo"], c["vo"], host(cgh), host(cga)), d.packed)
    got = unpack(d.packed, shape)
    ln = B.land_of(case)
    want = R.packed_coefficients(p, case["dt"], c["u0"], c["v0"], prep, ln)
    free = B.ice_free_nodes(case, ref)
    assert np.array_equal(got[0] > 2.0 ** 50, free)
    w = np.where(free, 2.0 ** -100, 1.0)
    for k in range(4):
        worst = max(worst, held(got[k] * w, want[k] * w, 1e-12, 1e-13 * np.max(np.abs(want[k] * w)), "packed[%d]" % k))
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])
    if ln is not None:
        assert ln.any() and np.array_equal(got[:, ln], want[:, ln]) and np.all(got[1][~ln] >= 0.0)
    print("%s helpers and packing: worst |difference| / bound %.4f" % (B.case_id(key), worst))


# ---- 2. the kinds at 70 x 9 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.KIND_CASES, ids=B.case_id)
def test_kind_matches_the_reference_70x9(ctx, key):
    """one sub-iteration of every kind through the marching kernel (variant 1); under an all-ocean mask the masked instantiation gives
    the reference too, and bit for bit what the unmasked one gives"""
    case, _ = B.built(key)
    d = Device(ctx, case)
    plain = d.launch(1)
    check_against_reference(key, d.result(plain), what="variant 1")
    ocean = Device(ctx, case, land_mask=np.zeros((9, 70), dtype=bool))
    masked = ocean.launch(1)
    check_against_reference(key, ocean.result(masked), what="variant 1, all-ocean mask")
    assert same(masked, plain)


@pytest.mark.parametrize("key", [k for k in B.KIND_CASES if k[0] in B.UNIFORM_KINDS], ids=B.case_id)
def test_two_kernel_form_matches_the_reference_70x9(ctx, key):
    """variant 0, nsdg_mevp_stress + nsdg_mevp_velocity behind nsdg_mevp_iterate, on the uniform kinds (it has no adaptive form); with
    an all-ocean mask it gives the same bits"""
    case, _ = B.built(key)
    d = Device(ctx, case)
    plain = d.launch(0)
    check_against_reference(key, d.result(plain), what="variant 0")
    ocean = Device(ctx, case, land_mask=np.zeros((9, 70), dtype=bool))
    assert same(ocean.launch(0), plain)


@pytest.mark.parametrize("key", B.ISLAND_CASES, ids=B.case_id)
def test_island_and_rock_stay_at_zero(ctx, key):
    """the masked instantiations, uniform and adaptive, with the island across the wave seam and the rock: the reference on the sea,
    velocity and stress exactly 0 on land, whatever the strip height; the uniform kind through the two-kernel form as well"""
    case, _ = B.built(key)
    land = mask_of(key)
    ln = R.land_nodes(land)
    d = Device(ctx, case, land_mask=land)
    for variant, strip in ((1, 0), (1, 3)) + (((0, 0),) if key[0] in B.UNIFORM_KINDS else ()):
        got = d.result(d.launch(variant, strip_rows=strip))
        check_against_reference(key, got, what="variant %d, strip_rows %d" % (variant, strip))
        assert np.all(got["u"][ln] == 0.0) and np.all(got["v"][ln] == 0.0)
        assert all(np.all(x[:, land] == 0.0) for x in got["S"])


# ---- 3. array widths and heights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.SHAPE_CASES, ids=B.case_id)
def test_shape_matches_the_reference_at_every_seam(ctx, key):
    """a wave of the marching kernel owns 63 columns of 64-element tiles, a workgroup of the four-stage pass 57: 1 x 1 and 1 x 5 (one
    column), 56 / 57 / 58 x 3 (the last owned column of a workgroup and the first of the next), 63 / 64 / 65 x 3 (the same for a wave,
    and the tile seam), 114 / 115 x 2 (two workgroups), 127 x 3 (a third wave of one column), 130 x 5 (a last tile of two), 190 x 2 (a
    fourth wave), 130 x 1 (one row), 3 x 70 (many short strips) -- uniform (plastic) and adaptive (ad_spread)"""
    case, _ = B.built(key)
    d = Device(ctx, case)
    check_against_reference(key, d.result(d.launch(1)), what="variant 1")


# ---- 4. the passes and the sub-cycle on the same inputs, bit for bit ------------------------------------------------------------------------
def differ(a, b, nx, what):
    """asserts that two results (three tiled stress arrays, u, v) hold the same bits at every element and node; the padding elements of
    the last tile belong to nobody and keep whatever the buffer held"""
    for k in range(3):
        x, y = abi.untile(a[k], nx), abi.untile(b[k], nx)
        assert torch.equal(x, y), what + (k, float((x - y).abs().max()))
    for k in (3, 4):
        assert torch.equal(a[k], b[k]), what + (k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("key", B.PIPELINE_CASES, ids=B.case_id)
def test_passes_and_subcycle_equal_single_launches_bitwise(ctx, key):
    """nsdg_mevp_iterate2 / 3 / 4 == 2 / 3 / 4 launches of variant 1 and nsdg_mevp_subcycle over 7 sub-iterations (a pass of 4 plus a
    pass of 3) == 7 launches, in every bit of every output, for the strip heights 0 (automatic), 1 and 3 -- on every kind and on the
    widths around the 57 owned columns of a workgroup; and no wait of the pipeline gave up"""
    case, _ = B.built(key)
    d = Device(ctx, case)
    ny = d.ny
    chain, cur = {}, None
    for n in range(1, 8):
        cur = d.launch(1, state=cur)
        chain[n] = cur
    cgh, cga, tax, tay = d.nodal_inputs()
    ctx.set_mevp_variant(4)
    for strip in (0, 1, 3):
        ctx.set_mevp_strip_rows(strip)
        for n in (2, 3, 4):
            out = d.outputs(7.0)
            getattr(ctx, "mevp_iterate%d" % n)(0, ny, d.S, out[:3], (d.u, d.v), (out[3], out[4]), d.packed, d.pg)
            torch.cuda.synchronize()
            differ(chain[n], out, d.nx, (B.case_id(key), "pass of %d" % n, strip))
        s, u, v = [x.clone() for x in d.S], d.u.clone(), d.v.clone()
        scratch = torch.zeros(10 * u.numel() + 3 * s[0].numel(), dtype=torch.float64, device="cuda")
        ctx.mevp_subcycle(case["dt"], 7, s, u, v, d.u0, d.v0, tax, tay, d.uo, d.vo, cgh, cga, d.pg, scratch)
        torch.cuda.synchronize()
        differ(chain[7], s + [u, v], d.nx, (B.case_id(key), "sub-cycle of 7", strip))
    assert ctx.pipeline_waits_given_up() == 0


# ---- 5. nothing outside the rows of a launch ------------------------------------------------------------------------------------------------
NX5, NY5 = 130, 5


def assert_nan_outside(out, e0, e1, g0, g1, what):
    """the stress keeps its NaN on every element row outside [e0, e1) and -- on every row -- on the padding elements of the last tile,
    the velocity on every node row outside [g0, g1)"""
    rows = np.ones(NY5, dtype=bool)
    rows[e0:e1] = False
    nodes = np.ones(2 * NY5 + 1, dtype=bool)
    nodes[g0:g1] = False
    for x in out[:3]:  # [ny, tiles, 8 * 64]
        assert np.all(np.isnan(host(x)[rows])), what
        pad = host(x)[:, -1].reshape(NY5, 4, 64, 2)[:, :, NX5 % 64:]  # coefficient pairs interleaved by element (abi.tile)
        assert np.all(np.isnan(pad)), what + ": padding elements of the last tile"
        assert not np.any(np.isnan(thost(x, NX5)[:, e0:e1])), what
    for x in out[3:]:
        assert np.all(np.isnan(host(x)[nodes])) and not np.any(np.isnan(host(x)[g0:g1])), what


@pytest.mark.parametrize("kind", ["plastic", "ad_spread"])
@pytest.mark.parametrize("rows", [(1, 2, 4), (2, 3, 5)], ids=["1-2-4", "2-3-5"])
def test_a_launch_writes_nothing_outside_its_rows(ctx, kind, rows):
    """130 x 5, outputs filled with NaN, ONE nsdg_mevp_iterate(k0, j0, j1) under variant 1: include/nsdg.h documents the stress on the
    element rows [k0, j1) and the velocity of the nodes owned by [j0, j1) -- node rows [2 j0, 2 j1), and the array's top row when j1 is
    its last.  Everything else keeps its NaN; inside, the launch is mevp_ref.iterate(k0, j0, j1)"""
    k0, j0, j1 = rows
    key = B.shape_case(kind, NX5, NY5)
    case, _ = B.built(key)
    d = Device(ctx, case)
    out = d.launch(1, rows=rows, fill=float("nan"))
    g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == NY5 else 0)
    assert (g0, g1) == {(1, 2, 4): (4, 8), (2, 3, 5): (6, 11)}[rows]
    assert_nan_outside(out, k0, j1, g0, g1, "rows %s" % (rows,))
    check_against_reference(key, d.result(out), B.reference(case, k0=k0, j0=j0, j1=j1), rows, "rows %s" % (rows,))


# nsdg_mevp_iterate4(j0, j1) asks for j0 == 0 or four ghost rows below and for j1 == ny or three above: of the proper sub-ranges of five
# rows it accepts [0, 2) and [4, 5) and refuses the ranges [2, 4) and [3, 5) of the single launches above
@pytest.mark.parametrize("kind", ["plastic", "ad_spread"])
@pytest.mark.parametrize("rows", [(0, 2), (4, 5)], ids=["0-2", "4-5"])
def test_a_pass_of_four_writes_only_its_final_rows(ctx, kind, rows):
    """130 x 5, outputs filled with NaN, ONE nsdg_mevp_iterate4(j0, j1): include/nsdg.h documents S_out = S^{p+4} on the element rows
    [j0, j1) and u_new = u^{p+4} on the nodes they own, [2 j0, 2 j1) and the top row when j1 == ny -- those are the final rows; the
    intermediate sub-iterations on the ghost rows never leave the chip.  Everything else keeps its NaN.  On the final rows the pass is
    four launches of variant 1 bit for bit, and four sub-iterations of the reference under the bound
    test_mevp_four_iterations_per_pass_equals_four_single_passes_bitwise holds four oracle sub-iterations to (1e-10 relative plus 1e-12
    of the largest value); the ranges the header excludes are refused and write nothing"""
    j0, j1 = rows
    key = B.shape_case(kind, NX5, NY5)
    case, _ = B.built(key)
    d = Device(ctx, case)
    cur = None
    for _ in range(4):
        cur = d.launch(1, state=cur)
    ctx.set_mevp_variant(4)
    out = d.outputs(float("nan"))
    ctx.mevp_iterate4(j0, j1, d.S, out[:3], (d.u, d.v), (out[3], out[4]), d.packed, d.pg)
    torch.cuda.synchronize()
    g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == NY5 else 0)
    assert_nan_outside(out, j0, j1, g0, g1, "rows %s" % (rows,))
    for a, b in zip(cur[:3], out[:3]):
        assert torch.equal(abi.untile(a, NX5)[:, j0:j1], abi.untile(b, NX5)[:, j0:j1])
    for a, b in zip(cur[3:], out[3:]):
        assert torch.equal(a[g0:g1], b[g0:g1])
    want, got, worst = B.reference_steps(case, 4), d.result(out), 0.0
    for g, w, name in zip(got["S"], want["S"], ("s11", "s12", "s22")):
        worst = max(worst, held(g[:, j0:j1], w[:, j0:j1], 1e-10, 1e-12 * np.max(np.abs(w)), name))
    for k in ("u", "v"):
        worst = max(worst, held(got[k][g0:g1], want[k][g0:g1], 1e-10, 1e-12 * np.max(np.abs(want[k])), k))
    print("%s pass of four on rows %s: worst |difference| / bound %.4f" % (B.case_id(key), rows, worst))
    for bad in ((2, 4), (3, 5)):
        out = d.outputs(float("nan"))
        with pytest.raises(abi.NsdgError, match="ghost rows"):
            ctx.mevp_iterate4(bad[0], bad[1], d.S, out[:3], (d.u, d.v), (out[3], out[4]), d.packed, d.pg)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(x).all()) for x in out)
    assert ctx.pipeline_waits_given_up() == 0

"""Every branch and seam of the brittle Bingham-Maxwell sub-iteration (csrc/bbm.hip, csrc/bbm_common.h) on the device against the numpy
restatement tests/bbm_ref.py, on the inputs of tests/bbm_cases.py that reach what tests/test_gpu_bbm.py stays clear of: compressive failure,
r = 1, damage outside [0, d_max] and healing that ends at 0, relax_exponent 1 and 2, hx != hy under the envelope, other mEVP parameters,
ice-free nodes and hg = 0; the array widths around the 63-column wave seam and the 64-element tile seam; strips and split launches bit
for bit; nothing written outside a launch's rows; and the launch geometry of 2048 x 2048.  The tolerance is that of
test_gpu_bbm.check_against_reference everywhere; that the cases keep their margins, reach their branches and are well conditioned is
asserted without a GPU in tests/test_bbm_cpu.py::test_device_case_holds_its_margins_branches_and_conditioning."""
import gc

import numpy as np
import pytest
import torch

import bbm_cases as B
import bbm_ref as R
from nextsimdg_amd import abi
from test_gpu_bbm import Device, assert_close, check_against_reference, host, same, thost

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
    ctx.set_mevp_strip_rows(0)
    ctx.set_land_mask(None)
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_bbm_params(ctx.bbm_default_params())


def device_of(ctx, case, land_mask=None):
    return Device(ctx, case["c"], bp=ctx.bbm_default_params(**case["bbm"]), dts=case["dts"], hx=case["hx"], hy=case["hy"], land_mask=land_mask,
                  mp=ctx.mevp_default_params(**case["mevp"]))


# ---- 1. the kinds at 70 x 9 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.KIND_CASES, ids=B.case_id)
def test_kind_matches_the_reference_70x9(ctx, key):
    """one sub-iteration of each kind of tests/bbm_cases.py.  icefree: the formula over all nodes (its floor is 1e-13 of the 1.4 m/s of
    the floor-mass nodes), then the nodes with ice once more under the floor of their own maximum"""
    case, ref = B.built(key)
    B.assert_margins(case, ref, B.case_id(key))
    got = device_of(ctx, case).iterate()
    check_against_reference(got, ref)
    if key[0] == "icefree":
        ice = ~B.ice_free_nodes(case, ref)
        assert np.max(np.abs(ref["u"][~ice])) > 2.0 * np.max(np.abs(ref["u"][ice])) > 0.0
        for k in ("u", "v"):
            assert_close(got[k][ice], ref[k][ice], 1e-11, 1e-13 * np.max(np.abs(ref[k][ice])), k + " (ice)")
    else:
        assert np.max(np.abs(ref["u"])) > 1e-5


def test_masked_instantiation_reaches_the_same_branches(ctx):
    """bbm_fused_kernel<true>: the branches case under an all-ocean mask (against the reference, and bit for bit what the unmasked
    instantiation gives) and with the island and the rock of test_gpu_bbm.py, where land stays exactly 0"""
    case, ref = B.built(B.KIND_CASES[0])
    plain = device_of(ctx, case).iterate()
    ocean = device_of(ctx, case, land_mask=np.zeros((9, 70), dtype=bool))
    got = ocean.iterate()
    ocean.close()
    check_against_reference(got, ref)
    assert same(got, plain)
    case, ref = B.built(B.ISLAND_CASE)
    B.assert_margins(case, ref, "island")
    land = case["c"]["land"]
    d = device_of(ctx, case, land_mask=land)
    got = d.iterate(strip_rows=3)
    d.close()
    check_against_reference(got, ref)
    ln = R.land_nodes(land)
    assert np.all(got["u"][ln] == 0.0) and np.all(got["v"][ln] == 0.0)
    assert np.all(got["D"][:, land] == 0.0) and all(np.all(x[:, land] == 0.0) for x in got["S"])


# ---- 2. array widths and heights, automatic strip height ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", B.SHAPE_CASES, ids=B.case_id)
def test_branches_match_the_reference_at_every_seam(ctx, key):
    """a wave owns 63 columns of 64-element tiles: 1 x 1 (lane 1 is the first and the last column, lane 0 recomputes a clamped one), 1 x 5
    (one column), 63 x 3 (one full wave), 64 x 3 (the second wave owns the last column of tile 0), 65 x 3 (its two columns straddle the
    tile seam), 127 x 3 (a third wave of one column), 130 x 5 (three waves, a last tile of two), 190 x 2 (a fourth wave), 130 x 1 (one
    row), 3 x 70 (35 strips of 2 rows)"""
    case, ref = B.built(key)
    B.assert_margins(case, ref, B.case_id(key))
    check_against_reference(device_of(ctx, case).iterate(), ref)


# ---- 3. bit for bit, and nothing outside the rows of a launch -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(130, 5), (3, 70)], ids=["130x5", "3x70"])
def test_strip_heights_and_split_launches_do_not_change_a_bit(ctx, shape):
    case, _ = B.built(B.SHAPE_CASES[B.SHAPES.index(shape)])
    d = device_of(ctx, case)
    base = d.iterate()
    for r in (3, 64):
        assert same(d.iterate(strip_rows=r), base), "strip_rows %d" % r
    if shape == (130, 5):
        for r in (0, 3):
            assert same(d.iterate(ranges=[(0, 0, 3), (2, 3, 5)], strip_rows=r), base), "two launches, strip_rows %d" % r


@pytest.mark.parametrize("rows", [(1, 2, 4), (2, 3, 5)], ids=["1-2-4", "2-3-5"])
def test_a_launch_writes_nothing_outside_its_rows(ctx, rows):
    """130 x 5, outputs filled with NaN, ONE launch (k0, j0, j1): stress and damage keep the NaN on every element row outside [k0, j1) --
    in the tiled stress arrays the padding of the last tile too --, the velocity on every node row outside [2 j0, 2 j1) (and the array's top
    row when j1 is its last); inside, the launch is the reference's iterate(k0, j0, j1)"""
    k0, j0, j1 = rows
    nx, ny = 130, 5
    case, ref = B.built(B.SHAPE_CASES[B.SHAPES.index((nx, ny))])
    c, d = case["c"], device_of(ctx, case)
    nan = lambda t: torch.full_like(t, float("nan"))
    So, Do, un, vn = [nan(x) for x in d.S], nan(d.D), nan(d.u), nan(d.v)
    ctx.bbm_iterate(k0, j0, j1, d.S, So, d.D, Do, (d.u, d.v), (un, vn), d.packed, d.gauss)
    torch.cuda.synchronize()
    g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == ny else 0)
    assert (g0, g1) == {(1, 2, 4): (4, 8), (2, 3, 5): (6, 11)}[rows]
    outside = np.ones(ny, dtype=bool)
    outside[k0:j1] = False
    node_outside = np.ones(2 * ny + 1, dtype=bool)
    node_outside[g0:g1] = False
    for x in So:  # [ny, tiles, 8 * 64]
        assert np.all(np.isnan(host(x)[outside]))
        pad = host(x)[:, -1].reshape(ny, 4, 64, 2)[:, :, nx % 64:]  # coefficient pairs interleaved by element (abi.tile)
        assert np.all(np.isnan(pad)), "padding elements of the last tile"
    assert np.all(np.isnan(host(Do)[:, outside]))
    assert np.all(np.isnan(host(un)[node_outside])) and np.all(np.isnan(host(vn)[node_outside]))
    mp, bp = R.mevp_par(**case["mevp"]), R.bbm_par(**case["bbm"])
    wS, wD, wu, wv = R.iterate(mp, bp, case["hx"], case["hy"], case["dts"], c["S"], c["D"], c["u"], c["v"], ref["gauss"], ref["nod"], k0=k0, j0=j0, j1=j1)
    got = dict(S=[thost(x, nx)[:, k0:j1] for x in So], D=host(Do)[:, k0:j1], u=host(un)[g0:g1], v=host(vn)[g0:g1])
    check_against_reference(got, dict(S=[x[:, k0:j1] for x in wS], D=wD[:, k0:j1], u=wu[g0:g1], v=wv[g0:g1]))


# ---- 4. the launch geometry of 2048 x 2048 ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def bbm_geometry(cus, nx, rows):
    """(R, strips, waves, rounds) of nsdg_bbm_iterate at the automatic strip height: nsdg_march_strip_rows (csrc/mevp_fused.hip) with 63
    owned columns per wave and one wave per SIMD, replicated"""
    ncw, slots = cdiv(nx, 63), 4 * cus
    best, R_ = None, 4
    for r in range(2, 65):
        rounds = cdiv(cdiv(rows, r) * ncw, slots)
        cost = rounds * (r + 1.0) + (1.5 if rounds == 1 else 0.0)
        if best is None or cost < best:
            best, R_ = cost, r
    waves = cdiv(rows, R_) * ncw
    return R_, cdiv(rows, R_), waves, cdiv(waves, slots)


FULL_N, FULL_SEED = 2048, 5


def device_branches_fields(n, seed):
    """the distributions of random_case and branch_damage (tests/bbm_cases.py), drawn on the device from a seeded generator"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    U = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, dtype=torch.float64, device="cuda", generator=g)

    def dg2(lo, hi, wiggle):
        f = U(-wiggle, wiggle, 6, n, n)
        f[0] = U(lo, hi, n, n)
        return f

    sn = U(1.5e3, 3.0e4, n, n) * torch.where(U(0.0, 1.0, n, n) < 0.5, -1.0, 1.0)
    d1, d2 = U(-2e4, 2e4, n, n), U(-2e4, 2e4, n, n)
    S = [U(-50.0, 50.0, 8, n, n) for _ in range(3)]
    S[0][0], S[1][0], S[2][0] = sn + d1, d2, sn - d1
    shape = (2 * n + 1, 2 * n + 1)
    u, v = U(-5e-5, 5e-5, *shape), U(-5e-5, 5e-5, *shape)
    for a in (u, v):
        a[0] = a[-1] = 0.0
        a[:, 0] = a[:, -1] = 0.0
    D = dg2(-0.2, 1.2, 0.01)
    tiny = U(0.0, 1.0, n, n) < 0.1
    D[:, tiny] = 0.0
    D[0][tiny] = B.TINY_DAMAGE
    return dict(nx=n, ny=n, S=S, u=u, v=v, H=dg2(0.35, 1.9, 0.01), A=dg2(0.72, 0.98, 0.004), D=D, ua=U(-10.0, 10.0, *shape), va=U(-10.0, 10.0, *shape),
                uo=U(-0.05, 0.05, *shape), vo=U(-0.05, 0.05, *shape), land=None)


def test_launch_geometry_of_2048x2048_matches_the_reference_on_slabs(ctx):
    """2048 x 2048, the size tools/bbm_timing.py times, on inputs of the branches recipe drawn on the device.  Automatic strip height
    (256 CUs, 33 column-waves against 1024 resident waves): R = 34, 61 strips (the last of 8 rows), 2013 waves, 2 rounds.  That launch,
    strip_rows = 3 and strip_rows = 64 agree bit for bit in every output, and the first equals the reference on three slabs of whole rows
    -- [0, 8), [58, 72) (strip seams 60, 63, 66, 69 of height 3, 64 of height 64, 68 of height 34) and the last 8 rows (the short last
    strip) --, each evaluated as a local array of its own with one margin row dropped on every side that is not the physical boundary
    (tests/test_bbm_cpu.py::test_a_slab_of_whole_rows_reproduces_the_full_reference_bitwise).  The margins are asserted on each slab"""
    n = FULL_N
    if ctx.num_cus() == 256:
        assert bbm_geometry(256, n, n) == (34, 61, 2013, 2)
    case = B.recipe("branches", device_branches_fields(n, FULL_SEED))
    d = device_of(ctx, case)

    def launch(strip_rows):  # as Device.iterate, but nothing travels to the host
        ctx.set_mevp_strip_rows(strip_rows)
        out = [torch.zeros_like(x) for x in d.S] + [torch.zeros_like(d.D), torch.full_like(d.u, 3.0), torch.full_like(d.v, 3.0)]
        ctx.bbm_iterate(0, 0, n, d.S, out[:3], d.D, out[3], (d.u, d.v), (out[4], out[5]), d.packed, d.gauss)
        ctx.set_mevp_strip_rows(0)
        torch.cuda.synchronize()
        return out

    base = launch(0)
    for r in (3, 64):
        other = launch(r)
        assert all(torch.equal(x, y) for x, y in zip(other, base)), "strip_rows %d" % r
        del other
    got_all = dict(S=base[:3], D=base[3], u=base[4], v=base[5])
    for r0, r1 in ((0, 8), (58, 72), (n - 8, n)):
        local = B.slab(case["c"], r0, r1)
        local = {k: [x.cpu().numpy() for x in v] if k == "S" else v.cpu().numpy() if torch.is_tensor(v) else v for k, v in local.items()}
        part = dict(case, c=local)
        ref = B.case_reference(part)
        B.assert_margins(part, ref, "rows [%d, %d)" % (r0, r1))
        e0, e1, n0, n1 = B.slab_interior(r0, r1, n)
        want = dict(S=[x[:, e0:e1] for x in ref["S"]], D=ref["D"][:, e0:e1], u=ref["u"][n0:n1], v=ref["v"][n0:n1])
        got = dict(S=[thost(x[r0 + e0:r0 + e1], n) for x in got_all["S"]], D=host(got_all["D"][:, r0 + e0:r0 + e1]),
                   u=host(got_all["u"][2 * r0 + n0:2 * r0 + n1]), v=host(got_all["v"][2 * r0 + n0:2 * r0 + n1]))
        assert np.max(np.abs(want["u"])) > 1e-5
        check_against_reference(got, want)
    del d, base, got_all, case
    gc.collect()
    torch.cuda.empty_cache()

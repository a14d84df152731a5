"""The snow load on the device (include/nsdg_snow.h): the SNOW instantiations of the two packing kernels against
the ones without a field by the header's substitution (bit for bit), fused against unfused, no change without a load, the diagnostic h'
against its numpy restatement, the sub-cycles of both rheologies against the CPU reference (tests/snow_ref.py) at the limits of
tests/test_gpu_parity.py and tests/test_gpu_bbm.py -- and far from the reference WITHOUT the load --, the free drift of the loaded mass,
the driver's block / graph / native / sub-step / restart equalities, and the misuse reports.

The packing shapes are 70 x 5 and 3 x 2.  At 70 x 5 the lattice is 141 x 11 nodes: three prepare workgroups in x and three in y, the last
of each partial, with tile seams at node columns 64 and 128 and node rows 4 and 8.  3 x 2 has no interior seam."""
import numpy as np
import pytest
import torch

import basal_ref as BR
import land_ref
import oracle_lib as O
import snow_ref as SR
from nextsimdg_amd import abi, rowblock, synthetic
from test_gpu_land import AD, FORMS, UNIFORM, mask_dev, report
from test_gpu_parity import Box, dev, host, tdev, thost
from thread_ranks import fields, gather, run_world

pytestmark = pytest.mark.gpu
PACK_SHAPES = [(70, 5), (3, 2)]
RHO = 330.0


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
    if ctx.nx:
        ctx.set_land_mask(None)
        ctx.set_basal_depth(None)
        ctx.set_snow_load(None)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


def pack_mask(nx, ny):
    """an island across the tile seam at node column 64 (elements 30..33) and a rock; 3 x 2: one land element"""
    land = np.zeros((ny, nx), dtype=bool)
    if nx >= 70:
        land[1:4, 30:34] = True
        land[ny - 1, 3] = True
    else:
        land[0, nx - 1] = True
    return land


class PackCase:
    """a Box whose cover holds open water, thin ice under deep snow and, in the snow, negative coefficients"""

    def __init__(self, ctx, nx, ny, nc, masked, seed=9):
        self.b = b = Box(ctx, nx, ny)
        self.nx, self.ny, self.nc = nx, ny, nc
        rng = np.random.default_rng(seed)
        snow = np.zeros((nc, ny, nx))
        snow[0] = 0.5 * rng.random((ny, nx))
        snow[1:] = 0.05 * rng.standard_normal((nc - 1, ny, nx))
        self.land = pack_mask(nx, ny) if masked else None
        if nx >= 70:
            b.H[:, :, 5:9] = 0.0  # open water
            b.A[:, :, 5:9] = 0.0
            b.H[:, 1:4, 44:50] = 0.0  # thin ice (H / A below min_thick) under deep snow: ice-free, h' unchanged
            b.H[0, 1:4, 44:50] = 0.004
            snow[0, 1:4, 44:50] = 2.0
            snow[0, :, 60:68] = -0.2  # negative snow: the clamp takes it (across the seam at node column 128)
        else:
            b.H[:, 0, 0] = 0.0
            b.A[:, 0, 0] = 0.0
            snow[0, 0, 0] = 0.4  # snow on the open water
            snow[0, 1, 1] = -0.2
        if masked:
            b.H[:, self.land] = 0.0
            b.A[:, self.land] = 0.0
        self.snow = snow
        shape = (2 * ny + 1, 2 * nx + 1)
        self.u0, self.v0 = 0.05 * rng.standard_normal(shape), 0.05 * rng.standard_normal(shape)
        z = lambda: torch.zeros(shape, dtype=torch.float64, device="cuda")
        self.d = d = {k: dev(getattr(b, k)) for k in ("H", "A", "ua", "va", "uo", "vo")}
        d.update(u0=dev(self.u0), v0=dev(self.v0), snow=dev(snow if nc > 1 else snow[0]), cgh=z(), cga=z(), cgs=z(), tax=z(), tay=z())
        ctx.set_land_mask(mask_dev(self.land) if masked else None)
        ctx.dg_to_cg(d["H"], d["cgh"])
        ctx.dg_to_cg(d["A"], d["cga"])
        ctx.dg_to_cg(dev(snow), d["cgs"])
        ctx.wind_stress(d["ua"], d["va"], d["tax"], d["tay"])
        torch.cuda.synchronize()
        self.cgh, self.cga, self.cgs = host(d["cgh"]), host(d["cga"]), host(d["cgs"])
        self.n = self.cgh.size

    def pack_nodal(self, ctx, cgh=None, fill=-3.0):
        d = self.d
        packed = torch.full((8 * self.n,), fill, dtype=torch.float64, device="cuda")
        ctx.mevp_pack_nodal(120.0, (d["u0"], d["v0"]), (d["tax"], d["tay"]), (d["uo"], d["vo"]), d["cgh"] if cgh is None else cgh, d["cga"], packed)
        torch.cuda.synchronize()
        return packed

    def prepare(self, ctx, fill=-3.0):
        d = self.d
        packed = torch.full((8 * self.n,), fill, dtype=torch.float64, device="cuda")
        ctx.mevp_prepare(120.0, d["H"], d["A"], (d["ua"], d["va"]), (d["uo"], d["vo"]), (d["u0"], d["v0"]), packed)
        torch.cuda.synchronize()
        return packed


# ------------------------------------------------------------------------------------------------ 1. the substitution
@pytest.mark.parametrize("masked", [False, True], ids=["ocean", "island"])
@pytest.mark.parametrize("nc", [1, 3, 6])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["70x5", "3x2"])
def test_packing_with_a_field_equals_packing_without_one_from_the_loaded_thickness(ctx, shape, nc, masked):
    """nsdg_mevp_pack_nodal with a snow field == nsdg_mevp_pack_nodal without one from cgH_ref, built in numpy (snow_ref.loaded_thickness)
    from the device's own nsdg_dg_to_cg results: all eight planes, bit for bit"""
    c = PackCase(ctx, *shape, nc, masked)
    po = c.b.po
    ctx.set_snow_load(c.d["snow"], RHO)
    with_field = c.pack_nodal(ctx)
    ctx.set_snow_load(None)
    href = SR.loaded_thickness(po, RHO, c.cgh, c.cga, c.cgs)
    from_ref = c.pack_nodal(ctx, dev(href))
    bare = c.pack_nodal(ctx)
    assert torch.equal(with_field, from_ref)
    assert not torch.equal(with_field, bare)  # the load is felt
    free = BR.ice_free(po, c.cgh, c.cga)
    ln = land_ref.land_nodes(c.land) if masked else np.zeros(free.shape, dtype=bool)
    c0 = lambda p: p.view(4, c.n, 2)[0, :, 0].cpu().numpy().reshape(free.shape)
    # open water, thin ice under deep snow (ice-free whatever lies on it: h' unchanged) and clamped negative snow are all in the state
    assert (free & (c.cgs > 0.1)).sum() >= 1 and np.array_equal(c0(with_field)[free], c0(bare)[free])
    loaded = ~free & ~ln & (c.cgs > 0)
    assert loaded.sum() >= 3 and np.all(c0(with_field)[loaded] > c0(bare)[loaded])
    clamped = ~free & ~ln & (c.cgs < 0)
    assert clamped.sum() >= 1 and np.array_equal(c0(with_field)[clamped], c0(bare)[clamped])
    if masked:
        assert ln.sum() >= 9 and np.all(c0(with_field)[ln] == po.h_min)


# ------------------------------------------------------------------------------------------------ 2. fused against unfused
@pytest.mark.parametrize("depth", [False, True], ids=["deep", "shoal"])
@pytest.mark.parametrize("masked", [False, True], ids=["ocean", "island"])
@pytest.mark.parametrize("nc", [1, 3, 6])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["70x5", "3x2"])
def test_prepare_equals_the_separate_kernels_under_a_snow_load(ctx, shape, nc, masked, depth):
    """nsdg_mevp_prepare == nsdg_dg_to_cg (H, A; the packing forms the snow's mean as the third) + nsdg_wind_stress +
    nsdg_mevp_pack_nodal: all eight planes bit for bit, in all four combinations of mask and depth array"""
    c = PackCase(ctx, *shape, nc, masked)
    if depth:
        ctx.set_basal_depth(dev(np.random.default_rng(4).uniform(0.05, 3.0, (c.ny, c.nx))))
    ctx.set_snow_load(c.d["snow"], RHO)
    fused, unfused = c.prepare(ctx), c.pack_nodal(ctx)
    assert torch.equal(fused, unfused)
    pairs = fused.view(4, c.n, 2)
    assert not bool((pairs[:3] == -3.0).any()) and bool((pairs[3] == -3.0).all()) != depth
    ctx.set_snow_load(None)
    bare = c.prepare(ctx)
    assert not torch.equal(bare, fused) and torch.equal(bare.view(4, c.n, 2)[3], pairs[3])  # T_b reads the ice alone
    if depth:
        assert float(pairs[3, :, 0].max()) > 0.0


# ------------------------------------------------------------------------------------------------ 3. no load, no change
@pytest.mark.parametrize("masked", [False, True], ids=["ocean", "island"])
@pytest.mark.parametrize("nc", [1, 6])
def test_no_load_means_no_change(ctx, gpu, nc, masked):
    """zero snow, snow <= 0 everywhere, rho_snow = 0 and a field set and then cleared each pack what a context that never had a field packs"""
    c = PackCase(ctx, 70, 5, nc, masked)
    fresh = abi.Context(gpu)
    fresh.set_grid(c.nx, c.ny, c.b.bt.hx, c.b.bt.hy)
    fresh.set_land_mask(mask_dev(c.land) if masked else None)
    want = c.prepare(fresh), c.pack_nodal(fresh)
    fresh.close()
    snow = c.d["snow"]
    negative = torch.zeros_like(snow)  # cell means <= 0 and no slopes: <= 0 at every node
    negative.view(-1, c.ny, c.nx)[0] = -snow.view(-1, c.ny, c.nx)[0].abs()
    for name, field, rho in (("zero snow", torch.zeros_like(snow), RHO), ("negative snow", negative, RHO), ("rho_snow = 0", snow, 0.0)):
        ctx.set_snow_load(field, rho)
        assert torch.equal(c.prepare(ctx), want[0]) and torch.equal(c.pack_nodal(ctx), want[1]), name
    ctx.set_snow_load(snow, RHO)
    assert not torch.equal(c.prepare(ctx), want[0])
    ctx.set_snow_load(None)
    assert torch.equal(c.prepare(ctx), want[0]) and torch.equal(c.pack_nodal(ctx), want[1])


# ------------------------------------------------------------------------------------------------ 4. the diagnostic
@pytest.mark.parametrize("masked", [False, True], ids=["ocean", "island"])
@pytest.mark.parametrize("nc", [1, 3, 6])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=["70x5", "3x2"])
def test_snow_load_nodal_equals_its_numpy_restatement_and_the_packing(ctx, shape, nc, masked):
    """max, one product and one sum: bit for bit; and it is the c[0] the packing stores, before the 2^100 scaling of an ice-free node"""
    c = PackCase(ctx, *shape, nc, masked)
    ctx.set_snow_load(c.d["snow"], RHO)
    out = torch.full_like(c.d["cgh"], -3.0)
    ctx.snow_load_nodal(c.d["cgh"], c.d["cga"], out)
    want = SR.load_nodal(c.b.po, RHO, c.cgh, c.cga, c.cgs, c.land)
    assert np.array_equal(host(out), want)
    c0 = c.pack_nodal(ctx).view(4, c.n, 2)[0, :, 0].cpu().numpy().reshape(want.shape)
    free = BR.ice_free(c.b.po, c.cgh, c.cga)
    if masked:
        free &= ~land_ref.land_nodes(c.land)
    assert np.array_equal(c0, np.where(free, 2.0 ** 100 * want, want))


# ------------------------------------------------------------------------------------------------ 5. the sub-cycles against snow_ref
NXS, NYS = 130, 5
KIND = {"uniform": "plastic", "adaptive": "ad_spread"}  # tests/mevp_cases.py: the mEVP family's inputs (alpha != beta; a spread of alpha_e)


def family_snow(nx=NXS, ny=NYS, seed=21):
    """0.1 .. 0.5 m of snow with small slopes, negative in one corner"""
    rng = np.random.default_rng(seed)
    snow = np.zeros((6, ny, nx))
    snow[0] = rng.uniform(0.1, 0.5, (ny, nx))
    snow[1:3] = 0.02 * rng.standard_normal((2, ny, nx))
    snow[0, :2, :3] = -0.1
    return snow


def far_from(what, got, bare, rtol, atol, factor=100.0):
    worst = float(np.max(np.abs(got - bare) / (atol + rtol * np.abs(bare))))
    print("%s: %.3g limits away from the reference WITHOUT the load" % (what, worst))
    assert worst > factor, what


def oracle_steps(case, po, n, snow):
    """n whole-array sub-iterations of the oracle from the case's state; snow: the DG field whose load the nodal thickness carries
    (snow_ref.loaded_thickness), or None.  Returns (u, v, [s11, s12, s22])"""
    c, nx, ny, hx, hy, dt = case["c"], case["c"]["nx"], case["c"]["ny"], case["hx"], case["hy"], case["dt"]
    pg, cgh, cga = O.ice_strength(nx, ny, po, c["H"], c["A"]), O.dg_to_cg(nx, ny, c["H"]), O.dg_to_cg(nx, ny, c["A"])
    tau = O.wind_stress(po, c["ua"], c["va"])
    if snow is not None:
        cgh = SR.loaded_thickness(po, RHO, cgh, cga, SR.nodal_snow(nx, ny, snow))
    ad = po.aevp_c > 0
    alpha_e = np.zeros((ny, nx)) if ad else None
    u, v, s = c["u"].copy(), c["v"].copy(), [x.copy() for x in c["S"]]
    for _ in range(n):
        O.mevp_stress(nx, ny, 0, ny, hx, hy, po, u, v, pg, *s, **(dict(dt=dt, cgh=cgh, cga=cga, alpha_e=alpha_e) if ad else {}))
        un, vn = np.zeros_like(u), np.zeros_like(v)
        O.mevp_velocity(nx, ny, 0, ny, hx, hy, dt, po, s, (u, v), (un, vn), (c["u0"], c["v0"]), tau, (c["uo"], c["vo"]), cgh, cga,
                        **(dict(alpha_e=alpha_e) if ad else {}))
        u, v = un, vn
    return u, v, s


@pytest.fixture(scope="module")
def family_reference():
    """per form: the case of tests/mevp_cases.py at 130 x 5 and the oracle's one and four sub-iterations on cgH_ref and on cgH: computed
    once, shared, left unchanged"""
    import mevp_cases as Mc

    out = {}
    for form, kind in KIND.items():
        case = Mc.built(Mc.shape_case(kind, NXS, NYS))[0]
        po = O.mevp_params(**case["par"])
        out[form] = {(key, n): oracle_steps(case, po, n, snow) for n in (1, 4) for key, snow in (("loaded", family_snow()), ("bare", None))}
        out[form].update(case=case, po=po)
    return out


def device_steps(ctx, case, variant, n, snow):
    """nsdg_mevp_prepare under the snow field and one pass of n = 1 or 4 sub-iterations from the case's state: (u, v, [s]) on the host"""
    c, nx, ny = case["c"], case["c"]["nx"], case["c"]["ny"]
    ctx.set_mevp_variant(variant)
    ctx.set_mevp_params(ctx.mevp_default_params(**case["par"]))
    ctx.set_grid(nx, ny, case["hx"], case["hy"])
    H, A = dev(c["H"]), dev(c["A"])
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(H, A, pg)
    du, dv = dev(c["u"]), dev(c["v"])
    ds, dso = [tdev(x) for x in c["S"]], [tdev(np.zeros_like(x)) for x in c["S"]]
    dun, dvn = torch.full_like(du, 3.0), torch.full_like(dv, 3.0)
    packed = torch.zeros(8 * du.numel(), dtype=torch.float64, device="cuda")
    ctx.set_snow_load(snow, RHO)
    ctx.mevp_prepare(case["dt"], H, A, (dev(c["ua"]), dev(c["va"])), (dev(c["uo"]), dev(c["vo"])), (dev(c["u0"]), dev(c["v0"])), packed)
    if n == 1:
        ctx.mevp_iterate(0, 0, ny, ds, dso, (du, dv), (dun, dvn), packed, pg)
    else:
        ctx.mevp_iterate4(0, ny, ds, dso, (du, dv), (dun, dvn), packed, pg)
    torch.cuda.synchronize()
    ctx.set_snow_load(None)
    return host(dun), host(dvn), [thost(x, nx) for x in dso], (dun, dvn, dso)


@pytest.mark.parametrize("variant,form", [(0, "uniform"), (1, "uniform"), (4, "uniform"), (1, "adaptive"), (4, "adaptive")])
def test_sub_iterations_under_a_snow_load_match_the_reference_and_not_the_one_without_it(ctx, family_reference, variant, form):
    """130 x 5, across the passes' 64-column seams, after an nsdg_mevp_prepare that saw the DG snow field, against the oracle on cgH_ref.
    Variants 0 and 1: one sub-iteration at the limits of test_gpu_parity.test_mevp_single_iteration_matches_oracle (stress 1e-12 and 1e-12
    of the largest value, velocity 1e-11 and 1e-13); variant 4: one pass of four at the limits of
    test_gpu_parity.test_mevp_four_iterations_per_pass_equals_four_single_passes_bitwise's comparison with the oracle (1e-10 and 1e-12).
    Each is more than 100 of its limits away from the oracle on cgH.  This is the test that fails without the feature"""
    ref = family_reference[form]
    n = 4 if variant == 4 else 1
    (srel, sabs), (vrel, vabs) = ((1e-12, 1e-12), (1e-11, 1e-13)) if n == 1 else ((1e-10, 1e-12), (1e-10, 1e-12))
    u, v, s, _ = device_steps(ctx, ref["case"], variant, n, dev(family_snow()))
    (wu, wv, ws), (bu, bv, _) = ref[("loaded", n)], ref[("bare", n)]
    assert np.max(np.abs(wu)) > 1e-4
    for got, want, name in zip(s, ws, ("s11", "s12", "s22")):
        report(name, got, want, srel, sabs * np.max(np.abs(want)))
    report("u_new", u, wu, vrel, vabs * np.max(np.abs(wu)))
    report("v_new", v, wv, vrel, vabs * np.max(np.abs(wv)))
    far_from("u", u, bu, vrel, vabs * np.max(np.abs(bu)))
    far_from("v", v, bv, vrel, vabs * np.max(np.abs(bv)))


@pytest.mark.parametrize("form", ["uniform", "adaptive"])
def test_passes_of_one_to_four_agree_bit_for_bit_under_a_snow_load(ctx, family_reference, form):
    """12 sub-iterations through nsdg_mevp_subcycle (which packs with nsdg_mevp_pack_nodal) as passes of 1, 2, 3 and 4"""
    case = family_reference[form]["case"]
    c, nx, ny = case["c"], NXS, NYS
    res = {}
    for variant in (1, 2, 3, 4):
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_params(ctx.mevp_default_params(**case["par"]))
        ctx.set_grid(nx, ny, case["hx"], case["hy"])
        H, A = dev(c["H"]), dev(c["A"])
        z = lambda: torch.zeros_like(dev(c["u"]))
        cgh, cga, tax, tay = z(), z(), z(), z()
        pg = ctx.private_zeros(9, ny, nx, "cuda")
        ctx.ice_strength(H, A, pg)
        ctx.dg_to_cg(H, cgh)
        ctx.dg_to_cg(A, cga)
        ctx.wind_stress(dev(c["ua"]), dev(c["va"]), tax, tay)
        du, dv, ds = dev(c["u"]), dev(c["v"]), [tdev(x) for x in c["S"]]
        scratch = torch.zeros(10 * du.numel() + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
        ctx.set_snow_load(dev(family_snow()), RHO)
        ctx.mevp_subcycle(case["dt"], 12, ds, du, dv, dev(c["u0"]), dev(c["v0"]), tax, tay, dev(c["uo"]), dev(c["vo"]), cgh, cga, pg, scratch)
        torch.cuda.synchronize()
        ctx.set_snow_load(None)
        res[variant] = [du, dv] + ds
    assert float(res[1][0].abs().max()) > 1e-4
    for variant in (2, 3, 4):
        assert all(torch.equal(x, y) for x, y in zip(res[1], res[variant])), variant


def test_brittle_sub_iteration_under_a_snow_load_matches_the_reference_and_not_the_one_without_it(ctx):
    """nsdg_bbm_iterate on 130 x 5 after a packing that saw the plane hsnow, against tests/bbm_ref.py from cgH_ref at the limits of
    tests/test_gpu_bbm.py (1e-11 relative, 1e-13 of the largest value)"""
    import bbm_ref as R
    import test_gpu_bbm as GB

    c = GB.random_case(NXS, NYS)
    snow = family_snow()[0]
    mp, bp = R.mevp_par(), R.bbm_par()
    gauss = R.prepare(mp, bp, c["H"], c["A"])
    nod = R.nodal_fields(mp, c["H"], c["A"], c["ua"], c["va"], c["uo"], c["vo"])
    bare = R.iterate(mp, bp, GB.HX, GB.HY, GB.DTS, c["S"], c["D"], c["u"], c["v"], gauss, nod)
    nod = dict(nod, cgh=SR.loaded_thickness(mp, RHO, nod["cgh"], nod["cga"], SR.nodal_snow(NXS, NYS, snow)))
    So, Do, un, vn = R.iterate(mp, bp, GB.HX, GB.HY, GB.DTS, c["S"], c["D"], c["u"], c["v"], gauss, nod)
    d = GB.Device(ctx, c)
    ctx.set_snow_load(dev(snow), RHO)
    zero = torch.zeros_like(d.u)
    ctx.mevp_prepare(GB.DTS, d.H, d.A, (dev(c["ua"]), dev(c["va"])), (dev(c["uo"]), dev(c["vo"])), (zero, zero), d.packed)
    got = d.iterate()
    d.close()
    GB.check_against_reference(got, dict(S=So, D=Do, u=un, v=vn))
    far_from("brittle u", got["u"], bare[2], 1e-11, 1e-13 * np.max(np.abs(bare[2])))
    far_from("brittle v", got["v"], bare[3], 1e-11, 1e-13 * np.max(np.abs(bare[3])))


# ------------------------------------------------------------------------------------------------ 6. free drift
def test_device_strengthless_cover_under_snow_reaches_the_free_drift_of_the_loaded_mass(ctx):
    """the device twin of tests/test_snow_cpu.py's free-drift test (and of test_gpu_parity's, whose shape, steps and 1e-10 it keeps):
    0.3 m of snow on 0.7 m of ice drifts as scipy's solution for m = rho_i h + rho_s s says"""
    from test_oracle_dynamics import free_drift_case, free_drift_solution

    nx, ny = 70, 9
    hx, hy, ua, va, uo, vo, cgh, cga = free_drift_case(nx, ny)
    pk = dict(pstar=0.0, alpha=5.0, beta=5.0)
    ctx.set_mevp_params(ctx.mevp_default_params(**pk))
    ctx.set_grid(nx, ny, hx, hy)
    po = O.mevp_params(**pk)
    tax, tay = torch.zeros_like(dev(ua)), torch.zeros_like(dev(ua))
    ctx.wind_stress(dev(ua), dev(va), tax, tay)
    u, v = torch.zeros_like(tax), torch.zeros_like(tax)
    s = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    scratch = torch.zeros(10 * u.numel() + 3 * s[0].numel(), dtype=torch.float64, device="cuda")
    duo, dvo, dh, da = dev(uo), dev(vo), dev(cgh), dev(cga)
    ctx.set_snow_load(torch.full((ny, nx), 0.3, dtype=torch.float64, device="cuda"), RHO)
    for _ in range(70):
        ctx.mevp_subcycle(600.0, 30, s, u, v, u.clone(), v.clone(), tax, tay, duo, dvo, dh, da, pg, scratch)
    want = free_drift_solution(po, 9.0, -4.0, 0.05, 0.02, (po.rho_ice * 0.7 + RHO * 0.3) / po.rho_ice, 0.85)
    bare = free_drift_solution(po, 9.0, -4.0, 0.05, 0.02, 0.7, 0.85)
    ui, vi = host(u)[1:-1, 1:-1], host(v)[1:-1, 1:-1]
    assert np.max(np.abs(ui - want[0])) < 1e-10 and np.max(np.abs(vi - want[1])) < 1e-10
    assert np.min(np.abs(ui - bare[0])) > 1e-3 and np.min(np.abs(vi - bare[1])) > 1e-3


# ------------------------------------------------------------------------------------------------ 7. the driver
NXF, NYF = 150, 128


def thick_fields(nx, ny):
    """thread_ranks.fields under the thick cover of tests/basal_ref.py (H ~ 2 m, A ~ 0.95), on which the adaptive form is stable at these
    sub-iteration counts"""
    bt, H, A, uo, vo, ua, va = fields(nx, ny)
    BR.thick_cover(H, A)
    return bt, H, A, uo, vo, ua, va


def driver_column(nx=NXF, ny=NYF):
    """the column planes of thread_ranks.run_rank with a snow field that varies across the boundaries of four row blocks (32, 64, 96)"""
    st, fo, _ = synthetic.column_fields(nx * ny, 5)
    column = {k: v.reshape(ny, nx) for k, v in {**st, **fo}.items()}
    column["wind"] = 0.2 * column["wind"]
    rng = np.random.default_rng(31)
    column["hsnow"] = 0.4 * rng.random((ny, nx)) * (1.0 + np.sin(np.arange(ny) * 0.2))[:, None]
    return column


KEYS = ("H", "A", "u", "v", "s11", "hsnow", "tice0")


@pytest.mark.parametrize("advect", [False, True], ids=["plane", "S"])
@pytest.mark.parametrize("pk", FORMS)
def test_one_block_equals_four_blocks_and_graphs_equal_no_graphs_under_a_snow_load(gpu, pk, advect):
    kw = dict(alpha=pk, core_kw=dict(snow_load=True, advect_column_state=advect), transport="native", native=True, column=driver_column(),
              data=thick_fields(NXF, NYF))
    ref = run_world(1, 4, True, NXF, NYF, 21, 3, **kw)[0]
    bare = run_world(1, 4, True, NXF, NYF, 21, 3, **dict(kw, core_kw=dict(advect_column_state=advect)))[0]
    assert float(ref["u"].abs().max()) > 1e-5 and float(ref["hsnow"].max()) > 0.05 and not torch.equal(ref["u"], bare["u"])
    assert all(bool(torch.isfinite(ref[k]).all()) for k in KEYS)
    for world, graph in ((4, False), (1, True), (4, True)):
        parts = run_world(world, 4, True, NXF, NYF, 21, 3, group=2, use_graph=graph, **kw)
        for key in KEYS:
            assert torch.equal(gather(parts, world, key), ref[key]), (key, world, graph)


@pytest.mark.parametrize("advect", [False, True], ids=["plane", "S"])
def test_native_equals_the_python_sequence_under_a_snow_load(gpu, advect):
    kw = dict(alpha=AD, core_kw=dict(snow_load=True, advect_column_state=advect), column=driver_column(), data=thick_fields(NXF, NYF))
    python = run_world(1, 4, True, NXF, NYF, 21, 2, **kw)[0]
    native = run_world(1, 4, True, NXF, NYF, 21, 2, transport="native", native=True, **kw)[0]
    assert float(python["u"].abs().max()) > 1e-5
    for key in KEYS:
        assert torch.equal(native[key], python[key]), key


def coupled_core(c, dt, nsub, advect, rheology="mevp", nx=NXF, ny=64, **kw):
    bt, H, A, uo, vo, ua, va = thick_fields(nx, ny)
    if rheology == "mevp":
        c.set_mevp_params(c.mevp_default_params(**AD))
    core = rowblock.CoupledCore(c, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, dt, nsub, torch.device("cuda"), native=True, snow_load=True,
                                advect_column_state=advect, rheology=rheology, **kw)
    core.load_global(H, A, uo, vo, ua, va)
    core.load_column(driver_column(nx, ny))
    return core


def full_state(core):
    torch.cuda.synchronize()
    out = {k: getattr(core, k).clone() for k in ("H", "A", "u", "v")}
    out.update(s11=core.s[0].clone(), hsnow=core.col["hsnow"].clone(), tice0=core.col["tice0"].clone())
    return out


@pytest.mark.parametrize("advect", [False, True], ids=["plane", "S"])
def test_substeps_and_restart_under_a_snow_load(gpu, advect):
    """advance(substeps=2) == two steps of half the length; 4 steps == 2 steps + state_dict + 2 steps: the snow is in the state already"""
    c = abi.Context(gpu)
    try:
        a = coupled_core(c, 240.0, 16, advect)
        a.advance(240.0, substeps=2)
        got = full_state(a)
        a.close()
        b = coupled_core(c, 120.0, 16, advect)
        b.step()
        b.step()
        want = full_state(b)
        assert float(want["u"].abs().max()) > 1e-5
        for k in want:
            assert torch.equal(got[k], want[k]), ("substeps", k)
        st = b.state_dict()  # (the owned rows of the one block: the whole domain)
        col = {k: v.clone() for k, v in b.col.items()}
        b.step()
        b.step()
        four = full_state(b)
        b.close()
        r = coupled_core(c, 120.0, 16, advect)
        r.load_state_dict(st)
        for k, v in col.items():  # the column planes a restart file carries beside the dynamics' state
            if not (advect and k == "hsnow"):
                r.col[k].copy_(v)
        r.time = 2 * 120.0
        r.step()
        r.step()
        again = full_state(r)
        r.close()
        for k in four:
            assert torch.equal(again[k], four[k]), ("restart", k)
        assert c.snow_load is None  # close() took the field off the context
    finally:
        c.close()


def test_brittle_driver_feels_the_load_and_native_equals_python(gpu):
    res = {}
    for name, kw in (("native", dict()), ("python", dict(native=False)), ("bare", dict(snow_load=False))):
        c = abi.Context(gpu)
        try:
            bt, H, A, uo, vo, ua, va = fields(70, 24)
            args = dict(native=True, snow_load=True, rheology="bbm")
            args.update(kw)
            core = rowblock.CoupledCore(c, rowblock.RowBlock(70, 24), bt.hx, bt.hy, 8.0, 8, torch.device("cuda"), **args)
            core.load_global(H, A, uo, vo, ua, va)
            core.load_column(driver_column(70, 24))
            core.step()
            core.step()
            res[name] = full_state(core)
            core.close()
        finally:
            c.close()
    assert float(res["native"]["u"].abs().max()) > 1e-7 and not torch.equal(res["native"]["u"], res["bare"]["u"])
    for k in res["native"]:
        assert torch.equal(res["native"][k], res["python"][k]), k


# ------------------------------------------------------------------------------------------------ 8. misuse
def test_snow_calls_report_misuse_and_launch_nothing(gpu):
    c = abi.Context(gpu)
    lib = c.lib
    f = torch.zeros(17, 17, dtype=torch.float64, device="cuda")
    s = torch.zeros(6, 8, 8, dtype=torch.float64, device="cuda")
    s[0] = 0.3
    assert lib.nsdg_snow_load_set(c.h, s.data_ptr(), 6, 330.0) == -3 and b"nsdg_grid_set" in lib.nsdg_last_error()  # NSDG_ERR_STATE
    assert lib.nsdg_snow_load_set(c.h, None, 6, 330.0) == -3
    assert lib.nsdg_snow_load_nodal(c.h, f.data_ptr(), f.data_ptr(), f.data_ptr()) == -3
    c.set_grid(8, 8, 1e3, 1e3)
    out = torch.full_like(f, -3.0)
    assert lib.nsdg_snow_load_nodal(c.h, f.data_ptr(), f.data_ptr(), out.data_ptr()) == -3 and b"nsdg_snow_load_set" in lib.nsdg_last_error()
    for ncoef in (0, 2, 4, 5, 7, -1):
        assert lib.nsdg_snow_load_set(c.h, s.data_ptr(), ncoef, 330.0) == -1, ncoef  # NSDG_ERR_ARG
    for rho in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert lib.nsdg_snow_load_set(c.h, s.data_ptr(), 6, rho) == -1, rho
    # nothing changed: there is still no field
    assert lib.nsdg_snow_load_nodal(c.h, f.data_ptr(), f.data_ptr(), out.data_ptr()) == -3
    c.set_snow_load(s)  # the wrapper keeps the tensor
    assert lib.nsdg_snow_load_set(c.h, s.data_ptr(), 2, 330.0) == -1 and lib.nsdg_snow_load_set(c.h, s.data_ptr(), 6, -1.0) == -1
    for args in ((None, f.data_ptr(), out.data_ptr()), (f.data_ptr(), None, out.data_ptr()), (f.data_ptr(), f.data_ptr(), None)):
        assert lib.nsdg_snow_load_nodal(c.h, *args) == -1
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())  # none of the refused calls launched
    f.fill_(1.0)
    c.snow_load_nodal(f, torch.ones_like(f), out)  # the refused sets changed nothing: 0.3 m of snow at 330 kg m^-3
    assert bool((out == 1.0 + (330.0 / c.mevp_default_params().rho_ice) * 0.3).all())
    c.set_snow_load(None, rho_snow=float("nan"))  # NULL clears; ncoef and rho_snow are then ignored
    assert lib.nsdg_snow_load_nodal(c.h, f.data_ptr(), f.data_ptr(), out.data_ptr()) == -3
    # a field that overlaps packed is refused at the packing call, with nothing launched
    n = f.numel()
    packed = torch.full((8 * n + 6 * 64,), -3.0, dtype=torch.float64, device="cuda")
    z = torch.zeros_like(f)
    H = torch.full((6, 8, 8), 0.5, dtype=torch.float64, device="cuda")
    for off in (0, 8 * n - 2):  # inside, and straddling the end (16-byte aligned: the 8 n doubles of packed end at 8 n)
        inside = packed[off:off + 6 * 64].view(6, 8, 8)
        c.set_snow_load(inside)
        with pytest.raises(abi.NsdgError, match="overlaps packed"):
            c.mevp_prepare(120.0, H, H, (z, z), (z, z), (z, z), packed)
        with pytest.raises(abi.NsdgError, match="overlaps packed"):
            c.mevp_pack_nodal(120.0, (z, z), (z, z), (z, z), f, f, packed)
    torch.cuda.synchronize()
    assert bool((packed == -3.0).all())
    c.set_snow_load(packed[8 * n:8 * n + 6 * 64].view(6, 8, 8))  # right behind packed: no overlap
    c.mevp_prepare(120.0, H, H, (z, z), (z, z), (z, z), packed)
    # the wrapper's own checks
    with pytest.raises(abi.NsdgError):
        c.set_snow_load(torch.zeros(8, 7, dtype=torch.float64, device="cuda"))
    with pytest.raises(abi.NsdgError):
        c.set_snow_load(torch.zeros(2, 8, 8, dtype=torch.float64, device="cuda"))
    with pytest.raises(abi.NsdgError):
        c.set_snow_load(torch.zeros(8, 8, dtype=torch.float32, device="cuda"))
    with pytest.raises(abi.NsdgError):
        c.snow_load_nodal(f, f, torch.zeros(16, 17, dtype=torch.float64, device="cuda"))
    # the same shape keeps the field, another shape drops it
    c.set_snow_load(s)
    c.set_grid(8, 8, 2e3, 1e3)
    assert c.snow_load is s and lib.nsdg_snow_load_nodal(c.h, f.data_ptr(), f.data_ptr(), out.data_ptr()) == 0
    c.set_grid(8, 9, 1e3, 1e3)
    g = torch.zeros(19, 17, dtype=torch.float64, device="cuda")
    assert c.snow_load is None and lib.nsdg_snow_load_nodal(c.h, g.data_ptr(), g.data_ptr(), g.data_ptr()) == -3
    assert lib.nsdg_snow_load_set(c.h, None, 0, 0.0) == 0
    torch.cuda.synchronize()
    c.close()

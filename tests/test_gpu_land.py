"""Land mask on the device (include/nsdg.h "land mask"): the LAND instantiations of the mEVP passes against the
unmasked ones (all-ocean mask), against the CPU reference (tests/land_ref.py: the unchanged oracle with land nodes zeroed after every
sub-iteration), a wall of land against the smaller domain, land staying exactly zero under an island, a bay and a rock, NaN on land
reaching nothing, the pass / block / graph equalities with a mask that crosses block boundaries, and the clear calls themselves.
Uniform and adaptive alpha / beta wherever a sub-cycle runs."""
import math
import threading

import numpy as np
import pytest
import torch

import land_ref
import oracle_lib as O
from nextsimdg_amd import abi, rowblock, synthetic
from test_gpu_parity import Box, assert_close, dev, host, mevp_state, tdev, thost
from thread_ranks import fields, gather, run_world

pytestmark = pytest.mark.gpu
UNIFORM = dict(alpha=300.0, beta=300.0)
AD = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=50.0)
FORMS = [pytest.param(UNIFORM, id="uniform"), pytest.param(AD, id="adaptive")]


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
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_transport_bounds(())


def mask_dev(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8)).cuda()


def report(what, got, want, rtol, atol):
    """prints the figure before it is asserted: the largest error in units of its own limit"""
    got, want = np.asarray(got), np.asarray(want)
    worst = float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))) if got.size else 0.0
    print("%s: largest error = %.3g of its limit (rtol %g, atol %.3g)" % (what, worst, rtol, atol))
    assert_close(got, want, rtol, atol, what)


def box_inputs(b, land):
    """the Box's fields with no ice on land, and what the oracle makes of them"""
    b.H[:, land] = 0.0
    b.A[:, land] = 0.0
    nx, ny = b.nx, b.ny
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    return pg, cgh, cga, tax, tay


def device_subcycle(ctx, b, nsub, inputs, land=None, u0=None):
    """nsdg_mevp_subcycle from rest (or from u0 = (u, v)) with the element mask `land` (None: no mask): (u, v, [s11, s12, s22])"""
    pg, cgh, cga, tax, tay = inputs
    nx, ny = b.nx, b.ny
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = (np.zeros(shape), np.zeros(shape)) if u0 is None else u0
    du, dv = dev(u), dev(v)
    ds = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
    scratch = torch.zeros(10 * du.numel() + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
    ctx.set_land_mask(None if land is None else mask_dev(land))
    ctx.mevp_subcycle(120.0, nsub, ds, du, dv, dev(u), dev(v), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh), dev(cga), tdev(pg), scratch)
    torch.cuda.synchronize()
    ctx.set_land_mask(None)
    return du, dv, ds


# ------------------------------------------------------------------------------------------------ a. all-ocean mask against no mask
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_all_ocean_mask_equals_no_mask_in_the_subcycle(ctx, variant, pk):
    """an all-ocean mask runs the LAND instantiations of the packing and of every pass on the same numbers: bit for bit the unmasked
    kernels for the marching kernels (variants 1-4; variant 0 in the adaptive form runs variant 1's kernel).  The two-kernel form of
    variant 0 is held to the round-off bound test_gpu_parity.test_mevp_subcycle_matches_oracle uses for 25 sub-iterations"""
    ctx.set_mevp_variant(variant)
    b = Box(ctx, 150, 40, **pk)
    inputs = box_inputs(b, np.zeros((b.ny, b.nx), dtype=bool))
    plain = device_subcycle(ctx, b, 25, inputs)
    ocean = device_subcycle(ctx, b, 25, inputs, land=np.zeros((b.ny, b.nx), dtype=bool))
    assert float(plain[0].abs().max()) > 1e-4
    same = torch.equal(plain[0], ocean[0]) and torch.equal(plain[1], ocean[1]) and all(torch.equal(a, c) for a, c in zip(plain[2], ocean[2]))
    print("variant %d: all-ocean mask bit for bit equal to no mask: %s" % (variant, same))
    if variant == 0:
        for a, c, name in ((ocean[0], plain[0], "u"), (ocean[1], plain[1], "v")):
            report(name, host(a), host(c), 1e-9, 1e-11 * float(c.abs().max()))
        for a, c in zip(ocean[2], plain[2]):
            report("stress", thost(a, b.nx), thost(c, b.nx), 1e-9, 1e-10 * float(c.abs().max()))
    else:
        assert same


def core_run(ctx, pk, nx, ny, land, nsteps, nsub=40, data=None, hxhy=None, cls=rowblock.DynamicsCore, each=None, **kw):
    """a DynamicsCore on the whole domain, loaded with thread_ranks.fields (or `data`), stepped nsteps times"""
    ctx.set_mevp_params(ctx.mevp_default_params(**pk))
    bt, H, A, uo, vo, ua, va = data if data is not None else fields(nx, ny)
    hx, hy = hxhy if hxhy is not None else (bt.hx, bt.hy)
    core = cls(ctx, rowblock.RowBlock(nx, ny), hx, hy, 120.0, nsub, torch.device("cuda"), land=land, **kw)
    core.load_global(H, A, uo, vo, ua, va)
    for step in range(nsteps):
        core.step()
        if each is not None:
            each(step, core)
    torch.cuda.synchronize()
    return core


def core_state(core):
    return {"H": core.H.clone(), "A": core.A.clone(), "u": core.u.clone(), "v": core.v.clone(), "s": [x.clone() for x in core.s]}


def assert_same_state(a, b, what=""):
    for k in ("H", "A", "u", "v"):
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))
    for x, y in zip(a["s"], b["s"]):
        assert torch.equal(x, y), (what, "stress")


@pytest.mark.parametrize("pk", FORMS)
def test_all_ocean_mask_equals_no_mask_in_a_coupled_run(ctx, pk):
    nx, ny = 150, 64
    runs = []
    for land in (None, np.zeros((ny, nx), dtype=bool)):
        core = core_run(ctx, pk, nx, ny, land, 3)
        runs.append(core_state(core))
        core.close()
    assert float(runs[0]["u"].abs().max()) > 1e-4
    assert_same_state(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ b. device against land_ref
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_single_sub_iteration_with_a_mask_matches_the_reference(ctx, variant, pk):
    """one sub-iteration from a random state; tolerances: those of test_gpu_parity.test_mevp_single_iteration_matches_oracle"""
    ctx.set_mevp_variant(variant)
    b = Box(ctx, 67, 21, **pk)
    nx, ny = b.nx, b.ny
    land = land_ref.shapes_mask(nx, ny)
    ln = land_ref.land_nodes(land)
    pg, cgh, cga, tax, tay = box_inputs(b, land)
    u, v, s = mevp_state(b, np.random.default_rng(17))
    u[ln] = v[ln] = 0.0
    for x in s:
        x[:, land] = 0.0
    u0, v0 = 0.9 * u, 0.9 * v
    ds, dso = [tdev(x) for x in s], [tdev(np.zeros_like(x)) for x in s]
    du, dv = dev(u), dev(v)
    dun, dvn = torch.full_like(du, 3.0), torch.full_like(dv, 3.0)
    packed = torch.zeros(8 * u.size, dtype=torch.float64, device="cuda")
    ctx.set_land_mask(mask_dev(land))
    ctx.mevp_pack_nodal(120.0, (dev(u0), dev(v0)), (dev(tax), dev(tay)), (dev(b.uo), dev(b.vo)), dev(cgh), dev(cga), packed)
    ctx.mevp_iterate(0, 0, ny, ds, dso, (du, dv), (dun, dvn), packed, tdev(pg))
    torch.cuda.synchronize()
    land_ref.subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 1, b.po, land, s, u, v, u0, v0, tax, tay, b.uo, b.vo, cgh, cga, pg)
    assert np.max(np.abs(u)) > 1e-3
    for d, o, name in zip(dso, s, ("s11", "s12", "s22")):
        report(name, thost(d, nx), o, 1e-12, 1e-12 * np.max(np.abs(o)))
    report("u_new", host(dun), u, 1e-11, 1e-13 * np.max(np.abs(u)))
    report("v_new", host(dvn), v, 1e-11, 1e-13 * np.max(np.abs(v)))
    assert np.all(host(dun)[ln] == 0) and np.all(host(dvn)[ln] == 0)


@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_subcycle_with_a_mask_matches_the_reference(ctx, variant, pk):
    """25 sub-iterations through nsdg_mevp_subcycle; tolerances: those of test_gpu_parity.test_mevp_subcycle_matches_oracle"""
    ctx.set_mevp_variant(variant)
    b = Box(ctx, 48, 40, **pk)
    nx, ny = b.nx, b.ny
    land = land_ref.shapes_mask(nx, ny)
    ln = land_ref.land_nodes(land)
    inputs = pg, cgh, cga, tax, tay = box_inputs(b, land)
    du, dv, ds = device_subcycle(ctx, b, 25, inputs, land=land)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = np.zeros(shape), np.zeros(shape)
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    land_ref.subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 25, b.po, land, s, u, v, u, v, tax, tay, b.uo, b.vo, cgh, cga, pg)
    assert np.max(np.abs(u)) > 1e-4
    report("u after the subcycle", host(du), u, 1e-9, 1e-11 * np.max(np.abs(u)))
    report("v after the subcycle", host(dv), v, 1e-9, 1e-11 * np.max(np.abs(v)))
    for d, o in zip(ds, s):
        report("stress after the subcycle", thost(d, nx), o, 1e-9, 1e-10 * np.max(np.abs(o)))
    assert np.all(host(du)[ln] == 0) and np.all(host(dv)[ln] == 0)
    for d in ds:
        assert np.all(thost(d, nx)[:, land] == 0)


# ------------------------------------------------------------------------------------------------ c. wall equivalence
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("m", [128, 100])
def test_wall_of_land_reproduces_the_smaller_domain_bitwise(ctx, m, pk):
    """192 x 48 with land columns ix >= m against the m x 48 domain, 5 steps of 40 sub-iterations: H, A, u, v on the ocean part bit for
    bit (the reference construction is: tests/test_land_cpu.py); m = 128 puts the coast on the edge of a 64-lane window of the passes,
    m = 100 inside one and inside a two-element lane of the transport"""
    nx, ny = 192, 48
    data = fields(nx, ny)
    bt, H, A, uo, vo, ua, va = data
    land = np.zeros((ny, nx), dtype=bool)
    land[:, m:] = True
    full = core_run(ctx, pk, nx, ny, land, 5, data=data)
    got = core_state(full)
    full.close()
    cut = lambda a: np.ascontiguousarray(a[:, :2 * m + 1])
    small = core_run(ctx, pk, m, ny, None, 5, data=(bt, np.ascontiguousarray(H[:, :, :m]), np.ascontiguousarray(A[:, :, :m]), cut(uo), cut(vo), cut(ua), cut(va)),
                     hxhy=(bt.hx, bt.hy))
    want = core_state(small)
    small.close()
    assert float(want["u"].abs().max()) > 1e-4
    for k in ("H", "A"):
        d = (got[k][:, :, :m] - want[k]).abs()
        print("%s: largest difference on the ocean part %.3g" % (k, float(d.max())))
        assert torch.equal(got[k][:, :, :m], want[k]), (k, float(d.max()))
        assert bool((got[k][:, :, m:] == 0).all()), k
    for k in ("u", "v"):
        d = (got[k][:, :2 * m + 1] - want[k]).abs()
        print("%s: largest difference on the ocean part %.3g" % (k, float(d.max())))
        assert torch.equal(got[k][:, :2 * m + 1], want[k]), (k, float(d.max()))
        assert bool((got[k][:, 2 * m:] == 0).all()), k


# ------------------------------------------------------------------------------------------------ d. island + bay + rock
@pytest.mark.parametrize("pk", FORMS)
def test_shapes_keep_land_at_zero_and_conserve_the_ice(ctx, pk):
    """256 x 192, island + bay + one-element rock, 10 steps of 40 sub-iterations: land H, A, stress and land-node u, v are EXACTLY 0 after
    every step and everything stays finite.  The relative drift of math.fsum of the cell means of H may be at most 8 x the drift of
    land_ref on the same case or 64 ulp of the total (1.42e-14), whichever is larger.  The reference's measured drift is printed beside
    the bound (on the 24 x 20 case of tests/test_land_cpu.py it is <= 3.4e-16)"""
    nx, ny, nsteps = 256, 192, 10
    data = fields(nx, ny)
    bt, H, A, uo, vo, ua, va = data
    land = land_ref.shapes_mask(nx, ny)
    ln = land_ref.land_nodes(land)
    tl, tln = torch.from_numpy(land).cuda(), torch.from_numpy(ln).cuda()
    H0 = H.copy()
    H0[:, land] = 0.0
    total0 = math.fsum(H0[0].ravel())
    drift, ref_drift = [], []

    def each(step, core):
        for f in (core.H, core.A):
            assert bool((f[:, tl] == 0).all()), step
        for x in core.s:
            assert bool((abi.untile(x, nx)[:, tl] == 0).all()), step
        assert bool((core.u[tln] == 0).all()) and bool((core.v[tln] == 0).all()), step
        assert all(bool(torch.isfinite(f).all()) for f in (core.H, core.A, core.u, core.v)), step
        drift.append(abs(math.fsum(core.H[0].cpu().numpy().ravel()) - total0) / total0)

    core = core_run(ctx, pk, nx, ny, land, nsteps, data=data, each=each)
    assert float(core.u.abs().max()) > 1e-4
    core.close()
    land_ref.coupled_steps(nx, ny, bt.hx, bt.hy, 120.0, 40, nsteps, O.mevp_params(**pk), land, H, A, uo, vo, ua, va, omp=True,
                           each=lambda step, st: ref_drift.append(abs(math.fsum(st["H"][0].ravel()) - total0) / total0))
    bound = max(8 * max(ref_drift), 64 * np.finfo(float).eps)
    print("relative drift of the total of H: device %.3g, land_ref %.3g, bound %.3g" % (max(drift), max(ref_drift), bound))
    assert max(drift) <= bound


# ------------------------------------------------------------------------------------------------ e. poison
@pytest.mark.parametrize("pk", FORMS)
def test_nan_on_land_reaches_no_ocean_value(ctx, pk):
    """NaN in the wind and the ocean current at land nodes and in H, A on land elements: bit for bit the unpoisoned run"""
    nx, ny = 150, 64
    data = fields(nx, ny)
    bt, H, A, uo, vo, ua, va = data
    land = land_ref.shapes_mask(nx, ny)
    ln = land_ref.land_nodes(land)
    clean = core_run(ctx, pk, nx, ny, land, 3, nsub=20, data=data)
    want = core_state(clean)
    clean.close()
    poisoned = [a.copy() for a in (H, A, uo, vo, ua, va)]
    for a in poisoned[:2]:
        a[:, land] = np.nan
    for a in poisoned[2:]:
        a[ln] = np.nan
    dirty = core_run(ctx, pk, nx, ny, land, 3, nsub=20, data=(bt, *poisoned))
    got = core_state(dirty)
    dirty.close()
    assert float(want["u"].abs().max()) > 1e-4
    assert_same_state(got, want)


def test_nan_forcing_on_land_leaves_the_column_state_there_at_zero(ctx):
    nx, ny = 96, 64
    data = fields(nx, ny)
    land = land_ref.shapes_mask(nx, ny)
    tl = torch.from_numpy(land).cuda()
    st, fo, _ = synthetic.column_fields(nx * ny, 5)
    column = {k: v.reshape(ny, nx).copy() for k, v in {**st, **fo}.items()}
    column["wind"] = 0.2 * column["wind"]
    for k in abi.FORCING:
        column[k][land] = np.nan
    ctx.set_mevp_params(ctx.mevp_default_params(**AD))
    ctx.set_column_params(ctx.column_default_params())
    bt, H, A, uo, vo, ua, va = data
    core = rowblock.CoupledCore(ctx, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, 120.0, 12, torch.device("cuda"), land=land)
    core.load_global(H, A, uo, vo, ua, va)
    core.load_column(column)
    for _ in range(2):
        core.step()
        torch.cuda.synchronize()
        for f in (core.H[0], core.A[0], core.col["hsnow"], core.newice):
            assert bool((f[tl] == 0).all())
    for f in (core.H, core.A, core.u, core.v):
        assert bool(torch.isfinite(f).all())
    assert bool(torch.isfinite(core.col["hsnow"][~tl]).all()) and float(core.u.abs().max()) > 1e-5
    core.close()


# ------------------------------------------------------------------------------------------------ f. equalities with a mask across blocks
NXF, NYF = 150, 128


def blocks_mask():
    """150 x 128: an island across the boundaries of four row blocks (rows 32, 64, 96), a rock on a boundary row, a coast with a bay"""
    m = land_ref.shapes_mask(NXF, NYF)
    m[20:110, 60:70] = True
    m[64, 20] = True
    return m


@pytest.mark.parametrize("pk", FORMS)
def test_passes_of_two_three_and_four_equal_single_sub_iterations_with_a_mask(ctx, pk):
    b = Box(ctx, NXF, 48, **pk)
    land = blocks_mask()[40:88]
    inputs = box_inputs(b, land)
    res = {}
    for variant in (1, 2, 3, 4):
        ctx.set_mevp_variant(variant)
        res[variant] = device_subcycle(ctx, b, 13, inputs, land=land)
    assert float(res[1][0].abs().max()) > 1e-4
    for variant in (2, 3, 4):
        assert torch.equal(res[1][0], res[variant][0]) and torch.equal(res[1][1], res[variant][1]), variant
        assert all(torch.equal(a, c) for a, c in zip(res[1][2], res[variant][2])), variant


@pytest.mark.parametrize("pk", FORMS)
def test_one_block_equals_four_blocks_and_graphs_equal_no_graphs_with_a_mask(gpu, pk):
    """the native driver on the in-process transport: 1 block == 4 blocks (groups of two passes of four, a remainder), with and without
    hipGraph replay, bit for bit"""
    land = blocks_mask()
    kw = dict(alpha=pk, core_kw=dict(land=land), transport="native", native=True)
    ref = run_world(1, 4, False, NXF, NYF, 21, 3, **kw)[0]
    assert float(ref["u"].abs().max()) > 1e-5
    ln = torch.from_numpy(land_ref.land_nodes(land)).cuda()
    assert bool((ref["u"][ln] == 0).all()) and bool((ref["H"][:, torch.from_numpy(land).cuda()] == 0).all())
    unmasked = run_world(1, 4, False, NXF, NYF, 21, 3, alpha=pk, transport="native", native=True)[0]
    assert not torch.equal(unmasked["u"], ref["u"])
    for world, graph in ((4, False), (1, True), (4, True)):
        parts = run_world(world, 4, False, NXF, NYF, 21, 3, group=2, use_graph=graph, **kw)
        for key in ("H", "A", "u", "v", "s11"):
            assert torch.equal(gather(parts, world, key), ref[key]), (key, world, graph)


@pytest.mark.parametrize("pk", FORMS)
def test_a_graph_plan_follows_the_mask_being_set_and_cleared(gpu, pk):
    """a use_graph plan run unmasked, then masked, then unmasked again equals plans without graphs (fresh launches every time): the
    graphs recorded with one instantiation of the passes are not replayed for the other"""
    nx, ny, nsub = NXF, 64, 14
    bt = synthetic.BoxTest(nx, ny)
    land = blocks_mask()[32:96]
    tland = mask_dev(land)
    H, A = bt.dg_fields()
    H[:, land] = 0.0
    A[:, land] = 0.0
    H, A = dev(H), dev(A)
    uo, vo = (dev(np.ascontiguousarray(x)) for x in bt.ocean())
    ua, va = (dev(np.ascontiguousarray(3.0 * x)) for x in bt.wind(0.0))
    results = []
    for use_graph in (False, True):
        c = abi.Context(gpu)
        c.set_grid(nx, ny, bt.hx, bt.hy)
        c.set_mevp_params(c.mevp_default_params(**pk))
        z = lambda: torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda")
        s2 = ([c.private_zeros(8, ny, nx, "cuda") for _ in range(3)], [c.private_zeros(8, ny, nx, "cuda") for _ in range(3)])
        uv2 = ((z(), z()), (z(), z()))
        pg = c.private_zeros(9, ny, nx, "cuda")
        packed = torch.zeros(8 * uv2[0][0].numel(), dtype=torch.float64, device="cuda")
        c.ice_strength(H, A, pg)
        run, _, _ = c.rb_mevp(rowblock.RowBlock(nx, ny, 0, 1), (None, None), nsub, True, use_graph, s2, uv2, packed, pg)
        par, snaps = 0, []
        for m in (None, tland, None, tland):
            c.set_land_mask(m)
            if m is not None:
                c.land_clear_nodes(*uv2[par])
            c.mevp_prepare(120.0, H, A, (ua, va), (uo, vo), uv2[par], packed)
            par = run(par)
            torch.cuda.synchronize()
            snaps.append([x.clone() for x in list(s2[par]) + list(uv2[par])])
        results.append(snaps)
        run.close()
        c.close()
    ln = torch.from_numpy(land_ref.land_nodes(land)).cuda()
    for k, (plain, graph) in enumerate(zip(*results)):
        assert float(plain[3].abs().max()) > 1e-6
        assert bool((plain[3][ln] == 0).all()) == (k % 2 == 1), k  # the masked runs hold the land nodes, the unmasked ones move them
        for a, b in zip(plain, graph):
            assert torch.equal(a, b), k


def test_auto_substeps_choose_the_same_n_on_one_and_four_blocks_with_a_mask(gpu):
    land = blocks_mask()
    data = fields(NXF, NYF)
    bt, H, A, uo, vo, ua, va = data
    group = [5000]

    def rank(r, world, out, gid):
        try:
            c = abi.Context(torch.device("cuda:0"))
            c.set_mevp_params(c.mevp_default_params(**AD))
            blk = rowblock.RowBlock(NXF, NYF, r, world, 4, 3) if world > 1 else rowblock.RowBlock(NXF, NYF)
            ex = rowblock.NativeHaloExchanger(c, blk, local_group=gid) if world > 1 else None
            core = rowblock.DynamicsCore(c, blk, bt.hx, bt.hy, 120.0, 16, torch.device("cuda"), exchanger=ex, native=True, land=land)
            core.load_global(H, A, uo, vo, ua, va)
            ns = [core.advance(240.0, substeps="auto", courant=0.3) for _ in range(2)]
            torch.cuda.synchronize()
            out[r] = (ns, {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")})
        except BaseException as e:  # noqa: BLE001
            out[r] = e

    res = {}
    for world in (1, 4):
        out = {}
        group[0] += 1
        ts = [threading.Thread(target=rank, args=(r, world, out, group[0])) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for r in range(world):
            if isinstance(out[r], BaseException):
                raise out[r]
        res[world] = out
    ns = res[1][0][0]
    assert min(ns) > 1, ns
    assert all(res[4][r][0] == ns for r in range(4)), (ns, [res[4][r][0] for r in range(4)])
    for k in ("H", "A", "u", "v"):
        got = torch.cat([res[4][r][1][k] for r in range(4)], dim=1 if k in ("H", "A") else 0)
        assert torch.equal(got, res[1][0][1][k]), k


# ------------------------------------------------------------------------------------------------ g. the clear calls
def test_land_clear_writes_only_land_entries_of_the_rows(ctx):
    nx, ny = 70, 23
    bt = synthetic.BoxTest(nx, ny)
    ctx.set_grid(nx, ny, bt.hx, bt.hy)
    land = land_ref.shapes_mask(nx, ny)
    tl = torch.from_numpy(land).cuda()
    f = torch.full((6, ny, nx), 7.0, dtype=torch.float64, device="cuda")
    f[2, 5, 20] = float("nan")
    ctx.land_clear(f)  # no mask: nothing happens
    assert bool((f[~torch.isnan(f)] == 7.0).all()) and int(torch.isnan(f).sum()) == 1
    ctx.set_land_mask(mask_dev(land))
    f[:, tl] = float("nan")
    g = f.clone()
    ctx.land_clear(g, 4, 17)
    rows = torch.zeros(ny, dtype=torch.bool, device="cuda")
    rows[4:17] = True
    inside = tl & rows[:, None]
    assert bool((g[:, inside] == 0).all())  # a store: the NaN is gone
    assert bool(torch.isnan(g[:, tl & ~rows[:, None]]).all())
    assert bool((g[:, ~tl][~torch.isnan(g[:, ~tl])] == 7.0).all()) and bool(torch.isnan(g[2, 5, 20]))
    p = f[3].clone()  # one plane
    ctx.land_clear(p)
    assert bool((p[tl] == 0).all()) and bool((p[~tl] == 7.0).all())
    ln = torch.from_numpy(land_ref.land_nodes(land_ref.shapes_mask(nx, ny))).cuda()
    u = torch.full((2 * ny + 1, 2 * nx + 1), float("nan"), dtype=torch.float64, device="cuda")
    v = torch.full_like(u, 5.0)
    ctx.land_clear_nodes(u, v)
    assert bool((u[ln] == 0).all()) and bool(torch.isnan(u[~ln]).all()) and bool((v[ln] == 0).all()) and bool((v[~ln] == 5.0).all())
    # the same shape keeps the mask, another shape drops it
    ctx.set_grid(nx, ny, 2 * bt.hx, bt.hy)
    q = torch.full((ny, nx), 7.0, dtype=torch.float64, device="cuda")
    ctx.land_clear(q)
    assert bool((q[tl] == 0).all())
    ctx.set_grid(nx, ny + 1, bt.hx, bt.hy)
    q = torch.full((ny + 1, nx), 7.0, dtype=torch.float64, device="cuda")
    ctx.land_clear(q)
    assert bool((q == 7.0).all()) and ctx.land_mask is None


def test_land_calls_report_misuse(gpu):
    c = abi.Context(gpu)
    lib, m = c.lib, torch.zeros(8, 8, dtype=torch.uint8, device="cuda")
    f = torch.zeros(8, 8, dtype=torch.float64, device="cuda")
    assert lib.nsdg_land_mask_set(c.h, m.data_ptr()) == -3 and b"nsdg_grid_set" in lib.nsdg_last_error()  # NSDG_ERR_STATE
    assert lib.nsdg_land_clear(c.h, 0, 8, 1, f.data_ptr()) == -3
    assert lib.nsdg_land_clear_nodes(c.h, f.data_ptr(), f.data_ptr()) == -3
    c.set_grid(8, 8, 1e3, 1e3)
    assert lib.nsdg_land_mask_set(c.h, m.data_ptr()) == 0
    for args in ((-1, 8, 1), (0, 9, 1), (5, 4, 1), (0, 8, 0)):
        assert lib.nsdg_land_clear(c.h, *args, f.data_ptr()) == -1, args  # NSDG_ERR_ARG
    assert lib.nsdg_land_clear(c.h, 0, 8, 1, None) == -1
    assert lib.nsdg_land_clear_nodes(c.h, None, None) == -1
    assert lib.nsdg_land_clear(c.h, 3, 3, 1, f.data_ptr()) == 0  # an empty range is no error
    with pytest.raises(abi.NsdgError):
        c.set_land_mask(torch.zeros(8, 7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(abi.NsdgError):
        c.set_land_mask(torch.zeros(8, 8, dtype=torch.float64, device="cuda"))
    assert lib.nsdg_land_mask_set(c.h, None) == 0
    c.close()

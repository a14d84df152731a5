"""Landfast ice on the device (include/nsdg_basal.h): the BASAL instantiations of the packing and of every pass
against the ones without a depth array (deep water: T_b = 0 everywhere, bit for bit), against the CPU reference (tests/basal_ref.py: the
unchanged oracle corrected node by node with D / (D + C_b)), the pass / strip / block / graph / native equalities with a shoal across the
seams, the diagnostic T_b against the reference and against what a packing stores, and the misuse reports.  Uniform and adaptive
alpha / beta wherever an mEVP sub-cycle runs.  The shoal case (10 m of water under H ~ 2 m, A ~ 0.95 inside 1000 m) is held without a
device to "the reference without the term differs by more than 10 % of the largest speed over the shoal"
(tests/test_basal_cpu.py): a device that lost the term cannot pass the comparisons with the reference here."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import basal_ref as BR
import land_ref
import oracle_lib as O
from nextsimdg_amd import abi, rowblock, synthetic
from test_gpu_land import AD, FORMS, assert_same_state, blocks_mask, box_inputs, core_run, core_state, mask_dev, report
from test_gpu_parity import Box, dev, host, mevp_state, tdev, thost
from thread_ranks import fields, gather, run_world

pytestmark = pytest.mark.gpu
DEEP = 5000.0
NXF, NYF = 150, 128


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
    ctx.set_basal_params(ctx.basal_default_params())
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_transport_bounds(())


def device_subcycle(ctx, b, nsub, inputs, land=None, depth=None, u0=None):
    """nsdg_mevp_subcycle from rest (or from u0 = (u, v)) with the element mask `land` and the water depth `depth` (None: not set):
    (u, v, [s11, s12, s22])"""
    pg, cgh, cga, tax, tay = inputs
    nx, ny = b.nx, b.ny
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = (np.zeros(shape), np.zeros(shape)) if u0 is None else u0
    du, dv = dev(u), dev(v)
    ds = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
    scratch = torch.zeros(10 * du.numel() + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
    ctx.set_land_mask(None if land is None else mask_dev(land))
    ctx.set_basal_depth(None if depth is None else dev(depth))
    ctx.mevp_subcycle(120.0, nsub, ds, du, dv, dev(u), dev(v), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh), dev(cga), tdev(pg), scratch)
    torch.cuda.synchronize()
    ctx.set_land_mask(None)
    ctx.set_basal_depth(None)
    return du, dv, ds


def same_run(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def shoal_box(ctx, nx, ny, pk, land, box=None):
    """the Box of tests/test_gpu_parity.py under the thick cover of the shoal case, with a shoal of 10 m inside 1000 m of water"""
    b = Box(ctx, nx, ny, **pk)
    BR.thick_cover(b.H, b.A)
    depth, shoal = BR.shoal_depth(nx, ny, box=box)
    return b, depth, shoal, box_inputs(b, land if land is not None else np.zeros((ny, nx), dtype=bool))


def thick_fields(nx, ny):
    """thread_ranks.fields under the thick cover of the shoal case"""
    bt, H, A, uo, vo, ua, va = fields(nx, ny)
    BR.thick_cover(H, A)
    return bt, H, A, uo, vo, ua, va


def blocks_depth():
    """150 x 128: a shoal across the boundaries of four row blocks (rows 32, 64, 96) and across the column seams of the passes (57, 63, 64,
    114, 126, 128); the island of blocks_mask() cuts through it"""
    return BR.shoal_depth(NXF, NYF, box=(20, 110, 40, 135))


# ------------------------------------------------------------------------------------------------ 1. deep water against no depth array
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_deep_water_equals_no_depth_array_in_the_subcycle(ctx, variant, pk):
    """5000 m everywhere runs the BASAL instantiations of the packing and of every pass with T_b = 0: bit for bit the kernels without the
    term for the marching kernels (variants 1-4, and variant 0 in the adaptive form, which runs variant 1's kernel).  The two-kernel form of
    variant 0, uniform alpha and beta only, is held to the round-off bound test_gpu_land.py uses for 25 sub-iterations"""
    ctx.set_mevp_variant(variant)
    b = Box(ctx, 150, 40, **pk)
    inputs = box_inputs(b, np.zeros((b.ny, b.nx), dtype=bool))
    plain = device_subcycle(ctx, b, 25, inputs)
    deep = device_subcycle(ctx, b, 25, inputs, depth=np.full((b.ny, b.nx), DEEP))
    assert float(plain[0].abs().max()) > 1e-4
    same = same_run(plain, deep)
    print("variant %d: 5000 m of water bit for bit equal to no depth array: %s" % (variant, same))
    if variant == 0 and not b.po.aevp_c > 0:  # the two-kernel form (uniform alpha, beta only)
        for a, c, name in ((deep[0], plain[0], "u"), (deep[1], plain[1], "v")):
            report(name, host(a), host(c), 1e-9, 1e-11 * float(c.abs().max()))
        for a, c in zip(deep[2], plain[2]):
            report("stress", thost(a, b.nx), thost(c, b.nx), 1e-9, 1e-10 * float(c.abs().max()))
    else:
        assert same


@pytest.mark.parametrize("pk", FORMS)
def test_deep_water_equals_no_depth_array_in_a_coupled_run(ctx, pk):
    nx, ny = 150, 64
    runs = []
    for depth in (None, np.full((ny, nx), DEEP)):
        core = core_run(ctx, pk, nx, ny, None, 3, bathymetry=depth)
        runs.append(core_state(core))
        if depth is not None:
            assert float(core.basal_read().abs().max()) == 0.0
        core.close()
    assert float(runs[0]["u"].abs().max()) > 1e-4
    assert_same_state(runs[0], runs[1])
    assert ctx.basal_depth is None  # close() took the depth array off the context


def test_deep_water_equals_no_depth_array_in_the_brittle_sub_iteration_and_run(ctx):
    import test_gpu_bbm as GB
    import test_gpu_bbm_native as GN

    c = GB.random_case(70, 9)
    res = []
    for depth in (None, np.full((9, 70), DEEP)):
        d = GB.Device(ctx, c)
        if depth is not None:  # the packing of Device() saw no depth array: pack again
            ctx.set_basal_depth(dev(depth))
            zero = torch.zeros_like(d.u)
            ctx.mevp_prepare(GB.DTS, d.H, d.A, (dev(c["ua"]), dev(c["va"])), (dev(c["uo"]), dev(c["vo"])), (zero, zero), d.packed)
        res.append(d.iterate())
        d.close()
        ctx.set_basal_depth(None)
    assert float(res[0]["ut"].abs().max()) > 1e-6 and GB.same(res[0], res[1])
    want = GN.one_block(GB.DNSUB, False)
    got = GN.one_block(GB.DNSUB, False, bathymetry=np.full((GN.DNY, GN.DNX), DEEP))
    assert float(want["u"].abs().max()) > 1e-4
    GN.assert_same(got, want, "brittle run over 5000 m")


# ------------------------------------------------------------------------------------------------ 2. device against basal_ref
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_single_sub_iteration_over_a_shoal_matches_the_reference(ctx, variant, pk):
    """one sub-iteration from a random state on the 67 x 21 box with the shapes of land_ref.shapes_mask and a shoal across the column
    seams of the passes (57, 63) and the tile seam (64), reaching into the bay; tolerances: those of
    test_gpu_parity.test_mevp_single_iteration_matches_oracle"""
    ctx.set_mevp_variant(variant)
    nx, ny = 67, 21
    land = land_ref.shapes_mask(nx, ny)
    b, depth, shoal, (pg, cgh, cga, tax, tay) = shoal_box(ctx, nx, ny, pk, land, box=(5, 17, 40, 67))
    ln = land_ref.land_nodes(land)
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
    ctx.set_basal_depth(dev(depth))
    ctx.mevp_pack_nodal(120.0, (dev(u0), dev(v0)), (dev(tax), dev(tay)), (dev(b.uo), dev(b.vo)), dev(cgh), dev(cga), packed)
    ctx.mevp_iterate(0, 0, ny, ds, dso, (du, dv), (dun, dvn), packed, tdev(pg))
    torch.cuda.synchronize()
    ub, vb = u.copy(), v.copy()
    tb = BR.subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 1, b.po, BR.basal_par(), depth, land, s, ub, vb, u0, v0, tax, tay, b.uo, b.vo, cgh, cga, pg)
    grounded = (tb > 0) & ~ln
    assert np.max(np.abs(ub)) > 1e-3 and grounded.sum() > 200 and grounded[:, 2 * 57 - 2:2 * 64 + 2].any() and (tb[~ln] == 0).sum() > 1000
    for d, o, name in zip(dso, s, ("s11", "s12", "s22")):
        report(name, thost(d, nx), o, 1e-12, 1e-12 * np.max(np.abs(o)))
    report("u_new", host(dun), ub, 1e-11, 1e-13 * np.max(np.abs(ub)))
    report("v_new", host(dvn), vb, 1e-11, 1e-13 * np.max(np.abs(vb)))
    assert np.all(host(dun)[ln] == 0) and np.all(host(dvn)[ln] == 0)


@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_subcycle_over_a_shoal_matches_the_reference(ctx, variant, pk):
    """25 sub-iterations through nsdg_mevp_subcycle on the 48 x 40 box (the case of tests/test_basal_cpu.py); tolerances: those of
    test_gpu_parity.test_mevp_subcycle_matches_oracle"""
    ctx.set_mevp_variant(variant)
    nx, ny = 48, 40
    land = land_ref.shapes_mask(nx, ny)
    b, depth, shoal, inputs = shoal_box(ctx, nx, ny, pk, land)
    pg, cgh, cga, tax, tay = inputs
    ln = land_ref.land_nodes(land)
    du, dv, ds = device_subcycle(ctx, b, 25, inputs, land=land, depth=depth)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = np.zeros(shape), np.zeros(shape)
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    BR.subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 25, b.po, BR.basal_par(), depth, land, s, u, v, u, v, tax, tay, b.uo, b.vo, cgh, cga, pg)
    assert np.max(np.abs(u)) > 1e-4
    report("u after the subcycle", host(du), u, 1e-9, 1e-11 * np.max(np.abs(u)))
    report("v after the subcycle", host(dv), v, 1e-9, 1e-11 * np.max(np.abs(v)))
    for d, o in zip(ds, s):
        report("stress after the subcycle", thost(d, nx), o, 1e-9, 1e-10 * np.max(np.abs(o)))
    assert np.all(host(du)[ln] == 0) and np.all(host(dv)[ln] == 0)


# ------------------------------------------------------------------------------------------------ 3. passes and strips
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("strip_rows", [0, 1])
def test_passes_of_two_three_and_four_equal_single_sub_iterations_over_a_shoal(ctx, pk, strip_rows):
    """13 sub-iterations as passes of 1, 2, 3 and 4 (with their remainders), at the automatic strip height and at the smallest (one row
    per strip: every row is a strip seam), with a shoal across the column seams and the mask of test_gpu_land.py: bit for bit"""
    land = blocks_mask()[40:88]
    b, _, _, inputs = shoal_box(ctx, NXF, 48, pk, land)
    depth = blocks_depth()[0][40:88]
    res = {}
    for variant in (1, 2, 3, 4):
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_strip_rows(strip_rows)
        res[variant] = device_subcycle(ctx, b, 13, inputs, land=land, depth=depth)
    ctx.set_mevp_variant(1)
    without = device_subcycle(ctx, b, 13, inputs, land=land)
    assert float(res[1][0].abs().max()) > 1e-5 and not torch.equal(res[1][0], without[0])
    for variant in (2, 3, 4):
        assert same_run(res[1], res[variant]), variant


# ------------------------------------------------------------------------------------------------ 4. blocks, graphs, sub-steps
@pytest.mark.parametrize("pk", FORMS)
def test_one_block_equals_four_blocks_and_graphs_equal_no_graphs_over_a_shoal(gpu, pk):
    """the native driver on the in-process transport: 1 block == 4 blocks (groups of two passes of four, a remainder), with and without
    hipGraph replay, bit for bit; the shoal and the island cross every block boundary"""
    land = blocks_mask()
    depth, shoal = blocks_depth()
    data = thick_fields(NXF, NYF)
    kw = dict(alpha=pk, core_kw=dict(land=land, bathymetry=depth), transport="native", native=True, data=data)
    ref = run_world(1, 4, False, NXF, NYF, 21, 3, **kw)[0]
    assert float(ref["u"].abs().max()) > 1e-5
    free = run_world(1, 4, False, NXF, NYF, 21, 3, alpha=pk, core_kw=dict(land=land), transport="native", native=True, data=data)[0]
    sn = torch.from_numpy(BR.shoal_nodes(shoal) & ~land_ref.land_nodes(land)).cuda()
    speed = lambda r: torch.hypot(r["u"], r["v"])[sn]
    print("largest speed over the shoal after 3 steps: %.3g m/s with the depth array, %.3g without" % (float(speed(ref).max()), float(speed(free).max())))
    assert float(speed(ref).max()) < 0.5 * float(speed(free).max())
    for world, graph in ((4, False), (1, True), (4, True)):
        parts = run_world(world, 4, False, NXF, NYF, 21, 3, group=2, use_graph=graph, **kw)
        for key in ("H", "A", "u", "v", "s11"):
            assert torch.equal(gather(parts, world, key), ref[key]), (key, world, graph)


@pytest.mark.parametrize("pk", FORMS)
def test_native_equals_the_python_sequence_over_a_shoal(gpu, pk):
    land = blocks_mask()
    depth, _ = blocks_depth()
    kw = dict(alpha=pk, core_kw=dict(land=land, bathymetry=depth), data=thick_fields(NXF, NYF))
    python = run_world(1, 4, False, NXF, NYF, 21, 2, **kw)[0]
    native = run_world(1, 4, False, NXF, NYF, 21, 2, transport="native", native=True, **kw)[0]
    assert float(python["u"].abs().max()) > 1e-5
    for key in ("H", "A", "u", "v", "s11"):
        assert torch.equal(native[key], python[key]), key


def test_native_equals_the_python_sequence_in_the_brittle_run_over_a_shoal(gpu):
    import test_gpu_bbm as GB
    import test_gpu_bbm_native as GN

    depth, shoal = BR.shoal_depth(GN.DNX, GN.DNY, shallow=1.0)
    want = GN.one_block(GB.DNSUB, False, bathymetry=depth)
    got = GN.one_block(GB.DNSUB, True, bathymetry=depth)
    free = GN.one_block(GB.DNSUB, False)
    assert float(want["u"].abs().max()) > 1e-4 and not torch.equal(want["u"], free["u"])
    sn = torch.from_numpy(BR.shoal_nodes(shoal)).cuda()
    assert float(torch.hypot(want["u"], want["v"])[sn].max()) < float(torch.hypot(free["u"], free["v"])[sn].max())
    GN.assert_same(got, want, "native brittle run over a shoal")


@pytest.mark.parametrize("pk", FORMS)
def test_a_graph_plan_follows_the_depth_array_being_set_and_cleared(gpu, pk):
    """a use_graph plan run without a depth array, then with one, then without again equals plans without graphs (fresh launches every
    time): the graphs recorded with one instantiation of the passes are not replayed for the other"""
    nx, ny, nsub = NXF, 64, 14
    bt = synthetic.BoxTest(nx, ny)
    depth, shoal = blocks_depth()
    depth, shoal = depth[32:96], shoal[32:96]
    tdepth = dev(depth)
    H, A = BR.thick_cover(*bt.dg_fields())
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
        for d in (None, tdepth, None, tdepth):
            c.set_basal_depth(d)
            for f in list(s2[par]) + list(uv2[par]):
                f.zero_()  # every run starts from rest: a run with the depth array is compared with the run before it
            c.mevp_prepare(120.0, H, A, (ua, va), (uo, vo), uv2[par], packed)
            par = run(par)
            torch.cuda.synchronize()
            snaps.append([x.clone() for x in list(s2[par]) + list(uv2[par])])
        results.append(snaps)
        run.close()
        c.close()
    sn = torch.from_numpy(BR.shoal_nodes(shoal)).cuda()
    for k, (plain, graph) in enumerate(zip(*results)):
        assert float(plain[3].abs().max()) > 1e-6
        for a, b in zip(plain, graph):
            assert torch.equal(a, b), k
    plain = results[0]
    assert all(torch.equal(a, b) for a, b in zip(plain[0], plain[2])) and all(torch.equal(a, b) for a, b in zip(plain[1], plain[3]))
    assert float(plain[1][3][sn].abs().max()) < 0.5 * float(plain[0][3][sn].abs().max())  # the runs with the depth array hold the shoal


def test_auto_substeps_choose_the_same_n_on_one_and_four_blocks_over_a_shoal(gpu):
    land = blocks_mask()
    depth, _ = blocks_depth()
    bt, H, A, uo, vo, ua, va = thick_fields(NXF, NYF)
    group = [7000]

    def rank(r, world, out, gid):
        try:
            c = abi.Context(torch.device("cuda:0"))
            c.set_mevp_params(c.mevp_default_params(**AD))
            blk = rowblock.RowBlock(NXF, NYF, r, world, 4, 3) if world > 1 else rowblock.RowBlock(NXF, NYF)
            ex = rowblock.NativeHaloExchanger(c, blk, local_group=gid) if world > 1 else None
            core = rowblock.DynamicsCore(c, blk, bt.hx, bt.hy, 120.0, 16, torch.device("cuda"), exchanger=ex, native=True, land=land, bathymetry=depth)
            core.load_global(H, A, uo, vo, ua, va)
            ns = [core.advance(240.0, substeps="auto", courant=0.3) for _ in range(2)]
            torch.cuda.synchronize()
            res = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
            res["tb"] = core.basal_read().clone()
            out[r] = (ns, res)
            core.close()
            c.close()
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
    assert float(res[1][0][1]["tb"].max()) > 1.0
    for k in ("H", "A", "u", "v", "tb"):
        got = torch.cat([res[4][r][1][k] for r in range(4)], dim=1 if k in ("H", "A") else 0)
        assert torch.equal(got, res[1][0][1][k]), k


# ------------------------------------------------------------------------------------------------ 6. the diagnostic T_b
def ulp_distance(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("masked", [False, True])
def test_basal_critical_matches_the_reference_and_the_packing(ctx, masked):
    """nsdg_basal_critical against basal_ref.critical_stress to 4 ulp (a product of four factors, one of them exp: the device's exp and
    the host's are each good to 1 ulp, the three multiplications and the subtraction h - h_c round once each; h - h_c is exact enough
    here because h_c is not within 1e-3 of h at any node of the case -- asserted), zero for zero; and against the fourth coefficient pair
    of the two packings, (T_b, 0) bit for bit in the layout of csrc/mevp_common.h.  The case has deep water, a shoal, ice-free nodes
    (thin, open and at the mass floor) and, masked, land"""
    nx, ny = 67, 21
    land = land_ref.shapes_mask(nx, ny) if masked else None
    b, depth, shoal, (pg, cgh, cga, tax, tay) = shoal_box(ctx, nx, ny, {}, land, box=(3, 19, 20, 67))
    # ice-free patches inside the shoal: no ice, a thin cover, open water
    b.H[:, 5:8, 25:30] = 0.0
    b.A[:, 5:8, 25:30] = 0.0
    b.H[:, 10:13, 25:30] = 0.0
    b.H[0, 10:13, 25:30] = 0.004
    b.A[0, 14:17, 25:30] = 0.0
    pg, cgh, cga, tax, tay = box_inputs(b, land if masked else np.zeros((ny, nx), dtype=bool))
    ctx.set_land_mask(mask_dev(land) if masked else None)
    ctx.set_basal_depth(dev(depth))
    tb = torch.full((2 * ny + 1, 2 * nx + 1), -3.0, dtype=torch.float64, device="cuda")
    ctx.basal_critical(dev(cgh), dev(cga), tb)
    want = BR.critical_stress(b.po, BR.basal_par(), cgh, cga, depth, land)
    got = host(tb)
    hc = np.clip(cga, 0, 1) * BR.nodal_depth(depth) / 8.0
    assert np.min(np.abs(cgh - hc)[want > 0]) > 1e-3
    free = BR.ice_free(b.po, cgh, cga)
    assert (want > 1.0).sum() > 500 and (want == 0).sum() > 1000 and (free & (BR.nodal_depth(depth) < 11)).sum() > 50
    assert np.array_equal(got == 0, want == 0)
    worst = int(ulp_distance(got, want).max())
    print("nsdg_basal_critical against the reference: largest distance %d ulp" % worst)
    assert worst <= 4
    if masked:
        assert np.all(got[land_ref.land_nodes(land)] == 0)
    # what the two packings store as the fourth pair
    n = got.size
    zero = torch.zeros_like(tb)
    for how in ("pack_nodal", "prepare"):
        packed = torch.full((8 * n,), -3.0, dtype=torch.float64, device="cuda")
        if how == "pack_nodal":
            ctx.mevp_pack_nodal(120.0, (zero, zero), (dev(tax), dev(tay)), (dev(b.uo), dev(b.vo)), dev(cgh), dev(cga), packed)
            ref = tb
        else:  # the prepare kernel forms the nodal means itself: T_b of ITS means
            ctx.mevp_prepare(120.0, dev(b.H), dev(b.A), (dev(b.ua), dev(b.va)), (dev(b.uo), dev(b.vo)), (zero, zero), packed)
            dh, da = torch.zeros_like(tb), torch.zeros_like(tb)
            ctx.dg_to_cg(dev(b.H), dh)
            ctx.dg_to_cg(dev(b.A), da)
            ref = torch.zeros_like(tb)
            ctx.basal_critical(dh, da, ref)
        pair3 = packed.view(4, n, 2)[3]
        assert torch.equal(pair3[:, 0], ref.reshape(-1)), how
        assert bool((pair3[:, 1] == 0).all()), how
    # without a depth array the packing leaves the fourth pair alone
    ctx.set_basal_depth(None)
    packed = torch.full((8 * n,), -3.0, dtype=torch.float64, device="cuda")
    ctx.mevp_pack_nodal(120.0, (zero, zero), (dev(tax), dev(tay)), (dev(b.uo), dev(b.vo)), dev(cgh), dev(cga), packed)
    assert bool((packed.view(4, n, 2)[3] == -3.0).all()) and not bool((packed.view(4, n, 2)[:3] == -3.0).any())


@pytest.mark.parametrize("pk", FORMS)
def test_one_grounded_node_reads_its_critical_stress_back_through_a_sub_iteration(ctx, pk):
    """ONE shallow element in deep water grounds exactly its centre node (every other node of it averages with 1000 m).  One sub-iteration
    with the depth array and one without differ at that node only, bit for bit elsewhere, and there
        u_without / u_with = (D + C_b) / D,    T_b = (u_without / u_with - 1) D (|u_old| + u0)
    gives back nsdg_basal_critical's value: what the pass read as the seventh coefficient is what the diagnostic reports.  Tolerance
    1e-11 relative, the single-iteration limit: the quotient minus one loses log2(D / C_b) bits (C_b / D is asserted above 1e-2: under 7
    bits, 1e-14), D is restated in numpy (a few ulp) and the device's reciprocals are good to 1 ulp"""
    nx, ny = 67, 21
    b = Box(ctx, nx, ny, **pk)
    BR.thick_cover(b.H, b.A)
    ex, ey = 63, 9  # the last column of the first wave of the single-iteration march
    depth = np.full((ny, nx), 1000.0)
    depth[ey, ex] = 10.0
    pg, cgh, cga, tax, tay = box_inputs(b, np.zeros((ny, nx), dtype=bool))
    u, v, s = mevp_state(b, np.random.default_rng(29))
    u0, v0 = 0.9 * u, 0.9 * v
    tb = torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda")
    ctx.set_basal_depth(dev(depth))
    ctx.basal_critical(dev(cgh), dev(cga), tb)
    tbh = host(tb)
    node = (2 * ey + 1, 2 * ex + 1)
    assert tbh[node] > 1.0 and (tbh > 0).sum() == 1
    out = {}
    for with_depth in (True, False):
        ctx.set_basal_depth(dev(depth) if with_depth else None)
        packed = torch.zeros(8 * u.size, dtype=torch.float64, device="cuda")
        ctx.mevp_pack_nodal(120.0, (dev(u0), dev(v0)), (dev(tax), dev(tay)), (dev(b.uo), dev(b.vo)), dev(cgh), dev(cga), packed)
        dso = [tdev(np.zeros_like(x)) for x in s]
        dun, dvn = torch.full_like(tb, 3.0), torch.full_like(tb, 3.0)
        ctx.mevp_iterate(0, 0, ny, [tdev(x) for x in s], dso, (dev(u), dev(v)), (dun, dvn), packed, tdev(pg))
        torch.cuda.synchronize()
        out[with_depth] = (host(dun), host(dvn), [x.clone() for x in dso])
    (ub, vb, sb), (uf, vf, sf) = out[True], out[False]
    others = np.ones(u.shape, dtype=bool)
    others[node] = False
    assert np.array_equal(ub[others], uf[others]) and np.array_equal(vb[others], vf[others]) and all(torch.equal(x, y) for x, y in zip(sb, sf))
    # the adaptive form's beta_n needs the oracle's alpha_e of this sub-iteration
    alpha_e = None
    if b.po.aevp_c > 0:
        alpha_e = np.zeros((ny, nx))
        O.mevp_stress(nx, ny, 0, ny, b.bt.hx, b.bt.hy, b.po, u, v, pg, *[x.copy() for x in s], dt=120.0, cgh=cgh, cga=cga, alpha_e=alpha_e)
    D = BR.denominator(b.po, 120.0, cgh, cga, u, v, b.uo, b.vo, BR.node_beta(b.po, cgh, cga, alpha_e))[node]
    speed = np.hypot(u[node], v[node])
    cb = tbh[node] / (speed + 5e-5)
    assert cb / D > 1e-2
    for name, f, g in (("u", uf, ub), ("v", vf, vb)):
        back = (f[node] / g[node] - 1.0) * D * (speed + 5e-5)
        print("%s: T_b read back through the sub-iteration %.15g, nsdg_basal_critical %.15g, relative difference %.3g" % (
            name, back, tbh[node], abs(back - tbh[node]) / tbh[node]))
        assert abs(back - tbh[node]) <= 1e-11 * tbh[node]


# ------------------------------------------------------------------------------------------------ 7. misuse
def test_basal_calls_report_misuse(gpu):
    c = abi.Context(gpu)
    lib = c.lib
    f = torch.zeros(17, 17, dtype=torch.float64, device="cuda")
    d = torch.full((8, 8), 10.0, dtype=torch.float64, device="cuda")
    assert lib.nsdg_basal_depth_set(c.h, d.data_ptr()) == -3 and b"nsdg_grid_set" in lib.nsdg_last_error()  # NSDG_ERR_STATE
    assert lib.nsdg_basal_critical(c.h, f.data_ptr(), f.data_ptr(), f.data_ptr()) == -3
    c.set_grid(8, 8, 1e3, 1e3)
    assert lib.nsdg_basal_critical(c.h, f.data_ptr(), f.data_ptr(), f.data_ptr()) == -3 and b"nsdg_basal_depth_set" in lib.nsdg_last_error()
    assert lib.nsdg_basal_depth_set(c.h, d.data_ptr()) == 0
    c.set_basal_depth(d)  # the wrapper keeps the tensor
    for args in ((None, f.data_ptr(), f.data_ptr()), (f.data_ptr(), None, f.data_ptr()), (f.data_ptr(), f.data_ptr(), None)):
        assert lib.nsdg_basal_critical(c.h, *args) == -1  # NSDG_ERR_ARG
    assert lib.nsdg_basal_critical(c.h, f.data_ptr(), f.data_ptr(), f.data_ptr()) == 0
    # parameters: k1 > 0, k2 >= 0, alpha_b >= 0, u0 > 0, all finite; a refused set changes nothing
    assert lib.nsdg_basal_params_set(c.h, None) == -1 and lib.nsdg_basal_params_set(None, C.byref(abi.basal_default_params())) == -1
    for bad in (dict(k1=0.0), dict(k1=-1.0), dict(k2=-1.0), dict(alpha_b=-0.5), dict(u0=0.0), dict(u0=-1e-5), dict(k1=float("nan")),
                dict(k2=float("inf")), dict(alpha_b=float("nan")), dict(u0=float("inf"))):
        assert lib.nsdg_basal_params_set(c.h, C.byref(abi.basal_default_params(**bad))) == -1, bad
    c.set_basal_params(abi.basal_default_params(k2=0.0, alpha_b=0.0))  # the closed ends of the ranges are allowed
    f.fill_(2.0)
    tb = torch.full_like(f, -1.0)
    c.basal_critical(f, torch.ones_like(f), tb)
    assert bool((tb == 0).all())  # k2 = 0
    c.set_basal_params(abi.basal_default_params())
    c.basal_critical(f, torch.ones_like(f), tb)
    assert bool((tb == 15.0 * (2.0 - 10.0 / 8.0)).all())
    # the wrapper's own checks
    with pytest.raises(abi.NsdgError):
        c.set_basal_depth(torch.zeros(8, 7, dtype=torch.float64, device="cuda"))
    with pytest.raises(abi.NsdgError):
        c.set_basal_depth(torch.zeros(8, 8, dtype=torch.float32, device="cuda"))
    with pytest.raises(abi.NsdgError):
        c.basal_critical(f, f, torch.zeros(16, 17, dtype=torch.float64, device="cuda"))
    # the same shape keeps the array, another shape drops it
    c.set_grid(8, 8, 2e3, 1e3)
    assert c.basal_depth is d and lib.nsdg_basal_critical(c.h, f.data_ptr(), f.data_ptr(), tb.data_ptr()) == 0
    c.set_grid(8, 9, 1e3, 1e3)
    g = torch.zeros(19, 17, dtype=torch.float64, device="cuda")
    assert c.basal_depth is None and lib.nsdg_basal_critical(c.h, g.data_ptr(), g.data_ptr(), g.data_ptr()) == -3
    assert lib.nsdg_basal_depth_set(c.h, None) == 0
    c.close()

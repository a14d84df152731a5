"""Landfast ice without a GPU (include/nsdg_basal.h): the reference construction itself (tests/basal_ref.py: the
unchanged oracle corrected node by node with the exact factor D / (D + C_b)) against its pure-Python form, T_b against hand values, the
steady balance of a strengthless cover over a shoal, the shoal case the device tests use, and the row-block driver on the reference
(rowblock.DynamicsCore(..., bathymetry=depth) over BasalOracleOps, one rank and gloo worlds of 2 and 3)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import basal_ref as BR  # noqa: E402
import land_ref  # noqa: E402
import oracle_lib as O  # noqa: E402
from nextsimdg_amd import rowblock, synthetic  # noqa: E402

DT = 120.0
UNIFORM = dict(alpha=200.0, beta=200.0)
ADAPTIVE = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=3.0, delta_min=2e-7)


def test_entry_points_without_a_context_and_the_defaults():
    from nextsimdg_amd import abi, build

    build.build_lib(verbose=False)
    lib = abi.load_library()
    assert sorted(abi.BASAL_SYMBOLS) == ["nsdg_basal_critical", "nsdg_basal_default_params", "nsdg_basal_depth_set", "nsdg_basal_params_set"]
    assert not set(abi.BASAL_SYMBOLS) & (set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS))
    p = abi.basal_default_params()
    assert (p.k1, p.k2, p.alpha_b, p.u0) == (8.0, 15.0, 20.0, 5e-5) == tuple(BR.DEFAULTS[k] for k in ("k1", "k2", "alpha_b", "u0"))
    assert lib.nsdg_basal_params_set(None, C.byref(p)) == -1 and b"null" in lib.nsdg_last_error()
    assert lib.nsdg_basal_depth_set(None, None) == -1 and b"null context" in lib.nsdg_last_error()
    assert lib.nsdg_basal_critical(None, None, None, None) == -1
    assert lib.nsdg_abi_version() == 6  # the section adds calls, it changes none
    with pytest.raises(abi.NsdgError, match="unknown basal parameter"):
        abi.basal_default_params(k3=1.0)


def small_case(nx, ny, pk, seed=7):
    """a small box with the thick cover of the shoal case and a shoal in its middle"""
    bt = synthetic.BoxTest(nx, ny, 40e3)
    p = O.mevp_params(**pk)
    H, A = BR.thick_cover(*bt.dg_fields(), seed=seed)
    depth, shoal = BR.shoal_depth(nx, ny, shallow=10.0)
    uo, vo = (np.ascontiguousarray(a) for a in bt.ocean())
    ua, va = (np.ascontiguousarray(3.0 * a) for a in bt.wind(0.0))
    c = dict(bt=bt, p=p, H=H, A=A, depth=depth, shoal=shoal, uo=uo, vo=vo)
    c["pg"] = O.ice_strength(nx, ny, p, H, A)
    c["cgh"], c["cga"] = O.dg_to_cg(nx, ny, H), O.dg_to_cg(nx, ny, A)
    c["tax"], c["tay"] = O.wind_stress(p, ua, va)
    return c


@pytest.mark.parametrize("pk", [UNIFORM, ADAPTIVE], ids=["uniform", "adaptive"])
def test_the_two_forms_of_the_reference_agree(pk):
    """the oracle form and the pure-Python form (tests/dyn_independent.py) of the corrected sub-iteration on an 8 x 6 box, three
    sub-iterations from a random state.  Their largest difference, relative to the largest speed, is printed: it is the spread the two CPU forms
    show among themselves, the yardstick of the device tests' tolerance rule.  Bound: 1e-12 per sub-iteration is what
    test_oracle_dynamics.test_oracle_agrees_with_the_independent_restatement holds ONE uncorrected sub-iteration to; three of them and
    the factor (a quotient of sums restated in both forms from the same numpy code) stay within 1e-11"""
    import dyn_independent as DI

    nx, ny, nsub = 8, 6, 3
    c = small_case(nx, ny, pk)
    bp = BR.basal_par()
    shape = c["uo"].shape
    rng = np.random.default_rng(3)
    ustart, vstart = 0.02 * rng.standard_normal(shape), 0.02 * rng.standard_normal(shape)
    for a in (ustart, vstart):
        a[0] = a[-1] = 0
        a[:, 0] = a[:, -1] = 0
    u0, v0 = 0.9 * ustart, 0.9 * vstart
    u, v = ustart.copy(), vstart.copy()
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    args = (c["tax"], c["tay"], c["uo"], c["vo"], c["cgh"], c["cga"])
    tb = BR.subcycle(nx, ny, c["bt"].hx, c["bt"].hy, DT, nsub, c["p"], bp, c["depth"], None, s, u, v, u0, v0, *args, c["pg"])
    assert tb.max() > 1.0 and (tb == 0).sum() > tb.size // 3  # grounded over the shoal, nothing in deep water
    par = {k: getattr(c["p"], k) for k in DI.PARAMS}
    par.update({k: getattr(c["p"], k) for k in ("aevp_c", "aevp_alpha_min")})
    S2, u2, v2 = BR.python_subcycle(par, bp, c["bt"].hx, c["bt"].hy, DT, nsub, c["depth"], [np.zeros((8, ny, nx)) for _ in range(3)], ustart, vstart,
                                    u0, v0, *args, c["pg"])
    scale = max(np.max(np.abs(u)), np.max(np.abs(v)))
    assert scale > 1e-3
    spread = max(np.max(np.abs(u - u2)), np.max(np.abs(v - v2))) / scale
    sspread = max(np.max(np.abs(a - b)) for a, b in zip(s, S2)) / max(np.max(np.abs(a)) for a in s)
    print("largest difference of the two CPU forms: velocity %.3g of the largest speed, stress %.3g of the largest coefficient" % (spread, sspread))
    assert spread < 1e-11 and sspread < 1e-11


def test_critical_stress_against_hand_values():
    """four nodes of a 2 x 1 array with uniform cover per case: deep water, grounded, a = 0 and ice-free"""
    p = O.mevp_params()
    bp = BR.basal_par()
    shape = (3, 5)
    full = lambda x: np.full(shape, float(x))
    # deep: h = 2, a = 0.9, 1000 m: h_c = 0.9 * 1000 / 8 = 112.5 > h
    assert np.all(BR.critical_stress(p, bp, full(2.0), full(0.9), full(1000.0)[:1, :2]) == 0.0)
    # grounded: h = 2, a = 0.9, 10 m: h_c = 1.125, T_b = 15 * 0.875 * exp(-2)
    tb = BR.critical_stress(p, bp, full(2.0), full(0.9), full(10.0)[:1, :2])
    assert np.allclose(tb, 15.0 * 0.875 * np.exp(-2.0), rtol=1e-15) and abs(tb[1, 2] - 1.7762755925) < 1e-9
    # the depth of a node is the mean over its elements: 10 m and 20 m side by side give 15 m on the shared edge
    tb = BR.critical_stress(p, bp, full(2.0), full(0.9), np.array([[10.0, 20.0]]))
    want = lambda hw: 15.0 * max(0.0, 2.0 - 0.9 * hw / 8.0) * np.exp(-2.0)
    assert np.allclose(tb[:, :2], want(10.0), rtol=1e-15) and np.allclose(tb[:, 2], want(15.0), rtol=1e-15) and np.allclose(tb[:, 3:], want(20.0))
    # a = 0 with ice (the rule off): h_c = 0, T_b = 15 h exp(-20)
    off = O.mevp_params(min_conc=0.0, min_thick=0.0)
    assert np.allclose(BR.critical_stress(off, bp, full(2.0), full(0.0), full(10.0)[:1, :2]), 30.0 * np.exp(-20.0), rtol=1e-15)
    # ice-free (the rule on, a below min_conc; h at the mass floor; thin true thickness): 0 whatever the formula says
    assert np.all(BR.critical_stress(p, bp, full(2.0), full(0.0), full(10.0)[:1, :2]) == 0.0)
    assert np.all(BR.critical_stress(p, bp, full(p.h_min), full(0.9), full(0.0)[:1, :2]) == 0.0)
    assert np.all(BR.critical_stress(p, bp, full(0.005), full(0.9), full(0.0)[:1, :2]) == 0.0)
    # land takes precedence
    land = np.array([[True, False]])
    tb = BR.critical_stress(p, bp, full(2.0), full(0.9), full(10.0)[:1, :2], land)
    assert np.all(tb[:, :3] == 0.0) and np.all(tb[:, 3:] > 1.0)
    # the thickness is NOT raised to h_min: h below every h_c gives 0, not k2 (h_min - h_c)
    assert np.all(BR.critical_stress(off, bp, full(0.0), full(0.9), full(0.0)[:1, :2]) == 0.0)


@pytest.mark.parametrize("hw,grounded", [(6.0, False), (2.0, True)])
def test_strengthless_cover_relaxes_to_the_balance_with_seabed_stress(hw, grounded):
    """P* = 0, f_c = 0, ocean at rest: every interior node is on its own and the steady state of the sweep is the root of
        (c_d |u| + T_b / (|u| + u0)) u = a tau_a,
    modelled on test_oracle_dynamics.test_strengthless_cover_reaches_the_free_drift_of_the_literature (same case, same 70 steps of 30
    sub-iterations, same 1e-10).  Over 6 m of water a |tau_a| > T_b and the ice moves (the balance's own time scale m / (2 c_d |u|) is
    ~500 s there, one model step; closer to T_b = a |tau_a| it grows beyond what 70 steps converge); over 2 m a |tau_a| < T_b and the
    speed stays below u0 a |tau_a| / (T_b - a |tau_a|)"""
    from scipy.optimize import brentq

    from test_oracle_dynamics import free_drift_case

    nx, ny = 6, 5
    hx, hy, ua, va, _, _, cgh, cga = free_drift_case(nx, ny)
    uo, vo = np.zeros_like(ua), np.zeros_like(ua)
    p = O.mevp_params(pstar=0.0, fc=0.0, alpha=5.0, beta=5.0)
    bp = BR.basal_par()
    tax, tay = O.wind_stress(p, ua, va)
    depth = np.full((ny, nx), hw)
    pg = np.zeros((9, ny, nx))
    u, v = np.zeros_like(ua), np.zeros_like(ua)
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    for _ in range(70):
        tb = BR.subcycle(nx, ny, hx, hy, 600.0, 30, p, bp, depth, None, s, u, v, u.copy(), v.copy(), tax, tay, uo, vo, cgh, cga, pg)
    h, a = 0.7, 0.85
    T = 15.0 * (h - a * hw / 8.0) * np.exp(-20.0 * (1.0 - a))
    assert np.allclose(tb, T, rtol=1e-14) and T > 0
    tau = a * p.c_atm * p.rho_atm * np.hypot(9.0, -4.0) ** 2
    cd = a * p.c_ocean * p.rho_ocean
    speed = brentq(lambda x: cd * x * x + T * x / (x + bp["u0"]) - tau, 0.0, 10.0, xtol=1e-16, rtol=1e-15)
    want = speed * np.array([9.0, -4.0]) / np.hypot(9.0, -4.0)
    ui, vi = u[1:-1, 1:-1], v[1:-1, 1:-1]
    print("depth %g m: T_b = %.4g, a |tau_a| = %.4g, steady speed %.4g m/s" % (hw, T, tau, speed))
    assert np.max(np.abs(ui - want[0])) < 1e-10 and np.max(np.abs(vi - want[1])) < 1e-10
    assert (tau < T) == grounded
    if grounded:
        assert 0 < np.max(np.hypot(ui, vi)) < bp["u0"] * tau / (T - tau) < 5e-4  # fast by Lemieux's criterion
    else:
        assert np.min(np.hypot(ui, vi)) > 1e-2


@pytest.mark.parametrize("pk", [UNIFORM, ADAPTIVE], ids=["uniform", "adaptive"])
def test_the_shoal_case_of_the_device_tests_needs_the_term(pk):
    """the case tests/test_gpu_basal.py runs: 10 m of water under H ~ 2 m, A ~ 0.95 inside 1000 m, 48 x 40, 25 sub-iterations, with the
    shapes of land_ref.shapes_mask.  The reference with the term and the reference without it differ by more than 10 % of the largest
    speed over the shoal: a device result that lost the term cannot pass against the first"""
    nx, ny = 48, 40
    bt = synthetic.BoxTest(nx, ny)
    p = O.mevp_params(**pk)
    land = land_ref.shapes_mask(nx, ny)
    H, A = BR.thick_cover(*bt.dg_fields())
    H[:, land] = 0.0
    A[:, land] = 0.0
    depth, shoal = BR.shoal_depth(nx, ny)
    uo, vo = (np.ascontiguousarray(a) for a in bt.ocean())
    ua, va = (np.ascontiguousarray(a) for a in bt.wind(0.0))
    pg = O.ice_strength(nx, ny, p, H, A)
    cgh, cga = O.dg_to_cg(nx, ny, H), O.dg_to_cg(nx, ny, A)
    tax, tay = O.wind_stress(p, ua, va)
    res = {}
    for basal in (True, False):
        u, v = np.zeros_like(uo), np.zeros_like(uo)
        s = [np.zeros((8, ny, nx)) for _ in range(3)]
        tb = BR.subcycle(nx, ny, bt.hx, bt.hy, DT, 25, p, BR.basal_par(), depth, land, s, u, v, u, v, tax, tay, uo, vo, cgh, cga, pg, basal=basal)
        res[basal] = np.hypot(u, v)
    sn = BR.shoal_nodes(shoal) & ~land_ref.land_nodes(land)
    assert sn.sum() > 100 and tb[sn].min() > 1.0 and tb[~land_ref.land_nodes(shoal)].max() == 0.0
    top = res[False][sn].max()
    diff = np.max(np.abs(res[True] - res[False])[sn])
    print("largest speed over the shoal: %.3g m/s without the term, %.3g with it; largest difference %.3g" % (top, res[True][sn].max(), diff))
    assert top > 1e-4 and diff > 0.1 * top
    assert res[True][sn].max() < 0.5 * top


# ---- the row-block driver on the reference ------------------------------------------------------------------------------------------
NXD, NYD, NSUBD = 20, 29, 9


def driver_case():
    bt = synthetic.BoxTest(NXD, NYD)
    H, A = BR.thick_cover(*bt.dg_fields(), seed=41)
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    # a shoal across the block boundaries of worlds 2 (row 14) and 3 (rows 9, 19)
    depth, shoal = BR.shoal_depth(NXD, NYD, box=(7, 21, 5, 12))
    return bt, H, A, np.ascontiguousarray(uo), np.ascontiguousarray(vo), np.ascontiguousarray(3.0 * ua), np.ascontiguousarray(3.0 * va), depth, shoal


def driver_land():
    m = np.zeros((NYD, NXD), dtype=bool)
    m[12:16, 10:14] = True  # an island that cuts into the shoal, across the boundary of world 2
    return m


def run_core(rank, world, pk, nsteps=2, **kw):
    bt, H, A, uo, vo, ua, va, depth, _ = driver_case()
    blk = rowblock.RowBlock(NXD, NYD, rank, world, 1, 1)
    core = rowblock.DynamicsCore(BR.BasalOracleOps(**pk), blk, bt.hx, bt.hy, DT, NSUBD, torch.device("cpu"), bathymetry=depth, land=driver_land(), **kw)
    core.load_global(H, A, uo, vo, ua, va)
    for _ in range(nsteps):
        core.step()
    return core


@pytest.mark.parametrize("pk", [UNIFORM, ADAPTIVE], ids=["uniform", "adaptive"])
def test_driver_on_the_reference_holds_the_shoal_and_reads_the_critical_stress(pk):
    bt, H, A, uo, vo, ua, va, depth, shoal = driver_case()
    land = driver_land()
    core = run_core(0, 1, pk)
    plain = rowblock.DynamicsCore(BR.BasalOracleOps(**pk), rowblock.RowBlock(NXD, NYD), bt.hx, bt.hy, DT, NSUBD, torch.device("cpu"), land=land)
    plain.load_global(H, A, uo, vo, ua, va)
    for _ in range(2):
        plain.step()
    sn = BR.shoal_nodes(shoal) & ~land_ref.land_nodes(land)
    fast, free = np.hypot(core.u.numpy(), core.v.numpy())[sn], np.hypot(plain.u.numpy(), plain.v.numpy())[sn]
    assert free.max() > 1e-4 and fast.max() < 0.5 * free.max()
    tb = core.basal_read().numpy()
    want = BR.critical_stress(core.ops.p, BR.basal_par(), O.dg_to_cg(NXD, NYD, core.H.numpy()), O.dg_to_cg(NXD, NYD, core.A.numpy()),
                              np.where(land, 0.0, depth), land)
    assert np.array_equal(tb, want) and tb[sn].min() > 1.0 and np.all(tb[land_ref.land_nodes(land)] == 0.0)
    core.close()
    plain.close()
    assert core.ops.depth is None  # close() leaves the ops object without a depth array
    with pytest.raises(ValueError, match="bathymetry="):
        plain.basal_read()


def test_driver_argument_checks():
    from oracle_ops import OracleOps

    bt = synthetic.BoxTest(8, 8)
    mk = lambda ops, **kw: rowblock.DynamicsCore(ops, rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu"), **kw)
    good = np.full((8, 8), 50.0)
    with pytest.raises(ValueError, match="set_basal_depth"):
        mk(OracleOps(), bathymetry=good)
    with pytest.raises(ValueError, match=r"\[8, 8\]"):
        mk(BR.BasalOracleOps(), bathymetry=np.zeros((8, 7)))
    for bad in (-1.0, np.nan, np.inf):
        d = good.copy()
        d[3, 5] = bad
        with pytest.raises(ValueError, match=r"row 3, column 5"):
            mk(BR.BasalOracleOps(), bathymetry=d)
        land = np.zeros((8, 8), dtype=bool)
        land[3, 5] = True
        core = mk(BR.BasalOracleOps(), bathymetry=d, land=land)  # on land the value is not looked at and stored as 0
        assert float(core.depth[3, 5]) == 0.0 and float(core.depth[3, 4]) == 50.0
        core.close()
    with pytest.raises(ValueError, match="need bathymetry="):
        mk(BR.BasalOracleOps(), basal=BR.basal_par())
    # parameters reach the ops object with the grid; no bathymetry: nothing is asked of it
    core = mk(BR.BasalOracleOps(), bathymetry=good, basal=BR.basal_par(k2=3.0))
    core._set_grid()
    assert core.ops.bp["k2"] == 3.0 and core.ops.depth is not None
    core.close()
    mk(OracleOps()).close()


def worker(rank, world, port, outdir, adaptive):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = run_core(rank, world, ADAPTIVE if adaptive else UNIFORM)
        out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
        out["s11"] = core.owned(core.s[0]).clone()
        out["tb"] = core.basal_read().clone()
        torch.save(out, os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,adaptive", [(2, False), (3, False), (3, True)])
def test_row_blocks_with_a_shoal_equal_the_single_domain_bitwise(world, adaptive, tmp_path):
    from test_rowblock_gloo import free_port

    ref = run_core(0, 1, ADAPTIVE if adaptive else UNIFORM)
    assert float(ref.u.abs().max()) > 1e-5
    mp.spawn(worker, args=(world, free_port(), str(tmp_path), adaptive), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(world)]
    for key, full in (("H", ref.H), ("A", ref.A), ("s11", ref.s[0])):
        assert torch.equal(torch.cat([p[key] for p in parts], dim=1), full), key
    for key, full in (("u", ref.u), ("v", ref.v), ("tb", ref.basal_read())):
        assert torch.equal(torch.cat([p[key] for p in parts], dim=0), full), key

"""The default mEVP pass and the transport march against the CPU oracle at the sizes the benchmark and the hosts run.

The launch geometry of the default kernels follows from the grid and the number of CUs: strip heights and dispatch rounds that
the small oracle-compared grids of tests/test_gpu_parity.py and tests/test_gpu_adaptive.py never reach (there: strips of 1 row
in the mEVP pass, of 4 rows in the march).  Here the oracle is the OpenMP build of oracle/dyn_oracle.c (bit-identical to the
serial one: tests/test_oracle_dynamics.py::test_openmp_oracle_is_bitwise_the_serial_oracle).  Strip heights stay automatic.  Each
test names the geometry its shapes reach on 256 CUs (an MI355X) and checks its statement against the rule replicated below, so a
change of the rule shows up here.  Element-wise parity holds for short sub-cycles only (a sub-cycle of 120 sub-iterations from
rest amplifies a relative 1e-15 perturbation to 1e-4 at 1024^2): the cases run 4 to 8 sub-iterations."""
import gc

import numpy as np
import pytest
import torch

import oracle_lib as O
from nextsimdg_amd import abi, rowblock, synthetic
from oracle_ops import OracleOps
from test_gpu_parity import adv_on_device, assert_close, dev, host, thost

pytestmark = pytest.mark.gpu

DT = 120.0
L = 512e3
# tests/test_gpu_adaptive.py::test_adaptive_subcycle_matches_oracle holds 25 sub-iterations to rtol 1e-9, atol 1e-10 max|f|; 8 from rest
# amplify round-off far less (1e-13 of max|f| for a 1e-15 input perturbation at 1024^2)
RTOL, ATOL = 1e-10, 1e-11
MODES = ("adaptive", "keep_delta_min")
BOUNDS = abi.H_A_BOUNDS  # the closure's fields: H in [0, inf), A in [0, 1] with the cell mean capped at 1


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
    ctx.set_mevp_occupancy(1)
    ctx.set_transport_variant(abi.DEFAULT_TRANSPORT_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_transport_bounds(())
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ launch rules (replicated)
def cdiv(a, b):
    return -(-a // b)


def fused4_geometry(cus, nx, ny, nst):
    """(R, workgroups, rounds) of nsdg_launch_mevp_fused4_ranges (csrc/mevp_fused4.hip) on one row range, automatic strip height"""
    ncw, extra = cdiv(nx, 57), 4 * nst - 3
    best, R = None, 64
    for r in range(1, 4097):
        groups = cdiv(ny, r) * ncw
        cost = cdiv(groups, cus) * (r + extra)
        if best is None or cost < best:
            best, R = cost, r
        if groups <= ncw:
            break
    groups = cdiv(ny, R) * ncw
    return R, groups, cdiv(groups, cus)


def fused_geometry(cus, nx, ny):
    """(R, waves, rounds) of nsdg_launch_mevp_fused (csrc/mevp_fused.hip, variant 1): 63 owned columns per wave, 2 waves per SIMD"""
    ncw, slots = cdiv(nx, 63), 8 * cus
    best, R = None, 4
    for r in range(2, 65):
        rounds = cdiv(cdiv(ny, r) * ncw, slots)
        cost = rounds * (r + 1.0) + (1.5 if rounds == 1 else 0.0)
        if best is None or cost < best:
            best, R = cost, r
    waves = cdiv(ny, R) * ncw
    return R, waves, cdiv(waves, slots)


def march_geometry(cus, nx, ny, order):
    """(R, waves) of launch_march (csrc/transport.hip): 64 - 2 (order + 1) owned columns per wave, strips cut for 4 waves per CU"""
    ncw = cdiv(nx, 64 - 2 * (order + 1))
    R = max(4, cdiv(ny, max(1, 4 * cus // ncw)))
    return R, ncw * cdiv(ny, R)


def check_geometry(ctx, got, stated, what):
    """the geometry a docstring states for 256 CUs is the one the rule gives (on another CU count the rule's own values stand)"""
    if ctx.num_cus() == 256:
        assert got == stated, "%s: the launch rule now gives %s, the docstring states %s" % (what, got, stated)


# ------------------------------------------------------------------------------------ helpers
def cmp(got, want, what, rtol=RTOL, atol=ATOL, spread=0.0):
    """element-wise against the oracle, plane by plane (full-size stress arrays are GBs), atol relative to the field's max.  spread: the
    largest change of the field that a 1-ulp perturbation of an input makes in the oracle itself; where the case amplifies round-off
    beyond atol, 10 x that spread is the absolute part of the limit"""
    scale = float(np.max(np.abs(want)))
    assert np.all(np.isfinite(got)), what
    floor = max(atol * scale, 10.0 * spread)
    what = "%s (oracle's own spread %.2e = %.1e of max|f|)" % (what, spread, spread / scale) if spread else what
    if want.ndim == 2:
        assert_close(got, want, rtol, floor, what)
    else:
        for k in range(want.shape[0]):
            assert_close(got[k], want[k], rtol, floor, "%s, coefficient %d" % (what, k))


def box_fields(nx, ny, seed=5):
    """the box test's H, A (A lowered and H roughened at random, as tests/test_gpu_parity.py Box does), ocean and wind"""
    bt = synthetic.BoxTest(nx, ny, L)
    rng = np.random.default_rng(seed)
    H, A = bt.dg_fields()
    A[0] -= 0.2 * rng.random((ny, nx))
    H[1:] += 0.01 * rng.standard_normal(H[1:].shape)
    uo, vo = [np.ascontiguousarray(a) for a in bt.ocean()]
    ua, va = [np.ascontiguousarray(a) for a in bt.wind(0.0)]
    return bt, H, A, uo, vo, ua, va


def subcycle_inputs(nx, ny, po, H, A, ua, va):
    """ice strength, nodal means and wind stress, from the oracle (the device sub-cycle gets the same numbers)"""
    pg = O.ice_strength(nx, ny, po, H, A, omp=True)
    cgh, cga = O.dg_to_cg(nx, ny, H, omp=True), O.dg_to_cg(nx, ny, A, omp=True)
    tax, tay = O.wind_stress(po, ua, va, omp=True)
    return pg, cgh, cga, tax, tay


def device_subcycle(ctx, nsub, u, v, s, u0, v0, tax, tay, uo, vo, cgh, cga, pg):
    """nsdg_mevp_subcycle from (u, v, s) on the device; returns the host copies of u, v and the stress planes"""
    nx = ctx.nx
    du, dv = dev(u), dev(v)
    ds = [abi.tile(dev(x)) for x in s]
    scratch = torch.zeros(10 * du.numel() + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_subcycle(DT, nsub, ds, du, dv, dev(u0), dev(v0), dev(tax), dev(tay), dev(uo), dev(vo), dev(cgh), dev(cga), abi.tile(dev(pg)),
                      scratch)
    out = [host(du), host(dv)] + [thost(x, nx) for x in ds]
    del du, dv, ds, scratch
    torch.cuda.empty_cache()
    return out


ULP = 1.0 + np.finfo(float).eps  # a relative perturbation of one ulp: the probe of the oracle's own conditioning


def oracle_state(nx, ny):
    shape = (2 * ny + 1, 2 * nx + 1)
    return np.zeros(shape), np.zeros(shape), [np.zeros((8, ny, nx)) for _ in range(3)]


NAMES = ("u", "v", "s11", "s12", "s22")


# ------------------------------------------------------------------------------------ 1. default mEVP pass, launch-geometry shapes
MEVP_SHAPES = {  # (nx, ny): (sub-iteration counts, stated geometry of a four-iteration pass: R, workgroups, rounds)
    (2048, 2048): ((7, 8), (293, 252, 1)),
    (4096, 4096): ((4,), (586, 504, 2)),
    (8192, 64): ((7, 8), (22, 432, 2)),
    (64, 8192): ((7, 8), (64, 256, 1)),
    (512, 2048): ((7, 8), (74, 252, 1)),  # 57 * 9 - 1 columns: 9 windows, the last one owns 56
    (513, 2048): ((7, 8), (74, 252, 1)),  # 57 * 9: 9 full windows
    (514, 2048): ((7, 8), (82, 250, 1)),  # 57 * 9 + 1: a 10th window of one column
}


@pytest.mark.parametrize("shape", list(MEVP_SHAPES), ids=["%dx%d" % s for s in MEVP_SHAPES])
def test_default_mevp_pass_matches_oracle_at_launch_geometry(ctx, shape):
    """nsdg_mevp_subcycle, library default variant 4, automatic strip height, from rest on the box test, adaptive and uniform
    (keep_delta_min) alpha, against the oracle element by element.  Four-iteration passes (256 CUs; the three-iteration remainder
    pass of nsub = 7 gets the same R):
    2048 x 2048: R = 293, 252 workgroups, 1 round (the benchmark); 4096 x 4096 (nsub = 4 only): R = 586, 504 workgroups, 2 rounds;
    8192 x 64: R = 22, 432 workgroups, 2 rounds; 64 x 8192: R = 64, 256 workgroups, 1 round;
    512 / 513 / 514 x 2048 (57 k - 1, 57 k, 57 k + 1 columns): R = 74 / 74 / 82, 252 / 252 / 250 workgroups, 1 round"""
    nx, ny = shape
    counts, stated = MEVP_SHAPES[shape]
    for nst in (4, 3):
        check_geometry(ctx, fused4_geometry(ctx.num_cus(), nx, ny, nst), stated, "%dx%d, %d iterations per pass" % (nx, ny, nst))
    bt, H, A, uo, vo, ua, va = box_fields(nx, ny)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    pg, cgh, cga, tax, tay = subcycle_inputs(nx, ny, O.mevp_params(), H, A, ua, va)  # alpha, beta and Delta_min do not enter
    del H, A
    for mode in MODES:
        sub = bt.subcycle_parameters(DT, mode)
        po = O.mevp_params(**sub)
        ctx.set_mevp_params(ctx.mevp_default_params(**sub))
        ctx.set_grid(nx, ny, bt.hx, bt.hy)
        # the oracle twice: as given and with the nodal mean thickness perturbed by one ulp (its own conditioning: 1e-15 .. 1e-13 of
        # max|f| on square elements; the adaptive form on the 128:1 elements of 8192 x 64 and 64 x 8192 reaches 1e-10)
        runs = [oracle_state(nx, ny), oracle_state(nx, ny)]
        zero = np.zeros_like(runs[0][0])
        done = 0
        for nsub in counts:  # the oracle goes on from the previous count: its sub-cycle keeps no state beyond (u, v, s)
            for (u, v, s), h in zip(runs, (cgh, cgh * ULP)):
                O.mevp_subcycle(nx, ny, bt.hx, bt.hy, DT, nsub - done, po, s, u, v, zero, zero, tax, tay, uo, vo, h, cga, pg, omp=True)
            done = nsub
            z0, z1, zs = oracle_state(nx, ny)
            got = device_subcycle(ctx, nsub, z0, z1, zs, zero, zero, tax, tay, uo, vo, cgh, cga, pg)
            del z0, z1, zs
            want, probe = [[u, v] + s for (u, v, s) in runs]
            assert np.max(np.abs(want[0])) > 1e-9  # the ice moved (1e-7 .. 5e-2 m/s: uniform alpha grows with 1 / h^2)
            for g, w, p, name in zip(got, want, probe, NAMES):
                cmp(g, w, "%dx%d %s nsub=%d %s" % (nx, ny, mode, nsub, name), spread=float(np.max(np.abs(p - w))))
            del got, want, probe
        del runs, zero
        gc.collect()


# ------------------------------------------------------------------------------------ 2. from a developed state
def bench_core(ctx, n, nsub, sub):
    """DynamicsCore as bench.py's build_core makes it on one GPU: library defaults, row block of plan_blocks (ghost depth (4, 3)),
    native driver, closure on, the box test's fields"""
    bt = synthetic.BoxTest(n, n, L)
    ctx.set_mevp_params(ctx.mevp_default_params(**sub))
    blk = rowblock.RowBlock(n, n, 0, 1, 4, 3)
    core = rowblock.DynamicsCore(ctx, blk, L / n, L / n, DT, nsub, torch.device("cuda"), native=True, closure=True)
    H, A = bt.dg_fields()
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    core.load_global(H, A, uo, vo, ua, va)
    return bt, core


def test_default_pass_from_a_developed_state_within_the_oracles_own_spread(ctx):
    """1024 x 1024, the benchmark's configuration (adaptive alpha, 120 sub-iterations, closure, native driver) run for 3 model steps;
    from that state one pass of 4 sub-iterations (variant 4: R = 74, 252 workgroups, 1 round on 256 CUs) on the device and on the
    oracle.  A developed state is noisy at element scale, so the tolerance comes from the oracle's own conditioning: the oracle run
    again with the nodal mean thickness perturbed by one ulp (relative); |device - oracle| <= 10 x that spread + 4 ulp of max|f|"""
    n = 1024
    check_geometry(ctx, fused4_geometry(ctx.num_cus(), n, n, 4), (74, 252, 1), "1024x1024")
    sub = synthetic.BoxTest(n, n, L).subcycle_parameters(DT)
    bt, core = bench_core(ctx, n, 120, sub)
    try:
        for _ in range(3):
            core.step()
        torch.cuda.synchronize()
        H, A = host(core.H), host(core.A)
        u, v = host(core.u), host(core.v)
        s = [thost(x, n) for x in core.s]
        uo, vo, ua, va = host(core.uo), host(core.vo), host(core.ua), host(core.va)
    finally:
        core.close()
        del core
    assert np.max(np.abs(u)) > 1e-3 and np.all(np.isfinite(u))
    po = O.mevp_params(**sub)
    ctx.set_mevp_params(ctx.mevp_default_params(**sub))
    ctx.set_grid(n, n, bt.hx, bt.hy)
    pg, cgh, cga, tax, tay = subcycle_inputs(n, n, po, H, A, ua, va)
    got = device_subcycle(ctx, 4, u, v, s, u, v, tax, tay, uo, vo, cgh, cga, pg)
    runs = []
    for h in (cgh, cgh * ULP):
        uu, vv, ss = u.copy(), v.copy(), [x.copy() for x in s]
        O.mevp_subcycle(n, n, bt.hx, bt.hy, DT, 4, po, ss, uu, vv, u, v, tax, tay, uo, vo, h, cga, pg, omp=True)
        runs.append([uu, vv] + ss)
    for g, w, p, name in zip(got, runs[0], runs[1], NAMES):
        scale = float(np.max(np.abs(w)))
        spread, err = float(np.max(np.abs(p - w))), float(np.max(np.abs(g - w)))
        assert spread > 0, name  # the perturbation reached the field
        assert err <= 10 * spread + 4 * np.finfo(float).eps * scale, (
            "%s: max |device - oracle| %.3e, the oracle's own spread for a 1-ulp change of the nodal H %.3e, max|%s| %.3e" % (name, err, spread, name, scale))


# ------------------------------------------------------------------------------------ 4. the occupancy-2 build of variant 1
@pytest.mark.parametrize("shape", [(2048, 2048), (130, 45)], ids=["2048x2048", "130x45"])
def test_occupancy_2_kernel_matches_occupancy_1_and_the_oracle(ctx, shape):
    """variant 1 (mevp_fused_kernel), automatic strip height, 8 sub-iterations from rest.  Uniform alpha: the 2-waves-per-SIMD build
    (nsdg_mevp_occupancy_set(ctx, 2)) is the 1-wave build bit for bit and the oracle to the tolerance of the default pass; adaptive
    alpha: the setting is ignored, the result is the same.  Geometry (256 CUs): 2048 x 2048: R = 17, 3993 waves, 2 rounds;
    130 x 45: R = 2, 69 waves, 1 round"""
    nx, ny = shape
    stated = {(2048, 2048): (17, 3993, 2), (130, 45): (2, 69, 1)}[shape]
    check_geometry(ctx, fused_geometry(ctx.num_cus(), nx, ny), stated, "%dx%d variant 1" % shape)
    bt, H, A, uo, vo, ua, va = box_fields(nx, ny)
    ctx.set_mevp_variant(1)
    pg, cgh, cga, tax, tay = subcycle_inputs(nx, ny, O.mevp_params(), H, A, ua, va)
    for mode in ("keep_delta_min", "adaptive"):
        sub = bt.subcycle_parameters(DT, mode)
        po = O.mevp_params(**sub)
        ctx.set_mevp_params(ctx.mevp_default_params(**sub))
        ctx.set_grid(nx, ny, bt.hx, bt.hy)
        res = {}
        for occ in (1, 2):
            ctx.set_mevp_occupancy(occ)
            u, v, s = oracle_state(nx, ny)
            res[occ] = device_subcycle(ctx, 8, u, v, s, u, v, tax, tay, uo, vo, cgh, cga, pg)
        ctx.set_mevp_occupancy(1)
        for a, b, name in zip(res[1], res[2], NAMES):
            assert np.array_equal(a, b), "%dx%d %s: occupancy 2 differs from occupancy 1 in %s" % (nx, ny, mode, name)
        if mode == "keep_delta_min":
            u, v, s = oracle_state(nx, ny)
            O.mevp_subcycle(nx, ny, bt.hx, bt.hy, DT, 8, po, s, u, v, u.copy(), v.copy(), tax, tay, uo, vo, cgh, cga, pg, omp=True)
            assert np.max(np.abs(u)) > 1e-9
            for g, w, name in zip(res[2], [u, v] + s, NAMES):
                cmp(g, w, "%dx%d occupancy 2 %s" % (nx, ny, name))
        del res
        gc.collect()


# ------------------------------------------------------------------------------------ 5. transport at full geometry
TRANSPORT_SHAPES = {  # (nx, ny): stated march geometry (R, waves) for DG0, DG1, DG2
    (2048, 2048): ((69, 1020), (71, 1015), (74, 1008)),
    (2047, 2048): ((69, 1020), (71, 1015), (74, 1008)),  # odd nx: the two-elements-per-lane stage kernel falls back
    (8192, 64): ((10, 931), (10, 959), (10, 994)),
    (64, 8192): ((16, 1024), (16, 1024), (16, 1024)),
}


@pytest.mark.parametrize("shape", list(TRANSPORT_SHAPES), ids=["%dx%d" % s for s in TRANSPORT_SHAPES])
def test_transport_matches_oracle_at_launch_geometry(ctx, shape):
    """one DG0 / DG1 / DG2 step of H and A with the closure's bounds (H >= 0; 0 <= A <= 1, cell mean capped) against the oracle's
    transport_step + transport_limit: the one-launch march (nsdg_transport_step_oop) and the staged step (nsdg_transport_step) with
    stage kernel variants 2 (two elements per lane; falls back on an odd nx) and 0.  March geometry (256 CUs), DG0 / DG1 / DG2:
    2048 x 2048 and 2047 x 2048: R = 69 / 71 / 74; 8192 x 64: R = 10; 64 x 8192: R = 16"""
    nx, ny = shape
    for order in (0, 1, 2):
        check_geometry(ctx, march_geometry(ctx.num_cus(), nx, ny, order), TRANSPORT_SHAPES[shape][order], "%dx%d DG%d" % (nx, ny, order))
    rng = np.random.default_rng(nx + 7 * ny)
    hx, hy = 1.0 / nx, 1.0 / ny
    from nextsimdg_amd import basis

    X, Y = basis.node_coords(nx, ny, 1.0, 1.0)
    u = np.ascontiguousarray(np.sin(3 * X) * np.cos(2 * Y) + 0.3)
    v = np.ascontiguousarray(np.cos(2 * X + 1) * np.sin(4 * Y) - 0.2)
    del X, Y
    ctx.set_grid(nx, ny, hx, hy)
    for order in (0, 1, 2):
        nc = basis.NCOEF[order]
        # means and slopes that leave [0, inf) and [0, 1]: the limiter and the cap act in many elements
        H = rng.uniform(-0.2, 2.0, (nc, ny, nx))
        A = rng.uniform(0.3, 1.2, (nc, ny, nx))
        H[1:] *= 0.3
        A[1:] *= 0.3
        dt = 0.1 * min(hx, hy) / 1.5 / (2 * order + 1)
        adv_o = O.prepare_advection(nx, ny, order, u, v, omp=True)
        adv_d = adv_on_device(ctx, nx, ny, order, u, v)
        want = [H.copy(), A.copy()]
        for f, (lo, hi, cap) in zip(want, BOUNDS):
            O.transport_step(nx, ny, hx, hy, order, dt, f, adv_o, omp=True)
            O.transport_limit(nx, ny, order, f, lo, hi, cap, omp=True)
        del adv_o
        assert float(want[1][0].max()) <= 1.0 and not np.array_equal(want[0], H)
        ctx.set_transport_bounds(BOUNDS)
        runs = {}
        fin = [dev(H), dev(A)]
        out = [torch.zeros_like(f) for f in fin]
        ctx.transport_step_oop(order, dt, fin, out, adv_d)
        runs["march"] = out
        del fin
        for tv in (2, 0):
            ctx.set_transport_variant(tv)
            f = [dev(H), dev(A)]
            scratch = torch.zeros(2 * sum(x.numel() for x in f), dtype=torch.float64, device="cuda")
            ctx.transport_step(order, dt, f, adv_d, scratch)
            runs["staged, stage variant %d" % tv] = f
            del scratch
        ctx.set_transport_variant(abi.DEFAULT_TRANSPORT_VARIANT)
        ctx.set_transport_bounds(())
        for what, fields in runs.items():
            for g, w, name in zip(fields, want, ("H", "A")):
                assert_close(host(g), w, 1e-12, 1e-13, "%dx%d DG%d %s %s" % (nx, ny, order, what, name))
        del runs, adv_d, want, H, A
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ 6. one step of the benchmark's driver
def test_one_step_of_the_bench_driver_matches_the_oracle_driver(ctx):
    """2048 x 2048, DynamicsCore exactly as bench.py's build_core makes it (variant 4, native driver, closure, adaptive alpha) but with
    nsub = 8 (two four-iteration passes: R = 293, 252 workgroups, 1 round on 256 CUs; DG2 march R = 74), one model step against the same
    driver on DynamicsCore(OracleOps(omp=True)): nsdg_mevp_prepare, ice strength, the nodal means, the sub-cycle, the advection
    velocities, the transport and the closure through the product's own call sequence"""
    n = 2048
    check_geometry(ctx, fused4_geometry(ctx.num_cus(), n, n, 4), (293, 252, 1), "2048x2048")
    sub = synthetic.BoxTest(n, n, L).subcycle_parameters(DT)
    bt, core = bench_core(ctx, n, 8, sub)
    try:
        core.step()
        torch.cuda.synchronize()
        got = dict(H=host(core.H), A=host(core.A), u=host(core.u), v=host(core.v))
        got.update({k: thost(x, n) for k, x in zip(NAMES[2:], core.s)})
    finally:
        core.close()
        del core
        torch.cuda.empty_cache()
    ref = rowblock.DynamicsCore(OracleOps(omp=True, **sub), rowblock.RowBlock(n, n), L / n, L / n, DT, 8, torch.device("cpu"))
    H, A = bt.dg_fields()
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    ref.load_global(H, A, uo, vo, ua, va)
    ref.step()
    want = dict(H=ref.H.numpy(), A=ref.A.numpy(), u=ref.u.numpy(), v=ref.v.numpy())
    want.update({k: x.numpy() for k, x in zip(NAMES[2:], ref.s)})
    assert np.max(np.abs(want["u"])) > 1e-6
    for k, w in want.items():
        cmp(got[k], w, "bench driver step, %s" % k)

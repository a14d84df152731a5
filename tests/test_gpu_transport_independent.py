"""Every kernel and entry point of csrc/transport.hip held to the independent restatement tests/transport_independent.py -- not to the
oracle -- at the orders 0, 1 and 2, through the C ABI: prepare_advection, the bare stage under both stage kernels and every
workgroup height, the staged in-place step, the marching step (nsdg_transport_step_oop) with and without its closure epilogue for
1, 2 and 4 fields, the march on row ranges, and the march against the analytic solution of a polynomial in a uniform flow.

The velocity is random and non-zero on the whole boundary, with inflow and outflow on every side (tests/transport_cases.py); the
device prepares its own advection arrays, as production does, the restatement its own.  The grids are the smallest at which each
kernel can go wrong: around the column window of the march (OWN = 62 / 60 / 58 columns at the orders 0 / 1 / 2), across its
4-row strips, at the 64-lane block edge of the stage and pair kernels, with an odd nx (variant 2 falls back), and degenerate ones.

Bound: rtol 1e-12, atol 1e-13 max|want| per array, the one the device meets against the oracle on three transport steps
(test_gpu_parity.py::test_prepare_advection_and_transport_match_oracle); the oracle lies within 0.014 of it against the
restatement (tests/test_transport_independent_cpu.py).  Polynomial exactness: atol 1e-13 max|want| on the compared zone.

Largest observed ratio of the device's distance from the restatement to that bound, per order (MI355X):
    order 0: 0.0071    order 1: 0.0054    order 2: 0.017    (all 192 cases; the oracle's own, same cases: 0.0080, 0.0071, 0.025)
and of the error of the polynomial test to its bound: 0 (order 0), 0.0042 (order 1), 0.025 (order 2)."""
import functools

import numpy as np
import pytest
import torch

import transport_cases as TC
import transport_independent as TI
from nextsimdg_amd import abi

pytestmark = pytest.mark.gpu

HX, HY = TC.HX, TC.HY
SENTINEL = -7.0
CASES = [pytest.param(order, nx, ny, id="p%d-%dx%d" % (order, nx, ny)) for order in (0, 1, 2) for nx, ny in TC.shapes(order)]
WORST = {}  # order -> largest ratio to the bound seen in this session


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()
    for order in sorted(WORST):
        print("\ntransport against the restatement, order %d: largest ratio to the bound %.3g" % (order, WORST[order]))


@pytest.fixture(autouse=True)
def _default_variant_and_no_bounds_afterwards(ctx):
    yield
    ctx.set_transport_variant(abi.DEFAULT_TRANSPORT_VARIANT, 0)
    ctx.set_transport_bounds(())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def filled(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")


def check(order, got, want, what):
    r = TC.ratio(got, want)
    WORST[order] = max(WORST.get(order, 0.0), r)
    print("order %d %s: %.3g of the bound" % (order, what, r))
    assert r <= 1.0, "%s: %.3g times the bound (rtol %g, atol %g max|want|)" % (what, r, TC.RTOL, TC.ATOL_OF_MAX)


def adv_on_device(ctx, nx, ny, order, u, v):
    ng, nc = order + 1, TC.NCOEF[order]
    adv = (filled(nc, ny, nx), filled(nc, ny, nx), filled(ng, ny, nx + 1), filled(ng, ny + 1, nx))
    ctx.prepare_advection(order, dev(u), dev(v), *adv)
    return adv


@functools.lru_cache(maxsize=None)
def reference(order, nx, ny):
    """the restatement's side of a case, computed once and shared by the tests (nobody writes to it): velocity, time step, advection
    arrays, four fields, and three steps of each field without a closure and with the closure BOUNDS[f] after every step"""
    u, v = TC.velocity(nx, ny, 7 * nx + ny)
    dt, adv = TC.time_step(u, v), TI.advection(u, v, nx, ny, order)
    fields = [TC.bounded_field(nx, ny, order, f, 11) for f in range(4)]
    free, bounded = [], []
    for f, F in enumerate(fields):
        a, b = [F], [F]
        for n in range(3):
            a.append(TI.step(a[-1], adv, HX, HY, dt, order))
            new = TI.step(b[-1], adv, HX, HY, dt, order)
            lim = TI.limit(new, *TC.BOUNDS[f], order)
            if n == 0:  # the closure works on both sides of every seam of the march
                TC.assert_closure_active_at_the_seams(nx, ny, order, f, new, lim)
            b.append(lim)
        free.append(a)
        bounded.append(b)
    return dict(u=u, v=v, dt=dt, adv=adv, fields=fields, free=free, bounded=bounded)


def moved(new, old):
    return float(np.abs(new - old).max()) > 0.0


# ------------------------------------------------------------------------------------------------ the advecting velocity
@pytest.mark.parametrize("order,nx,ny", CASES)
def test_prepare_advection(ctx, order, nx, ny):
    """all four arrays, the last edge column of un_x and the last edge row of un_y included (only the elements of the last column and
    row write them: the arrays start at a sentinel)"""
    R = reference(order, nx, ny)
    ctx.set_grid(nx, ny, HX, HY)
    got = [host(a) for a in adv_on_device(ctx, nx, ny, order, R["u"], R["v"])]
    for g, w, name in zip(got, R["adv"], ("vx_dg", "vy_dg", "un_x", "un_y")):
        check(order, g, w, name)
    check(order, got[2][:, :, -1], R["adv"][2][:, :, -1], "last edge column of un_x")
    check(order, got[3][:, -1, :], R["adv"][3][:, -1, :], "last edge row of un_y")
    assert np.abs(R["adv"][2][:, :, -1]).min() > 0.0 and np.abs(R["adv"][3][:, -1, :]).min() > 0.0


# ------------------------------------------------------------------------------------------------ the bare stage
@pytest.mark.parametrize("order,nx,ny", CASES)
def test_stage_under_both_kernels_and_every_workgroup_height(ctx, order, nx, ny):
    """nsdg_transport_stage with (a, b) = (0.75, 0.25) on two fields: the one-element-per-lane kernel (variant 0) and the pair kernel
    (variant 2; an odd nx falls back) with 0 (default), 1 and 3 rows per workgroup; and a row range inside the array, whose outside
    stays untouched"""
    R = reference(order, nx, ny)
    ctx.set_grid(nx, ny, HX, HY)
    adv = adv_on_device(ctx, nx, ny, order, R["u"], R["v"])
    phi0 = [TC.random_field(nx, ny, order, 21 + f) for f in range(2)]
    phis = [TC.random_field(nx, ny, order, 31 + f) for f in range(2)]
    want = [TI.stage(phi0[f], phis[f], R["adv"], HX, HY, R["dt"], 0.75, 0.25, order) for f in range(2)]
    d0, ds = [dev(p) for p in phi0], [dev(p) for p in phis]
    for f in range(2):
        assert moved(want[f], 0.75 * phi0[f] + 0.25 * phis[f])
    for variant in (0, 2):
        for rows in (0, 1, 3):
            ctx.set_transport_variant(variant, rows)
            out = [filled(*phis[0].shape) for _ in range(2)]
            ctx.transport_stage(order, 0, ny, R["dt"], 0.75, 0.25, d0, ds, out, adv)
            for f in range(2):
                check(order, host(out[f]), want[f], "stage, variant %d, %d rows, field %d" % (variant, rows, f))
    if ny >= 3:
        for variant in (0, 2):
            ctx.set_transport_variant(variant, 0)
            out = [filled(*phis[0].shape) for _ in range(2)]
            ctx.transport_stage(order, 1, ny - 1, R["dt"], 0.75, 0.25, d0, ds, out, adv)
            for f in range(2):
                got = host(out[f])
                check(order, got[:, 1:ny - 1], want[f][:, 1:ny - 1], "stage on the rows [1, %d), variant %d" % (ny - 1, variant))
                assert np.all(got[:, 0] == SENTINEL) and np.all(got[:, ny - 1] == SENTINEL)


# ------------------------------------------------------------------------------------------------ the staged step, in place
@pytest.mark.parametrize("order,nx,ny", CASES)
def test_staged_step_in_place(ctx, order, nx, ny):
    """nsdg_transport_step: one launch per stage, the last one into the field itself (order 0: into scratch, copied back); two steps of
    two fields without a closure, then one step with the closure as the stand-alone pass that ends the staged step"""
    R = reference(order, nx, ny)
    ctx.set_grid(nx, ny, HX, HY)
    adv = adv_on_device(ctx, nx, ny, order, R["u"], R["v"])
    fields = [dev(F) for F in R["fields"][:2]]
    scratch = filled(2 * sum(f.numel() for f in fields))
    for n in (1, 2):
        ctx.transport_step(order, R["dt"], fields, adv, scratch)
        for f in range(2):
            check(order, host(fields[f]), R["free"][f][n], "staged step %d, field %d" % (n, f))
            assert moved(R["free"][f][n], R["free"][f][n - 1])
    ctx.set_transport_bounds(TC.BOUNDS[:2])
    fields = [dev(F) for F in R["fields"][:2]]
    ctx.transport_step(order, R["dt"], fields, adv, scratch)
    for f in range(2):
        check(order, host(fields[f]), R["bounded"][f][1], "staged step with its closure, field %d" % f)
        assert moved(R["bounded"][f][1], R["fields"][f])


# ------------------------------------------------------------------------------------------------ the march
@pytest.mark.parametrize("closure", [False, True], ids=["bare", "closure"])
@pytest.mark.parametrize("order,nx,ny", CASES)
def test_marching_step(ctx, order, nx, ny, closure):
    """nsdg_transport_step_oop, the production launch: three steps between ping-pong buffers for 1, 2 and 4 fields; without bounds, and
    with bounds that differ from field to field, applied in the kernel's epilogue.  reference() asserts that every bounded field has
    capped, scaled and untouched elements on both sides of every window seam and strip seam"""
    R = reference(order, nx, ny)
    want = R["bounded"] if closure else R["free"]
    ctx.set_grid(nx, ny, HX, HY)
    adv = adv_on_device(ctx, nx, ny, order, R["u"], R["v"])
    for nf in (1, 2, 4):
        ctx.set_transport_bounds(TC.BOUNDS[:nf] if closure else ())
        a, b = [dev(F) for F in R["fields"][:nf]], [filled(*R["fields"][0].shape) for _ in range(nf)]
        for n in (1, 2, 3):
            ctx.transport_step_oop(order, R["dt"], a, b, adv)
            a, b = b, a
            for f in range(nf):
                check(order, host(a[f]), want[f][n], "march of %d field(s), step %d, field %d" % (nf, n, f))
                assert moved(want[f][n], want[f][n - 1])


@pytest.mark.parametrize("j0,j1", [(0, 9), (2, 7), (4, 5), (0, 3), (6, 9)])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_marching_step_on_a_row_range(ctx, order, j0, j1):
    """nsdg_transport_step_oop_rows on the (OWN + 1) x 9 grid: interior blocks with ghost rows and blocks that touch the bottom or the
    top of the array, against the restatement's step on the window of those rows; the rows outside keep the sentinel"""
    nx, ny = TC.OWN[order] + 1, 9
    R = reference(order, nx, ny)
    ctx.set_grid(nx, ny, HX, HY)
    adv = adv_on_device(ctx, nx, ny, order, R["u"], R["v"])
    keep = np.full_like(R["fields"][0], SENTINEL)
    for closure in (False, True):
        ctx.set_transport_bounds(TC.BOUNDS[:2] if closure else ())
        a, b = [dev(F) for F in R["fields"][:2]], [filled(*keep.shape) for _ in range(2)]
        ctx.transport_step_oop_rows(order, j0, j1, R["dt"], a, b, adv)
        for f in range(2):
            want = TI.step_rows(R["fields"][f], R["adv"], HX, HY, R["dt"], order, j0, j1, keep, TC.BOUNDS[f] if closure else None)
            got = host(b[f])
            check(order, got[:, j0:j1], want[:, j0:j1], "rows [%d, %d), field %d, closure %d" % (j0, j1, f, closure))
            assert np.array_equal(got[:, :j0], want[:, :j0]) and np.array_equal(got[:, j1:], want[:, j1:])
            assert moved(want[:, j0:j1], R["fields"][f][:, j0:j1])


# ------------------------------------------------------------------------------------------------ the analytic solution
@pytest.mark.parametrize("sign", TC.SIGNS, ids=["++", "--", "+-", "-+"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_march_advects_a_polynomial_exactly(ctx, order, sign):
    """the production kernel against the analytic solution with nothing in between: a global polynomial of total degree <= p in a
    uniform flow, one step on the (OWN + 1) x 13 grid; the new coefficients are those of the shifted polynomial -- written out by hand
    in transport_cases.poly_coefficients -- in every element further than p + 1 cells from the inflow sides"""
    nx, ny = TC.OWN[order] + 1, 13
    u, v, ux, vy, dt = TC.uniform_velocity(nx, ny, sign)
    zone = TC.exact_zone(nx, ny, order, 1, sign)
    assert 2 * zone.sum() >= nx * ny
    phi = TC.poly_coefficients(order, nx, ny)
    want = TC.poly_coefficients(order, nx, ny, ux * dt, vy * dt)
    ctx.set_grid(nx, ny, HX, HY)
    adv = adv_on_device(ctx, nx, ny, order, u, v)
    out = filled(*phi.shape)
    ctx.transport_step_oop(order, dt, [dev(phi)], [out], adv)
    got = host(out)
    tol = 1e-13 * np.abs(want).max()
    err = float(np.abs(got - want)[:, zone].max())
    print("order %d signs %s: error %.3g of the bound %.3g" % (order, sign, err, tol))
    assert err <= tol
    assert moved(got, phi)
    assert order == 0 or moved(want, phi)

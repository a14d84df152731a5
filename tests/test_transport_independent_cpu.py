"""The CPU oracle's DG transport (oracle/dyn_oracle.c) held to the independent restatement tests/transport_independent.py at the orders
0, 1 and 2, with an open boundary: advecting velocity, a bare stage, full steps, the closure, a step on a row range -- and both held
to the ANALYTIC solution of a polynomial in a uniform flow, which depends on no table at all.  No GPU.

Bound: the one the device meets against the oracle on three transport steps (tests/test_gpu_parity.py), rtol 1e-12 and
atol 1e-13 max|want| per array.  Measured when this was written: the oracle's largest distance is 0.0062 / 0.0053 / 0.014 of that bound
at the orders 0 / 1 / 2; the polynomial (max|phi| = 55) is reproduced within 0 / 0.0082 / 0.054 of
its bound by the oracle and 0 / 0.0075 / 0.035 by the restatement."""
import numpy as np
import pytest

import oracle_lib as O
import transport_cases as TC
import transport_independent as TI

HX, HY = TC.HX, TC.HY
GRIDS = ((61, 9), (13, 11), (2, 3), (1, 1))  # one window seam of the march at every order; small; no interior element; one element


def check(got, want, what):
    r = TC.ratio(got, want)
    assert r <= 1.0, "%s: %.3g times the bound (rtol %g, atol %g max|want|)" % (what, r, TC.RTOL, TC.ATOL_OF_MAX)
    return r


def case(nx, ny, order):
    u, v = TC.velocity(nx, ny, 1000 * order + 10 * nx + ny)
    return u, v, TC.time_step(u, v), O.prepare_advection(nx, ny, order, u, v), TI.advection(u, v, nx, ny, order)


def test_restatement_imports_nothing_of_the_project():
    import ast
    import inspect

    names = set()
    for node in ast.walk(ast.parse(inspect.getsource(TI))):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names == {"numpy"}, names


def test_the_comparison_notices_one_element_off_by_1e_minus_9():
    """the bound is sharp enough for what it is used for: one coefficient of one element next to a window seam off by 1e-9 of the
    array's maximum fails it, a perturbation of 1e-14 of the maximum does not"""
    want = TC.random_field(61, 9, 2, 5)
    for eps, ok in ((1e-9, False), (1e-14, True)):
        got = want.copy()
        got[3, 4, TC.OWN[2]] += eps * np.abs(want).max()
        assert (TC.ratio(got, want) <= 1.0) == ok


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("order", [0, 1, 2])
def test_velocity_on_all_four_sides_with_both_signs(order, nx, ny):
    u, v = TC.velocity(nx, ny, 1000 * order + 10 * nx + ny)
    for side in (u[:, 0], u[:, -1], v[0, :], v[-1, :]):
        assert side.min() < 0.0 < side.max()


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("order", [0, 1, 2])
def test_oracle_advection_stage_and_steps(order, nx, ny):
    """the advection arrays (the last edge column and row included), one bare stage with (a, b) = (0.75, 0.25), three full steps"""
    u, v, dt, adv_o, adv_i = case(nx, ny, order)
    for got, want, name in zip(adv_o, adv_i, ("vx_dg", "vy_dg", "un_x", "un_y")):
        check(got, want, name)
    assert np.abs(adv_i[2][:, :, -1]).min() > 0.0 and np.abs(adv_i[3][:, -1, :]).min() > 0.0  # the last edge column / row are live
    phi0, phis = TC.random_field(nx, ny, order, 1), TC.random_field(nx, ny, order, 2)
    out = np.full_like(phis, -7.0)
    O.transport_stage(nx, ny, 0, ny, HX, HY, order, dt, 0.75, 0.25, phi0, phis, out, adv_o)
    want = TI.stage(phi0, phis, adv_i, HX, HY, dt, 0.75, 0.25, order)
    check(out, want, "bare stage")
    assert np.abs(want - 0.75 * phi0 - 0.25 * phis).max() > 0.0
    phi = TC.random_field(nx, ny, order, 3)
    got, want = phi.copy(), phi
    for n in range(3):
        O.transport_step(nx, ny, HX, HY, order, dt, got, adv_o)
        new = TI.step(want, adv_i, HX, HY, dt, order)
        assert np.abs(new - want).max() > 0.0
        want = new
        check(got, want, "step %d" % n)
    assert np.abs(want).max() < 3.0  # the field stayed at O(1)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_shu_osher_pairs_compose_to_the_butcher_step(order):
    """the stage of the bare-stage entry point, chained with the pairs (a, b) DESIGN.md names (Euler / Heun / Shu-Osher), is the
    Butcher-form step of the restatement: the two forms of the tableau state the same scheme"""
    nx, ny = 13, 11
    u, v, dt, _, adv = case(nx, ny, order)
    pairs = {0: ((0.0, 1.0),), 1: ((0.0, 1.0), (0.5, 0.5)), 2: ((0.0, 1.0), (0.75, 0.25), (1.0 / 3.0, 2.0 / 3.0))}[order]
    phi = TC.random_field(nx, ny, order, 4)
    c = phi
    for a, b in pairs:
        c = TI.stage(phi, c, adv, HX, HY, dt, a, b, order)
    check(c, TI.step(phi, adv, HX, HY, dt, order), "Shu-Osher against Butcher")


@pytest.mark.parametrize("order", [0, 1, 2])
def test_oracle_closure(order):
    """cap + scaling limiter with the bounds [0, inf) uncapped and [0, 1] capped, on fields with capped, scaled and (mostly) untouched
    elements; each count is > 0 where the order and the bounds admit the kind"""
    nx, ny = 61, 9
    for f in (0, 1):
        lo, hi, cap = TC.BOUNDS[f]
        F = TC.bounded_field(nx, ny, order, f, 7 + order)
        want = TI.limit(F, lo, hi, cap, order)
        kind = TC.classify(F, want)
        n = {k: int(np.sum(kind == k)) for k in (TC.UNTOUCHED, TC.CAPPED, TC.SCALED)}
        for k in TC.kinds_expected(order, f):
            assert n[k] > 0, (order, f, n)
        assert n[TC.UNTOUCHED] > nx * ny // 2, n
        got = F.copy()
        O.transport_limit(nx, ny, order, got, lo, hi, cap)
        check(got, want, "closure of field %d" % f)
        # the closure does what it says: cell means kept (but for the cap), every point of the restatement inside the bounds
        assert np.array_equal(want[0], np.minimum(F[0], hi) if cap else F[0])
        for (x, y) in TI.limit_points(order):
            val = TI.evaluate(want, order, x, y)[0]
            assert val.min() >= lo - 1e-14 and val.max() <= hi + 1e-14


@pytest.mark.parametrize("order", [0, 1, 2])
def test_inputs_of_the_device_test_reach_every_seam(order):
    """what tests/test_gpu_transport_independent.py needs of its bounded fields, asserted here without a GPU: after the first step
    every bounded field has capped, scaled and untouched elements on both sides of every window seam and strip seam"""
    for nx, ny in TC.shapes(order):
        u, v = TC.velocity(nx, ny, 7 * nx + ny)
        dt, adv = TC.time_step(u, v), TI.advection(u, v, nx, ny, order)
        for f in range(4):
            new = TI.step(TC.bounded_field(nx, ny, order, f, 11), adv, HX, HY, dt, order)
            TC.assert_closure_active_at_the_seams(nx, ny, order, f, new, TI.limit(new, *TC.BOUNDS[f], order))


@pytest.mark.parametrize("j0,j1", [(0, 9), (2, 7), (4, 5), (0, 3), (6, 9)])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_row_range_step(order, j0, j1):
    """the restatement's step on a window of the array equals its step on the whole array on the rows [j0, j1) -- the domain of
    dependence is order + 1 rows -- and the oracle's step agrees there; the rows outside keep the sentinel"""
    nx, ny = 61, 9
    u, v, dt, adv_o, adv_i = case(nx, ny, order)
    phi = TC.bounded_field(nx, ny, order, 1, 13)
    sentinel = np.full_like(phi, -7.0)
    for closure in (None, TC.BOUNDS[1]):
        want = TI.step_rows(phi, adv_i, HX, HY, dt, order, j0, j1, sentinel, closure)
        full = TI.step(phi, adv_i, HX, HY, dt, order)
        got = phi.copy()
        O.transport_step(nx, ny, HX, HY, order, dt, got, adv_o)
        if closure:
            full = TI.limit(full, *closure, order)
            O.transport_limit(nx, ny, order, got, *closure)
        check(want[:, j0:j1], full[:, j0:j1], "window against whole array")
        check(got[:, j0:j1], want[:, j0:j1], "oracle on the rows")
        assert np.all(want[:, :j0] == -7.0) and np.all(want[:, j1:] == -7.0)
        assert np.abs(want[:, j0:j1] - phi[:, j0:j1]).max() > 0.0


@pytest.mark.parametrize("sign", TC.SIGNS)
@pytest.mark.parametrize("nx,ny", [(61, 25), (27, 29)])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_polynomial_in_a_uniform_flow_is_advected_exactly(order, nx, ny, sign):
    """a global polynomial of total degree <= p in a uniform flow: n steps return the L2 projection of phi(x - v n dt) -- the shifted
    polynomial itself -- in every element further than n (p + 1) cells from the inflow sides, to rounding.  The expected coefficients
    are written out by hand (transport_cases.poly_coefficients): no quadrature, no basis table, no Runge-Kutta table.  The oracle
    and the restatement both; the signs move the excluded zone to each pair of sides in turn"""
    n = 2
    u, v, ux, vy, dt = TC.uniform_velocity(nx, ny, sign)
    zone = TC.exact_zone(nx, ny, order, n, sign)
    assert 2 * zone.sum() >= nx * ny
    phi = TC.poly_coefficients(order, nx, ny)
    want = TC.poly_coefficients(order, nx, ny, ux * n * dt, vy * n * dt)
    assert order == 0 or np.abs(want - phi).max() > 1e-3
    adv_o, adv_i = O.prepare_advection(nx, ny, order, u, v), TI.advection(u, v, nx, ny, order)
    got_o, got_i = phi.copy(), phi
    for _ in range(n):
        O.transport_step(nx, ny, HX, HY, order, dt, got_o, adv_o)
        got_i = TI.step(got_i, adv_i, HX, HY, dt, order)
    tol = 1e-13 * np.abs(want).max()
    for got, name in ((got_o, "oracle"), (got_i, "restatement")):
        err = np.abs(got - want)[:, zone].max()
        assert err <= tol, (name, err, tol)
        assert order == 0 or np.abs(got - want)[:, ~zone].max() > 1e3 * tol  # the open boundary is felt outside the zone

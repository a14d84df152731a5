"""The column state transport on the device (include/nsdg.h "column state transport"): nsdg_tracer_weight / nsdg_tracer_recover bit for
bit against their numpy restatement (tests/column_transport_ref.py), the limiter on an unbounded field, and the Python driver's
CoupledCore(advect_column_state=True): the snow rides on the ice and is conserved by the transport, it takes the same operations as the
thickness, a uniform surface temperature stays uniform and the heat content sum H T is conserved, and one step equals the step composed
from the ABI calls."""
import numpy as np
import pytest
import torch

import column_transport_ref as R
from nextsimdg_amd import abi, rowblock, synthetic

pytestmark = pytest.mark.gpu

STATE = R.BOUNDS  # H, A, S, Q


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    """equal bit patterns (the sign of a zero included); a NaN matches a NaN whatever its payload"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,nx,ny,j0,j1", [(2, 37, 23, 3, 18), (2, 256, 256, 0, 256), (1, 129, 67, 5, 62), (0, 64, 9, 0, 9),
                                               (2, 1, 1, 0, 1), (2, 2048, 64, 7, 57)])
def test_weight_matches_numpy_bit_for_bit(ctx, order, nx, ny, j0, j1):
    nc = {0: 1, 1: 3, 2: 6}[order]
    rng = np.random.default_rng(nx * 31 + ny + order)
    H = rng.standard_normal((nc, ny, nx)) * rng.uniform(0.0, 3.0, (nc, ny, nx))
    T = rng.uniform(-30.0, 5.0, (ny, nx))
    H.flat[:: max(1, H.size // 7)] = np.nan
    T.flat[3 % T.size] = np.inf
    T.flat[:: max(1, T.size // 5)] = -0.0
    ctx.set_grid(nx, ny, 250.0, 250.0)
    Q0 = rng.standard_normal((nc, ny, nx))
    dQ = dev(Q0)
    ctx.tracer_weight(order, j0, j1, dev(H), dev(T), dQ)
    want = R.weight(H, T, j0, j1, Q=Q0)
    assert same_bits(dQ.cpu().numpy(), want)


@pytest.mark.parametrize("nx,ny,j0,j1", [(37, 23, 3, 18), (256, 256, 0, 256), (1, 1, 0, 1), (2048, 64, 7, 57)])
def test_recover_matches_numpy_bit_for_bit_on_random_inputs(ctx, nx, ny, j0, j1):
    rng = np.random.default_rng(nx + 7 * ny)
    H, A, Q = (rng.standard_normal((6, ny, nx)) for _ in range(3))
    H[0] = rng.uniform(-0.2, 2.0, (ny, nx))
    A[0] = rng.uniform(-0.1, 1.1, (ny, nx))
    A[0][rng.random((ny, nx)) < 0.1] = 1e-13
    H[0][rng.random((ny, nx)) < 0.1] = 0.0
    Q[0] = -8.0 * H[0] + rng.standard_normal((ny, nx))
    T = rng.uniform(-20.0, 0.0, (ny, nx))
    ctx.set_grid(nx, ny, 250.0, 250.0)
    for mc, mt in ((R.MIN_CONC, R.MIN_THICK), (0.0, 0.0), (0.3, 0.5)):
        dT = dev(T)
        ctx.tracer_recover(2, j0, j1, dev(H), dev(A), dev(Q), mc, mt, dT)
        want = R.recover(H, A, Q, T, mc, mt, j0, j1)
        assert same_bits(dT.cpu().numpy(), want), (mc, mt)
        assert not np.array_equal(want, T) or nx == 1


def test_recover_matches_numpy_on_the_edge_cases(ctx):
    from test_column_transport_cpu import edge_case_inputs

    cases = edge_case_inputs()
    n = len(cases)
    H, A, Q = np.zeros((6, 1, n)), np.zeros((6, 1, n)), np.zeros((6, 1, n))
    H[1:], A[1:], Q[1:] = 123.0, -5.0, 9.0
    T = np.zeros((1, n))
    for k, (h, a, q, t, _) in enumerate(cases):
        H[0, 0, k], A[0, 0, k], Q[0, 0, k], T[0, k] = h, a, q, t
    ctx.set_grid(n, 1, 250.0, 250.0)
    for mc, mt in ((R.MIN_CONC, R.MIN_THICK), (0.0, 0.0)):
        dT = dev(T)
        ctx.tracer_recover(2, 0, 1, dev(H), dev(A), dev(Q), mc, mt, dT)
        got = dT.cpu().numpy()
        assert same_bits(got, R.recover(H, A, Q, T, mc, mt))
        if mc > 0:
            assert same_bits(got[0], np.array([c[4] for c in cases]))


def test_argument_errors(ctx):
    lib = abi.load_library()
    nx, ny = 16, 8
    ctx.set_grid(nx, ny, 250.0, 250.0)
    H, A, Q, T = dev(np.ones((6, ny, nx))), dev(np.ones((6, ny, nx))), dev(np.zeros((6, ny, nx))), dev(np.full((ny, nx), -8.0))
    p = lambda t: abi.C.c_void_p(t.data_ptr())
    ERR = -1
    assert lib.nsdg_tracer_weight(None, 2, 0, ny, p(H), p(T), p(Q)) == ERR
    assert lib.nsdg_tracer_recover(None, 2, 0, ny, p(H), p(A), p(Q), 0.0, 0.0, p(T)) == ERR
    for order, j0, j1 in ((3, 0, ny), (-1, 0, ny), (2, -1, ny), (2, 0, ny + 1), (2, 5, 4)):
        assert lib.nsdg_tracer_weight(ctx.h, order, j0, j1, p(H), p(T), p(Q)) == ERR, (order, j0, j1)
        assert lib.nsdg_tracer_recover(ctx.h, order, j0, j1, p(H), p(A), p(Q), 0.0, 0.0, p(T)) == ERR, (order, j0, j1)
    for k in range(3):
        args = [p(H), p(T), p(Q)]
        args[k] = None
        assert lib.nsdg_tracer_weight(ctx.h, 2, 0, ny, *args) == ERR
    for k in range(4):
        args = [p(H), p(A), p(Q), p(T)]
        args[k] = None
        assert lib.nsdg_tracer_recover(ctx.h, 2, 0, ny, args[0], args[1], args[2], 0.0, 0.0, args[3]) == ERR
    assert "row range" in lib.nsdg_last_error().decode() or "null" in lib.nsdg_last_error().decode()
    # nothing was written, and an empty row range is no error
    torch.cuda.synchronize()
    assert float(Q.abs().max()) == 0.0 and float(T.max()) == -8.0
    assert lib.nsdg_tracer_weight(ctx.h, 2, 3, 3, p(H), p(T), p(Q)) == 0
    assert lib.nsdg_tracer_recover(ctx.h, 2, 3, 3, p(H), p(A), p(Q), 0.0, 0.0, p(T)) == 0
    # Q must not alias H or T, nor T (recover) H, A or Q: an overlap of the ranges -- nc(order) nx ny doubles of a DG field, nx ny of T -- is
    # refused whichever end touches, by one double or by all; arrays that only abut are fine.  Every array is a window of one buffer
    N = nx * ny
    big = dev(np.arange(40.0 * N) + 1.0)
    before = big.clone()
    at = lambda k: abi.C.c_void_p(big.data_ptr() + 8 * k)
    message = lambda: lib.nsdg_last_error().decode()
    for order, nc in ((0, 1), (1, 3), (2, 6)):
        h, t = 10 * N, 30 * N  # nsdg_tracer_weight: H at h, T at t
        for q in (h, h + nc * N - 1, h - nc * N + 1, t, t + N - 1, t - nc * N + 1):
            assert lib.nsdg_tracer_weight(ctx.h, order, 0, ny, at(h), at(t), at(q)) == ERR, (order, q)
            assert "nsdg_tracer_weight: Q must not alias or overlap H or T" in message()
            assert lib.nsdg_tracer_weight(ctx.h, order, 3, 3, at(h), at(t), at(q)) == ERR  # an empty row range is no excuse
        h, a, q = 4 * N, 14 * N, 24 * N  # nsdg_tracer_recover: H, A, Q
        for x in (h, a, q):
            for t in (x, x + nc * N - 1, x - N + 1):
                assert lib.nsdg_tracer_recover(ctx.h, order, 0, ny, at(h), at(a), at(q), 0.0, 0.0, at(t)) == ERR, (order, x, t)
                assert "nsdg_tracer_recover: T must not alias or overlap H, A or Q" in message()
    torch.cuda.synchronize()
    assert torch.equal(big, before)  # a refused call launches nothing
    for order, nc in ((0, 1), (1, 3), (2, 6)):
        h, t = 10 * N, 30 * N
        for q in (h + nc * N, h - nc * N, t + N, t - nc * N):
            assert lib.nsdg_tracer_weight(ctx.h, order, 0, ny, at(h), at(t), at(q)) == 0, (order, q)
        h, a, q = 4 * N, 14 * N, 24 * N
        for x in (h, a, q):
            for t in (x + nc * N, x - N):
                assert lib.nsdg_tracer_recover(ctx.h, order, 0, ny, at(h), at(a), at(q), 0.0, 0.0, at(t)) == 0, (order, x, t)
    torch.cuda.synchronize()


def test_limiter_leaves_an_unbounded_field_unchanged(ctx):
    nx, ny = 64, 48
    rng = np.random.default_rng(3)
    F = 50.0 * rng.standard_normal((6, ny, nx))
    F[0] = rng.uniform(-20.0, 20.0, (ny, nx))
    ctx.set_grid(nx, ny, 250.0, 250.0)
    before = ctx.transport_bounds if hasattr(ctx, "transport_bounds") else ()
    try:
        ctx.set_transport_bounds(((-np.inf, np.inf, False),))
        d = dev(F)
        ctx.transport_limit(2, 0, ny, [d])
        assert same_bits(d.cpu().numpy(), F)
        ctx.set_transport_bounds(STATE)  # and in the 4-field closure of the mode: the fourth field, Q
        fs = [dev(np.abs(F)), dev(np.clip(F, 0.0, 1.0)), dev(np.abs(F)), dev(F)]
        ctx.transport_limit(2, 0, ny, fs)
        assert same_bits(fs[3].cpu().numpy(), F)
        assert not same_bits(fs[0].cpu().numpy(), np.abs(F))  # the bounded ones were limited
    finally:
        ctx.set_transport_bounds(before)


# ---- the Python driver -------------------------------------------------------------------------------------------------------------------
def coupled(c, nx, ny, L, dt=120.0, nsub=16, native=True, **kw):
    bt = synthetic.BoxTest(nx, ny, L)
    c.set_mevp_params(c.mevp_default_params(**bt.subcycle_parameters(dt)))
    core = rowblock.CoupledCore(c, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, dt, nsub, torch.device("cuda"), native=native,
                                advect_column_state=True, **kw)
    return bt, core


def column_planes(core, nx, ny, hsnow, tice0):
    col = {k: np.zeros((ny, nx)) for k in core.col}
    col["hsnow"][:], col["tice0"][:] = hsnow, tice0
    # an ocean at its freezing point (no heat to melt the ice from below) under a long-wave flux that keeps the open water from freezing:
    # the column step changes the ice and the snow little, and forms no new ice
    col["sst"][:], col["sss"][:], col["tair"][:], col["tdew"][:] = -1.76, 32.0, -10.0, -12.0
    col["slp"][:], col["qlw"][:], col["mld"][:], col["wind"][:] = 1e5, 320.0, 10.0, 5.0
    return col  # qsw = snowfall = 0


def centroid(w, hx, hy):
    ny, nx = w.shape
    y, x = np.meshgrid((np.arange(ny) + 0.5) * hy, (np.arange(nx) + 0.5) * hx, indexing="ij")
    return np.array([np.sum(w * x), np.sum(w * y)]) / np.sum(w)


def test_snow_rides_on_the_ice_and_the_transport_conserves_it(gpu):
    """256^2 box of 250 m cells, a uniform wind, a patch of snow-covered ice in open water (snowfall 0): the snow-weighted centroid moves
    with the ice-volume centroid, and every step's transport conserves the total snow volume"""
    n, L, steps = 256, 64e3, 30
    c = abi.Context(gpu)
    try:
        bt, core = coupled(c, n, n, L)
        g = (np.arange(n) + 0.5) / n
        patch = np.outer((np.abs(g - 0.4) < 0.12), (np.abs(g - 0.4) < 0.12)).astype(float)
        H, A = np.zeros((6, n, n)), np.zeros((6, n, n))
        H[0], A[0] = 0.4 * patch, 0.6 * patch
        z = np.zeros((2 * n + 1, 2 * n + 1))
        core.load_global(H, A, z, z, z + 12.0, z + 8.0)  # uniform wind (12, 8) m/s, ocean at rest
        core.load_column(column_planes(core, n, n, 0.08 * patch, -8.0))
        S0 = core.S[0].cpu().numpy().copy()
        cs0, ch0 = centroid(S0, bt.hx, bt.hy), centroid(H[0], bt.hx, bt.hy)
        for k in range(steps):
            core._set_grid()
            core.external_forcing()
            core.thermodynamics()
            after_column = float(core.S[0].sum())
            core.momentum()
            core.transport()
            after_transport = float(core.S[0].sum())
            core.time += core.dt
            assert after_column > 0 and abs(after_transport - after_column) <= 1e-12 * after_column, (k, after_column, after_transport)
            assert core.col["hsnow"].data_ptr() == core.S[0].data_ptr()  # the column step reads the current snow
        S, Hn, An = core.S[0].cpu().numpy(), core.H[0].cpu().numpy(), core.A[0].cpu().numpy()
        assert float(np.sum(S)) > 0.5 * float(np.sum(S0))  # the snow is still there
        # the centroids of the drifting floe (A > 0.3): new ice that the column step forms in the open water is not part of it
        floe = An > 0.3
        ds, dh = centroid(S * floe, bt.hx, bt.hy) - cs0, centroid(Hn * floe, bt.hx, bt.hy) - ch0
        assert np.hypot(*dh) > 2 * bt.hx, dh  # the ice has moved by more than two elements
        assert np.hypot(*(ds - dh)) < bt.hx, (ds, dh)
        core.close()
    finally:
        c.close()


def test_snow_takes_the_same_operations_as_the_thickness(gpu):
    """with the column step off, S initialised with H's coefficients stays equal to H bit for bit (closure on, cyclone wind)"""
    n, steps = 128, 8
    c = abi.Context(gpu)
    try:
        bt, core = coupled(c, n, n, 512e3)
        H, A = bt.dg_fields()
        rng = np.random.default_rng(2)
        H[1:3] += 0.03 * rng.standard_normal((2, n, n))
        uo, vo = bt.ocean()
        ua, va = bt.wind(0.0)
        core.load_global(H, A, uo, vo, 4.0 * ua + 10.0, 4.0 * va + 6.0)  # the cyclone on a uniform wind
        core.S.copy_(core.H)
        core.col["tice0"].fill_(-8.0)
        for _ in range(steps):
            core._set_grid()
            core.momentum()
            core.transport()
            assert torch.equal(core.S, core.H)
        assert float(core.u.abs().max()) > 1e-4
        assert not np.array_equal(core.H.cpu().numpy(), H)
        core.close()
    finally:
        c.close()


def test_temperature_uniform_stays_uniform_and_heat_content_is_conserved(gpu):
    """column step off, the cyclone: a flow that converges in one place and diverges in another.  A uniform tice0 = -8 stays -8 in every
    element that holds ice; with a random tice0 on a cover where no element crosses the ice test, sum mean(H) T is conserved"""
    n, steps = 128, 10
    for uniform in (True, False):
        c = abi.Context(gpu)
        try:
            bt, core = coupled(c, n, n, 512e3)
            H, A = bt.dg_fields()
            rng = np.random.default_rng(4)
            if not uniform:
                H[0] = 0.5 + 0.2 * rng.random((n, n))
                A[0] = 0.9
            uo, vo = bt.ocean()
            ua, va = bt.wind(0.0)
            core.load_global(H, A, uo, vo, 4.0 * ua + 10.0, 4.0 * va + 6.0)  # the cyclone on a uniform wind
            T0 = np.full((n, n), -8.0) if uniform else rng.uniform(-14.0, -2.0, (n, n))
            core.col["tice0"].copy_(dev(T0))
            before = R.heat_content(H, T0, A)
            for _ in range(steps):
                core._set_grid()
                core.momentum()
                core.transport()
                Hn, An, T = core.H.cpu().numpy(), core.A.cpu().numpy(), core.col["tice0"].cpu().numpy()
                ice = R.holds_ice(Hn[0], An[0])
                if uniform:
                    assert np.max(np.abs(T[ice] + 8.0)) <= 1e-13 * 8.0
                else:
                    assert ice.all()
            assert float(core.u.abs().max()) > 1e-4
            if not uniform:
                after = R.heat_content(Hn, T, An)
                assert abs(after - before) <= 1e-12 * abs(before), (before, after)
                assert np.max(np.abs(T - T0)) > 1e-6
            core.close()
        finally:
            c.close()


@pytest.mark.parametrize("native", [True, False])
def test_one_step_equals_the_step_composed_from_abi_calls(gpu, native):
    """CoupledCore.step() with the mode on == column_step, the driver's momentum, nsdg_tracer_weight, a 4-field transport_step with the
    4-field closure and nsdg_tracer_recover, bit for bit"""
    n = 96
    runs = []
    for composed in (False, True):
        c = abi.Context(gpu)
        try:
            bt, core = coupled(c, n, n, 512e3, native=native and not composed)
            H, A = bt.dg_fields()
            H[1:3] += 0.02 * np.random.default_rng(6).standard_normal((2, n, n))
            uo, vo = bt.ocean()
            ua, va = bt.wind(0.0)
            core.load_global(H, A, uo, vo, 4.0 * ua + 10.0, 4.0 * va + 6.0)  # the cyclone on a uniform wind
            rng = np.random.default_rng(8)
            core.load_column(column_planes(core, n, n, 0.05 + 0.05 * rng.random((n, n)), rng.uniform(-12.0, -3.0, (n, n))))
            for _ in range(2):
                if not composed:
                    core.step()
                    continue
                core._set_grid()
                state = {"hice": core.H[0], "cice": core.A[0], "hsnow": core.S[0], "tice0": core.col["tice0"]}
                c.column_step(core.dt, state, {k: core.col[k] for k in core.COLUMN_FORCING}, core.newice)
                core.momentum()
                c.tracer_weight(2, 0, n, core.H, core.col["tice0"], core.Q)
                c.prepare_advection(2, core.u, core.v, *core.adv)
                c.set_transport_bounds(STATE)
                scratch = torch.zeros(2 * 4 * core.H.numel(), dtype=torch.float64, device="cuda")
                c.transport_step(2, core.dt, [core.H, core.A, core.S, core.Q], core.adv, scratch)
                c.tracer_recover(2, 0, n, core.H, core.A, core.Q, R.MIN_CONC, R.MIN_THICK, core.col["tice0"])
                core.time += core.dt
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy().copy() for k, v in (("H", core.H), ("A", core.A), ("S", core.S), ("T", core.col["tice0"]),
                                                                ("u", core.u))})
            core.close()
        finally:
            c.close()
    a, b = runs
    assert float(np.abs(a["u"]).max()) > 1e-5
    for k in a:
        assert same_bits(a[k], b[k]), k

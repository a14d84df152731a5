"""Ice tracers on the device (include/nsdg.h "ice tracers"): nsdg_tracers_weight / nsdg_tracers_recover /
nsdg_tracers_dilute bit for bit against their numpy restatement (tests/tracers_ref.py) and against the single-tracer kernel, their
refusals, a field advected as the second transport group against the same field listed third in the first, and the Python driver's
DynamicsCore / CoupledCore with tracers=: the analytic properties of tests/test_tracers_cpu.py (uniform stays uniform, the age is the
clock, the content is conserved, the tracer moves), growth dilutes, zero where there is no ice, the rest of the model bit-identical with
and without tracers, 1 block == 4 blocks, native == the Python sequence, sub-steps, checkpoint, and the brittle and column-state runs."""
import threading

import numpy as np
import pytest
import torch

import test_tracers_cpu as T
import thread_ranks
import tracers_ref as R
from nextsimdg_amd import abi, rowblock, synthetic
from test_gpu_column_transport import dev, same_bits

pytestmark = pytest.mark.gpu
DT = T.DT
SHAPES = [(1, 1, 0, 1), (70, 9, 0, 9), (70, 9, 2, 7)]
NC = {0: 1, 1: 3, 2: 6}


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()


def host(tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
def weight_inputs(rng, nc, nx, ny, n):
    H = rng.standard_normal((nc, ny, nx)) * rng.uniform(0.0, 3.0, (nc, ny, nx))
    H.flat[:: max(1, H.size // 7)] = np.nan
    Ts = [rng.uniform(-30.0, 5.0, (ny, nx)) for _ in range(n)]
    Ts[0].flat[3 % Ts[0].size] = np.inf
    Ts[-1].flat[:: max(1, nx * ny // 5)] = -0.0
    Ts[n // 2].flat[(nx * ny) // 2] = np.nan
    Q0 = [rng.standard_normal((nc, ny, nx)) for _ in range(n)]  # the sentinel: rows outside [j0, j1) keep it
    return H, Ts, Q0


def check_weight(ctx, rng, order, nx, ny, j0, j1, n):
    nc = NC[order]
    H, Ts, Q0 = weight_inputs(rng, nc, nx, ny, n)
    ctx.set_grid(nx, ny, 250.0, 250.0)
    dH, dT, dQ = dev(H), [dev(t) for t in Ts], [dev(q) for q in Q0]
    ctx.tracers_weight(order, j0, j1, dH, dT, dQ)
    got = host(dQ)
    want = R.weight(H, Ts, j0, j1, Q=Q0)
    single = [dev(q) for q in Q0]
    for k in range(n):  # n calls of the single-tracer kernel give the same bits
        ctx.tracer_weight(order, j0, j1, dH, dT[k], single[k])
    single = host(single)
    for k in range(n):
        assert same_bits(got[k], want[k]), (order, n, k)
        assert same_bits(got[k], single[k]), (order, n, k)
        assert same_bits(got[k][:, :j0], Q0[k][:, :j0]) and same_bits(got[k][:, j1:], Q0[k][:, j1:])
        assert not same_bits(got[k], Q0[k])


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("nx,ny,j0,j1", SHAPES)
def test_weight_matches_numpy_and_the_single_kernel_bit_for_bit(ctx, order, nx, ny, j0, j1):
    rng = np.random.default_rng(100 * order + nx + ny + j0)
    for n in (1, 2, 3, 4):
        check_weight(ctx, rng, order, nx, ny, j0, j1, n)


def recover_inputs(rng, nx, ny, n):
    H, A = (rng.standard_normal((6, ny, nx)) for _ in range(2))
    H[0] = rng.uniform(-0.2, 2.0, (ny, nx))
    A[0] = rng.uniform(-0.1, 1.1, (ny, nx))
    A[0][rng.random((ny, nx)) < 0.1] = 1e-13  # below min_conc
    H[0][rng.random((ny, nx)) < 0.1] = 0.0
    thin = rng.random((ny, nx)) < 0.1
    H[0][thin] = 0.005 * np.abs(A[0][thin])  # below min_thick A
    H[0][rng.random((ny, nx)) < 0.03] = np.nan
    A[0][rng.random((ny, nx)) < 0.03] = np.nan
    Qs = []
    for _ in range(n):
        Q = rng.standard_normal((6, ny, nx))
        Q[0] = 5.0 * H[0] + rng.standard_normal((ny, nx))
        Q[0][rng.random((ny, nx)) < 0.03] = np.nan
        Qs.append(Q)
    T0 = [rng.uniform(-20.0, 20.0, (ny, nx)) for _ in range(n)]
    T0[0].flat[0] = np.nan  # a stale NaN is replaced on either branch
    kinds = [int(k) for k in rng.integers(0, 2, n)]
    return H, A, Qs, T0, kinds


def check_recover(ctx, rng, nx, ny, j0, j1, n, order=2, tests=((R.MIN_CONC, R.MIN_THICK), (0.0, 0.0), (0.3, 0.5))):
    H, A, Qs, T0, kinds = recover_inputs(rng, nx, ny, n)
    ctx.set_grid(nx, ny, 250.0, 250.0)
    for mc, mt in tests:
        dT = [dev(t) for t in T0]
        ctx.tracers_recover(order, j0, j1, dev(H), dev(A), [dev(q) for q in Qs], kinds, 120.0, mc, mt, dT)
        got = host(dT)
        want = R.recover(H, A, Qs, kinds, 120.0, T0, mc, mt, j0, j1)
        for k in range(n):
            assert same_bits(got[k], want[k]), (n, k, mc, mt)
            assert same_bits(got[k][:j0], T0[k][:j0]) and same_bits(got[k][j1:], T0[k][j1:])
    if nx * (j1 - j0) > 100:  # every branch was taken: about a tenth of the elements and more on each
        ice = R.holds_ice(H[0], A[0])[j0:j1]
        assert 0.1 < ice.mean() < 0.9


def dilute_inputs(rng, nx, ny, n):
    hb = rng.uniform(-0.2, 2.0, (ny, nx))
    ha = hb + 0.3 * rng.standard_normal((ny, nx))  # growth and melt, about half each; a tenth and more ends without ice
    same = rng.random((ny, nx)) < 0.1
    ha[same] = hb[same]
    ha[rng.random((ny, nx)) < 0.05] = 0.0
    ha[rng.random((ny, nx)) < 0.03] = np.nan
    hb[rng.random((ny, nx)) < 0.03] = np.nan
    hb[rng.random((ny, nx)) < 0.05] = 0.0
    T0 = [rng.uniform(-20.0, 20.0, (ny, nx)) for _ in range(n)]
    T0[-1][rng.random((ny, nx)) < 0.05] = np.nan
    return hb, ha, T0


def check_dilute(ctx, rng, nx, ny, j0, j1, n):
    hb, ha, T0 = dilute_inputs(rng, nx, ny, n)
    ctx.set_grid(nx, ny, 250.0, 250.0)
    dT = [dev(t) for t in T0]
    ctx.tracers_dilute(j0, j1, dev(hb), dev(ha), dT)
    got = host(dT)
    want = R.dilute(hb, ha, T0, j0, j1)
    for k in range(n):
        assert same_bits(got[k], want[k]), (n, k)
        assert same_bits(got[k][:j0], T0[k][:j0]) and same_bits(got[k][j1:], T0[k][j1:])
    if nx * (j1 - j0) > 100:
        with np.errstate(invalid="ignore"):
            grown, none = (ha > np.maximum(hb, 0.0))[j0:j1], ~(ha > 0.0)[j0:j1]
        assert grown.mean() > 0.1 and none.mean() > 0.1 and (~grown & ~none).mean() > 0.1


@pytest.mark.parametrize("nx,ny,j0,j1", SHAPES)
def test_recover_and_dilute_match_numpy_bit_for_bit_on_random_inputs(ctx, nx, ny, j0, j1):
    rng = np.random.default_rng(7 * nx + ny + j1)
    for n in (1, 2, 3, 4):
        check_recover(ctx, rng, nx, ny, j0, j1, n, order=(2, 0, 1, 2)[n - 1])
        check_dilute(ctx, rng, nx, ny, j0, j1, n)


def test_recover_and_dilute_match_numpy_on_the_edge_cases(ctx):
    from test_column_transport_cpu import edge_case_inputs

    cases = edge_case_inputs()  # (H0, A0, Q0, T_before, _) on every branch of the ice test, NaN in each input among them
    m = len(cases)
    H, A, Q = np.zeros((6, 1, m)), np.zeros((6, 1, m)), np.zeros((6, 1, m))
    H[1:], A[1:], Q[1:] = 123.0, -5.0, 9.0
    T0 = np.zeros((1, m))
    for k, (h, a, q, t, _) in enumerate(cases):
        H[0, 0, k], A[0, 0, k], Q[0, 0, k], T0[0, k] = h, a, q, t
    ctx.set_grid(m, 1, 250.0, 250.0)
    for mc, mt in ((R.MIN_CONC, R.MIN_THICK), (0.0, 0.0)):
        dT = [dev(T0), dev(T0)]
        ctx.tracers_recover(2, 0, 1, dev(H), dev(A), [dev(Q), dev(Q)], (R.PASSIVE, R.AGE), 120.0, mc, mt, dT)
        got = host(dT)
        want = R.recover(H, A, [Q, Q], (R.PASSIVE, R.AGE), 120.0, [T0, T0], mc, mt)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        if mc > 0:  # the known answers of the single-tracer kernel where there is ice, 0 where it kept its value
            known = np.array([c[4] if R.holds_ice(np.float64(c[0]), np.float64(c[1])) else 0.0 for c in cases])
            assert same_bits(got[0][0], known)
            assert same_bits(got[1][0], np.where(R.holds_ice(H[0, 0], A[0, 0]), known + 120.0, 0.0))
    # dilute: h = 0, ha == hb, hb < 0, NaN in each input, infinities
    nan, inf = np.nan, np.inf
    rows = [  # (h_before, h_after, T, T afterwards)
        (1.0, 2.0, 6.0, 3.0), (1.0, 1.0, 6.0, 6.0), (1.0, 0.5, 6.0, 6.0), (0.0, 0.0, 6.0, 0.0), (1.0, 0.0, 6.0, 0.0), (1.0, -0.5, 6.0, 0.0),
        (0.0, 1.0, 6.0, 0.0), (-1.0, 1.0, 6.0, 0.0), (-1.0, -2.0, 6.0, 0.0), (nan, 1.0, 6.0, 0.0), (1.0, nan, 6.0, 0.0), (1.0, 2.0, nan, nan),
        (1.0, 1.0, nan, nan), (1.0, 0.0, nan, 0.0), (1.0, inf, 6.0, 0.0), (inf, inf, 6.0, 6.0), (1.0, 3.0, -0.0, -0.0), (-0.0, 1.0, 6.0, 0.0),
        (1e-300, 2e-300, 6.0, 3.0), (0.3, 0.9, 1.0, (1.0 * 0.3) / 0.9)]
    m = len(rows)
    hb, ha, t0 = (np.array([[r[k] for r in rows]]) for k in range(3))
    ctx.set_grid(m, 1, 250.0, 250.0)
    dT = [dev(t0), dev(-t0)]
    ctx.tracers_dilute(0, 1, dev(hb), dev(ha), dT)
    got = host(dT)
    want = R.dilute(hb, ha, [t0, -t0])
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    known = np.array([r[3] for r in rows])
    assert np.array_equal(got[0][0], known, equal_nan=True)  # (== : the sign of a zero is the restatement's to say)


def test_kernels_past_one_pass_of_the_grid_stride_loop(ctx, gpu):
    """more elements than the 256 x 8 x CU lanes of one pass: n = 4 at order 2"""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    nx = 768
    rows = (256 * 8 * cus) // nx + 3
    ny, j0 = rows + 3, 2
    j1 = j0 + rows
    assert nx * (j1 - j0) > 256 * 8 * cus
    rng = np.random.default_rng(12)
    check_weight(ctx, rng, 2, nx, ny, j0, j1, 4)
    check_recover(ctx, rng, nx, ny, j0, j1, 4, tests=((R.MIN_CONC, R.MIN_THICK),))
    check_dilute(ctx, rng, nx, ny, j0, j1, 4)


def test_argument_errors(ctx, gpu):
    lib = abi.load_library()
    nx, ny = 16, 8
    N = nx * ny
    ctx.set_grid(nx, ny, 250.0, 250.0)
    H, A = dev(np.ones((6, ny, nx))), dev(np.ones((6, ny, nx)))
    Qs = [dev(np.zeros((6, ny, nx))) for _ in range(4)]
    Ts = [dev(np.full((ny, nx), -8.0)) for _ in range(4)]
    hb, ha = dev(np.ones((ny, nx))), dev(np.full((ny, nx), 2.0))
    p = lambda t: None if t is None else abi.C.c_void_p(t.data_ptr())

    def arr(ts):
        a = (abi.VP * max(len(ts), 1))()
        for i, t in enumerate(ts):
            a[i] = None if t is None else (t if isinstance(t, int) else t.data_ptr())
        return a

    def kinds(*k):
        return (abi.I32 * len(k))(*k)

    def weight(h=ctx.h, order=2, j0=0, j1=ny, H=H, n=2, T=Ts, Q=Qs):
        return lib.nsdg_tracers_weight(h, order, j0, j1, p(H), n, None if T is None else arr(T), None if Q is None else arr(Q))

    def recover(h=ctx.h, order=2, j0=0, j1=ny, H=H, A=A, n=2, Q=Qs, kind=kinds(0, 1, 0, 0), T=Ts):
        return lib.nsdg_tracers_recover(h, order, j0, j1, p(H), p(A), n, None if Q is None else arr(Q), kind, 120.0, 0.0, 0.0,
                                        None if T is None else arr(T))

    def dilute(h=ctx.h, j0=0, j1=ny, hb=hb, ha=ha, n=2, T=Ts):
        return lib.nsdg_tracers_dilute(h, j0, j1, p(hb), p(ha), n, None if T is None else arr(T))

    ERR, STATE = -1, -3
    message = lambda: lib.nsdg_last_error().decode()
    assert weight() == 0 and recover() == 0 and dilute() == 0  # the calls as they stand are fine
    torch.cuda.synchronize()
    for q in Qs:
        q.zero_()
    for t in Ts:
        t.fill_(-8.0)
    fresh = abi.Context(gpu)  # no grid set
    try:
        assert weight(h=fresh.h) == STATE and recover(h=fresh.h) == STATE and dilute(h=fresh.h) == STATE
    finally:
        fresh.close()
    assert weight(h=None) == ERR and recover(h=None) == ERR and dilute(h=None) == ERR
    for order in (3, -1):
        assert weight(order=order) == ERR and recover(order=order) == ERR
    for j0, j1 in ((-1, ny), (0, ny + 1), (5, 4)):
        assert weight(j0=j0, j1=j1) == ERR and recover(j0=j0, j1=j1) == ERR and dilute(j0=j0, j1=j1) == ERR
        assert "row range" in message()
    for n in (0, 5, -1):
        assert weight(n=n) == ERR and recover(n=n) == ERR and dilute(n=n) == ERR
        assert "NSDG_TRACERS_MAX" in message()
    holed = lambda ts: [ts[0], None] + ts[2:]
    assert weight(H=None) == ERR and weight(T=None) == ERR and weight(Q=None) == ERR and weight(T=holed(Ts)) == ERR and weight(Q=holed(Qs)) == ERR
    assert recover(H=None) == ERR and recover(A=None) == ERR and recover(Q=None) == ERR and recover(T=None) == ERR and recover(kind=None) == ERR
    assert recover(Q=holed(Qs)) == ERR and recover(T=holed(Ts)) == ERR
    assert dilute(hb=None) == ERR and dilute(ha=None) == ERR and dilute(T=None) == ERR and dilute(T=holed(Ts)) == ERR
    assert "null pointer" in message()
    assert weight(T=holed(Ts), n=1, j0=3, j1=3) == 0 and dilute(T=holed(Ts), n=1, j0=3, j1=3) == 0  # entries past n are not read
    for bad in (2, -1):
        assert recover(kind=kinds(0, bad, 0, 0)) == ERR and "unknown tracer kind" in message()
    assert recover(kind=kinds(0, 2, 0, 0), n=1, j0=2, j1=2) == 0
    # aliasing: every array is a window of one buffer; an overlap by one double or by all is refused, arrays that only abut are fine
    big = dev(np.arange(60.0 * N) + 1.0)
    before = big.clone()
    at = lambda k: big.data_ptr() + 8 * k
    for order, nc in ((0, 1), (1, 3), (2, 6)):
        h, t0, t1, q0, q1 = 0, 7 * N, 8 * N, 10 * N, 17 * N
        for q in (h, h + nc * N - 1, t0 - nc * N + 1, t1 + N - 1, q1, q1 - nc * N + 1, q1 + nc * N - 1):
            for j0, j1 in ((0, ny), (3, 3)):  # an empty row range is no excuse
                assert lib.nsdg_tracers_weight(ctx.h, order, j0, j1, at(h), 2, arr([at(t0), at(t1)]), arr([at(q), at(q1)])) == ERR, (order, q)
                assert "nsdg_tracers_weight: Q must not alias or overlap H, any T or another Q" in message()
        for q in (q1 - nc * N, q1 + nc * N, t1 + N):
            assert lib.nsdg_tracers_weight(ctx.h, order, 3, 3, at(h), 2, arr([at(t0), at(t1)]), arr([at(q), at(q1)])) == 0, (order, q)
        h, a, q0, q1, t1 = 0, 7 * N, 14 * N, 21 * N, 30 * N
        for x in (h, a, q0, q1):
            for t in (x, x + nc * N - 1, x - N + 1):
                assert lib.nsdg_tracers_recover(ctx.h, order, 0, ny, at(h), at(a), 2, arr([at(q0), at(q1)]), kinds(0, 1), 1.0, 0.0, 0.0,
                                                arr([at(t) if t >= 0 else at(h), at(t1)])) == ERR, (order, x, t)
                assert "nsdg_tracers_recover: T must not alias or overlap H, A, any Q or another T" in message()
        for t in (t1, t1 + N - 1, t1 - N + 1):
            assert lib.nsdg_tracers_recover(ctx.h, order, 0, ny, at(h), at(a), 2, arr([at(q0), at(q1)]), kinds(0, 1), 1.0, 0.0, 0.0,
                                            arr([at(t), at(t1)])) == ERR
        assert lib.nsdg_tracers_recover(ctx.h, order, 3, 3, at(h), at(a), 2, arr([at(q0), at(q1)]), kinds(0, 1), 1.0, 0.0, 0.0,
                                        arr([at(t1 + N), at(t1)])) == 0
    b, a, t1 = 0, 2 * N, 6 * N
    for t in (b, b + N - 1, a, a - N + 1, a + N - 1, t1, t1 + N - 1, t1 - N + 1):
        assert lib.nsdg_tracers_dilute(ctx.h, 0, ny, at(b), at(a), 2, arr([at(t), at(t1)])) == ERR, t
        assert "nsdg_tracers_dilute: T must not alias or overlap h_before, h_after or another T" in message()
    assert lib.nsdg_tracers_dilute(ctx.h, 3, 3, at(b), at(a), 2, arr([at(t1 + N), at(t1)])) == 0
    # a refused call launches nothing, and an empty row range does nothing
    assert weight(j0=3, j1=3) == 0 and recover(j0=3, j1=3) == 0 and dilute(j0=3, j1=3) == 0
    torch.cuda.synchronize()
    assert torch.equal(big, before)
    assert all(float(q.abs().max()) == 0.0 for q in Qs) and all(float(t.max()) == -8.0 == float(t.min()) for t in Ts)
    # the binding refuses lists of the wrong length before the library is asked
    with pytest.raises(abi.NsdgError):
        ctx.tracers_weight(2, 0, ny, H, Ts, Qs[:3])
    with pytest.raises(abi.NsdgError):
        ctx.tracers_dilute(0, ny, hb, ha, [])
    with pytest.raises(abi.NsdgError, match="unknown tracer kind"):
        ctx.tracers_recover(2, 0, ny, H, A, Qs[:1], [7], 1.0, 0.0, 0.0, Ts[:1])


# ---- the second transport group ----------------------------------------------------------------------------------------------------------
UNBOUNDED = (-np.inf, np.inf, False)
GROUP1 = ((0.0, np.inf, False), (0.0, 1.0, True), UNBOUNDED)


def group_fields(n):
    from test_column_transport_cpu import box_flow

    rng = np.random.default_rng(21)
    H = np.zeros((6, n, n))
    H[0] = 0.5 + 0.4 * rng.random((n, n))
    H[1:] = 0.05 * rng.standard_normal((5, n, n))
    A = np.zeros((6, n, n))
    A[0] = 0.97 + 0.03 * rng.random((n, n))
    A[1:] = 0.02 * rng.standard_normal((5, n, n))  # the limiter and the cap have work to do
    F = H * rng.uniform(-5.0, 5.0, (n, n))[None]
    u, v = box_flow(n)
    return H, A, F, u, v


def test_a_field_of_the_second_group_has_the_bits_of_the_same_field_third_in_the_first(ctx):
    n, steps = 36, 2
    hx = 1.0 / n
    dt = 0.2 * hx / 0.3
    H, A, F, u, v = group_fields(n)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    ctx.set_grid(n, n, hx, hx)
    adv = (z(6, n, n), z(6, n, n), z(3, n, n + 1), z(3, n + 1, n))
    ctx.prepare_advection(2, dev(u), dev(v), *adv)
    blk = rowblock.RowBlock(n, n)
    before = getattr(ctx, "transport_bounds", ())
    try:
        def composed(fields, bounds):
            f = [dev(x) for x in fields]
            t1, t2 = [z(6, n, n) for _ in f], [z(6, n, n) for _ in f]
            ctx.set_transport_bounds(bounds)
            for _ in range(steps):
                ctx.transport_stage(2, 0, n, dt, 0.0, 1.0, f, f, t1, adv)
                ctx.transport_stage(2, 0, n, dt, 0.75, 0.25, f, t1, t2, adv)
                ctx.transport_stage(2, 0, n, dt, 1.0 / 3.0, 2.0 / 3.0, f, t2, t1, adv)
                if bounds:
                    ctx.transport_limit(2, 0, n, t1)
                f, t1 = t1, f
            return host(f)

        def native(fields, bounds):
            phi, t1, t2 = [dev(x) for x in fields], [z(6, n, n) for _ in fields], [z(6, n, n) for _ in fields]
            run = ctx.rb_transport(blk, (None, None), phi, t1, t2, adv, bounds=bounds)
            par = 0
            for _ in range(steps):
                par = run(dt, par)
            out = host((phi, t1)[par])
            run.close()
            return out

        for run in (composed, native):
            first = run([H, A, F], GROUP1)
            (second,) = run([F], ())
            assert same_bits(second, first[2]), run.__name__
            assert not same_bits(first[2], F) and float(np.max(np.abs(first[2][0] - F[0]))) > 1e-6
            assert not same_bits(first[1], run([A], ())[0])  # the bounded field was limited: the two groups do differ in that
        assert same_bits(composed([F], ())[0], native([F], ())[0])
    finally:
        ctx.set_transport_bounds(before)


# ---- the Python driver -------------------------------------------------------------------------------------------------------------------
def gpu_core(c, bt, tracers, cls=rowblock.DynamicsCore, native=True, nsub=16, **kw):
    c.set_mevp_params(c.mevp_default_params(**bt.subcycle_parameters(DT)))
    return cls(c, rowblock.RowBlock(bt.nx, bt.ny), bt.hx, bt.hy, DT, nsub, torch.device("cuda"), native=native, tracers=tracers, **kw)


@pytest.mark.parametrize("cls", [rowblock.DynamicsCore, rowblock.CoupledCore])
@pytest.mark.parametrize("native", [True, False])
def test_uniform_stays_uniform_age_is_the_clock_and_the_content_is_conserved(gpu, native, cls):
    """the 128^2 box of 4 km cells and the cyclone of the column state transport's core runs; the table of tests/test_tracers_cpu.py, on a
    DynamicsCore and on a CoupledCore (its column step off, as in those runs)"""
    c = abi.Context(gpu)
    try:
        T.run_properties(lambda bt, tracers: gpu_core(c, bt, tracers, cls=cls, native=native), 128, 512e3, 8)
    finally:
        c.close()


def run_one(gpu, cls, tracers, steps, n=64, native=True, resume=None, advance=None, land=None, load=None, dt=DT, **kw):
    """tests/test_tracers_cpu.py's run_one on the device: a closed pack with an open corner under the cyclone; returns the arrays"""
    c = abi.Context(gpu)
    try:
        bt, H, A, uo, vo, ua, va = T.pack(n, n * 4e3, closed=True, seed=11)
        A[0, :9, :13] = 0.0
        H[0, :9, :13] = 0.0
        core = gpu_core(c, bt, tracers, cls=cls, native=native, land=land, **kw)
        core.dt = dt
        core.load_global(H, A, uo, vo, ua, va)
        if cls is rowblock.CoupledCore:
            core.load_column(T.freezing_column(core, n))
        if tracers:
            core.load_tracers({name: T.origin_field(n, seed=3 + k) for k, name in enumerate(tracers) if load is None or name in load})
        if resume is not None:
            core.load_state_dict(resume)
        for _ in range(steps):
            if advance:
                core.advance(DT, substeps=advance)
            else:
                core.step()
        torch.cuda.synchronize()
        out = core.state_dict()
        out["umax"] = float(core.u.abs().max())
        core.close()
        return out
    finally:
        c.close()


def same_state(a, b, keys=("H", "A", "u", "v", "s11", "s12", "s22")):
    for k in keys:
        assert same_bits(a[k], b[k]), k
    for name in a.get("tracers", {}):
        assert same_bits(a["tracers"][name], b["tracers"][name]), name


@pytest.mark.parametrize("cls", [rowblock.DynamicsCore, rowblock.CoupledCore])
@pytest.mark.parametrize("native,use_graph", [(True, False), (False, False), (True, True)])
def test_the_rest_of_the_model_does_not_see_the_tracers(gpu, cls, native, use_graph):
    a = run_one(gpu, cls, ("age", "origin", "x", "y"), 3, native=native, use_graph=use_graph)
    b = run_one(gpu, cls, None, 3, native=native, use_graph=use_graph)
    assert "tracers" not in b and a["umax"] > 1e-4
    same_state(b, a)


@pytest.mark.parametrize("cls", [rowblock.DynamicsCore, rowblock.CoupledCore])
def test_native_equals_the_python_sequence(gpu, cls):
    a, b = (run_one(gpu, cls, ("age", "origin"), 3, native=native) for native in (True, False))
    same_state(a, b)
    assert float(np.abs(a["tracers"]["origin"] - T.origin_field(64, seed=4)).max()) > 1e-6


def test_n_steps_equal_half_plus_state_dict_plus_half(gpu):
    full = run_one(gpu, rowblock.DynamicsCore, ("age", "origin"), 4)
    half = run_one(gpu, rowblock.DynamicsCore, ("age", "origin"), 2)
    rest = run_one(gpu, rowblock.DynamicsCore, ("age", "origin"), 2, resume=rowblock.DynamicsCore.merge_states([half]))
    same_state(full, rest)
    assert np.any(full["tracers"]["origin"] == 0.0) and float(full["tracers"]["age"].max()) > 4 * DT


def test_advance_with_two_substeps_equals_two_steps_at_half_dt(gpu):
    a = run_one(gpu, rowblock.DynamicsCore, ("age", "origin"), 2, advance=2)
    b = run_one(gpu, rowblock.DynamicsCore, ("age", "origin"), 4, dt=DT / 2)
    same_state(a, b)


def test_zero_on_land_and_wherever_the_ice_test_fails(gpu):
    n = 64
    land = np.zeros((n, n), dtype=bool)
    land[20:29, 30:41] = True
    for cls in (rowblock.DynamicsCore, rowblock.CoupledCore):
        out = run_one(gpu, cls, ("age", "origin"), 3, land=land)
        ice = R.holds_ice(out["H"][0], out["A"][0])
        assert not ice[land].any() and ice.sum() > 0 and ((~ice).sum() > land.sum() or cls is rowblock.CoupledCore)
        for name, t in out["tracers"].items():
            assert np.all(t[land] == 0.0) and np.all(t[~ice] == 0.0), (cls.__name__, name)
        assert np.all(out["tracers"]["age"][ice] > 0.0)


def test_coupled_growth_dilutes_by_the_ratio_and_the_mean_age_lags_the_clock(gpu):
    n, steps = 64, 3
    c = abi.Context(gpu)
    try:
        bt, H, A, uo, vo, ua, va = T.pack(n, n * 4e3, closed=True, seed=11)
        A[0, :9, :13] = 0.0
        H[0, :9, :13] = 0.0
        core = gpu_core(c, bt, ("age", "origin"), cls=rowblock.CoupledCore)
        core.load_global(H, A, uo, vo, ua, va)
        core.load_column(T.freezing_column(core, n))
        core.load_tracers({"origin": T.origin_field(n)})  # the age starts at 0
        grew = 0
        for k in range(steps):
            core._set_grid()
            core.external_forcing()
            hb, tb = core.H[0].cpu().numpy(), host(core._tr)
            core.thermodynamics()
            ha, ta = core.H[0].cpu().numpy(), host(core._tr)
            want = R.dilute(hb, ha, tb)
            assert same_bits(ta[0], want[0]) and same_bits(ta[1], want[1])
            had = (ha > np.maximum(hb, 0.0)) & (tb[1] > 0.0)
            grew += int(had.sum())
            assert np.all(ta[1][had] < tb[1][had])
            core.momentum()
            core.transport()
            core.time += core.dt
        assert grew > n * n // 2
        ice = R.holds_ice(core.H[0].cpu().numpy(), core.A[0].cpu().numpy())
        assert 0.0 < float(core._tr[0].cpu().numpy()[ice].mean()) < steps * DT
        core.close()
    finally:
        c.close()


def test_brittle_run_stays_finite_and_uniform(gpu):
    import test_gpu_bbm_native as B

    c = abi.Context(gpu)
    try:
        core = B.run_core(c, torch.device("cuda"), B.G.DNSUB, True, nsteps=0, tracers=("age", "origin"))
        core.load_tracers({"origin": np.full((B.DNY, B.DNX), 7.0)})
        for k in range(1, 4):
            core.step()
            assert all(bool(torch.isfinite(f).all()) for f in (core.H, core.A, core.D, core.u, *core._tr))
            T.assert_uniform(core, "origin", 7.0, k)
            T.assert_uniform(core, "age", k * B.DDT, k)
        core.close()
    finally:
        c.close()


def test_column_state_run_stays_finite_and_uniform(gpu):
    n = 64
    c = abi.Context(gpu)
    try:
        bt, H, A, uo, vo, ua, va = T.pack(n, n * 4e3)
        core = gpu_core(c, bt, ("age", "origin"), cls=rowblock.CoupledCore, advect_column_state=True)
        core.load_global(H, A, uo, vo, ua, va)
        core.load_column(T.freezing_column(core, n))
        core.load_tracers({"origin": np.full((n, n), 7.0)})
        for k in range(1, 4):  # the column step off, as in the uniform-temperature test of the column state transport
            core._set_grid()
            core.momentum()
            core.transport()
            assert all(bool(torch.isfinite(f).all()) for f in (core.H, core.A, core.S, core.Q, core.u, *core._tr))
            T.assert_uniform(core, "origin", 7.0, k)
            T.assert_uniform(core, "age", k * DT, k)
        assert float(core.u.abs().max()) > 1e-4
        core.close()
    finally:
        c.close()


# ---- row blocks --------------------------------------------------------------------------------------------------------------------------
def world_run(world, native, nx=48, ny=64, nsub=18, steps=3):
    """`world` thread ranks (tests/thread_ranks.py), each with a context and a row block of its own: a CoupledCore with two tracers on the
    native plans and the native exchange's in-process transport, or on the Python sequence and the mailbox"""
    data = thread_ranks.fields(nx, ny)
    data[2][0, 30:36, 5:17] = 0.0  # (A) a lead across a block boundary: the ice test fails there
    data[1][0, 30:36, 5:17] = 0.0
    rng = np.random.default_rng(17)
    init = {"age": rng.uniform(0.0, 1e6, (ny, nx)), "origin": rng.uniform(-3.0, 3.0, (ny, nx))}
    st, fo, _ = synthetic.column_fields(nx * ny, 5)
    column = {k: v.reshape(ny, nx) for k, v in {**st, **fo}.items()}
    column["wind"] = 0.2 * column["wind"]
    mailbox, out = thread_ranks.Mailbox(), {}
    thread_ranks._local_group[0] += 1
    gid = thread_ranks._local_group[0]

    def rank_main(rank):
        try:
            c = abi.Context(torch.device("cuda:0"))
            c.comm_deadline(60.0)
            c.set_mevp_params(c.mevp_default_params(alpha=300.0, beta=300.0))
            blk = rowblock.RowBlock(nx, ny, rank, world, 4, 3)
            if native:
                exchanger = rowblock.NativeHaloExchanger(c, blk, local_group=gid) if world > 1 else None
            else:
                exchanger = thread_ranks.ThreadExchanger(blk, mailbox)
            bt, H, A, uo, vo, ua, va = data
            core = rowblock.CoupledCore(c, blk, bt.hx, bt.hy, DT, nsub, torch.device("cuda"), exchanger=exchanger, native=native,
                                        tracers=("age", "origin"))
            core.load_global(H, A, uo, vo, ua, va)
            core.load_column(column)
            core.load_tracers(init)
            for _ in range(steps):
                core.step()
            torch.cuda.synchronize()
            res = core.state_dict()
            res["ghosts"] = {name: t.cpu().numpy() for name, t in zip(core.tracers, core._tr)}, blk.elem_slice()
            core.close()
            c.close()
            out[rank] = res
        except BaseException as e:  # noqa: BLE001 -- wake the peers up; re-raised in the main thread
            with mailbox.cv:
                mailbox.error = e
                mailbox.cv.notify_all()
            out[rank] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    merged = rowblock.DynamicsCore.merge_states([{k: v for k, v in out[r].items() if k != "ghosts"} for r in range(world)])
    for r in range(world):  # the ghost rows of the tracers equal their owners without a message of their own
        local, es = out[r]["ghosts"]
        for name, t in local.items():
            assert same_bits(t, merged["tracers"][name][es]), (r, name)
    return merged


@pytest.mark.parametrize("native", [True, False])
def test_one_block_equals_four_blocks_bit_for_bit(gpu, native):
    one, four = world_run(1, native), world_run(4, native)
    same_state(one, four)
    assert np.any(one["tracers"]["origin"] == 0.0) and float(np.abs(one["u"]).max()) > 1e-5

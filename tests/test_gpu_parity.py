"""GPU parity tests: every call goes through the C ABI of libnsdg.so (hand-written HIP kernels) and is
compared with the CPU oracle on the same seeded inputs.

Tolerances (fp64, stated per test): the column step uses device exp/sqrt instead of glibc's and FMA
contraction, so element-wise agreement is required to 1e-11 relative (+ a tiny absolute floor);
DG transport and the mEVP operators involve only + - * / sqrt and agree to ~1e-13; long mEVP
sub-cycles to 1e-9 of the velocity scale.  Index/connectivity is exact by construction (identical
array layouts are compared entry by entry)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from nextsimdg_amd import abi, basis, synthetic

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "column_known_answers.json")))


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _no_closure_left_on_the_shared_context(ctx):
    """a DynamicsCore states the closure's bounds (H, A) on its context; tests that call the transport entry points with other field
    lists on the SAME context must not inherit them"""
    yield
    ctx.set_transport_bounds(())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tdev(a):
    """coefficient planes [nc, ny, nx] (oracle layout) -> tiled device array (stress, ice strength)"""
    return abi.tile(dev(a))


def thost(t, nx):
    return abi.untile(t, nx).cpu().numpy()


def host(t):
    return t.cpu().numpy()


def assert_close(got, want, rtol, atol, what=""):
    got, want = np.asarray(got), np.asarray(want)
    err = np.abs(got - want)
    lim = atol + rtol * np.abs(want)
    bad = err > lim
    if bad.any():
        w = int(np.argmax(np.where(bad, err - lim, -np.inf)))  # the entry that exceeds its own limit by most
        raise AssertionError("%s: %d/%d entries differ, worst violation at %d: err %.3e, limit %.3e (want %.17g got %.17g)" % (
            what, bad.sum(), bad.size, w, err.flat[w], np.broadcast_to(lim, err.shape).flat[w], want.flat[w], got.flat[w]))


# ------------------------------------------------------------------------------------ column physics
def test_column_known_answers_through_abi(ctx):
    """the reference's own known-answer tests (tests/golden/column_known_answers.json), on the GPU"""
    for case in GOLD["cases"]:
        p = ctx.column_default_params(**case["params"])
        ctx.set_column_params(p)
        inp = case["inputs"]
        state = {k: dev(np.array([inp[k]])) for k in abi.STATE}
        forcing = {k: dev(np.array([inp[k]])) for k in abi.FORCING}
        newice = dev(np.array([inp["newice"]]))
        diag = torch.zeros(abi.NDIAG, 1, dtype=torch.float64, device="cuda")
        ctx.column_step(case["dt"], state, forcing, newice, diag)
        got = {k: float(diag[i, 0]) for i, k in enumerate(abi.DIAG)}
        got.update({k: float(v[0]) for k, v in state.items()})
        got["newice"] = float(newice[0])
        for key, (want, rtol) in case["expect"].items():
            tol = max(rtol, 1e-12) * abs(want) + (1e-12 if want == 0.0 and rtol > 0 else 0.0)
            assert abs(got[key] - want) <= tol, (case["name"], key, got[key], want)
    ctx.set_column_params(ctx.column_default_params())


@pytest.mark.parametrize("pk", [dict(), dict(freezing="unesco", albedo="ccsm", ccsm_ice_albedo=0.63, ccsm_snow_albedo=0.88),
                                dict(albedo="smu2", flooding=0)], ids=["default", "unesco_ccsm", "smu2_noflood"])
def test_column_step_matches_oracle(ctx, pk):
    n = 50_001  # ragged: not a multiple of the block size
    state, forcing, newice = synthetic.column_fields(n)
    ctx.set_column_params(ctx.column_default_params(**pk))
    po = O.column_params(**pk)
    dstate = {k: dev(v) for k, v in state.items()}
    dforc = {k: dev(v) for k, v in forcing.items()}
    dnew = dev(newice)
    diag = torch.zeros(abi.NDIAG, n, dtype=torch.float64, device="cuda")
    for step in range(10):
        want_diag = O.column_step(po, 600.0, state, forcing, newice, want_diag=True)
        ctx.column_step(600.0, dstate, dforc, dnew, diag)
        # the oracle state is re-synchronised from the GPU state after the comparison so that a
        # legitimately flipped branch in one element cannot snowball over the 10 steps
        for k in abi.STATE:
            assert_close(host(dstate[k]), state[k], 1e-11, 1e-13, "step %d %s" % (step, k))
            state[k][:] = host(dstate[k])
        assert_close(host(dnew), newice, 1e-10, 1e-16, "step %d newice" % step)
        newice[:] = host(dnew)
        d = host(diag)
        for i, k in enumerate(abi.DIAG):
            scale = np.max(np.abs(want_diag[k])) + 1e-300
            assert_close(d[i], want_diag[k], 1e-10, 1e-13 * scale, "step %d diag %s" % (step, k))
    # forcing and sst/sss are read-only (core/src/PrognosticData.cpp:63-71 never touches sst/sss)
    for k in abi.FORCING:
        assert np.array_equal(host(dforc[k]), forcing[k])
    ctx.set_column_params(ctx.column_default_params())


RC_META, RC = O.ref_column_fixture()
RC_SETS = list(RC_META["sets"])


def assert_same_class(got, want, what):
    """NaN where the reference has NaN, +-Inf where it has the same Inf; nothing else is special"""
    for name, f in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
        bad = f(got) != f(want)
        assert not bad.any(), "%s: %s differs at %d entries (first %d)" % (what, name, bad.sum(), np.argmax(bad))


def assert_close_ref(got, want, rtol, atol, what):
    assert_same_class(got, want, what)
    fin = np.isfinite(want)
    assert_close(got[fin], want[fin], rtol, atol, what)


@pytest.mark.parametrize("name", RC_SETS)
def test_column_step_matches_reference_build(ctx, name):
    """nsdg_column_step against the reference's own column physics, recorded case by case (tests/golden/ref_column_v1.npz:
    random draw, the edge grid at each recorded dt, and 10 chained steps with forcing that changes per step), per module set.
    Chains are re-synchronised from the recording before every step.  1e-11 relative (device exp / sqrt / pow and FMA
    contraction against glibc) plus the tiny absolute floors of test_column_step_matches_oracle; NaN and Inf class for class."""
    ctx.set_column_params(ctx.column_default_params(**O.ref_column_set_params(RC_META, name)))
    for g in (x for x in RC_META["groups"] if x["set"] == name):
        key, ikey = "%s/%s/" % (name, g["group"]), g["inputs"] + "in/"
        nsteps = g["nsteps"]
        rec = RC.get(key + "out/record")
        for step in range(nsteps):
            if step == 0:
                state = {k: RC[ikey + k] for k in abi.STATE}
                newice = np.zeros(state["hice"].size)
            else:
                state = {k: rec[step - 1][i] for i, k in enumerate(abi.STATE)}
                newice = rec[step - 1][4]
            forcing = {k: RC[ikey + k][step] if nsteps > 1 else RC[ikey + k] for k in abi.FORCING}
            ds, df, dn = {k: dev(v) for k, v in state.items()}, {k: dev(v) for k, v in forcing.items()}, dev(newice)
            diag = torch.zeros(abi.NDIAG, newice.size, dtype=torch.float64, device="cuda")
            ctx.column_step(g["dt"], ds, df, dn, diag)
            if rec is not None:
                want = {k: rec[step][i] for i, k in enumerate(abi.STATE + ["newice"])}
            else:
                want = {k: RC[key + "out/" + k] for k in abi.STATE + ["newice"]}
            what = "%s step %d" % (key, step)
            for k in abi.STATE:
                assert_close_ref(host(ds[k]), want[k], 1e-11, 1e-13, "%s %s" % (what, k))
            assert_close_ref(host(dn), want["newice"], 1e-11, 1e-16, what + " newice")
            if step == nsteps - 1:
                d, wd = host(diag), RC[key + "out/diag"]
                for i, k in enumerate(abi.DIAG):
                    fin = np.isfinite(wd[i])
                    scale = (np.max(np.abs(wd[i][fin])) if fin.any() else 0.0) + 1e-300
                    assert_close_ref(d[i], wd[i], 1e-11, 1e-13 * scale, "%s diag %s" % (what, k))
    ctx.set_column_params(ctx.column_default_params())


def test_column_edge_cases(ctx):
    # empty input is a no-op
    e = torch.zeros(0, dtype=torch.float64, device="cuda")
    ctx.column_step(600.0, {k: e for k in abi.STATE}, {k: e for k in abi.FORCING}, e)
    # all-open-water and fully-covered columns, NaN propagation (no clamping is added)
    n = 4
    state = dict(hice=np.array([0.0, 2.0, 1.0, np.nan]), cice=np.array([0.0, 1.0, 1.0, 0.5]),
                 hsnow=np.array([0.0, 0.2, 0.0, 0.1]), tice0=np.array([-5.0, -5.0, -0.1, -5.0]))
    forcing = {k: np.full(n, v) for k, v in dict(sst=-1.5, sss=32.0, tair=-10.0, tdew=-12.0, slp=1e5, qsw=10.0,
                                                   qlw=250.0, mld=20.0, snowfall=1e-5, wind=7.0).items()}
    newice = np.zeros(n)
    ds = {k: dev(v) for k, v in state.items()}
    df = {k: dev(v) for k, v in forcing.items()}
    dn = dev(newice)
    O.column_step(O.column_params(), 600.0, state, forcing, newice)
    ctx.column_step(600.0, ds, df, dn)
    for k in abi.STATE:
        g, w = host(ds[k]), state[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), k
        assert_close(g[:3], w[:3], 1e-11, 1e-14, k)
    # bad arguments are reported, not ignored
    with pytest.raises(abi.NsdgError):
        ctx.set_column_params(ctx.column_default_params(albedo_kind=7))


def same_class(g, w):
    """NaN where NaN, +Inf where +Inf, -Inf where -Inf"""
    return (np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isposinf(g), np.isposinf(w))
            and np.array_equal(np.isneginf(g), np.isneginf(w)))


@pytest.mark.parametrize("dt", [600.0, 0.0])
def test_column_zero_denominators_follow_the_reference_arithmetic(ctx, dt):
    """The divisions of the reference whose denominator is a free input or a difference of data
    (NextsimPhysics.cpp:236,241 -- mixed-layer heat capacity and deltaTml; BasicIceOceanHeatFlux.cpp:24 and the other
    x/dt; ThermoIce0.cpp:58-63) are IEEE divisions on the device too, and the reciprocal-based ones end in the IEEE
    special-case fix-up: a zero mixed-layer depth, dt == 0, a flux that vanishes exactly, a concentration at and below
    the cut-off ON O(1) CELL MEANS (true thicknesses of 1e12-1e13 m) and an Inf forcing value give the oracle's
    Inf / NaN / finite values in every state variable and diagnostic, class for class and to 1e-11 where finite.

    Stated band for the ill-conditioned columns (profiles/r03_column_cutoff_cause.md): updateThickness,
    hi += (newice - hi del_c) / (c + del_c) (NextsimPhysics.cpp:257-260,278), cancels a true thickness h = H / c of
    up to 1e13 m down to O(1), so one ulp of h -- the difference between two correctly-working divisions, or between
    two libm exp -- is up to 1e-3 of the result.  The thickness and snow results are therefore compared to
    1e-11 |want| + 32 ulp(max(h_in, hs_in)) c_new (the snow can flood into ice of that thickness: H_new = hi_new c_new is the difference of two
    products of size h c_new, each rounded three or four times on either side); for c >= 1e-5 that band is below
    1e-11 |want| and changes nothing.  The cut-off DECISION (c_new < min_conc, NextsimPhysics.cpp:211) never differs: `cice` must
    agree exactly in being zero or not."""
    n = 4096
    state, forcing, newice = synthetic.column_fields(n, seed=99)
    rng = np.random.default_rng(5)
    forcing["mld"][rng.random(n) < 0.25] = 0.0  # mlbhc == 0: deltaTml = -+Inf (or NaN when the cooling flux is 0 too)
    state["cice"][rng.random(n) < 0.1] = 1e-12  # exactly min_conc, on O(1) cell means
    state["cice"][rng.random(n) < 0.05] = 1e-13  # below it
    state["hice"][rng.random(n) < 0.05] = 5e-324  # subnormal thickness
    forcing["qlw"][:7] = np.inf  # -> Q_ia = -Inf -> snow melt -Inf -> the thickness -Inf is cut off to zero
    # a column whose open-water flux vanishes exactly is not constructible from inputs; a zero wind and equal
    # temperatures remove all turbulent fluxes instead
    forcing["wind"][rng.random(n) < 0.3] = 0.0
    po = O.column_params()
    ctx.set_column_params(ctx.column_default_params())
    ds, df, dn = {k: dev(v) for k, v in state.items()}, {k: dev(v) for k, v in forcing.items()}, dev(newice)
    diag = torch.zeros(abi.NDIAG, n, dtype=torch.float64, device="cuda")
    def ulps8(x):  # 32 ulp of the true thickness that updateThickness cancels (0 where there is none)
        with np.errstate(all="ignore"):
            return np.nan_to_num(32 * np.spacing(np.abs(x)), nan=0.0, posinf=0.0)

    for step in range(3):
        with np.errstate(all="ignore"):
            h_in = np.where(state["cice"] != 0, state["hice"] / state["cice"], 0.0)
            hs_in = np.where(state["cice"] != 0, state["hsnow"] / state["cice"], 0.0)
            want = O.column_step(po, dt, state, forcing, newice, want_diag=True)
        ctx.column_step(dt, ds, df, dn, diag)
        got = {k: host(ds[k]) for k in abi.STATE}
        got["newice"] = host(dn)
        wantv = dict(state, newice=newice)
        c_new = np.nan_to_num(np.abs(state["cice"]), nan=0.0, posinf=0.0)
        # the thickness that is cancelled is the one ThermoIce0 leaves: h_in, or the ice flooded from hs_in of snow
        big = ulps8(np.maximum(np.abs(h_in), np.abs(hs_in)))
        band = {"hice": big * c_new, "hsnow": big * c_new}
        assert np.array_equal(got["cice"] == 0, state["cice"] == 0), step  # the cut-off decision itself never differs
        for k in list(abi.STATE) + ["newice"]:
            assert same_class(got[k], wantv[k]), (step, k)
            fin = np.isfinite(wantv[k])
            assert_close(got[k][fin], wantv[k][fin], 1e-11, 1e-13 + band.get(k, np.zeros(n))[fin], "step %d %s" % (step, k))
        d = host(diag)
        dband = {"hi": big, "hs": big, "hifroms": big}  # hifroms = draught - hi: the same cancellation
        for i, k in enumerate(abi.DIAG):
            assert same_class(d[i], want[k]), (step, k)
            fin = np.isfinite(want[k])
            scale = np.max(np.abs(want[k][fin])) if fin.any() else 1.0
            atol = dband[k][fin] + 1e-13 if k in dband else 1e-13 * scale
            assert_close(d[i][fin], want[k][fin], 1e-10, atol, "step %d diag %s" % (step, k))
        for k in abi.STATE:  # re-synchronise (see test_column_step_matches_oracle)
            state[k][:] = got[k]
        newice[:] = got["newice"]
    if dt > 0:
        assert np.isfinite(state["hice"]).mean() > 0.7  # the irregular inputs poison their own columns only
    # the production (two elements per lane, no diagnostics) kernel gives the same state as the diagnostic one
    ds2, dn2 = {k: dev(v) for k, v in state.items()}, dev(newice)
    ds3, dn3 = {k: dev(v) for k, v in state.items()}, dev(newice)
    ctx.column_step(dt, ds2, df, dn2, None)
    ctx.column_step(dt, ds3, df, dn3, diag)
    for k in abi.STATE:
        a, b = host(ds2[k]), host(ds3[k])
        assert same_class(a, b) and np.array_equal(a[np.isfinite(a)], b[np.isfinite(b)]), k


# ------------------------------------------------------------------------------------ DG transport
def adv_on_device(ctx, nx, ny, order, u, v):
    nc, ng = basis.NCOEF[order], order + 1
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    adv = (z(nc, ny, nx), z(nc, ny, nx), z(ng, ny, nx + 1), z(ng, ny + 1, nx))
    ctx.prepare_advection(order, dev(u), dev(v), *adv)
    return adv


@pytest.mark.parametrize("order", [0, 1, 2])
def test_prepare_advection_and_transport_match_oracle(ctx, order):
    nx, ny = 70, 37  # ragged in both directions
    rng = np.random.default_rng(3 + order)
    hx, hy = 1.0 / nx, 0.8 / ny
    X, Y = basis.node_coords(nx, ny, 1.0, 0.8)
    u = np.ascontiguousarray(np.sin(3 * X) * np.cos(2 * Y) + 0.3)
    v = np.ascontiguousarray(np.cos(2 * X + 1) * np.sin(4 * Y) - 0.2)
    ctx.set_grid(nx, ny, hx, hy)
    adv_o = O.prepare_advection(nx, ny, order, u, v)
    adv_d = adv_on_device(ctx, nx, ny, order, u, v)
    for a, b, name in zip(adv_d, adv_o, ("vx", "vy", "unx", "uny")):
        assert_close(host(a), b, 1e-13, 1e-14, name)
    nc = basis.NCOEF[order]
    phi = [rng.uniform(-1, 1, (nc, ny, nx)) for _ in range(2)]
    dphi = [dev(p) for p in phi]
    scratch = torch.zeros(2 * 2 * nc * nx * ny, dtype=torch.float64, device="cuda")
    dt = 0.1 * min(hx, hy) / 1.5 / (2 * order + 1)
    for _ in range(3):
        for p in phi:
            O.transport_step(nx, ny, hx, hy, order, dt, p, adv_o)
        ctx.transport_step(order, dt, dphi, adv_d, scratch)
    for p, d in zip(phi, dphi):
        assert_close(host(d), p, 1e-12, 1e-13, "transport order %d" % order)


def test_transport_stage_row_range_and_aliasing(ctx):
    nx, ny, order = 40, 12, 2
    ctx.set_grid(nx, ny, 0.1, 0.1)
    rng = np.random.default_rng(11)
    u = rng.uniform(-1, 1, (2 * ny + 1, 2 * nx + 1))
    v = rng.uniform(-1, 1, (2 * ny + 1, 2 * nx + 1))
    adv_o = O.prepare_advection(nx, ny, order, u, v)
    adv_d = adv_on_device(ctx, nx, ny, order, u, v)
    phi0 = rng.uniform(0, 1, (6, ny, nx))
    phis = rng.uniform(0, 1, (6, ny, nx))
    out_o = np.full((6, ny, nx), -7.0)
    O.transport_stage(nx, ny, 3, 9, 0.1, 0.1, order, 1e-3, 0.75, 0.25, phi0, phis, out_o, adv_o)
    out_d = torch.full((6, ny, nx), -7.0, dtype=torch.float64, device="cuda")
    ctx.transport_stage(order, 3, 9, 1e-3, 0.75, 0.25, [dev(phi0)], [dev(phis)], [out_d], adv_d)
    assert_close(host(out_d), out_o, 1e-12, 1e-13, "row range stage")
    assert np.all(host(out_d)[:, :3] == -7.0) and np.all(host(out_d)[:, 9:] == -7.0)  # rows outside untouched
    with pytest.raises(abi.NsdgError):
        ctx.transport_stage(order, 0, ny, 1e-3, 0.0, 1.0, [out_d], [out_d], [out_d], adv_d)
    with pytest.raises(abi.NsdgError):
        ctx.transport_stage(order, 0, ny + 1, 1e-3, 0.0, 1.0, [dev(phi0)], [dev(phis)], [out_d], adv_d)


# ------------------------------------------------------------------------------------ mEVP
class Box:
    def __init__(self, ctx, nx, ny, **pk):
        self.bt = bt = synthetic.BoxTest(nx, ny)
        self.nx, self.ny = nx, ny
        self.po = O.mevp_params(**pk)
        ctx.set_mevp_params(ctx.mevp_default_params(**pk))
        ctx.set_grid(nx, ny, bt.hx, bt.hy)
        rng = np.random.default_rng(5)
        H, A = bt.dg_fields()
        A[0] -= 0.2 * rng.random((ny, nx))
        H[1:] += 0.01 * rng.standard_normal(H[1:].shape)
        self.H, self.A = H, A
        self.uo, self.vo = [np.ascontiguousarray(a) for a in bt.ocean()]
        self.ua, self.va = [np.ascontiguousarray(a) for a in bt.wind(0.0)]


def test_mevp_helpers_match_oracle(ctx):
    b = Box(ctx, 37, 29)
    nx, ny = b.nx, b.ny
    pg_o = O.ice_strength(nx, ny, b.po, b.H, b.A)
    pg_d = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(dev(b.H), dev(b.A), pg_d)
    assert_close(thost(pg_d, nx), pg_o, 1e-12, 1e-10, "ice strength")
    for f in (b.H, b.A):
        cg_d = torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda")
        ctx.dg_to_cg(dev(f), cg_d)
        assert_close(host(cg_d), O.dg_to_cg(nx, ny, f), 1e-13, 1e-14, "dg_to_cg")
    tax_o, tay_o = O.wind_stress(b.po, b.ua, b.va)
    tax_d, tay_d = torch.zeros_like(dev(b.ua)), torch.zeros_like(dev(b.ua))
    ctx.wind_stress(dev(b.ua), dev(b.va), tax_d, tay_d)
    assert_close(host(tax_d), tax_o, 1e-13, 1e-16, "tax")
    assert_close(host(tay_d), tay_o, 1e-13, 1e-16, "tay")


@pytest.mark.parametrize("strain", [(2e-6, -1e-6, 0.5e-6), (-3e-6, -1e-6, 0.0), (0.0, 0.0, 1.5e-6)])
def test_device_stress_lies_on_hiblers_elliptic_yield_curve(ctx, strain):
    """The HIP stress update held to the LITERATURE directly, no oracle in between (the CPU twin of this test,
    tests/test_oracle_dynamics.py, does the same for the oracle and the independent restatement): a uniform strain rate far above
    Delta_min on a uniform cover relaxes to a uniform stress whose principal values lie on Hibler's ellipse
    ((s1 + s2) / P + 1)^2 + e^2 ((s1 - s2) / P)^2 = 1, e = 2, coaxial with the strain rate, strain rate normal to the yield curve."""
    from nextsimdg_amd import basis

    e11, e22, e12 = strain
    nx, ny, hx, hy = 70, 5, 500.0, 400.0
    pk = dict(alpha=2.0, beta=2.0, delta_min=2e-9)
    ctx.set_mevp_params(ctx.mevp_default_params(**pk))
    ctx.set_grid(nx, ny, hx, hy)
    po = O.mevp_params(**pk)
    H = np.zeros((6, ny, nx)); H[0] = 0.8
    A = np.zeros((6, ny, nx)); A[0] = 0.93
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(dev(H), dev(A), pg)
    P = po.pstar * 0.8 * np.exp(-po.compaction * 0.07)
    assert abs(float(abi.untile(pg, nx)[0, 0, 0]) - P) < 1e-9 * P
    X, Y = basis.node_coords(nx, ny, nx * hx, ny * hy)
    u, v = dev(e11 * X + e12 * Y), dev(e12 * X + e22 * Y)
    s = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
    for _ in range(80):  # alpha = 2: the distance to sigma(u, v) halves per sweep
        ctx.mevp_stress(0, ny, u, v, pg, *s)
    S = [thost(x, nx) for x in s]
    for c in range(3):
        assert np.max(np.abs(S[c][1:])) < 1e-9 * P and np.ptp(S[c][0]) < 1e-9 * P
    s11, s12, s22 = (float(S[c][0, 2, 33]) for c in range(3))
    mean, dev_ = 0.5 * (s11 + s22), np.hypot(0.5 * (s11 - s22), s12)
    s1, s2 = mean + dev_, mean - dev_
    assert abs(((s1 + s2) / P + 1.0) ** 2 + 4.0 * ((s1 - s2) / P) ** 2 - 1.0) < 1e-5
    d_eps, d_sig = np.array([0.5 * (e11 - e22), e12]), np.array([0.5 * (s11 - s22), s12])
    assert abs(d_eps[0] * d_sig[1] - d_eps[1] * d_sig[0]) < 1e-9 * np.linalg.norm(d_eps) * P and d_eps @ d_sig >= 0.0
    eI, eII = e11 + e22, 2.0 * np.linalg.norm(d_eps)
    gI, gII = 2.0 * ((s1 + s2) / P + 1.0), 8.0 * (s1 - s2) / P
    assert abs(eI * gII - eII * gI) < 2e-5 * np.hypot(eI, eII) * np.hypot(gI, gII)
    ctx.set_mevp_params(ctx.mevp_default_params())


@pytest.mark.parametrize("variant", [1, abi.DEFAULT_MEVP_VARIANT])
def test_device_strengthless_cover_reaches_the_free_drift_of_the_literature(ctx, variant):
    """P* = 0 on the device, through nsdg_mevp_subcycle (the pipelined kernel and the single-iteration one): after 70 model steps every
    interior node sits at the steady free drift -- scipy's solution of the published momentum balance (tests/test_oracle_dynamics.py:
    free_drift_solution), no oracle in between; ~2 % of the wind speed, to the right of the wind (f > 0)."""
    from test_oracle_dynamics import free_drift_case, free_drift_solution

    nx, ny = 70, 9
    hx, hy, ua, va, uo, vo, cgh, cga = free_drift_case(nx, ny)
    pk = dict(pstar=0.0, alpha=5.0, beta=5.0)
    ctx.set_mevp_variant(variant)
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
    for _ in range(70):
        ctx.mevp_subcycle(600.0, 30, s, u, v, u.clone(), v.clone(), tax, tay, duo, dvo, dh, da, pg, scratch)
    want = free_drift_solution(po, 9.0, -4.0, 0.05, 0.02, 0.7, 0.85)
    ui, vi = host(u)[1:-1, 1:-1], host(v)[1:-1, 1:-1]
    assert np.max(np.abs(ui - want[0])) < 1e-10 and np.max(np.abs(vi - want[1])) < 1e-10
    assert all(float(x.abs().max()) < 1e-12 for x in s)
    rel = np.array([want[0] - 0.05, want[1] - 0.02])
    assert 0.01 < np.linalg.norm(rel) / np.hypot(9.0, -4.0) < 0.03 and 9.0 * rel[1] + 4.0 * rel[0] < 0
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


def test_device_converged_subcycle_solves_the_implicit_vp_step(ctx):
    """the defining property of mEVP on the device: 2500 sub-iterations of the default (pipelined) kernel through nsdg_mevp_subcycle,
    then ONE Picard sweep of the implicit viscous-plastic step by the independent restatement (tests/test_oracle_dynamics.py:
    check_implicit_vp_fixed_point) returns the same stress and velocity -- no oracle in between"""
    from test_oracle_dynamics import check_implicit_vp_fixed_point, implicit_vp_case

    c = implicit_vp_case()
    nx, ny = c["nx"], c["ny"]
    ctx.set_mevp_params(ctx.mevp_default_params(**c["pk"]))
    ctx.set_grid(nx, ny, c["hx"], c["hy"])
    u, v = dev(c["u0"]), dev(c["v0"])
    s = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
    scratch = torch.zeros(10 * u.numel() + 3 * s[0].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_subcycle(c["dt"], 2500, s, u, v, dev(c["u0"]), dev(c["v0"]), dev(c["tax"]), dev(c["tay"]), dev(c["uo"]), dev(c["vo"]),
                      dev(c["cgh"]), dev(c["cga"]), tdev(c["pg"]), scratch)
    check_implicit_vp_fixed_point(c, host(u), host(v), [thost(x, nx) for x in s])
    ctx.set_mevp_params(ctx.mevp_default_params())


def pack(ctx, dt, u0, v0, tax, tay, uo, vo, cgh, cga):
    packed = torch.zeros(8 * u0.size, dtype=torch.float64, device="cuda")
    ctx.mevp_pack_nodal(dt, (dev(u0), dev(v0)), (dev(tax), dev(tay)), (dev(uo), dev(vo)), dev(cgh), dev(cga), packed)
    return packed


def mevp_state(b, rng):
    nx, ny = b.nx, b.ny
    shape = (2 * ny + 1, 2 * nx + 1)
    u = 0.05 * rng.standard_normal(shape)
    v = 0.05 * rng.standard_normal(shape)
    for a in (u, v):
        a[0] = a[-1] = 0
        a[:, 0] = a[:, -1] = 0
    s = [1e3 * rng.standard_normal((8, ny, nx)) for _ in range(3)]
    return u, v, s


@pytest.mark.parametrize("variant", [0, 1])
def test_mevp_single_iteration_matches_oracle(ctx, variant):
    ctx.set_mevp_variant(variant)
    b = Box(ctx, 67, 21)
    nx, ny = b.nx, b.ny
    rng = np.random.default_rng(17)
    u, v, s = mevp_state(b, rng)
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    u0, v0 = 0.9 * u, 0.9 * v
    ds = [tdev(x) for x in s]
    du, dv = dev(u), dev(v)
    dun, dvn = torch.full_like(du, 3.0), torch.full_like(dv, 3.0)
    packed = pack(ctx, 120.0, u0, v0, tax, tay, b.uo, b.vo, cgh, cga)
    dso = [torch.zeros_like(x) for x in ds]
    ctx.mevp_iterate(0, 0, ny, ds, dso, (du, dv), (dun, dvn), packed, tdev(pg))
    ds = dso
    # oracle
    O.mevp_stress(nx, ny, 0, ny, b.bt.hx, b.bt.hy, b.po, u, v, pg, *s)
    un, vn = np.full_like(u, 3.0), np.full_like(v, 3.0)
    O.mevp_velocity(nx, ny, 0, ny, b.bt.hx, b.bt.hy, 120.0, b.po, s, (u, v), (un, vn), (u0, v0), (tax, tay),
                    (b.uo, b.vo), cgh, cga)
    for d, o, name in zip(ds, s, ("s11", "s12", "s22")):
        assert_close(thost(d, nx), o, 1e-12, 1e-12 * np.max(np.abs(o)), name)
    assert_close(host(dun), un, 1e-11, 1e-13 * np.max(np.abs(un)), "u_new")
    assert_close(host(dvn), vn, 1e-11, 1e-13 * np.max(np.abs(vn)), "v_new")
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_mevp_subcycle_matches_oracle(ctx, variant):
    """25 sub-iterations through nsdg_mevp_subcycle against the oracle's 25, for EVERY kernel variant directly (round-4 review:
    the default, variant 4, reached the oracle only through its bitwise equality with variant 1): variant 4 runs 6 passes of four
    and one single sub-iteration, variant 3 eight passes of three and one, variant 2 twelve of two and one"""
    ctx.set_mevp_variant(variant)
    b = Box(ctx, 48, 40, alpha=300.0, beta=300.0)
    nx, ny = b.nx, b.ny
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = np.zeros(shape), np.zeros(shape)
    u0, v0 = u.copy(), v.copy()
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    du, dv, ds = dev(u), dev(v), [tdev(x) for x in s]
    scratch = torch.zeros(10 * u.size + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
    nsub = 25  # odd: exercises the copy-back of the ping-pong buffers
    ctx.mevp_subcycle(120.0, nsub, ds, du, dv, dev(u0), dev(v0), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh),
                      dev(cga), tdev(pg), scratch)
    O.mevp_subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, nsub, b.po, s, u, v, u0, v0, tax, tay, b.uo, b.vo, cgh, cga, pg)
    assert np.max(np.abs(u)) > 1e-4
    assert_close(host(du), u, 1e-9, 1e-11 * np.max(np.abs(u)), "u after subcycle")
    assert_close(host(dv), v, 1e-9, 1e-11 * np.max(np.abs(v)), "v after subcycle")
    for d, o in zip(ds, s):
        assert_close(thost(d, nx), o, 1e-9, 1e-10 * np.max(np.abs(o)), "stress after subcycle")
    # Dirichlet rows/columns are exactly zero
    g = host(du)
    assert np.all(g[0] == 0) and np.all(g[-1] == 0) and np.all(g[:, 0] == 0) and np.all(g[:, -1] == 0)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)


@pytest.mark.parametrize("variant", [abi.DEFAULT_MEVP_VARIANT, 1])
def test_mevp_baseline_subcycle_of_120_matches_oracle(ctx, variant):
    """The sub-cycle LENGTH of the BASELINE configs -- 120 sub-iterations = 30 passes of the default four-iteration kernel -- on a
    96 x 80 box test with alpha = beta from BoxTest.stable_alpha (the bench's choice), against 120 sub-iterations of
    oracle/dyn_oracle.c.  Tolerance: 1e-8 of the largest velocity / stress (25 sub-iterations hold 1e-11; the round-off of the two
    arithmetic orders is carried through 120 relaxations of a stable iteration).  Parity unpinned: the oracle is this
    repository's own restatement, the reference has no dynamics (CMakeLists.txt:43-46)."""
    ctx.set_mevp_variant(variant)
    nx, ny, nsub, dt = 96, 80, 120, 120.0
    alpha = synthetic.BoxTest(nx, ny).stable_alpha(dt)
    b = Box(ctx, nx, ny, alpha=alpha, beta=alpha)
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = np.zeros(shape), np.zeros(shape)
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    du, dv, ds = dev(u), dev(v), [tdev(x) for x in s]
    scratch = torch.zeros(10 * u.size + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_subcycle(dt, nsub, ds, du, dv, dev(u), dev(v), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh), dev(cga), tdev(pg), scratch)
    O.mevp_subcycle(nx, ny, b.bt.hx, b.bt.hy, dt, nsub, b.po, s, u, v, u.copy(), v.copy(), tax, tay, b.uo, b.vo, cgh, cga, pg)
    assert np.max(np.abs(u)) > 1e-4 and np.all(np.isfinite(u))
    assert_close(host(du), u, 1e-8, 1e-8 * np.max(np.abs(u)), "u after 120 sub-iterations")
    assert_close(host(dv), v, 1e-8, 1e-8 * np.max(np.abs(v)), "v after 120 sub-iterations")
    for d, o in zip(ds, s):
        assert_close(thost(d, nx), o, 1e-8, 1e-8 * np.max(np.abs(o)), "stress after 120 sub-iterations")
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


def test_mevp_row_block_equals_full_domain_bitwise(ctx):
    """A row-block 'rank' (ghost row below, redundant stress update on it) reproduces the full-domain
    result bit for bit: the gather formulation makes the arithmetic independent of the decomposition."""
    for variant in (0, 1):
        ctx.set_mevp_variant(variant)
        b = Box(ctx, 40, 24)
        nx, ny = b.nx, b.ny
        rng = np.random.default_rng(23)
        u, v, s = mevp_state(b, rng)
        pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
        cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
        tax, tay = O.wind_stress(b.po, b.ua, b.va)
        full = [torch.zeros_like(tdev(x)) for x in s]
        un, vn = torch.zeros_like(dev(u)), torch.zeros_like(dev(v))
        packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
        ctx.mevp_iterate(0, 0, ny, [tdev(x) for x in s], full, (dev(u), dev(v)), (un, vn), packed, tdev(pg))
        # upper rank: owns element rows [12, 24); local array = rows [11, 24) (ghost row below)
        r0 = 12
        lo = r0 - 1
        sl_e = lambda a: np.ascontiguousarray(a[:, lo:])
        sl_n = lambda a: np.ascontiguousarray(a[2 * lo:])
        ctx.set_grid(nx, ny - lo, b.bt.hx, b.bt.hy)
        part = [torch.zeros_like(tdev(sl_e(x))) for x in s]
        pun, pvn = torch.zeros_like(dev(sl_n(u))), torch.zeros_like(dev(sl_n(v)))
        ppacked = pack(ctx, 120.0, *[sl_n(x) for x in (0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)])
        ctx.mevp_iterate(0, 1, ny - lo, [tdev(sl_e(x)) for x in s], part, (dev(sl_n(u)), dev(sl_n(v))), (pun, pvn), ppacked,
                         tdev(sl_e(pg)))
        for f, p in zip(full, part):
            assert torch.equal(f[lo:], p)  # tiled arrays: element rows are the leading dimension
        assert torch.equal(un[2 * r0:], pun[2:])
        assert torch.equal(vn[2 * r0:], pvn[2:])
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)


def test_mevp_fused_strip_size_does_not_change_results(ctx):
    """the fused marching kernel recomputes strip-boundary rows/columns redundantly; whatever the strip
    height, results are bit-identical, and they agree with the two-kernel variant to round-off"""
    b = Box(ctx, 130, 45)
    nx, ny = b.nx, b.ny
    rng = np.random.default_rng(29)
    u, v, s = mevp_state(b, rng)
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
    results = []
    for variant, rows in ((0, 16), (1, 1), (1, 7), (1, 16), (1, 64), (1, 0)):
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_strip_rows(rows)
        so = [torch.zeros_like(tdev(x)) for x in s]
        un, vn = torch.full_like(dev(u), 9.0), torch.full_like(dev(v), 9.0)
        ctx.mevp_iterate(0, 0, ny, [tdev(x) for x in s], so, (dev(u), dev(v)), (un, vn), packed, tdev(pg))
        results.append(so + [un, vn])
    for r in results[2:]:
        for a, c in zip(results[1], r):
            assert torch.equal(a, c)
    for a, c in zip(results[0], results[1]):
        assert_close(host(c), host(a), 1e-12, 1e-13 * float(a.abs().max()), "fused vs two-kernel")
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)


def test_mevp_split_sub_iteration_equals_single_launch_bitwise(ctx):
    """the multi-rank driver computes the boundary rows first (so that their node rows can travel while the
    interior is computed): three launches over row ranges must reproduce the single launch bit for bit"""
    b = Box(ctx, 70, 24)
    nx, ny = b.nx, b.ny
    rng = np.random.default_rng(31)
    u, v, s = mevp_state(b, rng)
    pg = tdev(O.ice_strength(nx, ny, b.po, b.H, b.A))
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
    s_in = [tdev(x) for x in s]
    one = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
    ctx.mevp_iterate(0, 0, ny, s_in, one[:3], (dev(u), dev(v)), (one[3], one[4]), packed, pg)
    three = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
    ctx.mevp_iterate(ny - 2, ny - 1, ny, s_in, three[:3], (dev(u), dev(v)), (three[3], three[4]), packed, pg)
    ctx.mevp_iterate(0, 0, 1, s_in, three[:3], (dev(u), dev(v)), (three[3], three[4]), packed, pg)
    ctx.mevp_iterate(0, 1, ny - 1, s_in, three[:3], (dev(u), dev(v)), (three[3], three[4]), packed, pg)
    for a, c in zip(one, three):
        assert torch.equal(a, c)


def test_coupled_step_matches_oracle(ctx):
    """config-5-style step (column physics on the DG cell means, then mEVP + transport) through the
    row-block driver: HIP kernels vs the same driver running on the oracle"""
    from oracle_ops import OracleOps
    from nextsimdg_amd import rowblock

    nx, ny, nsub = 40, 31, 6
    bt = synthetic.BoxTest(nx, ny)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((ny, nx))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    state, forcing, _ = synthetic.column_fields(nx * ny, 9)
    col = {k: v.reshape(ny, nx) for k, v in {**state, **forcing}.items()}
    col["wind"] = 0.2 * col["wind"]
    ctx.set_mevp_params(ctx.mevp_default_params(alpha=200.0, beta=200.0))
    ctx.set_column_params(ctx.column_default_params())
    cores = []
    for ops, device in ((ctx, torch.device("cuda")), (OracleOps(alpha=200.0, beta=200.0), torch.device("cpu"))):
        core = rowblock.CoupledCore(ops, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, 120.0, nsub, device)
        core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
        core.load_column(col)
        for _ in range(2):
            core.step()
        cores.append(core)
    g, o = cores
    assert float((o.A[0] - dev(A[0]).cpu()).abs().max()) > 1e-3
    for name in ("H", "A", "u", "v"):
        a, b = getattr(g, name).cpu().numpy(), getattr(o, name).numpy()
        assert_close(a, b, 1e-9, 1e-11 * np.max(np.abs(b)), "coupled " + name)
    assert_close(g.col["tice0"].cpu().numpy(), o.col["tice0"].numpy(), 1e-10, 1e-12, "coupled tice0")
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_transport_bounds(())  # the cores set the closure's bounds (H, A) on the shared context


def test_mevp_two_iterations_per_pass_equals_two_single_passes_bitwise(ctx):
    """variant 2 keeps the intermediate stress / velocity of a pair of sub-iterations in registers;
    it must reproduce two launches of the single-iteration fused kernel bit for bit, for any strip
    height, and agree with the oracle"""
    for (nx, ny) in ((130, 45), (61, 9), (200, 3)):
        b = Box(ctx, nx, ny)
        rng = np.random.default_rng(37)
        u, v, s = mevp_state(b, rng)
        pg_o = O.ice_strength(nx, ny, b.po, b.H, b.A)
        cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
        tax, tay = O.wind_stress(b.po, b.ua, b.va)
        packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
        pg = tdev(pg_o)
        s_in = [tdev(x) for x in s]
        # reference: two single-iteration passes
        ctx.set_mevp_variant(1)
        ctx.set_mevp_strip_rows(0)
        mid = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
        ctx.mevp_iterate(0, 0, ny, s_in, mid[:3], (dev(u), dev(v)), (mid[3], mid[4]), packed, pg)
        ref = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
        ctx.mevp_iterate(0, 0, ny, mid[:3], ref[:3], (mid[3], mid[4]), (ref[3], ref[4]), packed, pg)
        ctx.set_mevp_variant(2)
        for rows in (1, 4, 7, 16, 64, 0):
            ctx.set_mevp_strip_rows(rows)
            out = [torch.zeros_like(x) for x in s_in] + [torch.full_like(dev(u), 7.0), torch.full_like(dev(v), 7.0)]
            ctx.mevp_iterate2(0, ny, s_in, out[:3], (dev(u), dev(v)), (out[3], out[4]), packed, pg)
            for a, c in zip(ref, out):
                assert torch.equal(a, c), (nx, ny, rows)
        # and against the oracle
        so = [x.copy() for x in s]
        uo_, vo_ = u.copy(), v.copy()
        O.mevp_subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 2, b.po, so, uo_, vo_, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga, pg_o)
        assert_close(host(ref[3]), uo_, 1e-10, 1e-12 * np.max(np.abs(uo_)), "u after two sub-iterations")
        assert_close(thost(ref[0], nx), so[0], 1e-10, 1e-12 * np.max(np.abs(so[0])), "s11 after two sub-iterations")
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)


def test_mevp_three_iterations_per_pass_equals_three_single_passes_bitwise(ctx):
    """variant 3 pipelines three sub-iterations per pass (A -> B in registers, B -> C through LDS); it must
    reproduce three launches of the single-iteration fused kernel bit for bit, for any strip height, for
    widths around the 59 owned columns of a wave, for sub-ranges of rows, and inside nsdg_mevp_subcycle
    (remainders of 2 and 1 sub-iterations through the kernels of variants 2 and 1)"""
    for (nx, ny) in ((130, 45), (59, 9), (60, 11), (200, 3), (58, 1), (7, 5)):
        b = Box(ctx, nx, ny)
        rng = np.random.default_rng(53)
        u, v, s = mevp_state(b, rng)
        pg_o = O.ice_strength(nx, ny, b.po, b.H, b.A)
        cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
        tax, tay = O.wind_stress(b.po, b.ua, b.va)
        packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
        pg = tdev(pg_o)
        s_in = [tdev(x) for x in s]
        ctx.set_mevp_variant(1)
        ctx.set_mevp_strip_rows(0)
        cur = s_in + [dev(u), dev(v)]
        for _ in range(3):
            nxt = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
            ctx.mevp_iterate(0, 0, ny, cur[:3], nxt[:3], (cur[3], cur[4]), (nxt[3], nxt[4]), packed, pg)
            cur = nxt
        ref = cur
        ctx.set_mevp_variant(3)
        for rows in (1, 2, 5, 16, 64, 0):
            ctx.set_mevp_strip_rows(rows)
            out = [torch.zeros_like(x) for x in s_in] + [torch.full_like(dev(u), 7.0), torch.full_like(dev(v), 7.0)]
            ctx.mevp_iterate3(0, ny, s_in, out[:3], (dev(u), dev(v)), (out[3], out[4]), packed, pg)
            for k, (a, c) in enumerate(zip(ref, out)):
                assert torch.equal(a, c), (nx, ny, rows, k, float((a - c).abs().max()))
        if ny >= 11:  # a sub-range with ghost rows on both sides: rows [3, ny - 2)
            ctx.set_mevp_strip_rows(0)
            out = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
            ctx.mevp_iterate3(3, ny - 2, s_in, out[:3], (dev(u), dev(v)), (out[3], out[4]), packed, pg)
            assert torch.equal(abi.untile(out[0], nx)[:, 3:ny - 2], abi.untile(ref[0], nx)[:, 3:ny - 2])
            assert torch.equal(out[3][6:2 * (ny - 2)], ref[3][6:2 * (ny - 2)])
        # against the oracle
        so = [x.copy() for x in s]
        uo_, vo_ = u.copy(), v.copy()
        O.mevp_subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 3, b.po, so, uo_, vo_, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga, pg_o)
        assert_close(host(ref[3]), uo_, 1e-10, 1e-12 * np.max(np.abs(uo_)), "u after three sub-iterations")
        assert_close(thost(ref[0], nx), so[0], 1e-10, 1e-12 * np.max(np.abs(so[0])), "s11 after three sub-iterations")
    # whole sub-cycle: 3-passes + remainder 2 (nsub = 8) and remainder 1 (nsub = 7) against variant 1
    b = Box(ctx, 70, 33, alpha=300.0, beta=300.0)
    nx, ny = b.nx, b.ny
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    shape = (2 * ny + 1, 2 * nx + 1)
    for nsub in (8, 7, 9):
        res = {}
        for variant in (1, 3):
            ctx.set_mevp_variant(variant)
            du, dv = dev(np.zeros(shape)), dev(np.zeros(shape))
            ds = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
            scratch = torch.zeros(10 * du.numel() + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
            ctx.mevp_subcycle(120.0, nsub, ds, du, dv, du.clone(), dv.clone(), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh), dev(cga),
                              tdev(pg), scratch)
            res[variant] = (du, dv, ds)
        assert torch.equal(res[1][0], res[3][0]) and torch.equal(res[1][1], res[3][1]), nsub
        assert all(torch.equal(a, c) for a, c in zip(res[1][2], res[3][2])), nsub
        assert float(res[3][0].abs().max()) > 0
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_mevp_params(ctx.mevp_default_params())


def test_mevp_four_iterations_per_pass_equals_four_single_passes_bitwise(ctx):
    """variant 4 runs four sub-iterations per pass, one pipeline stage per wave of a four-wave workgroup (hand-over
    through LDS, point to point: counters in LDS, no barrier in the march); it must reproduce four launches of the single-iteration
    fused kernel bit for bit, for any strip height, for widths around the 57 owned columns of a workgroup, for
    sub-ranges of rows, for two ranges in one launch, and inside nsdg_mevp_subcycle (remainders of 3, 2 and 1
    sub-iterations: passes of 3 / 2 stages of the same kernel, and the single-iteration kernel)"""
    for (nx, ny) in ((130, 45), (57, 9), (58, 13), (200, 3), (56, 1), (7, 5), (115, 22)):
        b = Box(ctx, nx, ny)
        rng = np.random.default_rng(59)
        u, v, s = mevp_state(b, rng)
        pg_o = O.ice_strength(nx, ny, b.po, b.H, b.A)
        cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
        tax, tay = O.wind_stress(b.po, b.ua, b.va)
        packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
        pg = tdev(pg_o)
        s_in = [tdev(x) for x in s]
        ctx.set_mevp_variant(1)
        ctx.set_mevp_strip_rows(0)
        cur = s_in + [dev(u), dev(v)]
        for _ in range(4):
            nxt = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
            ctx.mevp_iterate(0, 0, ny, cur[:3], nxt[:3], (cur[3], cur[4]), (nxt[3], nxt[4]), packed, pg)
            cur = nxt
        ref = cur
        ctx.set_mevp_variant(4)
        for rows in (1, 2, 5, 16, 64, 0):
            ctx.set_mevp_strip_rows(rows)
            out = [torch.zeros_like(x) for x in s_in] + [torch.full_like(dev(u), 7.0), torch.full_like(dev(v), 7.0)]
            ctx.mevp_iterate4(0, ny, s_in, out[:3], (dev(u), dev(v)), (out[3], out[4]), packed, pg)
            for k, (a, c) in enumerate(zip(ref, out)):
                assert torch.equal(a, c), (nx, ny, rows, k, float((a - c).abs().max()))
        if ny >= 13:  # a sub-range with ghost rows on both sides: rows [4, ny - 3)
            for rows in (0, 3):
                ctx.set_mevp_strip_rows(rows)
                out = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
                ctx.mevp_iterate4(4, ny - 3, s_in, out[:3], (dev(u), dev(v)), (out[3], out[4]), packed, pg)
                assert torch.equal(abi.untile(out[0], nx)[:, 4:ny - 3], abi.untile(ref[0], nx)[:, 4:ny - 3])
                assert torch.equal(out[3][8:2 * (ny - 3)], ref[3][8:2 * (ny - 3)])
        if ny >= 22:  # two disjoint ranges in one launch == two launches
            ctx.set_mevp_strip_rows(0)
            ra, rb = (ny - 7, ny - 3), (4, 9)
            one = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
            two = [torch.zeros_like(x) for x in s_in] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
            ctx.mevp_iterate4_pair(ra, rb, s_in, one[:3], (dev(u), dev(v)), (one[3], one[4]), packed, pg)
            for r in (ra, rb):
                ctx.mevp_iterate4(r[0], r[1], s_in, two[:3], (dev(u), dev(v)), (two[3], two[4]), packed, pg)
            assert all(torch.equal(a, c) for a, c in zip(one, two))
            assert torch.equal(abi.untile(one[1], nx)[:, 4:9], abi.untile(ref[1], nx)[:, 4:9])
            assert torch.equal(one[4][2 * (ny - 7):2 * (ny - 3)], ref[4][2 * (ny - 7):2 * (ny - 3)])
        # against the oracle
        so = [x.copy() for x in s]
        uo_, vo_ = u.copy(), v.copy()
        O.mevp_subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, 4, b.po, so, uo_, vo_, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga, pg_o)
        assert_close(host(ref[3]), uo_, 1e-10, 1e-12 * np.max(np.abs(uo_)), "u after four sub-iterations")
        assert_close(thost(ref[0], nx), so[0], 1e-10, 1e-12 * np.max(np.abs(so[0])), "s11 after four sub-iterations")
    # whole sub-cycle: 4-passes + remainders 3 (nsub = 11), 2 (10), 1 (9), 0 (8) against variant 1
    b = Box(ctx, 70, 33, alpha=300.0, beta=300.0)
    nx, ny = b.nx, b.ny
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    shape = (2 * ny + 1, 2 * nx + 1)
    for nsub in (11, 10, 9, 8):
        res = {}
        for variant in (1, 4):
            ctx.set_mevp_variant(variant)
            du, dv = dev(np.zeros(shape)), dev(np.zeros(shape))
            ds = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
            scratch = torch.zeros(10 * du.numel() + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
            ctx.mevp_subcycle(120.0, nsub, ds, du, dv, du.clone(), dv.clone(), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh), dev(cga),
                              tdev(pg), scratch)
            res[variant] = (du, dv, ds)
        assert torch.equal(res[1][0], res[4][0]) and torch.equal(res[1][1], res[4][1]), nsub
        assert all(torch.equal(a, c) for a, c in zip(res[1][2], res[4][2])), nsub
        assert float(res[4][0].abs().max()) > 0
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_mevp_params(ctx.mevp_default_params())


def test_mevp_subcycle_variant2_matches_oracle(ctx):
    ctx.set_mevp_variant(2)
    b = Box(ctx, 48, 40, alpha=300.0, beta=300.0)
    nx, ny = b.nx, b.ny
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = np.zeros(shape), np.zeros(shape)
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    du, dv, ds = dev(u), dev(v), [tdev(x) for x in s]
    scratch = torch.zeros(10 * u.size + 3 * ds[0].numel(), dtype=torch.float64, device="cuda")
    nsub = 25  # 12 double passes + one single sub-iteration
    ctx.mevp_subcycle(120.0, nsub, ds, du, dv, dev(u.copy()), dev(v.copy()), dev(tax), dev(tay), dev(b.uo), dev(b.vo), dev(cgh),
                      dev(cga), tdev(pg), scratch)
    O.mevp_subcycle(nx, ny, b.bt.hx, b.bt.hy, 120.0, nsub, b.po, s, u, v, u.copy(), v.copy(), tax, tay, b.uo, b.vo, cgh, cga, pg)
    assert_close(host(du), u, 1e-9, 1e-11 * np.max(np.abs(u)), "u after subcycle (variant 2)")
    assert_close(thost(ds[0], nx), s[0], 1e-9, 1e-10 * np.max(np.abs(s[0])), "s11 after subcycle (variant 2)")
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)


def test_mevp_two_per_pass_row_block_equals_full_domain_bitwise(ctx):
    """variant 2 on a row-block sub-domain (2 ghost element rows below, 1 above, as the multi-rank driver
    keeps them) reproduces the full-domain pass bit for bit on the rows it owns"""
    ctx.set_mevp_variant(2)
    b = Box(ctx, 90, 40)
    nx, ny = b.nx, b.ny
    rng = np.random.default_rng(53)
    u, v, s = mevp_state(b, rng)
    pg = O.ice_strength(nx, ny, b.po, b.H, b.A)
    cgh, cga = O.dg_to_cg(nx, ny, b.H), O.dg_to_cg(nx, ny, b.A)
    tax, tay = O.wind_stress(b.po, b.ua, b.va)
    packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
    full = [torch.zeros_like(tdev(x)) for x in s] + [torch.zeros_like(dev(u)), torch.zeros_like(dev(v))]
    ctx.mevp_iterate2(0, ny, [tdev(x) for x in s], full[:3], (dev(u), dev(v)), (full[3], full[4]), packed, tdev(pg))
    # middle rank: owns global rows [14, 27); local array = rows [12, 28)
    r0, r1 = 14, 27
    lo, hi = r0 - 2, r1 + 1
    sl_e = lambda a: np.ascontiguousarray(a[:, lo:hi])
    sl_n = lambda a: np.ascontiguousarray(a[2 * lo:2 * hi + 1])
    ctx.set_grid(nx, hi - lo, b.bt.hx, b.bt.hy)
    ppacked = pack(ctx, 120.0, *[sl_n(x) for x in (0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)])
    part = [torch.zeros_like(tdev(sl_e(x))) for x in s] + [torch.zeros_like(dev(sl_n(u))), torch.zeros_like(dev(sl_n(v)))]
    for (j0, j1) in ((2, 4), (4, 10), (10, r1 - lo)):  # three launches over row ranges, like the overlapping driver
        ctx.mevp_iterate2(j0, j1, [tdev(sl_e(x)) for x in s], part[:3], (dev(sl_n(u)), dev(sl_n(v))), (part[3], part[4]), ppacked,
                          tdev(sl_e(pg)))
    for k in range(3):
        assert torch.equal(full[k][r0:r1], part[k][2:2 + r1 - r0])
    for k in (3, 4):
        assert torch.equal(full[k][2 * r0:2 * r1], part[k][4:4 + 2 * (r1 - r0)])


@pytest.mark.parametrize("nx", [131, 132, 2])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_transport_pair_kernel_equals_gather_kernel_bitwise(ctx, order, nx):
    """the two-elements-per-lane kernel (16-byte accesses, even nx; an odd nx falls back) and the one-lane-per-element gather
    kernel run the same transport_rhs arithmetic: bit-identical for any workgroup height, ragged sizes, row ranges, one to
    three fields"""
    ny = 37
    rng = np.random.default_rng(61 + order)
    ctx.set_grid(nx, ny, 0.01, 0.02)
    u = rng.uniform(-1, 1, (2 * ny + 1, 2 * nx + 1))
    v = rng.uniform(-1, 1, (2 * ny + 1, 2 * nx + 1))
    adv = adv_on_device(ctx, nx, ny, order, u, v)
    nc = basis.NCOEF[order]
    phi0 = [dev(rng.uniform(0, 1, (nc, ny, nx))) for _ in range(3)]
    phis = [dev(rng.uniform(0, 1, (nc, ny, nx))) for _ in range(3)]
    outs = []
    for variant, rows in ((0, 0), (0, 1), (2, 0), (2, 1), (2, 3)):
        ctx.set_transport_variant(variant, rows)
        out = [torch.full((nc, ny, nx), -3.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        ctx.transport_stage(order, 0, ny, 1e-3, 0.75, 0.25, phi0, phis, out, adv)
        ctx.transport_stage(order, 4, 29, 2e-3, 0.0, 1.0, phi0[:2], phis[:2], out[:2], adv)  # overwrite a row range of two fields
        ctx.transport_stage(order, 30, 31, 3e-3, 1.0 / 3.0, 2.0 / 3.0, phi0[2:], phis[2:], out[2:], adv)  # ... and one row of the third
        outs.append(out)
    for o in outs[1:]:
        for a, c in zip(outs[0], o):
            assert torch.equal(a, c)
    with pytest.raises(abi.NsdgError, match="removed"):
        ctx.set_transport_variant(1, 0)
    ctx.set_transport_variant(abi.DEFAULT_TRANSPORT_VARIANT, 0)


def test_mevp_prepare_equals_separate_kernels_bitwise(ctx):
    """the fused per-step nodal preparation (nodal means of H, A + wind stress + packing) writes exactly
    what dg_to_cg x2 + wind_stress + mevp_pack_nodal write"""
    b = Box(ctx, 97, 41)
    nx, ny = b.nx, b.ny
    rng = np.random.default_rng(67)
    shape = (2 * ny + 1, 2 * nx + 1)
    u0, v0 = dev(0.1 * rng.standard_normal(shape)), dev(0.1 * rng.standard_normal(shape))
    dH, dA = dev(b.H), dev(b.A)
    ua, va, uo, vo = dev(b.ua), dev(b.va), dev(b.uo), dev(b.vo)
    z = lambda: torch.zeros(shape, dtype=torch.float64, device="cuda")
    cgh, cga, tax, tay = z(), z(), z(), z()
    ctx.dg_to_cg(dH, cgh)
    ctx.dg_to_cg(dA, cga)
    ctx.wind_stress(ua, va, tax, tay)
    p1 = torch.zeros(8 * u0.numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_pack_nodal(120.0, (u0, v0), (tax, tay), (uo, vo), cgh, cga, p1)
    p2 = torch.zeros_like(p1)
    ctx.mevp_prepare(120.0, dH, dA, (ua, va), (uo, vo), (u0, v0), p2)
    assert torch.equal(p1, p2)


# ------------------------------------------------------------------------------------ frozen oracle outputs (self-fixture)
def frozen(case):
    """arrays of one case of tests/golden/dyn_selfcheck_v1 (self-fixture -- NOT reference parity, see tests/dyn_fixture_cases.py)"""
    import json
    import os

    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    idx = json.load(open(os.path.join(golden, "dyn_selfcheck_v1.json")))
    data = np.fromfile(os.path.join(golden, idx["data_file"]), dtype="<f8")
    return {e["name"]: data[e["offset"]:e["offset"] + int(np.prod(e["shape"]))].reshape(e["shape"]) for e in idx["arrays"] if e["case"] == case}


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_hip_path_matches_the_frozen_oracle_outputs(ctx, variant):
    """The HIP path against the COMMITTED outputs of oracle/dyn_oracle.c (tests/golden/dyn_selfcheck_v1.*), at the
    tolerances of the live comparisons above: DG0/1/2 transport (3 steps, 70 x 37), one mEVP sub-iteration (67 x 21), the
    25-sub-iteration cycle (48 x 40), one coupled step (40 x 32).  Self-fixture, not reference parity: it pins the kernels
    to what the specification computed when the fixture was written, whatever the oracle in the tree computes today."""
    import dyn_fixture_cases as cases

    ctx.set_mevp_variant(variant)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    # ---- transport
    for order in cases.ORDERS:
        want = frozen("transport_dg%d" % order)
        i = cases.inputs_transport(order)
        nx, ny = i["nx"], i["ny"]
        ctx.set_grid(nx, ny, i["hx"], i["hy"])
        adv = adv_on_device(ctx, nx, ny, order, i["u"], i["v"])
        for a, name in zip(adv, ("vx", "vy", "unx", "uny")):
            assert_close(host(a), want[name], 1e-13, 1e-14, "frozen %s order %d" % (name, order))
        phi = [dev(i["phi"])]
        scratch = z(2 * phi[0].numel())
        for _ in range(i["nsteps"]):
            ctx.transport_step(order, i["dt"], phi, adv, scratch)
        assert_close(host(phi[0]), want["phi"], 1e-12, 1e-13, "frozen transport order %d" % order)
    # ---- one mEVP sub-iteration
    want = frozen("mevp_single")
    b, u, v, s = cases.inputs_mevp_single()
    nx, ny = b.nx, b.ny
    ctx.set_mevp_params(ctx.mevp_default_params(**b.params))
    ctx.set_grid(nx, ny, b.bt.hx, b.bt.hy)
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(dev(b.H), dev(b.A), pg)
    assert_close(thost(pg, nx), want["pg"], 1e-12, 1e-10, "frozen ice strength")
    cgh, cga, tax, tay = z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1)
    ctx.dg_to_cg(dev(b.H), cgh)
    ctx.dg_to_cg(dev(b.A), cga)
    ctx.wind_stress(dev(b.ua), dev(b.va), tax, tay)
    for g, name in ((cgh, "cgh"), (cga, "cga")):
        assert_close(host(g), want[name], 1e-13, 1e-14, "frozen " + name)
    for g, name in ((tax, "tax"), (tay, "tay")):
        assert_close(host(g), want[name], 1e-13, 1e-16, "frozen " + name)
    packed = z(8 * cgh.numel())
    ctx.mevp_pack_nodal(120.0, (dev(0.9 * u), dev(0.9 * v)), (tax, tay), (dev(b.uo), dev(b.vo)), cgh, cga, packed)
    ds, dso = [tdev(x) for x in s], [torch.zeros_like(tdev(x)) for x in s]
    dun, dvn = z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1)
    ctx.mevp_iterate(0, 0, ny, ds, dso, (dev(u), dev(v)), (dun, dvn), packed, pg)
    for d, name in zip(dso, ("s11", "s12", "s22")):
        assert_close(thost(d, nx), want[name], 1e-12, 1e-12 * np.max(np.abs(want[name])), "frozen " + name)
    assert_close(host(dun), want["u"], 1e-11, 1e-13 * np.max(np.abs(want["u"])), "frozen u_new")
    assert_close(host(dvn), want["v"], 1e-11, 1e-13 * np.max(np.abs(want["v"])), "frozen v_new")
    # ---- the 25-sub-iteration cycle
    want = frozen("mevp_cycle")
    b, nsub = cases.inputs_mevp_cycle()
    nx, ny = b.nx, b.ny
    ctx.set_mevp_params(ctx.mevp_default_params(**b.params))
    ctx.set_grid(nx, ny, b.bt.hx, b.bt.hy)
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(dev(b.H), dev(b.A), pg)
    cgh, cga, tax, tay = z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1)
    ctx.dg_to_cg(dev(b.H), cgh)
    ctx.dg_to_cg(dev(b.A), cga)
    ctx.wind_stress(dev(b.ua), dev(b.va), tax, tay)
    du, dv = z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1)
    ds = [ctx.private_zeros(8, ny, nx, "cuda") for _ in range(3)]
    scratch = z(10 * du.numel() + 3 * ds[0].numel())
    ctx.mevp_subcycle(120.0, nsub, ds, du, dv, z(2 * ny + 1, 2 * nx + 1), z(2 * ny + 1, 2 * nx + 1), tax, tay, dev(b.uo), dev(b.vo), cgh, cga, pg, scratch)
    assert np.max(np.abs(want["u"])) > 1e-4
    assert_close(host(du), want["u"], 1e-9, 1e-11 * np.max(np.abs(want["u"])), "frozen u after the cycle")
    assert_close(host(dv), want["v"], 1e-9, 1e-11 * np.max(np.abs(want["v"])), "frozen v after the cycle")
    for d, name in zip(ds, ("s11", "s12", "s22")):
        assert_close(thost(d, nx), want[name], 1e-9, 1e-10 * np.max(np.abs(want[name])), "frozen %s after the cycle" % name)
    # ---- one coupled step through the driver (column physics + sub-cycle + transport)
    want = frozen("coupled_step")
    c = cases.COUPLED
    ctx.set_mevp_params(ctx.mevp_default_params(alpha=c["alpha"], beta=c["beta"]))
    ctx.set_column_params(ctx.column_default_params())
    core = cases.run_coupled(ctx, torch.device("cuda"), native=(variant >= 2))  # variants 0 / 1: the Python sequence of single sub-iterations
    torch.cuda.synchronize()
    for k in ("H", "A"):
        assert_close(host(getattr(core, k)), want[k], 1e-10, 1e-12, "frozen coupled " + k)
    for k in ("u", "v"):
        assert_close(host(getattr(core, k)), want[k], 1e-9, 1e-11 * np.max(np.abs(want[k])), "frozen coupled " + k)
    for d, name in zip(core.s, ("s11", "s12", "s22")):
        assert_close(thost(d, c["nx"]), want[name], 1e-9, 1e-10 * np.max(np.abs(want[name])), "frozen coupled " + name)
    for k in ("tice0", "hsnow"):
        assert_close(host(core.col[k]), want[k], 1e-10, 1e-12, "frozen coupled " + k)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


@pytest.mark.parametrize("variant", [1, abi.DEFAULT_MEVP_VARIANT])
def test_hip_path_matches_the_independent_restatement(ctx, variant):
    """the HIP path against tests/golden/dyn_independent_v3.npz -- the outputs of the independent dense numpy restatement of
    DESIGN.md section 3 (tests/dyn_independent.py), which the oracle is held to on the CPU: ice strength, nodal means, wind
    stress, ONE mEVP sub-iteration and ONE DG2 transport stage on the 6 x 5 case, through the C ABI.  Not reference parity
    (the snapshot has no dynamics code, /root/reference/CMakeLists.txt:43-46): it removes the common mode of oracle and kernels.
    The one DG2 stage here reaches the default stage kernel on a closed box only; the transport as a whole -- every order, kernel and
    entry point, the open boundary, the march and its closure -- is held to its own restatement in
    tests/test_gpu_transport_independent.py."""
    import dyn_independent as D

    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dyn_independent_v3.npz"))
    c, nx, ny = D.CASE, D.CASE["nx"], D.CASE["ny"]
    I = lambda k: np.ascontiguousarray(fix["in_" + k])
    W = lambda k: fix["out_" + k]
    ctx.set_grid(nx, ny, c["hx"], c["hy"])
    ctx.set_mevp_params(ctx.mevp_default_params(**{k: D.PARAMS[k] for k in D.PARAMS}))
    ctx.set_mevp_variant(variant)
    ctx.set_mevp_strip_rows(0)
    H, A = dev(I("H")), dev(I("A"))
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(H, A, pg)
    assert_close(thost(pg, nx), W("pg"), 1e-12, 1e-13 * np.max(W("pg")), "ice strength")
    cgh, cga = torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda"), torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda")
    ctx.dg_to_cg(H, cgh)
    ctx.dg_to_cg(A, cga)
    assert_close(host(cgh), W("cgh"), 1e-12, 1e-14, "nodal mean of H")
    assert_close(host(cga), W("cga"), 1e-12, 1e-14, "nodal mean of A")
    tax, tay = torch.zeros_like(cgh), torch.zeros_like(cgh)
    ctx.wind_stress(dev(I("ua")), dev(I("va")), tax, tay)
    assert_close(host(tax), W("tax"), 1e-12, 1e-14, "wind stress")
    # one sub-iteration through nsdg_mevp_subcycle (the variant's kernel for a single sub-iteration and the packing)
    u, v = dev(I("u")), dev(I("v"))
    S = [tdev(np.ascontiguousarray(x)) for x in I("S")]
    scratch = torch.zeros(10 * u.numel() + 3 * S[0].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_subcycle(c["dt"], 1, S, u, v, dev(I("u0")), dev(I("v0")), tax, tay, dev(I("uo")), dev(I("vo")), cgh, cga, pg, scratch)
    for k, name in enumerate(("s11", "s12", "s22")):
        assert_close(thost(S[k], nx), W(name), 1e-11, 1e-12 * np.max(np.abs(W(name))), name)
    assert_close(host(u), W("u_new"), 1e-11, 1e-12 * np.max(np.abs(W("u_new"))), "u after one sub-iteration")
    assert_close(host(v), W("v_new"), 1e-11, 1e-12 * np.max(np.abs(W("v_new"))), "v after one sub-iteration")
    # advection velocity and one RK stage of the DG2 transport
    adv = adv_on_device(ctx, nx, ny, 2, I("u"), I("v"))
    for a, name in zip(adv, ("vx_dg", "vy_dg", "un_x", "un_y")):
        assert_close(host(a), W(name), 1e-12, 1e-13 * np.max(np.abs(W(name))), name)
    out = torch.zeros(6, ny, nx, dtype=torch.float64, device="cuda")
    ctx.transport_stage(2, 0, ny, c["dt"], c["rk_a"], c["rk_b"], [dev(I("phi0"))], [dev(I("phi"))], [out], adv)
    assert_close(host(out), W("phi_stage"), 1e-12, 1e-13 * np.max(np.abs(W("phi_stage"))), "DG2 transport stage")
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


@pytest.mark.parametrize("order", [0, 1, 2])
def test_fused_stages_transport_step_equals_staged_step_bitwise(ctx, order):
    """nsdg_transport_step_oop performs all Runge-Kutta stages of a step in ONE launch (a march: a wave owns a window of
    64 - 2 (order + 1) columns and a strip of rows, stage k runs k rows behind the newest row); it must reproduce
    nsdg_transport_step -- one launch per stage -- bit for bit, for grids around the window width, narrower than a window, with
    fewer rows than a strip or than the stages need, for several fields, over several steps"""
    for (nx, ny, nf) in ((70, 37, 1), (33, 17, 2), (5, 3, 1), (128, 64, 3), (31, 50, 4), (58, 9, 1), (59, 2, 1), (60, 1, 2), (61, 4, 1), (62, 5, 1),
                         (63, 7, 1), (64, 8, 1), (117, 1, 1), (1, 1, 1), (1, 40, 1), (2, 3, 2), (300, 260, 1)):
        rng = np.random.default_rng(77 + order)
        nc = basis.NCOEF[order]
        ctx.set_grid(nx, ny, 1.0 / nx, 1.3 / ny)
        u, v = 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1)), 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1))
        adv = adv_on_device(ctx, nx, ny, order, u, v)
        fields = [dev(np.concatenate([1.0 + 0.2 * rng.standard_normal((1, ny, nx)), 0.1 * rng.standard_normal((nc - 1, ny, nx))])) for _ in range(nf)]
        staged = [f.clone() for f in fields]
        a, b = [f.clone() for f in fields], [torch.full_like(f, 7.0) for f in fields]
        scratch = torch.zeros(2 * sum(f.numel() for f in fields), dtype=torch.float64, device="cuda")
        dt = 0.02 / max(nx, ny)
        for step in range(3):
            ctx.transport_step(order, dt, staged, adv, scratch)
            ctx.transport_step_oop(order, dt, a, b, adv)
            a, b = b, a
            for k in range(nf):
                assert torch.equal(a[k], staged[k]), (order, nx, ny, nf, step, k, float((a[k] - staged[k]).abs().max()))
        assert float((staged[0] - fields[0]).abs().max()) > 0
    with pytest.raises(abi.NsdgError, match="alias"):
        ctx.transport_step_oop(order, 1e-3, [a[0]], [a[0]], adv)
    # the fields of a launch run concurrently: a ping-pong with PERMUTED lists (output 0 is input 1), partially overlapping
    # buffers and two identical outputs are refused as well (compared as ranges of nc nx ny doubles)
    x, y = torch.zeros_like(a[0]), torch.zeros_like(a[0])
    with pytest.raises(abi.NsdgError, match="alias"):
        ctx.transport_step_oop(order, 1e-3, [x, y], [y, x], adv)
    with pytest.raises(abi.NsdgError, match="alias"):
        ctx.transport_step_oop(order, 1e-3, [x, y], [a[0], a[0]], adv)
    big = torch.zeros(2 * x.numel(), dtype=torch.float64, device="cuda")
    half = x.numel() // 2
    with pytest.raises(abi.NsdgError, match="alias"):
        ctx.transport_step_oop(order, 1e-3, [big[:x.numel()].view_as(x)], [big[half:half + x.numel()].view_as(x)], adv)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_fused_transport_step_on_a_row_range_equals_the_full_step_there(ctx, order):
    """nsdg_transport_step_oop_rows advances the rows [j0, j1) only, from the rows around them (a row block's own rows and its
    ghost rows): there it must equal the step on the whole array bit for bit, and it must not write any other row"""
    rng = np.random.default_rng(5 + order)
    nc = basis.NCOEF[order]
    for (nx, ny, ranges) in ((70, 41, ((0, 41), (3, 38), (5, 6), (12, 29), (0, 7), (36, 41), (20, 20))), (130, 23, ((4, 19), (3, 4)))):
        ctx.set_grid(nx, ny, 1.0 / nx, 1.3 / ny)
        u, v = 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1)), 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1))
        adv = adv_on_device(ctx, nx, ny, order, u, v)
        fields = [dev(np.concatenate([1.0 + 0.2 * rng.standard_normal((1, ny, nx)), 0.1 * rng.standard_normal((nc - 1, ny, nx))])) for _ in range(2)]
        dt = 0.02 / max(nx, ny)
        full = [torch.zeros_like(f) for f in fields]
        ctx.transport_step_oop(order, dt, fields, full, adv)
        for (j0, j1) in ranges:
            part = [torch.full_like(f, 7.0) for f in fields]
            ctx.transport_step_oop_rows(order, j0, j1, dt, fields, part, adv)
            for k in range(2):
                assert torch.equal(part[k][:, j0:j1], full[k][:, j0:j1]), (order, nx, ny, j0, j1, k)
                assert bool((part[k][:, :j0] == 7.0).all()) and bool((part[k][:, j1:] == 7.0).all()), (order, nx, ny, j0, j1, k)
    with pytest.raises(abi.NsdgError, match="row range"):
        ctx.transport_step_oop_rows(order, 3, ny + 1, dt, fields, full, adv)

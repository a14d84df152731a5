"""The momentum budget on the device (include/nsdg_budget.h): nsdg_momentum_budget against its numpy restatement
(tests/budget_ref.py) in five settings at four shapes, the identities that hold the residual to the existing velocity kernel and the terms
to each other, the invariances (land and Dirichlet nodes, NaN forcing on land, canaries behind the planes nobody asked for), and the
row totals in the header's order of summation.

The shapes (nx, ny) are (3, 2), (64, 4), (65, 5) and (129, 9): one partial wave, the exact 64 x 4 tile, one element past it in both
directions, and three trips of the lane stride.

Tolerance per value: 1e-12 * (sum over the eight terms of |F_x| + |F_y| at that node), plus 1e-12 * the plane's maximum -- the project's own
bound for mEVP operators (header of tests/test_gpu_parity.py: ~1e-13) with a margin of 10 for the eight-term sum.  Every figure is printed
before it is asserted."""
import numpy as np
import pytest
import torch

import budget_ref as BU
import land_ref
import mevp_ref as MR
from nextsimdg_amd import abi
from test_gpu_land import AD, UNIFORM, mask_dev
from test_gpu_parity import Box, dev, host, tdev

pytestmark = pytest.mark.gpu
SHAPES = [(3, 2), (64, 4), (65, 5), (129, 9)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]
SETTINGS = ("plain", "land", "depth", "snow", "ssh", "all")
EPS = 2.0 ** -53
G = 9.81
DT = 120.0
CANARY = -3.0


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
        ctx.set_tilt(None)
    ctx.set_block(0, 0)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


def budget_mask(nx, ny):
    """an island, a one-element rock and a coast at the tile seam (element columns 63 | 64) where the array reaches it"""
    land = np.zeros((ny, nx), dtype=bool)
    if nx < 16:
        land[ny - 1, 1] = True  # the rock
        return land
    land[1:3, 10:13] = True  # the island
    land[ny - 1, 20] = True  # the rock
    land[0:2, 63:min(65, nx)] = True  # the coast at the seam
    return land


def height(nx, ny, land=None, seed=3):
    """a height with curvature and node-to-node noise, NaN at the nodes no ocean element touches"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(2 * nx + 1.0), np.arange(2 * ny + 1.0))
    eta = 0.3 * np.sin(0.11 * gx + 0.07 * gy) + 0.02 * gx + 0.01 * rng.standard_normal(gx.shape)
    if land is not None:
        eta[~land_ref.land_nodes(~land)] = np.nan
    return eta


class State:
    """a Box with open water in it, a random velocity and stress, and the setting's fields on the context; packed by nsdg_mevp_prepare"""

    def __init__(self, ctx, nx, ny, setting, pk=UNIFORM, nan_on_land=False, seed=11, ocean=True):
        self.b = b = Box(ctx, nx, ny, **pk)
        self.nx, self.ny, self.shape = nx, ny, (2 * ny + 1, 2 * nx + 1)
        self.hx, self.hy = b.bt.hx, b.bt.hy
        rng = np.random.default_rng(seed)
        if nx >= 32:
            b.H[:, :, 5:9] = 0.0  # open water: ice-free nodes
            b.A[:, :, 5:9] = 0.0
        self.land = budget_mask(nx, ny) if setting in ("land", "all") else None
        ln = land_ref.land_nodes(self.land) if self.land is not None else np.zeros(self.shape, dtype=bool)
        if self.land is not None:
            b.H[:, self.land] = 0.0
            b.A[:, self.land] = 0.0
        edge = np.zeros(self.shape, dtype=bool)
        edge[0] = edge[-1] = edge[:, 0] = edge[:, -1] = True
        rest = ln | edge
        self.u, self.v = (np.where(rest, 0.0, 0.05 * rng.standard_normal(self.shape)) for _ in range(2))
        self.u0, self.v0 = (np.where(rest, 0.0, 0.05 * rng.standard_normal(self.shape)) for _ in range(2))
        self.S = [2e3 * rng.standard_normal((8, ny, nx)) for _ in range(3)]
        self.ua, self.va = b.ua.copy(), b.va.copy()
        self.uo, self.vo = (b.uo.copy(), b.vo.copy()) if ocean else (np.zeros(self.shape), np.zeros(self.shape))
        self.eta = height(nx, ny, self.land) if setting in ("ssh", "all") else None
        if nan_on_land:
            inside = ~land_ref.land_nodes(~self.land)  # no ocean element touches the node
            assert inside.any()
            for f in (self.ua, self.va, self.uo, self.vo):
                f[ln] = np.nan
        self.depth = rng.uniform(0.05, 3.0, (ny, nx)) if setting in ("depth", "all") else None
        self.snow = 0.4 * rng.random((ny, nx)) if setting in ("snow", "all") else None
        self.ln = ln
        self.d = d = {k: dev(getattr(self, k)) for k in ("u", "v", "u0", "v0", "ua", "va", "uo", "vo")}
        d.update(H=dev(b.H), A=dev(b.A), s=[tdev(x) for x in self.S])
        n = self.shape[0] * self.shape[1]
        d["packed"] = torch.full((8 * n,), CANARY, dtype=torch.float64, device="cuda")
        self.keep = [mask_dev(self.land) if self.land is not None else None, dev(self.depth) if self.depth is not None else None,
                     dev(self.snow) if self.snow is not None else None, dev(self.eta) if self.eta is not None else None]
        self.apply(ctx)

    def apply(self, ctx):
        d = self.d
        ctx.set_land_mask(self.keep[0])
        ctx.set_basal_depth(self.keep[1])
        ctx.set_snow_load(self.keep[2])
        ctx.set_tilt(self.keep[3], G)
        ctx.mevp_prepare(DT, d["H"], d["A"], (d["ua"], d["va"]), (d["uo"], d["vo"]), (d["u0"], d["v0"]), d["packed"])
        torch.cuda.synchronize()

    def budget(self, ctx, names=BU.PLANES, power=True, j0=0, j1=None, row0=0):
        """the launch: ({plane: host array}, power [9, rows] or None, the device tensors)"""
        d = self.d
        j1 = self.ny if j1 is None else j1
        planes = {k: torch.full(self.shape, CANARY, dtype=torch.float64, device="cuda") for k in names}
        pw = torch.full((9, j1 - row0), CANARY, dtype=torch.float64, device="cuda") if power else None
        ctx.momentum_budget(j0, j1, d["H"], d["A"], (d["ua"], d["va"]), d["s"], (d["u"], d["v"]), d["packed"], planes, pw, row0)
        torch.cuda.synchronize()
        return {k: host(t) for k, t in planes.items()}, (host(pw) if power else None), planes

    def reference(self, ctx):
        c, tb = BU.unpack(host(self.d["packed"]), self.shape)
        return BU.forces(self.b.po, DT, self.hx, self.hy, c, self.b.A, self.ua, self.va, self.S, self.u, self.v,
                         tb=tb if self.depth is not None else None, u0=abi.basal_default_params().u0, eta=self.eta, g=G)


def check_planes(what, got, want, factor=1e-12):
    """|got - want| <= factor * (sum of |terms| at the node + the plane's maximum); prints the worst case in units of the bound"""
    scale = BU.scale(want)
    worst = 0.0
    for k in BU.PLANES:
        lim = factor * (scale + np.max(np.abs(want[k])))
        err = np.abs(got[k] - want[k])
        assert np.isfinite(got[k]).all(), k
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(lim > 0.0, err / lim, np.where(err > 0.0, np.inf, 0.0))
        worst = max(worst, float(r.max()))
        assert np.all(err <= lim), "%s %s: %.3g of its bound" % (what, k, float(r.max()))
    print("%s: largest |device - restatement| = %.3g of 1e-12 (sum|terms| + max|plane|)" % (what, worst * factor / 1e-12))
    return worst


# ------------------------------------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_planes_and_totals_against_the_restatement(ctx, shape, setting):
    st = State(ctx, *shape, setting)
    got, power, _ = st.budget(ctx)
    want = st.reference(ctx)
    check_planes("%dx%d %s" % (shape + (setting,)), got, want)
    # every term that the setting has is felt, and the ones it has not are exactly 0
    live = ~want["fixed"]
    for t in BU.TERMS:
        big = max(np.abs(got[t + "_x"][live]).max(), np.abs(got[t + "_y"][live]).max())
        if t == "basal" and st.depth is None:
            assert big == 0.0
        else:
            assert big > 1e-6, t
    # land and Dirichlet nodes are exactly 0
    for k in BU.PLANES:
        assert np.all(got[k][want["fixed"]] == 0.0), k
    if st.land is not None:
        assert st.ln.sum() >= 9
    # the row totals: in the header's order of summation from the device's own planes, bit for bit; and against the restatement's
    # forces within the bound the planes' bound implies: sum_n M_n (|u| + |v|) 1e-12 (sum|terms| + max|plane|), plus the summation's
    # own (4 nx + 6) eps sum|p|, which that bound covers a hundred times
    F_dev = dict(got, m=want["m"], fixed=want["fixed"])
    mine = BU.row_totals(F_dev, st.u, st.v, st.hx, st.hy, 0, st.ny)
    assert np.array_equal(power, mine), np.argwhere(power != mine)[:4]
    ref = BU.row_totals(want, st.u, st.v, st.hx, st.hy, 0, st.ny)
    area = st.hx * st.hy
    scale = BU.scale(want)
    for q, t in enumerate(BU.TERMS):
        fmax = max(np.abs(want[t + "_x"]).max(), np.abs(want[t + "_y"]).max())
        node = area * (np.abs(st.u) + np.abs(st.v)) * 1e-12 * (scale + fmax)  # M_n <= hx hy / 2.25
        lim = np.array([node[2 * iy:2 * iy + 2].sum() for iy in range(st.ny)])
        assert np.all(np.abs(power[q] - ref[q]) <= lim), t
    assert np.array_equal(power[BU.KE], ref[BU.KE])  # products and sums only: the restatement IS the arithmetic
    assert power[BU.KE].min() > 0.0


@pytest.mark.parametrize("setting", ["plain", "all"])
def test_uniform_and_adaptive_parameters_give_identical_planes(ctx, setting):
    """the balance does not see alpha, beta: the planes under the adaptive form's parameters are those under the uniform form's"""
    runs = []
    for pk in (UNIFORM, AD, dict(alpha=7.0, beta=11.0)):
        st = State(ctx, 65, 5, setting, pk=pk)
        got, power, _ = st.budget(ctx)
        runs.append((got, power))
    for got, power in runs[1:]:
        for k in BU.PLANES:
            assert np.array_equal(got[k], runs[0][0][k]), k
        assert np.array_equal(power, runs[0][1])


# ------------------------------------------------------------------------------------------------ 2. identities on the device
@pytest.mark.parametrize("setting", ["plain", "land", "depth", "all"])
@pytest.mark.parametrize("shape", [(65, 5), (129, 9)], ids=["65x5", "129x9"])
def test_residual_against_one_more_velocity_update(ctx, shape, setting):
    """(a) under uniform alpha = beta, u' = nsdg_mevp_velocity(S, u): R = (K2 h' + drag [+ C_b]) (u' - u) at every non-Dirichlet node within
    64 eps sum|terms|.  beta = 1: the identity holds for any beta, but the rounding of u' is that of its largest term K1 h' u = beta mdt u,
    and what the bound is relative to -- the terms of the balance -- does not grow with beta; with beta = 1 that term is one of them"""
    pk = dict(alpha=1.0, beta=1.0)
    st = State(ctx, *shape, setting, pk=pk)
    ctx.set_mevp_variant(0)
    got, _, _ = st.budget(ctx, power=False)
    d = st.d
    un, vn = torch.full_like(d["u"], CANARY), torch.full_like(d["v"], CANARY)
    ctx.mevp_velocity(0, st.ny, d["s"], (d["u"], d["v"]), (un, vn), d["packed"])
    torch.cuda.synchronize()
    un, vn = host(un), host(vn)
    c, tb = BU.unpack(host(d["packed"]), st.shape)
    s = np.where(c[0] > 2.0 ** 50, 2.0 ** -100, 1.0)
    hp, cd = s * c[0], s * c[1]
    po = st.b.po
    k2 = po.rho_ice * (1.0 + po.beta) / DT
    drag = cd * np.sqrt((c[4] - st.u) ** 2 + (c[5] - st.v) ** 2)
    cb = tb / (np.sqrt(st.u ** 2 + st.v ** 2) + abi.basal_default_params().u0) if st.depth is not None else 0.0
    den = k2 * hp + drag + cb
    scale = BU.scale(got)
    fixed = BU.fixed_nodes(c)
    worst = 0.0
    for k, (new, old) in (("residual_x", (un, st.u)), ("residual_y", (vn, st.v))):
        want = den * (new - old)
        err = np.abs(got[k] - want)[~fixed]
        lim = 64 * EPS * scale[~fixed]
        worst = max(worst, float(np.max(err / lim)))
        assert np.all(err <= lim), "%s: %.3g of 64 eps sum|terms|" % (k, float(np.max(err / lim)))
        assert np.abs(got[k][~fixed]).max() > 1e-3
        assert np.all(got[k][fixed] == 0.0) and np.all(new[fixed] == 0.0)
    print("residual against one more update %dx%d %s: worst %.3g of 64 eps sum|terms|" % (shape + (setting, worst)))


@pytest.mark.parametrize("setting", ["plain", "all"])
def test_residual_against_one_more_velocity_update_at_the_production_beta(ctx, setting):
    """(a) where users run, alpha = beta = 300: u' is a rounded sum whose largest term is K1 h' u = beta mdt u, so its rounding -- and that of
    (K2 h' + drag + C_b) (u' - u) -- is relative to that term too: the same 64 eps, of sum|terms| + K1 h' (|u| + |v|)"""
    st = State(ctx, 129, 9, setting, pk=UNIFORM)
    ctx.set_mevp_variant(0)
    got, _, _ = st.budget(ctx, power=False)
    d = st.d
    un, vn = torch.full_like(d["u"], CANARY), torch.full_like(d["v"], CANARY)
    ctx.mevp_velocity(0, st.ny, d["s"], (d["u"], d["v"]), (un, vn), d["packed"])
    torch.cuda.synchronize()
    c, tb = BU.unpack(host(d["packed"]), st.shape)
    s = np.where(c[0] > 2.0 ** 50, 2.0 ** -100, 1.0)
    hp, cd = s * c[0], s * c[1]
    po = st.b.po
    k1, k2 = po.rho_ice * po.beta / DT, po.rho_ice * (1.0 + po.beta) / DT
    drag = cd * np.sqrt((c[4] - st.u) ** 2 + (c[5] - st.v) ** 2)
    cb = tb / (np.sqrt(st.u ** 2 + st.v ** 2) + abi.basal_default_params().u0) if st.depth is not None else 0.0
    live = ~BU.fixed_nodes(c)
    lim = 64 * EPS * (BU.scale(got) + k1 * hp * (np.abs(st.u) + np.abs(st.v)))
    assert po.beta == 300.0
    for k, new, old in (("residual_x", host(un), st.u), ("residual_y", host(vn), st.v)):
        err = np.abs(got[k] - (k2 * hp + drag + cb) * (new - old))
        print("residual against one more update, beta = 300, %s %s: worst %.3g of 64 eps (sum|terms| + K1 h' |u|)" % (setting, k, float(np.max(err[live] / lim[live]))))
        assert np.all(err[live] <= lim[live]), k


@pytest.mark.parametrize("setting", SETTINGS)
def test_sum_of_the_seven_terms_is_the_residual(ctx, setting):
    """(b) within 16 eps sum|terms|"""
    st = State(ctx, 129, 9, setting)
    got, _, _ = st.budget(ctx, power=False)
    scale = BU.scale(got)
    for c in "xy":
        total = sum(got[t + "_" + c] for t in BU.TERMS[:-1])
        err = np.abs(total - got["residual_" + c])
        print("sum of terms %s %s: worst %.3g of 16 eps sum|terms|" % (setting, c, float(np.max(err[scale > 0] / (16 * EPS * scale[scale > 0])))))
        assert np.all(err <= 16 * EPS * scale)


def drift_solution(p, h, a, tax, tay, uo, vo, tilt):
    """0 = a tau + a C_w rho_w |u_o - u| (u_o - u) + m f_c k x ... + tilt: the steady free drift, solved by scipy and polished by Newton steps"""
    from scipy.optimize import fsolve

    m, cd = p.rho_ice * h, a * p.c_ocean * p.rho_ocean

    def balance(w):
        sp = np.hypot(uo - w[0], vo - w[1])
        return np.array([a * tax + cd * sp * (uo - w[0]) + m * p.fc * w[1] + tilt[0], a * tay + cd * sp * (vo - w[1]) - m * p.fc * w[0] + tilt[1]])

    sol = fsolve(balance, [0.05, -0.05], xtol=1e-13)
    for _ in range(3):  # Newton with a central-difference Jacobian: the residual at the rounding level of its terms
        J = np.array([(balance(sol + e) - balance(sol - e)) / 2e-7 for e in (np.array([1e-7, 0.0]), np.array([0.0, 1e-7]))]).T
        sol = sol - np.linalg.solve(J, balance(sol))
    return sol


@pytest.mark.parametrize("slope", [False, True], ids=["geostrophic", "slope"])
def test_steady_free_drift_has_no_inertia_and_no_residual(ctx, slope):
    """(c) a strengthless cover (S = 0), uniform forcing, u = u^n = the steady free drift that scipy solves: inertia and residual vanish
    within 1e-12 sum|terms| (neither is an exact 0: c2 is a rounded sum); with a linear eta the tilt is -rho_i h' g slope"""
    nx, ny = 65, 5
    h, a = 0.7, 0.85
    pk = dict(pstar=0.0, alpha=5.0, beta=5.0)
    b = Box(ctx, nx, ny, **pk)
    po, hx, hy = b.po, b.bt.hx, b.bt.hy
    shape = (2 * ny + 1, 2 * nx + 1)
    ua, va, uo, vo = 7.0, -3.0, 0.04, 0.02
    tax, tay = (po.c_atm * po.rho_atm) * np.hypot(ua, va) * ua, (po.c_atm * po.rho_atm) * np.hypot(ua, va) * va
    m = po.rho_ice * h
    sx, sy = 2e-5, -1e-5
    tilt = (-m * G * sx, -m * G * sy) if slope else (-m * po.fc * vo, m * po.fc * uo)
    w = drift_solution(po, h, a, tax, tay, uo, vo, tilt)
    assert np.hypot(*w) > 0.05
    H, A = np.zeros((6, ny, nx)), np.zeros((6, ny, nx))
    H[0], A[0] = h, a
    full = lambda x: dev(np.full(shape, x))
    u, v = full(w[0]), full(w[1])
    eta = None
    if slope:
        gx, gy = np.meshgrid(np.arange(2 * nx + 1.0), np.arange(2 * ny + 1.0))
        eta = dev(sx * (0.5 * hx) * gx + sy * (0.5 * hy) * gy)
    ctx.set_tilt(eta, G)
    packed = torch.zeros(8 * u.numel(), dtype=torch.float64, device="cuda")
    dH, dA, wind, ocean = dev(H), dev(A), (full(ua), full(va)), (full(uo), full(vo))
    ctx.mevp_prepare(DT, dH, dA, wind, ocean, (u, v), packed)
    s = [tdev(np.zeros((8, ny, nx))) for _ in range(3)]
    planes = {k: torch.zeros(shape, dtype=torch.float64, device="cuda") for k in BU.PLANES}
    ctx.momentum_budget(0, ny, dH, dA, wind, s, (u, v), packed, planes)
    torch.cuda.synchronize()
    got = {k: host(t) for k, t in planes.items()}
    scale = BU.scale(got)
    inner = np.zeros(shape, dtype=bool)
    inner[1:-1, 1:-1] = True
    assert scale[inner].min() > 0.1 and np.all(scale[~inner] == 0.0)
    for k in ("inertia_x", "inertia_y", "residual_x", "residual_y"):
        r = float(np.max(np.abs(got[k][inner]) / scale[inner]))
        print("steady free drift (%s) %s: %.3g sum|terms|" % ("slope" if slope else "geostrophic", k, r))
        assert r <= 1e-12, k
    assert np.all(got["internal_x"] == 0.0) and np.all(got["basal_y"] == 0.0)
    if slope:
        for k, want in (("tilt_x", tilt[0]), ("tilt_y", tilt[1])):
            assert np.max(np.abs(got[k][inner] - want)) <= 8 * EPS * abs(want) + 4 * EPS * m * G * np.max(np.abs(host(eta))) / min(hx, hy), k


def test_power_of_the_internal_stress_is_minus_the_deformation_work(ctx):
    """(d) integration by parts: the domain total of power[internal] equals -sum_e int sigma : eps_dot, the integral in numpy from S and the
    strain rate of u at the scheme's 3 x 3 Gauss points (exact for the integrand: degree 4 per direction); random S, u zero on the
    Dirichlet nodes, ice at every node.  Tolerance 1e-12 sum_e int |sigma : eps_dot|"""
    nx, ny = 129, 9
    b = Box(ctx, nx, ny, **UNIFORM)
    b.H[0] += 1.0  # no ice-free node
    rng = np.random.default_rng(21)
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = 0.05 * rng.standard_normal(shape), 0.05 * rng.standard_normal(shape)
    for f in (u, v):
        f[0] = f[-1] = 0.0
        f[:, 0] = f[:, -1] = 0.0
    S = [2e3 * rng.standard_normal((8, ny, nx)) for _ in range(3)]
    du, dv, dH, dA = dev(u), dev(v), dev(b.H), dev(b.A)
    wind, ocean = (dev(b.ua), dev(b.va)), (dev(b.uo), dev(b.vo))
    packed = torch.zeros(8 * du.numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_prepare(DT, dH, dA, wind, ocean, (du, dv), packed)
    power = torch.zeros(9, ny, dtype=torch.float64, device="cuda")
    ctx.momentum_budget(0, ny, dH, dA, wind, [tdev(x) for x in S], (du, dv), packed, None, power)
    torch.cuda.synchronize()
    c, _ = BU.unpack(host(packed), shape)
    assert c[0].max() < 2.0 ** 50
    ul, vl = MR.local_nodal(u, 0, ny), MR.local_nodal(v, 0, ny)
    hx, hy = b.bt.hx, b.bt.hy
    e11, e22 = MR.apply(MR.PHIX_Q, ul) / hx, MR.apply(MR.PHIY_Q, vl) / hy
    e12 = 0.5 * (MR.apply(MR.PHIY_Q, ul) / hy + MR.apply(MR.PHIX_Q, vl) / hx)
    s11, s12, s22 = (MR.apply(MR.PSI_Q, x) for x in S)
    wq = MR._W3[:, None, None] * (hx * hy)
    work = float(np.sum(wq * (s11 * e11 + 2.0 * s12 * e12 + s22 * e22)))
    size = float(np.sum(wq * (np.abs(s11 * e11) + 2.0 * np.abs(s12 * e12) + np.abs(s22 * e22))))
    total = 0.0
    for p in host(power)[BU.TERMS.index("internal")]:  # rows added in row order
        total = total + p
    print("integration by parts: power %.17g, -work %.17g, difference %.3g of 1e-12 sum int|sigma:eps|" % (total, -work, abs(total + work) / (1e-12 * size)))
    assert abs(work) > 1e-3 * size
    assert abs(total + work) <= 1e-12 * size


def test_water_drag_opposes_the_motion_over_an_ocean_at_rest(ctx):
    """(e) u . water <= 0 at every node"""
    st = State(ctx, 65, 5, "land", ocean=False)
    got, power, _ = st.budget(ctx, names=("water_x", "water_y"))
    dot = st.u * got["water_x"] + st.v * got["water_y"]
    assert np.all(dot <= 0.0) and dot.min() < -1e-6
    assert np.all(power[BU.TERMS.index("water")] < 0.0)


def test_residual_falls_with_the_sub_iterations(ctx):
    """(f) the box test at 16 x 16: max|R| after 480 sub-iterations is smaller than after 30, and the device's ratio agrees with the ratio
    of the restatement, evaluated at the device's two states, to 1e-9 relative.  The ratio itself is printed, not asserted"""
    nx = ny = 16
    b = Box(ctx, nx, ny)
    shape = (2 * ny + 1, 2 * nx + 1)
    dH, dA = dev(b.H), dev(b.A)
    wind, ocean = (dev(b.ua), dev(b.va)), (dev(b.uo), dev(b.vo))
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    ctx.ice_strength(dH, dA, pg)
    u = [torch.zeros(shape, dtype=torch.float64, device="cuda") for _ in range(4)]
    s = [[tdev(np.zeros((8, ny, nx))) for _ in range(3)] for _ in range(2)]
    packed = torch.zeros(8 * u[0].numel(), dtype=torch.float64, device="cuda")
    ctx.mevp_prepare(DT, dH, dA, wind, ocean, (u[0], u[1]), packed)
    calls = [ctx.bind_mevp_iterate(0, 0, ny, s[k], s[1 - k], (u[2 * k], u[2 * k + 1]), (u[2 - 2 * k], u[3 - 2 * k]), packed, pg) for k in range(2)]
    c, _ = BU.unpack(host(packed), shape)
    rmax, rref = [], []
    done = 0
    for nsub in (30, 480):
        while done < nsub:
            calls[done % 2]()
            done += 1
        k = done % 2  # the buffers the last call wrote
        planes = {key: torch.zeros(shape, dtype=torch.float64, device="cuda") for key in ("residual_x", "residual_y")}
        ctx.momentum_budget(0, ny, dH, dA, wind, s[k], (u[2 * k], u[2 * k + 1]), packed, planes)
        torch.cuda.synchronize()
        rmax.append(max(float(planes[key].abs().max()) for key in planes))
        S = [abi.untile(x, nx).cpu().numpy() for x in s[k]]
        F = BU.forces(b.po, DT, b.bt.hx, b.bt.hy, c, b.A, b.ua, b.va, S, host(u[2 * k]), host(u[2 * k + 1]))
        rref.append(max(np.abs(F["residual_x"]).max(), np.abs(F["residual_y"]).max()))
    print("box test 16 x 16: max|R| = %.6e after 30, %.6e after 480 sub-iterations: ratio %.6e (restatement %.6e)" % (
        rmax[0], rmax[1], rmax[1] / rmax[0], rref[1] / rref[0]))
    assert rmax[1] < rmax[0]
    assert abs(rmax[1] / rmax[0] - rref[1] / rref[0]) <= 1e-9 * (rref[1] / rref[0])


# ------------------------------------------------------------------------------------------------ 3. invariance
def test_nan_forcing_on_land_reaches_no_ocean_value(ctx):
    """NaN wind, current and eta on land: every value is finite and equals the finite-forcing run bit for bit"""
    runs = []
    for nan in (False, True):
        st = State(ctx, 129, 9, "all", nan_on_land=nan)
        assert np.isnan(st.eta).any() and (np.isnan(st.ua).any() == nan)
        got, power, _ = st.budget(ctx)
        assert all(np.isfinite(x).all() for x in got.values()) and np.isfinite(power).all()
        runs.append((got, power))
    for k in BU.PLANES:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("names", [("residual_x",), ("wind_y", "internal_x", "residual_y"), ()], ids=["one", "three", "totals-only"])
def test_only_the_planes_asked_for_are_written(ctx, names):
    """one allocation holds canary | plane | canary | ... : the planes asked for lie between canaries that stay, the values equal the
    launch that asks for all sixteen, and so do the totals"""
    st = State(ctx, 65, 5, "all")
    full, power_full, _ = st.budget(ctx)
    n = st.shape[0] * st.shape[1]
    pad = 64
    slab = torch.full(((len(names) + 1) * (n + pad),), CANARY, dtype=torch.float64, device="cuda")
    planes = {k: slab[pad + i * (n + pad): pad + i * (n + pad) + n] for i, k in enumerate(names)}
    pw = torch.full((9, st.ny + 2), CANARY, dtype=torch.float64, device="cuda")
    d = st.d
    ctx.momentum_budget(0, st.ny, d["H"], d["A"], (d["ua"], d["va"]), d["s"], (d["u"], d["v"]), d["packed"], planes, pw, -1)
    torch.cuda.synchronize()
    for i, k in enumerate(names):
        assert np.array_equal(host(planes[k]).reshape(st.shape), full[k]), k
        assert bool((slab[i * (n + pad): i * (n + pad) + pad] == CANARY).all())
    assert bool((slab[len(names) * (n + pad):] == CANARY).all())
    assert np.array_equal(host(pw[:, 1:-1]), power_full) and bool((pw[:, 0] == CANARY).all()) and bool((pw[:, -1] == CANARY).all())


def test_a_row_range_writes_its_own_nodes_and_totals_only(ctx):
    """rows [2, 6) of 9 write the node rows 4 .. 11 and the totals of their rows: what the whole range writes there, bit for bit; with and
    without totals (the two launch geometries) the planes are the same"""
    st = State(ctx, 129, 9, "all")
    full, power_full, _ = st.budget(ctx)
    part, power, _ = st.budget(ctx, j0=2, j1=6, row0=2)
    tiles, _, _ = st.budget(ctx, j0=2, j1=6, power=False)
    for k in BU.PLANES:
        assert np.array_equal(part[k][4:12], full[k][4:12]) and np.all(part[k][:4] == CANARY) and np.all(part[k][12:] == CANARY), k
        assert np.array_equal(tiles[k], part[k]), k
    assert np.array_equal(power, power_full[:, 2:6])

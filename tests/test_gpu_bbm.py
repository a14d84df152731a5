"""The brittle Bingham-Maxwell sub-cycle on the device (csrc/bbm.hip) against the independent numpy restatement
(tests/bbm_ref.py), against itself bit for bit (strips, split launches, an all-ocean mask, row blocks, checkpoint) and against the
literature with no reference in between (envelope, Hooke's law, free drift).  Shapes: nx = 70 is two column-waves with a seam and an odd
tile remainder, ny = 9 with strip_rows 3 is three strips with prologue rows, 2 x 2 is the smallest array."""
import math
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bbm_ref as R  # noqa: E402
from bbm_cases import dg2, random_case, reference  # noqa: E402,F401 -- the inputs and their reference, shared with the CPU conditions
from nextsimdg_amd import abi, rowblock  # noqa: E402

pytestmark = pytest.mark.gpu
HX = HY = 1000.0
DTS = 1.0


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # a field already on the device stays there


def tdev(a):
    return abi.tile(dev(a))


def thost(t, nx):
    return abi.untile(t, nx).cpu().numpy()


def host(t):
    return t.cpu().numpy()


def assert_close(got, want, rtol, atol, what):
    err, lim = np.abs(got - want), atol + rtol * np.abs(want)
    print("%-8s max err %.3e, max |want| %.3e, worst err / limit %.3f" % (what, err.max(), np.abs(want).max(), (err / lim).max()))
    assert np.all(err <= lim), "%s: %d of %d entries differ, worst err / limit %.3g" % (what, (err > lim).sum(), err.size, (err / lim).max())


def assert_branch_margins(diag, first=True):
    """the reference stays clear of the scheme's two discontinuities (Pt at sigma_n = 0, d_c at sigma_n = -N), no Gauss point excluded"""
    N = R.bbm_par()["compr_strength"]
    assert np.min(np.abs(diag["sn_old"])) >= 1e3 and np.min(diag["sn_new"]) > -0.5 * N
    assert diag["emax"] <= 1e-6
    if first:
        share = float(np.mean(diag["failing"]))
        print("failing share %.3f, dt_s / t_d in [%.4f, %.4f]" % (share, diag["r"].min(), diag["r"].max()))
        assert 0.1 <= share <= 0.9 and diag["r"].max() < 1.0


class Device:
    """the device arrays of a case and one sub-iteration on them through the C ABI"""

    def __init__(self, ctx, c, bp=None, dts=DTS, hx=HX, hy=HY, land_mask=None, mp=None):
        nx, ny = c["nx"], c["ny"]
        self.ctx, self.nx, self.ny = ctx, nx, ny
        ctx.set_mevp_params(mp or ctx.mevp_default_params())
        ctx.set_bbm_params(bp or ctx.bbm_default_params())
        ctx.set_grid(nx, ny, hx, hy)
        self.mask = None if land_mask is None else torch.from_numpy(np.ascontiguousarray(land_mask).astype(np.uint8)).cuda()
        ctx.set_land_mask(self.mask)
        self.H, self.A, self.D = dev(c["H"]), dev(c["A"]), dev(c["D"])
        self.S = [tdev(x) for x in c["S"]]
        self.u, self.v = dev(c["u"]), dev(c["v"])
        self.gauss = [ctx.private_zeros(9, ny, nx, "cuda") for _ in range(3)]
        ctx.bbm_prepare(self.H, self.A, *self.gauss)
        self.packed = torch.zeros(8 * self.u.numel(), dtype=torch.float64, device="cuda")
        zero = torch.zeros_like(self.u)
        ctx.mevp_prepare(dts, self.H, self.A, (dev(c["ua"]), dev(c["va"])), (dev(c["uo"]), dev(c["vo"])), (zero, zero), self.packed)

    def iterate(self, ranges=None, strip_rows=0):
        ctx = self.ctx
        ctx.set_mevp_strip_rows(strip_rows)
        So, Do = [torch.zeros_like(x) for x in self.S], torch.zeros_like(self.D)
        un, vn = torch.full_like(self.u, 3.0), torch.full_like(self.v, 3.0)
        for (k0, j0, j1) in ranges or [(0, 0, self.ny)]:
            ctx.bbm_iterate(k0, j0, j1, self.S, So, self.D, Do, (self.u, self.v), (un, vn), self.packed, self.gauss)
        ctx.set_mevp_strip_rows(0)
        torch.cuda.synchronize()
        return dict(St=So, Dt=Do, ut=un, vt=vn, S=[thost(x, self.nx) for x in So], D=host(Do), u=host(un), v=host(vn))

    def close(self):
        self.ctx.set_land_mask(None)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a["St"] + [a["Dt"], a["ut"], a["vt"]], b["St"] + [b["Dt"], b["ut"], b["vt"]]))


@pytest.fixture(scope="module")
def case70():
    c = random_case(70, 9)
    return c, reference(c)


# ---- 1. prepare -------------------------------------------------------------------------------------------------------------------------
def test_prepare_matches_the_reference(ctx, case70):
    """hg, eg, pm at 1e-12 relative (the tolerance of nsdg_ice_strength in test_gpu_parity.py, whose absolute floor 1e-10 belongs to a
    strength of ~8e3: 1.25e-14 of the largest value here); a clamped thickness and concentration are part of the case"""
    c, _ = case70
    c = dict(c, H=c["H"].copy(), A=c["A"].copy())
    c["H"][0, 2, 5:9], c["A"][0, 3, 40:50], c["A"][0, 4, 10] = -0.1, 1.3, -0.2
    want = R.prepare(R.mevp_par(), R.bbm_par(), c["H"], c["A"])
    d = Device(ctx, c)
    for got, w, name in zip(d.gauss, want, ("hg", "eg", "pm")):
        assert_close(thost(got, 70), w, 1e-12, 1.25e-14 * np.max(np.abs(w)), name)
    assert np.any(want[0] == 0.0) and np.any(want[1] == 1.0)


# ---- 2. one sub-iteration against the reference -----------------------------------------------------------------------------------------
def check_against_reference(got, ref):
    for g, w, name in zip(got["S"], ref["S"], ("s11", "s12", "s22")):
        assert_close(g, w, 1e-11, 1e-13 * np.max(np.abs(w)), name)
    for k in ("D", "u", "v"):
        assert_close(got[k], ref[k], 1e-11, 1e-13 * np.max(np.abs(ref[k])), k)


def test_one_sub_iteration_matches_the_reference_70x9(ctx, case70):
    c, ref = case70
    assert_branch_margins(ref["diag"])
    assert np.max(np.abs(ref["u"])) > 1e-5
    check_against_reference(Device(ctx, c).iterate(), ref)


def test_one_sub_iteration_matches_the_reference_2x2(ctx):
    """the smallest array: one interior node; the shares of failing points are those of 36 Gauss points, so only the margins are asked"""
    c = random_case(2, 2, seed=4)
    ref = reference(c)
    assert_branch_margins(ref["diag"], first=False)
    check_against_reference(Device(ctx, c).iterate(), ref)


# ---- 3. bitwise ---------------------------------------------------------------------------------------------------------------------------
def test_strips_split_launches_and_an_ocean_mask_do_not_change_a_bit(ctx, case70):
    c, _ = case70
    d = Device(ctx, c)
    base = d.iterate()
    for r in (3, 64):
        assert same(d.iterate(strip_rows=r), base), "strip_rows %d" % r
    for r in (0, 3):
        assert same(d.iterate(ranges=[(0, 0, 4), (3, 4, 9)], strip_rows=r), base), "two launches, strip_rows %d" % r
    m = Device(ctx, c, land_mask=np.zeros((9, 70), dtype=bool))
    assert same(m.iterate(), base) and same(m.iterate(strip_rows=3), base)
    m.close()


# ---- 4. land ------------------------------------------------------------------------------------------------------------------------------
def test_land_stays_at_zero_and_the_ocean_finite(ctx):
    """an island across the wave seam (columns 60..66) and a rock, NaN wind over land: land-node velocities, land stress and land damage
    stay EXACTLY 0 over three sub-iterations, no ocean value is NaN, and the first sub-iteration matches the reference"""
    land = np.zeros((9, 70), dtype=bool)
    land[2:6, 60:67] = True
    land[7, 3] = True
    c = random_case(70, 9, seed=5, land=land)
    ref = reference(c)
    d = Device(ctx, c, land_mask=land)
    ln = R.land_nodes(land)
    got = d.iterate(strip_rows=3)
    check_against_reference(got, ref)
    for _ in range(3):
        assert np.all(got["u"][ln] == 0.0) and np.all(got["v"][ln] == 0.0)
        assert np.all(got["D"][:, land] == 0.0) and all(np.all(x[:, land] == 0.0) for x in got["S"])
        assert all(np.all(np.isfinite(x)) for x in got["S"] + [got["D"], got["u"], got["v"]])
        d.S, d.D, d.u, d.v = got["St"], got["Dt"], got["ut"], got["vt"]
        got = d.iterate()
    d.close()


# ---- 5. literature, no reference in between ---------------------------------------------------------------------------------------------
def test_device_returns_a_supercritical_stress_to_the_envelope(ctx):
    from test_bbm_cpu import envelope_case, envelope_expectation, uniform_state

    mpar, bp, e = R.mevp_par(), R.bbm_par(), envelope_case()
    nx, ny = 70, 3
    H, A, D, S = uniform_state(nx, ny, e["h"], e["a"], e["d"], e["s"])
    z = np.zeros((2 * ny + 1, 2 * nx + 1))
    c = dict(nx=nx, ny=ny, H=H, A=A, D=D, S=S, u=z, v=z, ua=z, va=z, uo=z, vo=z)
    got = Device(ctx, c, dts=e["dts"], hx=e["hx"], hy=e["hy"]).iterate()
    s11, s12, s22 = (R.apply(R.PSI_Q, x) for x in got["S"])
    env = np.sqrt(0.25 * (s11 - s22) ** 2 + s12 ** 2) + bp["tan_phi"] * 0.5 * (s11 + s22)
    dh, dc, coh = envelope_expectation(mpar, bp, e)
    print("envelope: max |sigma_s + tan(phi) sigma_n - c| / c = %.3e" % (np.max(np.abs(env - coh)) / coh))
    assert np.max(np.abs(env - coh)) <= 1e-12 * coh
    assert np.max(np.abs(R.apply(R.PSI_Q[:, :6], got["D"]) - (dh + (1.0 - dh) * (1.0 - dc)))) <= 1e-12


def test_device_without_relaxation_and_failure_is_hookes_law(ctx):
    from test_bbm_cpu import hooke_case, hooke_expectation, uniform_state

    nx, ny, hx, hy, dts = 70, 4, 1000.0, 800.0, 1.0
    s0, d0 = (2.0e3, -1.0e3, 3.0e3), 0.1
    H, A, D, S = uniform_state(nx, ny, 1.0, 1.0, d0, s0)
    u, v, eps = hooke_case(nx, ny, hx, hy)
    z = np.zeros_like(u)
    c = dict(nx=nx, ny=ny, H=H, A=A, D=D, S=S, u=u, v=v, ua=z, va=z, uo=z, vo=z)
    bp = ctx.bbm_default_params(cohesion_lab=1e30, lambda0=1e30)
    got = Device(ctx, c, bp=bp, dts=dts, hx=hx, hy=hy).iterate()
    for g, want in zip(got["S"], hooke_expectation(R.bbm_par(), dts, s0, eps, d0)):
        print("Hooke: max |sigma - closed form| / |closed form| = %.3e" % (np.max(np.abs(g[0] - want)) / abs(want)))
        assert np.max(np.abs(g[0] - want)) <= 1e-12 * abs(want) and np.max(np.abs(g[1:])) <= 1e-12 * abs(want)
    ctx.set_bbm_params(ctx.bbm_default_params())


def test_device_stiffnessless_cover_reaches_the_free_drift_of_the_literature(ctx):
    """a cover without stiffness carries no stress: every interior node integrates its own momentum balance with the BBM launch constants
    (explicit Coriolis, implicit drag) and must end at the steady free drift scipy solves from the published balance, to 1e-10 m/s.
    nsdg_bbm_params_set refuses young = 0, so the stiffness is 1e-200 Pa: the stress stays below 1e-190 Pa."""
    from test_oracle_dynamics import free_drift_case, free_drift_solution

    nx, ny = 70, 9
    hx, hy, ua, va, uo, vo, cgh, cga = free_drift_case(nx, ny)
    H, A, D = np.zeros((6, ny, nx)), np.zeros((6, ny, nx)), np.zeros((6, ny, nx))
    H[0], A[0] = 0.7, 0.85
    z = np.zeros_like(ua)
    c = dict(nx=nx, ny=ny, H=H, A=A, D=D, S=[np.zeros((8, ny, nx)) for _ in range(3)], u=z, v=z, ua=ua, va=va, uo=uo, vo=vo)
    d = Device(ctx, c, bp=ctx.bbm_default_params(young=1e-200), dts=60.0, hx=hx, hy=hy)
    S, Sb, D, Db = d.S, [torch.zeros_like(x) for x in d.S], d.D, torch.zeros_like(d.D)
    u, v, ub, vb = d.u, d.v, torch.zeros_like(d.u), torch.zeros_like(d.v)
    change, n = 1.0, 0
    while change >= 1e-12 and n < 20000:
        for _ in range(50):
            ctx.bbm_iterate(0, 0, ny, S, Sb, D, Db, (u, v), (ub, vb), d.packed, d.gauss)
            S, Sb, D, Db, u, ub, v, vb = Sb, S, Db, D, ub, u, vb, v
        n += 50
        change = max(float((u - ub).abs().max()), float((v - vb).abs().max()))
    print("free drift: %d sub-iterations, last change %.3e m/s" % (n, change))
    assert change < 1e-12
    want = free_drift_solution(types.SimpleNamespace(**R.mevp_par()), 9.0, -4.0, 0.05, 0.02, 0.7, 0.85)
    ui, vi = host(u)[1:-1, 1:-1], host(v)[1:-1, 1:-1]
    print("free drift: max |u - want| %.3e, |v - want| %.3e" % (np.max(np.abs(ui - want[0])), np.max(np.abs(vi - want[1]))))
    assert np.max(np.abs(ui - want[0])) < 1e-10 and np.max(np.abs(vi - want[1])) < 1e-10
    assert all(float(x.abs().max()) < 1e-150 for x in S)
    ctx.set_bbm_params(ctx.bbm_default_params())


# ---- 6. the driver ------------------------------------------------------------------------------------------------------------------------
DNX, DNY, DNSUB, DNSTEPS, DDT = 24, 18, 10, 3, 2.5  # sub-iterations of 0.25 s: the elastic wave crosses 0.22 cells


def driver_fields():
    """24 x 18 cells of 1 km, full cover, smooth fields -- an unbalanced stress of amplitude s travels as an elastic wave of amplitude s, so
    the compression sigma_n = -2.5e4 Pa is uniform and what varies (the shear 3.6e4 +- 0.6e4 Pa, 10 % of the thickness) stays far below
    it: sigma_n keeps its sign.  The shear crosses the envelope on about a third of the domain.  A converging wind of at most 3 m/s, the
    ocean at rest"""
    nx, ny = DNX, DNY
    xc = (np.arange(nx) + 0.5)[None, :] / nx + 0.0 * np.arange(ny)[:, None]
    yc = (np.arange(ny) + 0.5)[:, None] / ny + 0.0 * np.arange(nx)[None, :]
    H, A, D = np.zeros((6, ny, nx)), np.zeros((6, ny, nx)), np.zeros((6, ny, nx))
    H[0] = 1.0 + 0.1 * np.sin(2 * np.pi * xc) * np.sin(np.pi * yc)
    A[0] = 1.0
    D[0] = 0.3 + 0.2 * np.cos(np.pi * xc) * np.sin(2 * np.pi * yc)
    S = [np.zeros((8, ny, nx)) for _ in range(3)]
    S[0][0] = S[2][0] = -2.5e4
    S[1][0] = 3.6e4 + 0.6e4 * np.cos(2 * np.pi * xc) * np.cos(2 * np.pi * yc)
    X = 0.5 * HX * np.arange(2 * nx + 1)[None, :] + 0.0 * np.arange(2 * ny + 1)[:, None]
    Y = 0.5 * HY * np.arange(2 * ny + 1)[:, None] + 0.0 * np.arange(2 * nx + 1)[None, :]
    ua, va = -3.0 * (2.0 * X / (nx * HX) - 1.0), -3.0 * (2.0 * Y / (ny * HY) - 1.0)
    z = np.zeros_like(ua)
    return dict(H=H, A=A, D=D, S=S, ua=np.ascontiguousarray(ua), va=np.ascontiguousarray(va), uo=z, vo=z)


def start_state(f):
    z = np.zeros((2 * DNY + 1, 2 * DNX + 1))
    return dict(rows=(0, DNY), ny_global=DNY, nx=DNX, H=f["H"], A=f["A"], D=f["D"], u=z, v=z, s11=f["S"][0], s12=f["S"][1], s22=f["S"][2])


def run_driver(ops, device, rank=0, world=1, exchanger=None, nsteps=DNSTEPS, resume=None):
    f = driver_fields()
    blk = rowblock.RowBlock(DNX, DNY, rank, world, 1, 1)
    core = rowblock.DynamicsCore(ops, blk, HX, HY, DDT, DNSUB, device, exchanger=exchanger, rheology="bbm")
    core.load_global(f["H"], f["A"], f["uo"], f["vo"], f["ua"], f["va"])
    core.load_state_dict(resume if resume is not None else start_state(f))
    for _ in range(nsteps):
        core.step()
    return core


def reference_driver():
    record = []
    core = run_driver(R.make_ops(record=record), torch.device("cpu"))
    return core, record


def assert_driver_margins(record):
    """over all sub-iterations of the reference run: the old sigma_n, where Pt is evaluated, stays away from 0 by 1e-6 of the largest
    stress, the new one above -N / 2; failing and non-failing points are each >= 10 % in every sub-iteration"""
    N = R.bbm_par()["compr_strength"]
    assert len(record) == DNSTEPS * DNSUB
    worst = min(float(np.min(np.abs(d["sn_old"])) / d["smax"]) for d in record)
    shares = [float(np.mean(d["failing"])) for d in record]
    print("min |sigma_n| / max |sigma| over the run %.3e; failing share per sub-iteration: first %.3f, max %.3f, last %.3f"
          % (worst, shares[0], max(shares), shares[-1]))
    assert worst >= 1e-6 and all(np.min(d["sn_new"]) > -0.5 * N for d in record)
    assert all(0.1 <= x <= 0.9 for x in shares)


def thread_world(world):
    from thread_ranks import Mailbox, ThreadExchanger

    mailbox, out = Mailbox(), {}

    def rank_main(rank):
        try:
            c = abi.Context(torch.device("cuda:0"))
            blk = rowblock.RowBlock(DNX, DNY, rank, world, 1, 1)
            core = run_driver(c, torch.device("cuda"), rank, world, ThreadExchanger(blk, mailbox))
            torch.cuda.synchronize()
            res = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "D", "u", "v")}
            res["s11"] = core.owned(core.s[0]).clone()
            core.close()
            c.close()
            out[rank] = res
        except BaseException as e:  # noqa: BLE001 -- wake the peers up, then re-raise in the main thread
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
    return out


def test_driver_matches_the_reference_driver_and_three_blocks_bit_for_bit(ctx):
    ref, record = reference_driver()
    assert_driver_margins(record)
    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_bbm_params(ctx.bbm_default_params())
    one = run_driver(ctx, torch.device("cuda"))
    got = {k: host(getattr(one, k)) for k in ("H", "A", "D", "u", "v")}
    assert np.max(np.abs(got["u"])) > 1e-4
    for k in ("H", "A", "D", "u", "v"):
        w = getattr(ref, k).numpy()
        assert_close(got[k], w, 1e-9, 1e-11 * np.max(np.abs(w)), k)
    for a, b, name in zip(one.s, ref.s, ("s11", "s12", "s22")):
        assert_close(thost(a, DNX), b.numpy(), 1e-9, 1e-11 * np.max(np.abs(b.numpy())), name)
    assert all(np.all(np.isfinite(x)) for x in got.values())
    D9 = R.apply(R.PSI_Q[:, :6], got["D"])
    assert got["D"][0].min() >= 0.0 and got["D"][0].max() <= 1.0 and D9.min() >= 0.0 and D9.max() <= 1.0
    total0, total = math.fsum(driver_fields()["H"][0].ravel()), math.fsum(got["H"][0].ravel())
    print("relative drift of the total of the cell means of H: %.3e" % (abs(total - total0) / total0))
    assert abs(total - total0) <= 1e-13 * total0
    parts = thread_world(3)
    for k in ("H", "A", "D", "s11", "u", "v"):
        full = one.owned(one.s[0]) if k == "s11" else getattr(one, k)
        assert torch.equal(torch.cat([parts[r][k] for r in range(3)], dim=1 if k in ("H", "A", "D") else 0), full), k
    # checkpoint: 2 steps, state_dict, a fresh core, load_state_dict, 1 step == 3 steps
    first = run_driver(ctx, torch.device("cuda"), nsteps=2)
    state = rowblock.DynamicsCore.merge_states([first.state_dict()])
    assert state["D"].shape == (6, DNY, DNX)
    again = run_driver(ctx, torch.device("cuda"), nsteps=1, resume=state)
    for k in ("H", "A", "D", "u", "v"):
        assert torch.equal(getattr(again, k), getattr(one, k)), k
    assert all(torch.equal(a, b) for a, b in zip(again.s, one.s))
    for core in (one, first, again):
        core.close()


# ---- 7. ABI errors ------------------------------------------------------------------------------------------------------------------------
def test_abi_errors(gpu):
    c = abi.Context(gpu)
    nx, ny = 8, 6
    c.set_grid(nx, ny, HX, HY)
    lib, h = c.lib, c.h
    S = [c.private_zeros(8, ny, nx, "cuda") for _ in range(6)]
    G = [c.private_zeros(9, ny, nx, "cuda") for _ in range(3)]
    D, Db = torch.zeros(6, ny, nx, dtype=torch.float64, device="cuda"), torch.zeros(6, ny, nx, dtype=torch.float64, device="cuda")
    u, v, ub, vb = (torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda") for _ in range(4))
    packed = torch.zeros(8 * u.numel(), dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()

    def call(k0=0, j0=0, j1=ny, s_out=S[3:], d_in=D, d_out=Db, un=ub, pk=packed):
        ts = S[:3] + list(s_out) + [d_in, d_out, u, v, un, vb, pk] + G
        return lib.nsdg_bbm_iterate(h, k0, j0, j1, *[p(t) for t in ts])

    assert call() == -3 and b"nsdg_bbm_iterate" in lib.nsdg_last_error()  # NSDG_ERR_STATE: before any packing
    H = torch.ones(6, ny, nx, dtype=torch.float64, device="cuda")
    c.mevp_prepare(1.0, H, H, (u, v), (u, v), (u, v), packed)
    assert call() == 0
    assert call(pk=None) == -1 and call(d_in=None) == -1  # null pointers
    assert call(d_out=D) == -1 and b"damage" in lib.nsdg_last_error()
    assert call(s_out=S[:3]) == -1 and call(un=u) == -1
    assert call(k0=1, j0=3) == -1 and call(k0=2, j0=2) == -1 and call(k0=0, j0=0, j1=ny + 1) == -1  # k0 not in {j0 - 1, 0}, rows outside
    assert call(k0=2, j0=3) == 0 and call(k0=0, j0=1) == 0
    assert lib.nsdg_bbm_prepare(h, 0, ny + 1, p(H), p(H), p(G[0]), p(G[1]), p(G[2])) == -1
    assert lib.nsdg_bbm_prepare(h, 0, ny, p(H), None, p(G[0]), p(G[1]), p(G[2])) == -1
    for bad in (dict(young=0.0), dict(young=float("nan")), dict(relax_exponent=0), dict(d_max=1.0), dict(d_max=0.0), dict(lambda0=-1.0),
                dict(t_heal=0.0), dict(tan_phi=float("inf"))):
        with pytest.raises(abi.NsdgError):
            c.set_bbm_params(c.bbm_default_params(**bad))
    c.set_bbm_params(c.bbm_default_params(relax_exponent=1))
    torch.cuda.synchronize()
    c.close()

"""Drifters on the device (csrc/drifters.hip; include/nsdg.h "drifters"): nsdg_drifters_advance against the float64
reference (tests/drifters_ref.py) on the inputs of tests/drifters_cases.py, its row ranges and checks, the closed form of a solid-body
rotation, and the Python driver on 1 row block against 3.

The position bound, 64 * 2^-52 * max(Lx, Ly), is derived, not measured: the local coordinate x / hx - ix carries an absolute error of about
nx * 2^-53; the velocity changes by at most h / dt across an element when it is sampled at the clamp, so that error moves the step by at
most about nx * 2^-53 * h = 2^-53 * L; the weights, the two sums of nine products (FMA contraction either way) and the Heun sum add a few
dozen roundings of that size; the final add rounds at ulp(L) = 2^-52 L.  tests/test_drifters_cpu.py holds the float64 reference itself to a
quarter of the bound against extended precision.  Statuses must match exactly and no drifter is left out of a comparison."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import drifters_cases as cases  # noqa: E402
import drifters_ref as R  # noqa: E402
import thread_ranks  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_refs = {}


def case(nx, ny, n):
    """the inputs and the float64 reference of one case, computed once and left unchanged"""
    if (nx, ny, n) not in _refs:
        c = cases.make(nx, ny, n)
        want = cases.reference(c)
        want.setflags(write=False)
        _refs[(nx, ny, n)] = (c, want)
    return _refs[(nx, ny, n)]


def place(ctx, c, lo=0, hi=None, ny_global=0):
    """the grid, the placement and the land mask of the rows [lo, hi) of case c; returns the device arrays u, v, A of those rows"""
    ny, nx = c["A0"].shape
    hi = ny if hi is None else hi
    ctx.set_grid(nx, hi - lo, c["hx"], c["hy"])
    ctx.set_block(lo, ny_global)
    ctx.set_land_mask(dev(c["land"][lo:hi]))
    A = np.zeros((6, hi - lo, nx))
    A[0] = c["A0"][lo:hi]
    A[1:] = 7.0  # only the cell mean is read
    return dev(c["u"][2 * lo:2 * hi + 1]), dev(c["v"][2 * lo:2 * hi + 1]), dev(A)


def advance(ctx, c, j0=0, j1=None, lo=0, hi=None, ny_global=0):
    u, v, A = place(ctx, c, lo, hi, ny_global)
    d = dev(c["d"])
    out = torch.full_like(d, float("nan"))
    ctx.drifters_advance(j0, ctx.ny if j1 is None else j1, c["dt"], c["min_conc"], u, v, A, d, out)
    torch.cuda.synchronize()
    ctx.set_land_mask(None)
    assert torch.equal(d, dev(c["d"]))  # out of place: the input is untouched
    return out.cpu().numpy()


def compare(got, want, c, what):
    ny, nx = c["A0"].shape
    bound = R.bound(nx * c["hx"], ny * c["hy"])
    assert np.array_equal(got[2], want[2]), (what, "statuses differ at", np.flatnonzero(got[2] != want[2])[:10])
    err = float(np.abs(got[:2] - want[:2]).max())  # every drifter: a stopped one must not have moved at all
    print("%s largest position difference %.3e m, bound %.3e m (%.4f of it)" % (what, err, bound, err / bound))
    assert err <= bound, (what, err, bound)
    stopped = want[2] != 0
    assert np.array_equal(got[:2, stopped], c["d"][:2, stopped])


# ------------------------------------------------------------------------------------------------ the kernel against the reference
@pytest.mark.parametrize("nx,ny,n", cases.CASES)
def test_one_step_matches_the_reference(ctx, nx, ny, n):
    assert abi.DRIFTERS_BLOCK == cases.BLOCK
    c, want = case(nx, ny, n)
    got = advance(ctx, c)
    assert np.all(np.isfinite(got))  # a single domain owns every drifter
    compare(got, want, c, "%dx%d n=%d:" % (nx, ny, n))
    if n >= 1000:
        assert all((want[2] == s).sum() > 5 for s in (0, 1, 2, 3)) and (want[2] == 0).sum() > 300


def test_two_row_ranges_and_their_maximum_equal_one_launch(ctx):
    c, want = case(70, 9, 1000)
    whole = advance(ctx, c)
    a, b = advance(ctx, c, 0, 4), advance(ctx, c, 4, 9)
    rows = np.array([R.locate(y, c["hy"], 9) for y in c["d"][1]])
    for part, (j0, j1) in ((a, (0, 4)), (b, (4, 9))):
        outside = (rows < j0) | (rows >= j1)
        assert outside.any() and np.all(np.isneginf(part[:, outside])) and np.all(np.isfinite(part[:, ~outside]))
    assert np.array_equal(np.maximum(a, b), whole)
    assert np.all(np.isneginf(advance(ctx, c, 3, 3)))  # an empty range owns nothing


def test_a_row_block_with_ghost_rows_computes_what_the_domain_computes(ctx):
    """rows [3, 6) of the 9 as a local array [2, 7) placed by nsdg_block_set, and the blocks at the two ends: bit for bit the single domain"""
    c, want = case(70, 9, 1000)
    whole = advance(ctx, c)
    merged = np.full_like(whole, -np.inf)
    for (lo, hi, j0, j1) in ((0, 4, 0, 3), (2, 7, 1, 4), (5, 9, 1, 4)):
        merged = np.maximum(merged, advance(ctx, c, j0, j1, lo, hi, 9))
    assert np.array_equal(merged, whole)


def test_checks(ctx, gpu):
    c, _ = case(70, 9, 255)
    u, v, A = place(ctx, c)
    d = dev(c["d"])
    out = torch.empty_like(d)
    call = lambda *a: ctx.lib.nsdg_drifters_advance(ctx.h, *a)
    ptr = lambda t: abi.C.c_void_p(t.data_ptr())
    good = [0, 9, 120.0, 0.15, 255, ptr(u), ptr(v), ptr(A), ptr(d), ptr(out)]
    assert call(*good) == 0

    def refused(k, value, text):
        args = list(good)
        args[k] = value
        assert call(*args) == -1, (k, value)
        assert text in ctx.lib.nsdg_last_error().decode(), ctx.lib.nsdg_last_error()

    refused(9, ptr(d), "out of place")
    refused(0, -1, "row range")
    refused(1, 10, "row range")
    refused(4, -1, "n must be >= 0")
    refused(2, float("nan"), "finite")
    refused(3, float("inf"), "finite")
    for k in (5, 6, 7, 8, 9):
        refused(k, None, "null pointer")
    args = list(good)
    args[4] = 0
    args[5:] = [None] * 5
    assert call(*args) == 0  # n == 0 does nothing
    # a local array inside the domain: its first and last rows have no neighbour row to read
    ctx.set_block(2, 20)
    refused(0, 0, "the ghost row below row 0 is missing")
    args = list(good)
    args[0], args[1] = 1, 9
    assert call(*args) == -1 and "the ghost row above row 8 is missing" in ctx.lib.nsdg_last_error().decode()
    args[1] = 8
    assert call(*args) == 0
    ctx.set_block(0, 0)
    torch.cuda.synchronize()
    ctx.set_land_mask(None)
    fresh = abi.Context(gpu)
    try:
        assert fresh.lib.nsdg_drifters_advance(fresh.h, *good) == -3  # NSDG_ERR_STATE: no grid
        t = torch.arange(6, dtype=torch.float64, device="cuda")
        fresh.comm_max_f64_array(t)  # no communicator: a no-op
        assert t.tolist() == [0, 1, 2, 3, 4, 5]
    finally:
        fresh.close()


def test_solid_body_rotation_on_the_device_follows_heuns_closed_form(ctx):
    u, v, h, dt, centre, r0 = cases.rotation()
    theta, nsteps = 0.05, 50
    ctx.set_grid(70, 9, h, h)
    ctx.set_block(0, 0)
    ctx.set_land_mask(None)
    A = torch.ones(6, 9, 70, dtype=torch.float64, device="cuda")
    start = np.array([[centre[0] + r0 * np.cos(a), centre[1] + r0 * np.sin(a), 0.0] for a in (0.0, 0.7, 2.0, 4.1)]).T
    d, e = dev(start), dev(start)
    ud, vd = dev(u), dev(v)
    for _ in range(nsteps):
        ctx.drifters_advance(0, 9, dt, 0.15, ud, vd, A, d, e)
        d, e = e, d
    got = d.cpu().numpy()
    assert np.all(got[2] == 0)
    for k in range(got.shape[1]):
        er, ea = cases.rotation_check(got[0, k], got[1, k], start[0, k], start[1, k], centre, theta, nsteps)
        print("rotation, drifter %d: radius off by %.2e, angle by %.2e (relative)" % (k, er, ea))
        assert er <= 1e-12 and ea <= 1e-12, (k, er, ea)


# ------------------------------------------------------------------------------------------------ the driver: 1 row block against 3
NX, NY, NSUB, NSTEPS, WIND = 64, 48, 24, 6, 3.0


def seeds():
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(5)
    xy = []
    for row in (16, 32):  # the boundaries of three row blocks
        for off in (0.0, 0.01, -0.01, 1.0, -1.0, 5.0, -5.0):
            for fx in np.linspace(0.08, 0.92, 9):
                xy.append((fx * bt.L, row * bt.hy + off))
    xy += [(x, y) for x, y in zip(rng.uniform(0, bt.L, 60), rng.uniform(0, bt.L, 60))]
    xy += [(0.0, 0.0), (bt.L, bt.L), (0.0, 0.5 * bt.L), (0.5 * bt.L, bt.L), (bt.hx * 7, bt.hy * 7)]
    return np.array(xy)


def drifter_rank(rank, world, variant, mailbox, out, local_group, drifters, steps=NSTEPS, resume=None, record=False):
    """thread_ranks.run_rank cannot return the drifters: the same set-up around thread_ranks.Mailbox and thread_ranks.fields"""
    try:
        ctx = abi.Context(torch.device("cuda:0"))
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_params(ctx.mevp_default_params(alpha=300.0, beta=300.0))
        bt, H, A, uo, vo, ua, va = thread_ranks.fields(NX, NY, WIND)
        depth = (variant, variant - 1) if variant >= 2 else (1, 1)
        blk = rowblock.RowBlock(NX, NY, rank, world, *depth)
        exchanger = None
        if world > 1:
            ctx.comm_deadline(60.0)
            exchanger = rowblock.NativeHaloExchanger(ctx, blk, local_group=local_group)
        core = rowblock.DynamicsCore(ctx, blk, bt.hx, bt.hy, 120.0, NSUB, torch.device("cuda"), exchanger=exchanger, drifters=drifters)
        core.load_global(H, A, uo, vo, ua, va)
        if resume is not None:
            core.load_state_dict(resume)
        res = {"steps": []}
        for _ in range(steps):
            before = core.drifters_read() if record else None
            core.step()
            if record:
                torch.cuda.synchronize()
                res["steps"].append((before, core.u.cpu().numpy(), core.v.cpu().numpy(), core.A[0].cpu().numpy(), core.drifters_read()))
        torch.cuda.synchronize()
        res.update({k: core.owned(getattr(core, k)).cpu().numpy() for k in ("H", "A", "u", "v")})
        res["drifters"] = core.drifters_read() if drifters is not None else None
        res["state"] = core.state_dict()
        core.close()
        out[rank] = res
    except BaseException as e:  # noqa: BLE001 -- wake the peers up, then re-raise in the main thread
        with mailbox.cv:
            mailbox.error = e
            mailbox.cv.notify_all()
        out[rank] = e


def run_world(world, variant, drifters, **kw):
    mailbox, out = thread_ranks.Mailbox(), {}
    thread_ranks._local_group[0] += 1
    threads = [threading.Thread(target=drifter_rank, args=(r, world, variant, mailbox, out, thread_ranks._local_group[0], drifters), kwargs=kw)
               for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return out


@pytest.fixture(scope="module")
def one_block(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    return run_world(1, 4, seeds(), record=True)[0]


def test_one_block_every_step_is_the_reference_step(one_block):
    """after every step the positions equal the reference applied to the u, v, A downloaded at that step and to the device's own previous
    positions, within the bound; statuses exactly"""
    bt = synthetic.BoxTest(NX, NY)
    bound = R.bound(bt.L, bt.L)
    assert len(one_block["steps"]) == NSTEPS
    for k, (before, u, v, A0, after) in enumerate(one_block["steps"]):
        d = np.stack([before["x"], before["y"], before["status"].astype(np.float64)])
        want = R.advance(u, v, A0, d, bt.hx, bt.hy, 120.0, 0.15)
        assert np.array_equal(after["status"], want[2].astype(np.int64)), k
        err = max(float(np.abs(after["x"] - want[0]).max()), float(np.abs(after["y"] - want[1]).max()))
        print("step %d: largest position difference %.3e m, bound %.3e m (%.4f of it)" % (k, err, bound, err / bound))
        assert err <= bound, (k, err, bound)
    start, end = seeds(), one_block["drifters"]
    assert (end["status"] == 0).sum() > 100 and np.abs(end["y"] - start[:, 1]).max() > 1.0
    block = lambda y: np.array([R.locate(yy, bt.hy, NY) for yy in y]) // 16
    crossed = block(start[:, 1]) != block(end["y"])
    print("%d drifters crossed a block boundary" % crossed.sum())
    assert crossed.sum() >= 1, "no drifter crossed a block boundary: the seeds do not test the hand-over"


@pytest.mark.parametrize("variant", [4, 1])
def test_three_blocks_equal_one_block(one_block, variant):
    """thread ranks on the native exchange's local transport: positions and statuses agree bit for bit on every rank; variant 1 runs the
    ghost depth (1, 1), whose upper ghost node rows only the drifters' own exchange completes"""
    parts = run_world(3, variant, seeds())
    for r in range(3):
        for k in ("x", "y", "status"):
            assert np.array_equal(parts[r]["drifters"][k], one_block["drifters"][k]), (r, k)
        assert np.array_equal(parts[r]["state"]["drifters"], one_block["state"]["drifters"])
    for k in ("H", "A"):
        assert np.array_equal(np.concatenate([parts[r][k] for r in range(3)], axis=1), one_block[k]), k
    for k in ("u", "v"):
        assert np.array_equal(np.concatenate([parts[r][k] for r in range(3)], axis=0), one_block[k]), k
    merged = rowblock.DynamicsCore.merge_states([parts[r]["state"] for r in range(3)])
    assert np.array_equal(merged["drifters"], one_block["state"]["drifters"])


def test_checkpoint_and_resume_agree_bit_for_bit(one_block):
    first = run_world(1, 4, seeds(), steps=NSTEPS // 2)[0]
    state = rowblock.DynamicsCore.merge_states([first["state"]])
    moved_on = seeds()
    moved_on[:, 0] = 1.0  # the state's list replaces the constructor's
    second = run_world(1, 4, moved_on, steps=NSTEPS - NSTEPS // 2, resume=state)[0]
    for k in ("x", "y", "status"):
        assert np.array_equal(second["drifters"][k], one_block["drifters"][k]), k
    assert np.array_equal(second["u"], one_block["u"]) and np.array_equal(second["H"], one_block["H"])


def test_the_fields_do_not_know_about_the_drifters(one_block):
    plain = run_world(1, 4, None)[0]
    assert plain["drifters"] is None and "drifters" not in plain["state"]
    for k in ("H", "A", "u", "v"):
        assert plain[k].tobytes() == one_block[k].tobytes(), k

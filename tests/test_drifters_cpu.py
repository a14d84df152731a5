"""Drifters without a GPU (include/nsdg.h "drifters"): the reference restatement against the literature and against
itself in extended precision, the statuses and the predictor clamp, the built library's exports, the Python driver on gloo worlds with the
reference behind an ops object, and the constructor's refusals."""
import ctypes as C
import os
import re
import socket
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

import drifters_cases as cases  # noqa: E402
import drifters_ref as R  # noqa: E402
from nextsimdg_amd import abi, build, rowblock, synthetic  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_solid_body_rotation_follows_heuns_closed_form():
    """Heun on u = -w (y - yc), v = w (x - xc): r_n / r_0 = (1 + theta^4 / 4)^(n / 2), the angle grows by atan2(theta, 1 - theta^2 / 2) per
    step.  50 steps, both to 1e-12 relative: rounding only (a position of a few h carries 2^-53 per operation, a few dozen operations per
    step)"""
    u, v, h, dt, centre, r0 = cases.rotation()
    theta, nsteps = 0.05, 50
    A0 = np.ones((9, 70))
    start = np.array([[centre[0] + r0 * np.cos(a), centre[1] + r0 * np.sin(a), 0.0] for a in (0.0, 0.7, 2.0, 4.1)]).T
    d = start.copy()
    for _ in range(nsteps):
        d = R.advance(u, v, A0, d, h, h, dt, 0.15)
    assert np.all(d[2] == 0)
    for k in range(d.shape[1]):
        er, ea = cases.rotation_check(d[0, k], d[1, k], start[0, k], start[1, k], centre, theta, nsteps)
        assert er <= 1e-12 and ea <= 1e-12, (k, er, ea)
    # Euler in place of Heun would miss by theta^2 / 2 per step
    assert (1 + theta ** 2) ** (nsteps / 2) - (1 + theta ** 4 / 4) ** (nsteps / 2) > 1e-2


def test_biquadratic_velocity_is_reproduced():
    """CG2 holds a biquadratic polynomial exactly: sampled at random points it comes back to 1e-13 of its maximum"""
    nx, ny, hx, hy = 7, 5, 1000.0, 800.0
    rng = np.random.default_rng(3)
    cu, cv = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
    poly = lambda c, x, y: sum(c[a, b] * (x / (nx * hx)) ** a * (y / (ny * hy)) ** b for a in range(3) for b in range(3))
    X, Y = np.meshgrid(np.arange(2 * nx + 1) * (hx / 2), np.arange(2 * ny + 1) * (hy / 2))
    u, v = poly(cu, X, Y), poly(cv, X, Y)
    scale = max(np.abs(u).max(), np.abs(v).max())
    for _ in range(200):
        x, y = rng.uniform(0, nx * hx), rng.uniform(0, ny * hy)
        ix, iy = R.locate(x, hx, nx), R.locate(y, hy, ny)
        uu, vv = R.velocity(u, v, ix, iy, iy, np.float64(x), np.float64(y), np.float64(hx), np.float64(hy), np.float64)
        assert abs(uu - poly(cu, x, y)) <= 1e-13 * scale and abs(vv - poly(cv, x, y)) <= 1e-13 * scale
    # the closed forms of the header are the product formula of the reference
    for t in (-0.5, -0.2, 0.0, 0.31, 0.5):
        assert np.allclose(R.lagrange(np.float64(t), np.float64), [2 * t * t - t, 1 - 4 * t * t, 2 * t * t + t], rtol=0, atol=1e-15)


def test_every_status_is_reached_and_a_stopped_drifter_stays():
    nx, ny, h, dt = 6, 5, 1000.0, 100.0
    u = np.full((2 * ny + 1, 2 * nx + 1), 2.0)  # 200 m per step eastwards
    v = np.zeros_like(u)
    A0 = np.ones((ny, nx))
    A0[1, 1] = 0.1
    A0[3, 3] = np.nan  # a NaN concentration is not "<": the drifter moves
    land = np.zeros((ny, nx), dtype=np.uint8)
    land[2, 2] = land[1, 1] = 1  # land goes before the ice test
    d = np.array([[5900.0, 500.0, 0], [500.0, 1500.0, 0], [2500.0, 2500.0, 0], [1500.0, 1500.0, 0], [3500.0, 3500.0, 0], [100.0, 100.0, 2]]).T
    A0[1, 0] = 0.1
    out = R.advance(u, v, A0, d, h, h, dt, 0.15, land=land)
    assert list(out[2]) == [1, 2, 3, 3, 0, 2]
    assert np.array_equal(out[:2, [0, 1, 2, 3, 5]], d[:2, [0, 1, 2, 3, 5]])  # whoever stops keeps its position
    assert out[0, 4] == 3700.0 and out[1, 4] == 3500.0
    again = R.advance(u, v, np.ones((ny, nx)), out, h, h, dt, 0.15)  # ice everywhere, no land: the stopped ones stay stopped
    assert np.array_equal(again[:, [0, 1, 2, 3, 5]], out[:, [0, 1, 2, 3, 5]]) and again[0, 4] == 3900.0


def test_predictor_is_clamped_to_the_neighbourhood_whatever_the_row_blocks():
    """a predictor that would leave the 3 x 3 elements around the drifter is clamped to them -- by the drifter's own indices, so cutting the
    domain into row blocks (each with one ghost row, nothing valid beyond) changes nothing"""
    nx, ny, h, dt = 8, 12, 1000.0, 100.0
    rng = np.random.default_rng(11)
    u, v = rng.uniform(-40, 40, (2 * ny + 1, 2 * nx + 1)), rng.uniform(-40, 40, (2 * ny + 1, 2 * nx + 1))  # up to 4 h per step
    A0 = np.ones((ny, nx))
    n = 300
    d = np.stack([rng.uniform(0, nx * h, n), rng.uniform(0, ny * h, n), np.zeros(n)])
    whole = R.advance(u, v, A0, d, h, h, dt, 0.15)
    assert (whole[2] == 0).sum() > 20 and (whole[2] == 1).sum() > 20
    # one drifter by hand: predictor beyond the clamp
    k = int(np.flatnonzero(whole[2] == 0)[0])
    x, y = d[0, k], d[1, k]
    ix, iy = int(x // h), int(y // h)
    u1, v1 = R.velocity(u, v, ix, iy, iy, x, y, h, h, np.float64)
    xp, yp = np.clip(x + dt * u1, max(ix - 1, 0) * h, min(ix + 2, nx) * h), np.clip(y + dt * v1, max(iy - 1, 0) * h, min(iy + 2, ny) * h)
    ix2, iy2 = min(max(R.locate(xp, h, nx), max(ix - 1, 0)), min(ix + 1, nx - 1)), min(max(R.locate(yp, h, ny), max(iy - 1, 0)), min(iy + 1, ny - 1))
    u2, v2 = R.velocity(u, v, ix2, iy2, iy2, xp, yp, h, h, np.float64)
    assert whole[0, k] == x + 0.5 * dt * (u1 + u2) and whole[1, k] == y + 0.5 * dt * (v1 + v2)
    clamped = sum(1 for i in range(n) if abs(dt * R.velocity(u, v, int(d[0, i] // h), int(d[1, i] // h), int(d[1, i] // h), d[0, i], d[1, i], h, h, np.float64)[0]) > 2 * h)
    assert clamped > 10  # the clamp was active
    for world in (2, 3):
        merged = np.full_like(whole, -np.inf)
        for rank in range(world):
            b = rowblock.RowBlock(nx, ny, rank, world)
            ul, vl = u[b.node_slice()].copy(), v[b.node_slice()].copy()
            part = R.advance(ul, vl, A0[b.elem_slice()], d, h, h, dt, 0.15, row0=b.lo, ny_global=ny, j0=b.j0, j1=b.j1)
            owned = np.isfinite(part[2])
            assert np.all(np.isneginf(part[:, ~owned])) and not np.any(owned & np.isfinite(merged[2]))  # exactly one owner
            merged = np.maximum(merged, part)
        assert np.array_equal(merged, whole)


@pytest.mark.parametrize("nx,ny,n", cases.CASES)
def test_float64_and_longdouble_references_agree_within_a_quarter_of_the_bound(nx, ny, n):
    """the inputs of tests/test_gpu_drifters.py: the float64 reference is within a quarter of the GPU test's bound of the same arithmetic in
    extended precision, statuses identical -- the bound leaves the device three quarters"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("this platform's long double is a double")
    c = cases.make(nx, ny, n)
    a, b = cases.reference(c), cases.reference(c, dtype=np.longdouble)
    assert np.array_equal(a[2], b[2].astype(np.float64))
    assert (a[2] == 0).any() and (n < 100 or all((a[2] == s).any() for s in (1, 2, 3)) or nx * ny <= 3)
    diff = np.abs(a[:2].astype(np.longdouble) - b[:2]).max()
    print("float64 against longdouble: %.3g of the bound" % (float(diff) / R.bound(nx * c["hx"], ny * c["hy"])))
    assert diff <= R.bound(nx * c["hx"], ny * c["hy"]) / 4


# ---------------------------------------------------------------------------------------------------------------- the built library
def test_library_exports_and_binds_the_drifter_calls():
    build.build_lib(verbose=False)
    lib = abi.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsdg.h")).read(), flags=re.S)
    for name in ("nsdg_drifters_advance", "nsdg_comm_max_f64_array"):
        assert hasattr(lib, name), "libnsdg.so does not export " + name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "include/nsdg.h does not declare " + name
        assert name in abi.SYMBOLS
    assert callable(getattr(abi.Context, "drifters_advance", None)) and callable(getattr(abi.Context, "comm_max_f64_array", None))
    # without a context: argument errors, never a crash
    assert lib.nsdg_drifters_advance(None, 0, 0, 1.0, 0.15, 0, None, None, None, None, None) == -1
    assert lib.nsdg_comm_max_f64_array(None, None, 0) == -1
    assert (abi.DRIFTER_ACTIVE, abi.DRIFTER_LEFT, abi.DRIFTER_NO_ICE, abi.DRIFTER_LAND) == (R.ACTIVE, R.LEFT, R.NO_ICE, R.LAND)
    assert abi.DRIFTERS_BLOCK == cases.BLOCK


# ---------------------------------------------------------------------------------------------------------------- the driver on the CPU
NX, NY, NSUB, NSTEPS = 16, 24, 5, 6


def drifter_ops(variant):
    from oracle_ops import OracleOps

    class DrifterOps(OracleOps):
        """the oracle ops with the drifter call of abi.Context, backed by the reference"""
        row0, ny_glob = 0, None

        def set_block(self, row0, ny_global):
            self.row0, self.ny_glob = row0, ny_global

        def drifters_advance(self, j0, j1, dt, min_conc, u, v, A, d_in, d_out):
            assert d_in.data_ptr() != d_out.data_ptr()
            d_out.numpy()[:] = R.advance(u.numpy(), v.numpy(), A.numpy()[0], d_in.numpy(), self.hx, self.hy, dt, min_conc, row0=self.row0,
                                         ny_global=self.ny_glob, j0=j0, j1=j1)

    return DrifterOps(mevp_variant=variant, alpha=200.0, beta=200.0)


def seeds():
    """on and next to the boundaries of 2 and 3 row blocks (rows 12; 8 and 16), and a few anywhere"""
    bt = synthetic.BoxTest(NX, NY)
    xy = []
    for row in (8, 12, 16):
        for kx, off in enumerate((0.0, 1e-6, -1e-6, 1e-3, -1e-3, 0.05, -0.05, 1.0, -1.0)):
            for fx in (0.2, 0.45, 0.8):
                xy.append(((fx + 0.01 * kx) * bt.L, row * bt.hy + off))
    xy += [(0.3 * bt.L, 0.3 * bt.L), (0.0, 0.0), (bt.L, bt.L), (0.5 * bt.L, 0.77 * bt.L)]
    return np.array(xy)


def run_core(rank, world, variant=1, steps=NSTEPS, resume=None, record=None, drifters="seeds"):
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(41)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    depth = (variant, variant - 1) if variant >= 2 else (1, 1)
    blk = rowblock.RowBlock(NX, NY, rank, world, *depth)
    core = rowblock.DynamicsCore(drifter_ops(variant), blk, bt.hx, bt.hy, 120.0, NSUB, torch.device("cpu"),
                                 drifters=seeds() if isinstance(drifters, str) else drifters)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    if resume is not None:
        core.load_state_dict(resume)
    for _ in range(steps):
        core.step()
        if record is not None:
            record.append(core.drifters_read())
    return core


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def worker(rank, world, port, outdir, variant):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = run_core(rank, world, variant)
        states = [None] * world
        dist.all_gather_object(states, core.state_dict())
        merged = rowblock.DynamicsCore.merge_states(states)  # asserts that the ranks hold the same list
        out = {"drifters": core.drifters_read(), "state": merged["drifters"], "u": core.owned(core.u).clone()}
        torch.save(out, os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def one_block():
    record = []
    core = run_core(0, 1, record=record)
    return core, record


@pytest.mark.parametrize("world,variant", [(2, 1), (3, 2)])
def test_row_blocks_move_the_drifters_as_the_single_domain_does(world, variant, one_block, tmp_path):
    """6 steps on 16 x 24 as gloo worlds of 2 (one sub-iteration per pass, ghost depth (1, 1)) and 3 (two per pass, (2, 1)): positions and
    statuses equal the 1-block run bit for bit on every rank, and some drifter changed its owner on the way"""
    ref, record = one_block
    want = ref.drifters_read()
    assert (want["status"] == 0).sum() > 50 and float(ref.u.abs().max()) > 1e-5
    start = seeds()
    moved = np.abs(want["y"] - start[:, 1])
    assert moved[want["status"] == 0].max() > 1e-4
    # owners along the 1-block run: the block whose rows hold the drifter's element
    hy = synthetic.BoxTest(NX, NY).hy
    bounds = [rowblock.split_rows(NY, world, r) for r in range(world)]
    owner = lambda y: np.array([[r for r, (a, b) in enumerate(bounds) if a <= R.locate(yy, hy, NY) < b][0] for yy in y])
    owners = np.stack([owner(start[:, 1])] + [owner(rec["y"]) for rec in record])
    assert (owners != owners[0]).any(axis=0).sum() >= 1, "no drifter changed its owner: the seeds do not test the hand-over"
    mp.spawn(worker, args=(world, free_port(), str(tmp_path), variant), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r), weights_only=False) for r in range(world)]
    assert torch.equal(torch.cat([p["u"] for p in parts], dim=0), ref.u)
    for p in parts:
        for k in ("x", "y", "status"):
            assert np.array_equal(p["drifters"][k], want[k]), k
        assert np.array_equal(p["state"], ref.state_dict()["drifters"])


def test_checkpoint_and_resume_carries_the_drifters(one_block):
    ref, _ = one_block
    first = run_core(0, 1, steps=NSTEPS // 2)
    state = rowblock.DynamicsCore.merge_states([first.state_dict()])
    assert state["drifters"].shape == (3, len(seeds()))
    fresh = seeds().copy()
    fresh[:, 0] = 1.0  # what the constructor gets is replaced by the state's
    core = run_core(0, 1, steps=NSTEPS - NSTEPS // 2, resume=state, drifters=fresh)
    for k in ("x", "y", "status"):
        assert np.array_equal(core.drifters_read()[k], ref.drifters_read()[k]), k
    assert torch.equal(core.u, ref.u) and torch.equal(core.H, ref.H)
    del state["drifters"]
    with pytest.raises(ValueError, match="'drifters' in the state"):
        run_core(0, 1, steps=0, resume=state)


def test_without_drifters_nothing_is_called_or_allocated(one_block):
    ref, _ = one_block
    from oracle_ops import OracleOps

    bt = synthetic.BoxTest(NX, NY)
    core = rowblock.DynamicsCore(OracleOps(alpha=200.0, beta=200.0), rowblock.RowBlock(NX, NY), bt.hx, bt.hy, 120.0, NSUB, torch.device("cpu"))
    assert core._drifters is None and "drifters" not in core.state_dict()  # OracleOps has no drifters_advance to call
    with pytest.raises(ValueError, match="drifters="):
        core.drifters_read()
    plain = run_core(0, 1, drifters=None)  # the fields do not know about the drifters
    assert torch.equal(plain.u, ref.u) and torch.equal(plain.A, ref.A)


def test_advance_moves_the_drifters_once_per_substep():
    a = run_core(0, 1, steps=0)
    a.advance(240.0, substeps=2)
    b = run_core(0, 1, steps=2)
    assert np.array_equal(a.drifters_read()["y"], b.drifters_read()["y"]) and np.array_equal(a.drifters_read()["x"], b.drifters_read()["x"])


def test_coupled_core_moves_the_drifters_too():
    """CoupledCore.step() has a call sequence of its own: the drifters move there as well, by the same velocity, and change no field"""
    def coupled(drifters, steps=2):
        bt = synthetic.BoxTest(NX, NY)
        H, A = bt.dg_fields()
        A[0] -= 0.2
        core = rowblock.CoupledCore(drifter_ops(1), rowblock.RowBlock(NX, NY), bt.hx, bt.hy, 120.0, NSUB, torch.device("cpu"), drifters=drifters)
        ua, va = bt.wind(0.0)
        core.load_global(H, A, *bt.ocean(), 3.0 * ua, 3.0 * va)
        state, forcing, _ = synthetic.column_fields(NX * NY, 5)
        col = {k: v.reshape(NY, NX) for k, v in {**state, **forcing}.items()}
        col["wind"] = 0.2 * col["wind"]
        core.load_column(col)
        for _ in range(steps):
            core.step()
        return core

    with_, without = coupled(seeds()), coupled(None)
    got = with_.drifters_read()
    assert (got["status"] == 0).sum() > 10 and np.abs(got["y"] - seeds()[:, 1]).max() > 1e-5
    assert (got["status"] == 2).any()  # the random column forcing opens water: those drifters lost their ice
    assert torch.equal(with_.u, without.u) and torch.equal(with_.H, without.H) and torch.equal(with_.col["tice0"], without.col["tice0"])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_constructor_refusals_name_the_cause():
    from oracle_ops import OracleOps

    bt = synthetic.BoxTest(NX, NY)
    mk = lambda ops=None, blk=None, exchanger=None, **kw: rowblock.DynamicsCore(ops or drifter_ops(1), blk or rowblock.RowBlock(NX, NY), bt.hx, bt.hy,
                                                                               120.0, NSUB, torch.device("cpu"), exchanger=exchanger, **kw)
    ok = [[1000.0, 2000.0]]
    with pytest.raises(ValueError, match="OracleOps has no drifters_advance"):
        mk(ops=OracleOps(), drifters=ok)
    with pytest.raises(ValueError, match=r"\[n, 2\].*\[n, 3\].*shape \(3,\)"):
        mk(drifters=[1.0, 2.0, 0.0])
    with pytest.raises(ValueError, match="drifter 1 has a non-finite value"):
        mk(drifters=[[0.0, 0.0], [np.nan, 1.0]])
    with pytest.raises(ValueError, match="drifter 0 .* is outside the domain"):
        mk(drifters=[[-1.0, 5.0]])
    with pytest.raises(ValueError, match="drifter 1 .* is outside the domain"):
        mk(drifters=[[0.0, bt.L], [0.0, np.nextafter(bt.L, np.inf)]])
    with pytest.raises(ValueError, match="drifter 0 has the status 4.0"):
        mk(drifters=[[1.0, 1.0, 4.0]])
    with pytest.raises(ValueError, match="drifter 0 has the status 0.5"):
        mk(drifters=[[1.0, 1.0, 0.5]])
    with pytest.raises(ValueError, match="drifter_min_conc must be finite"):
        mk(drifters=ok, drifter_min_conc=float("nan"))
    assert not dist.is_initialized()
    blk = rowblock.RowBlock(NX, NY, 0, 2)
    with pytest.raises(ValueError, match="HaloExchanger has neither"):
        mk(blk=blk, exchanger=rowblock.HaloExchanger(blk), drifters=ok)
    core = mk(drifters=[[1.0, 1.0, 3.0], [5.0, 5.0, 0.0]], drifter_min_conc=0.3)
    assert core.drifters_read()["status"].tolist() == [3, 0] and core.drifter_min_conc == 0.3


# ---------------------------------------------------------------------------------------------------------------- the C++ host's keys
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    import subprocess

    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


GOOD = "# x y [status]\n100 200\n3.5e3 4e3 2\n\n480 7 8000 8000 0\n"
KEYS = ["--model.drifters_file=seeds.txt", "--model.drifters_output=track.txt"]


@pytest.mark.parametrize("step,seeds_txt,args,env,why", [
    ("DynamicsStep", GOOD, KEYS, {"WORLD_SIZE": "2", "RANK": "0"}, "model.drifters_file is set in a run of 2 processes"),
    ("DynamicsStep", GOOD, KEYS + ["--dynamics.loopback_world=3"], {}, "model.drifters_file is set with dynamics.loopback_world"),
    ("DynamicsStep", GOOD, KEYS[:1], {}, "model.drifters_output must name the file"),
    ("DynamicsStep", GOOD, KEYS[1:], {}, "model.drifters_output is set without model.drifters_file"),
    ("DynamicsStep", GOOD, KEYS + ["--model.drifters_period=100"], {}, "model.drifters_period = 100 s is no multiple of model.time_step = 120 s"),
    ("DynamicsStep", GOOD, KEYS + ["--model.drifters_period=-120"], {}, "model.drifters_period must not be negative"),
    ("DynamicsStep", GOOD, KEYS + ["--model.drifters_min_conc=nan"], {}, "\"nan\" of model.drifters_min_conc has the wrong type"),
    ("DynamicsStep", None, KEYS, {}, "model.drifters_file: cannot read seeds.txt"),
    ("DynamicsStep", "1 2\n3 four\n", KEYS, {}, "seeds.txt, line 2: \"four\" is not a number"),
    ("DynamicsStep", "1 2 0 0\n", KEYS, {}, "seeds.txt, line 1: 4 columns"),
    ("DynamicsStep", "1 2\n1 8000.5\n", KEYS, {}, "seeds.txt, line 2: the position is outside the domain"),
    ("DynamicsStep", "nan 2\n", KEYS, {}, "seeds.txt, line 1: the position is outside the domain"),
    ("DynamicsStep", "1 2 5\n", KEYS, {}, "seeds.txt, line 1: unknown status"),
    ("HipStep", GOOD, KEYS, {}, "Nextsim::HipStep has no ice velocity to move drifters with"),
], ids=["two_processes", "loopback", "no_output", "no_file", "period_no_multiple", "period_negative", "min_conc", "file_missing", "not_a_number",
        "four_columns", "outside", "nan_position", "status", "hipstep"])
def test_host_refuses_before_any_device(host_build, tmp_path, step, seeds_txt, args, env, why):
    """every refusal of the model.drifters_* keys comes from configure(): no device is asked for (there is none here), nothing is written"""
    import subprocess

    tmp = str(tmp_path)
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::%s\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 240\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 8000\n"
                % (step, os.path.join(tmp, "x.nsdg")))
    if seeds_txt is not None:
        with open(os.path.join(tmp, "seeds.txt"), "w") as f:
            f.write(seeds_txt)
    p = subprocess.run([os.path.join(host_build, "nextsim_amd"), "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, cwd=tmp, env=dict(os.environ, **env))
    out = p.stdout.decode()
    assert p.returncode != 0 and why in out and "no HIP device" not in out, out
    assert not [n for n in os.listdir(tmp) if n.startswith("track") or n.endswith(".nsdg")]


def test_host_accepts_a_good_file_and_then_asks_for_a_device(host_build, tmp_path):
    """the good file passes every check of configure(): what stops the run on a machine without a GPU is the device"""
    import subprocess

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    tmp = str(tmp_path)
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 240\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 8000\n" % os.path.join(tmp, "x.nsdg"))
    with open(os.path.join(tmp, "seeds.txt"), "w") as f:
        f.write(GOOD)
    p = subprocess.run([os.path.join(host_build, "nextsim_amd"), "--config-file", cfg] + KEYS + ["--model.drifters_period=240"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
    assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()

"""History output without a GPU (include/nsdg.h "history output"): the numpy statement of the samples
(tests/history_ref.py) held to known answers, the Python driver's history= on the oracle ops (one block == gloo worlds of 2 and 3, bit
for bit; a run without it is unchanged; what it refuses), the C ABI's host-only calls and checks, and the C++ host's output_tests."""
import ctypes as C
import os
import socket
import subprocess
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

import history_ref as R  # noqa: E402
from nextsimdg_amd import abi, build, rowblock, synthetic  # noqa: E402

NX, NY, NSUB, NSTEPS = 20, 29, 5, 3
DYN_FIELDS = ("hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s")
ALL_COUPLED = DYN_FIELDS + ("hsnow", "tice")


# ------------------------------------------------------------------------------------------------ a. the reference against known answers
def lattice(nx, ny, hx, hy):
    """coordinates of the CG2 nodes: node (gy, gx) sits at (gx hx / 2, gy hy / 2)"""
    x = 0.5 * hx * np.arange(2 * nx + 1)[None, :] * np.ones((2 * ny + 1, 1))
    y = 0.5 * hy * np.arange(2 * ny + 1)[:, None] * np.ones((1, 2 * nx + 1))
    return x, y


def test_rigid_rotation_has_no_divergence_and_no_shear():
    nx, ny, hx, hy, w = 7, 5, 512.0, 256.0, 2.0 ** -13  # powers of two: every product and quotient below is exact
    x, y = lattice(nx, ny, hx, hy)
    u, v = -w * (y - 300.0), w * (x - 100.0)
    for name in ("divergence", "shear"):
        assert np.all(R.sample(name, hx, hy, u=u, v=v) == 0.0), name
    want = np.hypot(R.centre(u), R.centre(v))
    assert np.allclose(R.sample("speed", hx, hy, u=u, v=v), want, rtol=4 * R.EPS, atol=0)


def test_linear_stretching_gives_a_plus_b_and_their_difference():
    nx, ny, hx, hy, a, b = 6, 4, 1024.0, 512.0, 3.0 * 2.0 ** -20, -1.0 * 2.0 ** -21
    x, y = lattice(nx, ny, hx, hy)
    u, v = a * x, b * y
    assert np.all(R.sample("divergence", hx, hy, u=u, v=v) == a + b)
    assert np.all(R.sample("shear", hx, hy, u=u, v=v) == abs(a - b))
    # a general cell size and rate: to rounding
    hx, hy, a, b = 1300.0, 700.0, 1.7e-6, 4.1e-7
    x, y = lattice(nx, ny, hx, hy)
    u, v = a * x + 0.3, b * y - 0.1
    scale = R.rounding_scale("divergence", hx, hy, u=u, v=v)
    assert np.max(np.abs(R.sample("divergence", hx, hy, u=u, v=v) - (a + b))) <= 16 * R.EPS * scale
    assert np.max(np.abs(R.sample("shear", hx, hy, u=u, v=v) - abs(a - b))) <= 16 * R.EPS * scale


def test_pure_shear_and_a_biquadratic_velocity():
    nx, ny, hx, hy, c = 5, 6, 512.0, 1024.0, 5.0 * 2.0 ** -22
    x, y = lattice(nx, ny, hx, hy)
    u, v = c * y, np.zeros_like(x)
    assert np.all(R.sample("divergence", hx, hy, u=u, v=v) == 0.0)
    assert np.all(R.sample("shear", hx, hy, u=u, v=v) == c)
    # the mid-edge differences are the EXACT derivatives of a biquadratic at the centre: u = x^2 y, v = x y^2 in units of the cell
    xs, ys = x / hx, y / hy
    u, v = xs * xs * ys, xs * ys * ys
    xc, yc = R.centre(xs), R.centre(ys)
    e11, e22, g = 2 * xc * yc / hx, 2 * xc * yc / hy, xc * xc / hy + yc * yc / hx
    scale = R.rounding_scale("shear", hx, hy, u=u, v=v)
    assert np.max(np.abs(R.sample("divergence", hx, hy, u=u, v=v) - (e11 + e22))) <= 16 * R.EPS * scale
    assert np.max(np.abs(R.sample("shear", hx, hy, u=u, v=v) - np.hypot(e11 - e22, g))) <= 16 * R.EPS * scale


def test_stress_invariants_and_copy_fields():
    rng = np.random.default_rng(3)
    s11, s12, s22 = (rng.standard_normal((8, 4, 9)) for _ in range(3))
    s11[0], s22[0], s12[0] = -3.0, -1.0, 0.0  # uniaxial: sigma_n = -2, sigma_s = 1
    assert np.all(R.sample("sigma_n", 1.0, 1.0, s11=s11, s22=s22) == -2.0)
    assert np.all(R.sample("sigma_s", 1.0, 1.0, s11=s11, s12=s12, s22=s22) == 1.0)
    s11[0], s22[0], s12[0] = 5.0, 5.0, 2.0  # isotropic + shear: sigma_s = |s12|
    assert np.all(R.sample("sigma_s", 1.0, 1.0, s11=s11, s12=s12, s22=s22) == 2.0)
    H = rng.standard_normal((6, 4, 9))
    u = rng.standard_normal((9, 19))
    assert np.array_equal(R.sample("hice", 1.0, 1.0, H=H), H[0]) and np.array_equal(R.sample("damage", 1.0, 1.0, D=H), H[0])
    assert np.array_equal(R.sample("u", 1.0, 1.0, u=u), u[1::2, 1::2]) and R.sample("u", 1.0, 1.0, u=u).shape == (4, 9)
    acc = np.full((1, 2, 9), np.nan)
    R.accumulate(acc, H[:1], 1, 3, True, row0=1)
    R.accumulate(acc, H[:1], 2, 3, False, row0=1)
    assert np.array_equal(acc[0, 0], H[0, 1]) and np.array_equal(acc[0, 1], H[0, 2] + H[0, 2])


# ------------------------------------------------------------------------------------------------ b. the C ABI on the host
@pytest.fixture(scope="module")
def lib():
    build.build_lib(verbose=False)
    return abi.load_library()


def test_field_names_and_ids_agree_with_the_binding(lib):
    assert abi.HISTORY_FIELDS == R.FIELDS
    for k, name in enumerate(abi.HISTORY_FIELDS):
        assert lib.nsdg_history_field_name(k) == name.encode() and lib.nsdg_history_field_id(name.encode()) == k
    assert lib.nsdg_history_field_name(len(abi.HISTORY_FIELDS)) is None and lib.nsdg_history_field_name(-1) is None
    assert lib.nsdg_history_field_id(b"thickness") == -1 and lib.nsdg_history_field_id(None) == -1 and lib.nsdg_history_field_id(b"") == -1
    assert [n for n, _ in abi.HistorySources._fields_] == list(abi.HISTORY_SOURCES)
    assert lib.nsdg_history_accumulate(None, 0, 0, 1, None, None, 1, 0, 0, None) == -1  # no context: an argument error, never a crash
    assert lib.nsdg_abi_version() == 6


# ------------------------------------------------------------------------------------------------ c. the driver on the oracle ops
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def column_fields_2d(seed=5):
    state, forcing, _ = synthetic.column_fields(NX * NY, seed)
    f = {k: v.reshape(NY, NX) for k, v in {**state, **forcing}.items()}
    f["wind"] = 0.2 * f["wind"]
    return f


def make_core(rank, world, history, coupled=False, ops=None, **kw):
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(41)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    blk = rowblock.RowBlock(NX, NY, rank, world)
    cls = rowblock.CoupledCore if coupled else rowblock.DynamicsCore
    ops = R.HistoryOps(alpha=200.0, beta=200.0) if ops is None else ops
    core = cls(ops, blk, bt.hx, bt.hy, 120.0, NSUB, torch.device("cpu"), history=history, **kw)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    if coupled:
        core.load_column(column_fields_2d())
    return core, bt


def worker(rank, world, port, outdir, history, coupled):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core, _ = make_core(rank, world, history, coupled)
        for _ in range(NSTEPS):
            core.step()
        torch.save(core.history_read(), os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single():
    """the one-block runs the tests below share: (core after NSTEPS steps, its record, the per-step states), dynamics and coupled"""
    out = {}
    for coupled, fields in ((False, DYN_FIELDS), (True, ALL_COUPLED)):
        core, bt = make_core(0, 1, fields, coupled)
        states = []
        for _ in range(NSTEPS):
            core.step()
            st = core.state_dict()
            if coupled:
                st["hsnow"], st["tice"] = core.col["hsnow"].numpy().copy(), core.col["tice0"].numpy().copy()
            states.append(st)
        out[coupled] = (core, core.history_read(reset=False), states, bt)
    return out


@pytest.mark.parametrize("coupled", [False, True])
def test_means_are_the_sequential_sum_of_the_per_step_samples(single, coupled):
    core, rec, states, bt = single[coupled]
    fields = ALL_COUPLED if coupled else DYN_FIELDS
    assert rec["count"] == NSTEPS and rec["rows"] == (0, NY) and set(rec) == {"rows", "count"} | set(fields)
    acc = np.full((len(fields), NY, NX), np.nan)
    for k, st in enumerate(states):
        x = R.samples(fields, bt.hx, bt.hy, H=st["H"], A=st["A"], u=st["u"], v=st["v"], s11=st["s11"], s12=st["s12"], s22=st["s22"],
                      hsnow=st.get("hsnow"), tice=st.get("tice"))
        R.accumulate(acc, x, 0, NY, k == 0)
    for k, name in enumerate(fields):
        assert rec[name].dtype == np.float64 and rec[name].shape == (NY, NX)
        assert np.array_equal(rec[name], acc[k] / NSTEPS), name
    assert np.max(np.abs(rec["speed"])) > 1e-5 and np.max(np.abs(rec["shear"])) > 0 and np.max(np.abs(rec["sigma_s"])) > 0


@pytest.mark.parametrize("world,coupled", [(2, False), (3, False), (2, True)])
def test_one_block_equals_gloo_worlds_bitwise(single, world, coupled, tmp_path):
    fields = ALL_COUPLED if coupled else DYN_FIELDS
    ref = single[coupled][1]
    mp.spawn(worker, args=(world, free_port(), str(tmp_path), fields, coupled), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r), weights_only=False) for r in range(world)]
    assert [p["rows"] for p in parts] == [rowblock.split_rows(NY, world, r) for r in range(world)]
    got = rowblock.DynamicsCore.merge_history(parts[::-1])
    assert got["rows"] == (0, NY) and got["count"] == NSTEPS
    for name in fields:
        assert np.array_equal(got[name], ref[name]), name


def test_history_none_leaves_the_run_unchanged(single):
    core, _ = make_core(0, 1, None)
    assert core.history is None and core._history is None
    for _ in range(NSTEPS):
        core.step()
    a, b = core.state_dict(), single[False][0].state_dict()
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    with pytest.raises(ValueError, match="history="):
        core.history_read()


def test_windows_reset_and_advance_samples_once():
    core, _ = make_core(0, 1, ("hice", "speed"))
    with pytest.raises(ValueError, match="no sample"):
        core.history_read()
    core._history.acc.fill_(float("nan"))  # the first sample of a window stores: what the accumulator held is dropped
    core.step()
    first = core.history_read()
    assert first["count"] == 1 and np.array_equal(first["hice"], core.H[0].numpy())
    assert core.advance(120.0, substeps=2) == 2  # two sub-steps, ONE sample, of the state after the last of them
    rec = core.history_read(reset=False)
    assert rec["count"] == 1 and np.array_equal(rec["hice"], core.H[0].numpy())
    core.step()
    assert core.history_read()["count"] == 2  # reset=False kept the window open


def test_construction_refuses_what_it_cannot_sample():
    from oracle_ops import OracleOps

    with pytest.raises(ValueError, match="unknown history field 'thickness'"):
        make_core(0, 1, ("hice", "thickness"))
    with pytest.raises(ValueError, match="'damage' needs rheology='bbm'"):
        make_core(0, 1, ("damage",))
    with pytest.raises(ValueError, match="'hsnow'.*needs a CoupledCore"):
        make_core(0, 1, ("hice", "hsnow"))
    with pytest.raises(ValueError, match="'tice'.*needs a CoupledCore"):
        make_core(0, 1, ("tice",))
    with pytest.raises(ValueError, match="OracleOps has no history_accumulate"):
        make_core(0, 1, ("hice",), ops=OracleOps(alpha=200.0, beta=200.0))
    with pytest.raises(ValueError, match="listed twice"):
        make_core(0, 1, ("hice", "u", "hice"))
    with pytest.raises(ValueError, match="at least one field"):
        make_core(0, 1, ())
    core, _ = make_core(0, 1, None, ops=OracleOps(alpha=200.0, beta=200.0))  # off: nothing is asked of the ops object
    core.step()
    with pytest.raises(ValueError, match="different numbers of samples"):
        rowblock.DynamicsCore.merge_history([{"rows": (0, 2), "count": 1}, {"rows": (2, 4), "count": 2}])
    with pytest.raises(ValueError, match="do not join"):
        rowblock.DynamicsCore.merge_history([{"rows": (0, 2), "count": 1}, {"rows": (3, 4), "count": 1}])


# ------------------------------------------------------------------------------------------------ d. the C++ host
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_output_tests_program(host_build, tmp_path):
    """host/test/output_tests.cpp: the window arithmetic, every refusal of configure(), both record formats read back, one flush"""
    p = subprocess.run([os.path.join(host_build, "output_tests"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "output tests:" in out and " 0 failures" in out, out


@pytest.mark.parametrize("step,args,why", [
    ("DynamicsStep", ["--model.output_period=500", "--model.output_file=ice.nsdg"], "not a whole multiple of model.time_step"),
    ("DynamicsStep", ["--model.output_period=240"], "model.output_file must name the record files"),
    ("DynamicsStep", ["--model.output_period=240", "--model.output_file=ice.nsdg", "--model.output_fields=hice,damage"], "brittle rheology"),
    ("DynamicsStep", ["--model.output_period=240", "--model.output_file=ice.nsdg", "--model.output_fields=tice"], "needs dynamics.thermodynamics"),
    ("HipStep", ["--model.output_period=240", "--model.output_file=ice.nsdg"], "Nextsim::HipStep writes no history output"),
])
def test_host_refuses_the_keys_before_any_device(host_build, tmp_path, step, args, why):
    tmp = str(tmp_path)
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::%s\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 240\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n" % (step, os.path.join(tmp, "x.nsdg")))
    p = subprocess.run([os.path.join(host_build, "nextsim_amd"), "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, cwd=tmp)
    out = p.stdout.decode()
    assert p.returncode != 0 and why in out and "no HIP device" not in out, out
    assert not [n for n in os.listdir(tmp) if n.startswith("ice.")]

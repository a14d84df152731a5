"""Forcing from a file (include/nsdg.h "forcing from a file") without a GPU: the numpy restatement of the sampling rule held to closed-form
cases, the C++ reader and converter (host/test/forcing_tests.cpp), the host's refusal of a missing file before any device is touched, and
the Python driver's ForcingSeries over gloo with the oracle in place of the kernels."""
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

import forcing_file_ref as R  # noqa: E402
from nextsimdg_amd import build, rowblock, synthetic  # noqa: E402

HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


# ---- the sampling rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["nodes", "elements"])
def test_constant_fields_come_out_exactly_constant(where):
    for nyr, nxr in ((1, 1), (3, 7), (23, 37), (300, 200)):
        for c in (-1.0, 311.0, 1e5, 2.5e-7):
            rec = np.full((nyr, nxr), c)
            for nx, ny, row0, nyg in ((16, 12, 0, 12), (37, 9, 5, 23)):
                out = R.sample(rec, where, nx, ny, row0, nyg)
                assert np.all(out == c)
                assert out.shape == ((2 * ny + 1, 2 * nx + 1) if where == "nodes" else (ny, nx))


def test_linear_field_is_reproduced_inside_the_lattice():
    """a field linear in x and y is reproduced wherever a target lies between lattice points; outside it is the edge value (clamping)"""
    nx, ny, nxr, nyr = 48, 40, 7, 5
    a, b, c = 0.25, -0.75, 3.0
    i, j = np.arange(nxr, dtype=np.float64), np.arange(nyr, dtype=np.float64)
    rec = a * i[None, :] + b * j[:, None] + c  # a linear function of the index-space coordinate
    for where in ("nodes", "elements"):
        out = R.sample(rec, where, nx, ny)
        if where == "nodes":
            sx = (np.arange(2 * nx + 1) * nxr - nx) / (2.0 * nx)
            sy = (np.arange(2 * ny + 1) * nyr - ny) / (2.0 * ny)
        else:
            sx = ((2 * np.arange(nx) + 1) * nxr - nx) / (2.0 * nx)
            sy = ((2 * np.arange(ny) + 1) * nyr - ny) / (2.0 * ny)
        want = a * np.clip(sx, 0, nxr - 1)[None, :] + b * np.clip(sy, 0, nyr - 1)[:, None] + c
        assert np.max(np.abs(out - want)) <= 1e-14 * np.max(np.abs(want))
        inside = ((sx > 0) & (sx < nxr - 1))[None, :] & ((sy > 0) & (sy < nyr - 1))[:, None]
        assert inside.sum() > 0.5 * inside.size


def test_clamping_at_all_four_edges():
    """targets outside the first / last lattice point take the edge point with weight 0: the outer bands are the 1-d samples of the
    edge rows and columns, and the corners are the corner values, bit for bit"""
    rng = np.random.default_rng(9)
    nyr, nxr, nx, ny = 3, 4, 40, 30
    rec = rng.standard_normal((nyr, nxr))
    out = R.sample(rec, "nodes", nx, ny)
    # node gx: num = 4 gx - 40 <= 0 for gx <= 10, >= 3 * 80 for gx >= 70; node gy: 3 gy - 30 <= 0 for gy <= 10, >= 2 * 60 for gy >= 50
    left, right = R.sample(rec[:, :1], "nodes", nx, ny)[:, 0], R.sample(rec[:, -1:], "nodes", nx, ny)[:, 0]
    bottom, top = R.sample(rec[:1, :], "nodes", nx, ny)[0], R.sample(rec[-1:, :], "nodes", nx, ny)[0]
    for gx in range(0, 11):
        assert np.array_equal(out[:, gx], left)
    for gx in range(70, 81):
        assert np.array_equal(out[:, gx], right)
    for gy in range(0, 11):
        assert np.array_equal(out[gy], bottom)
    for gy in range(50, 61):
        assert np.array_equal(out[gy], top)
    assert not np.array_equal(out[:, 11], left) and not np.array_equal(out[11], bottom)  # the bands end where the lattice begins
    assert (out[0, 0], out[0, -1], out[-1, 0], out[-1, -1]) == (rec[0, 0], rec[0, -1], rec[-1, 0], rec[-1, -1])
    el = R.sample(rec, "elements", nx, ny)  # element ix: num = 4 (2 ix + 1) - 40 <= 0 for ix <= 4
    assert (el[0, 0], el[-1, -1]) == (rec[0, 0], rec[-1, -1]) and np.all(el[:, :5] == el[:, :1])


def test_coincident_lattice_is_the_identity_and_one_point_is_constant():
    rng = np.random.default_rng(3)
    nx, ny = 29, 17
    rec = rng.standard_normal((ny, nx))
    assert np.array_equal(R.sample(rec, "elements", nx, ny), rec)  # bit for bit
    # a row block of the coincident lattice is its rows
    assert np.array_equal(R.sample(rec, "elements", nx, 6, row0=4, ny_global=ny), rec[4:10])
    # nxr = 1: constant along x; nyr = 1: constant along y
    col = rng.standard_normal((5, 1))
    out = R.sample(col, "nodes", 12, 10)
    assert np.all(out == out[:, :1])
    row = rng.standard_normal((1, 6))
    out = R.sample(row, "elements", 12, 10)
    assert np.all(out == out[:1, :])
    assert np.all(R.sample(np.array([[4.5]]), "nodes", 3, 2) == 4.5)


def test_time_weight_and_row_blocks():
    rng = np.random.default_rng(5)
    r0, r1 = rng.standard_normal((9, 11)), rng.standard_normal((9, 11))
    nx, ny = 40, 30
    full0 = R.forcing_sample("nodes", [r0], [r1], 0.0, nx, ny)[0]
    assert np.array_equal(full0, R.sample(r0, "nodes", nx, ny))  # w = 0 is rec0's sample, bit for bit
    full1 = R.forcing_sample("nodes", [r0], [r1], 1.0, nx, ny)[0]
    assert np.max(np.abs(full1 - R.sample(r1, "nodes", nx, ny))) <= 1e-15 * np.max(np.abs(r1)) * 4
    mid = R.forcing_sample("elements", [r0], [r1], 0.3, nx, ny)[0]
    assert np.max(np.abs(mid - (0.7 * R.sample(r0, "elements", nx, ny) + 0.3 * R.sample(r1, "elements", nx, ny)))) <= 1e-14 * 4
    # a row block (ghost rows included) computes the global result's rows, bit for bit
    for lo, hi in ((0, 9), (7, 19), (21, 30)):
        blk = R.forcing_sample("nodes", [r0], [r1], 0.3, nx, hi - lo, lo, ny)[0]
        assert np.array_equal(blk, R.forcing_sample("nodes", [r0], [r1], 0.3, nx, ny)[0][2 * lo:2 * hi + 1])
        blk = R.forcing_sample("elements", [r0], [r1], 0.3, nx, hi - lo, lo, ny)[0]
        assert np.array_equal(blk, mid[lo:hi])


def test_bracket():
    t = [0.0, 3600.0, 7200.0]
    assert R.bracket(t, 0.0) == (0, 1, 0.0)
    assert R.bracket(t, 1800.0) == (0, 1, 0.5)
    assert R.bracket(t, 3600.0) == (1, 2, 0.0)
    assert R.bracket(t, 7200.0) == (2, 2, 0.0)
    for bad in (-1.0, 7200.5):
        with pytest.raises(ValueError, match="outside the forcing records"):
            R.bracket(t, bad)
    s = rowblock.ForcingSeries(t, {"wind_u": np.zeros((3, 2, 2)), "wind_v": np.zeros((3, 2, 2))})
    for x in (0.0, 1800.0, 3600.0, 5000.0, 7200.0):
        assert s.bracket(x) == R.bracket(t, x)
    with pytest.raises(ValueError, match="outside the forcing records"):
        s.bracket(-0.5)


def test_forcing_series_checks_its_input():
    z = lambda nt=2, a=3, b=4: np.zeros((nt, a, b))
    with pytest.raises(ValueError, match="strictly increasing"):
        rowblock.ForcingSeries([0.0, 0.0], {"tair": z()})
    with pytest.raises(ValueError, match="come as a pair"):
        rowblock.ForcingSeries([0.0, 1.0], {"wind_u": z()})
    with pytest.raises(ValueError, match="one lattice"):
        rowblock.ForcingSeries([0.0, 1.0], {"wind_u": z(), "wind_v": z(2, 3, 5)})
    with pytest.raises(ValueError, match="shape"):
        rowblock.ForcingSeries([0.0, 1.0], {"tair": z(3)})
    with pytest.raises(ValueError, match="unknown forcing field"):
        rowblock.ForcingSeries([0.0, 1.0], {"Tair": z()})
    bad = z()
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite value in record 1"):
        rowblock.ForcingSeries([0.0, 1.0], {"tair": bad})


# ---- the C++ reader and converter; the host refuses a missing file -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_build():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_forcing_tests_program(host_build):
    p = subprocess.run([os.path.join(host_build, "forcing_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "forcing tests:" in out and " 0 failures" in out, out


def host_config(tmp, dynamics):
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\n%s"
                % (os.path.join(tmp, "x.nsdg"), dynamics))
    return cfg


def test_host_refuses_a_missing_forcing_file_before_any_device(host_build, tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(host_build, "nextsim_amd")
    missing = os.path.join(tmp, "no_forcing_here.nc")
    cfg = host_config(tmp, "thermodynamics = true\n")
    for args in (["--dynamics.forcing=file", "--dynamics.forcing_file=" + missing],):
        p = subprocess.run([exe, "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        out = p.stdout.decode()
        assert p.returncode != 0 and missing in out and "no HIP device" not in out, out
    p = subprocess.run([exe, "--config-file", cfg, "--dynamics.forcing=file"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
    assert p.returncode != 0 and "dynamics.forcing = file needs dynamics.forcing_file" in p.stdout.decode()
    p = subprocess.run([exe, "--config-file", cfg, "--dynamics.forcing=files"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
    assert p.returncode != 0 and "dynamics.forcing must be host, dummy, winter or file" in p.stdout.decode()
    # a file without the column variables that thermodynamics needs, made by make_forcing: refused, naming the file and the variable
    np.save(os.path.join(tmp, "t.npy"), np.array([0.0, 3600.0]))
    np.save(os.path.join(tmp, "u.npy"), np.ones((2, 3, 3)))
    made = os.path.join(tmp, "wind.nc")
    subprocess.check_call([os.path.join(host_build, "make_forcing"), "--out", made, "--time", os.path.join(tmp, "t.npy"),
                           "wind_u=" + os.path.join(tmp, "u.npy"), "wind_v=" + os.path.join(tmp, "u.npy")], stdout=subprocess.DEVNULL)
    p = subprocess.run([exe, "--config-file", cfg, "--dynamics.forcing=file", "--dynamics.forcing_file=" + made], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
    out = p.stdout.decode()
    assert p.returncode != 0 and made in out and "no variable tair" in out and "no HIP device" not in out, out


# ---- the Python driver over gloo ------------------------------------------------------------------------------------------------------
NX, NY, NSUB, DT = 20, 29, 6, 600.0


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def forcing_ops():
    from oracle_ops import OracleOps

    class ForcingOps(OracleOps):
        """the oracle plus the numpy restatements of nsdg_block_set, nsdg_forcing_sample and nsdg_column_wind"""

        row0, ny_glob = 0, None

        def set_block(self, row0, ny_global):
            self.row0, self.ny_glob = row0, ny_global

        def forcing_sample(self, where, rec0, rec1, w, out):
            res = R.forcing_sample(where, [r.numpy() for r in rec0], [r.numpy() for r in rec1], w, self.nx, self.ny, self.row0, self.ny_glob)
            for o, r in zip(out, res):
                o.numpy()[:] = r

        def column_wind(self, ua, va, wind):
            u, v = ua.numpy()[1::2, 1::2], va.numpy()[1::2, 1::2]
            wind.numpy()[:] = np.sqrt(u * u + v * v)

    return ForcingOps(mevp_variant=4, alpha=200.0, beta=200.0)


def series():
    """hourly records on a coarse 7 x 5 lattice, varying in space and time: wind, ocean and the column planes"""
    rng = np.random.default_rng(11)
    nt, nyr, nxr = 4, 5, 7
    t = 3600.0 * np.arange(nt) - 1800.0
    base = {"tair": (-12.0, 4.0), "tdew": (-14.0, 3.0), "slp": (1.0e5, 800.0), "qsw": (60.0, 40.0), "qlw": (250.0, 30.0),
            "mld": (20.0, 5.0), "snowfall": (2e-5, 1e-5), "wind_u": (0.0, 12.0), "wind_v": (0.0, 12.0), "ocean_u": (0.0, 0.05),
            "ocean_v": (0.0, 0.05)}
    fields = {k: m + s * rng.uniform(-1, 1, (nt, nyr, nxr)) for k, (m, s) in base.items()}
    fields["qsw"] = np.abs(fields["qsw"])
    fields["snowfall"] = np.abs(fields["snowfall"])
    return rowblock.ForcingSeries(t, fields)


def column_fields():
    c = {k: np.zeros((NY, NX)) for k in rowblock.CoupledCore.COLUMN_STATE + rowblock.CoupledCore.COLUMN_FORCING}
    c["hsnow"][:] = 0.05
    c["tice0"][:] = -8.0
    c["sst"][:] = -1.76
    c["sss"][:] = 32.0
    return c


def run(rank, world, steps=4):
    bt = synthetic.BoxTest(NX, NY)
    H, A = bt.dg_fields()
    blk = rowblock.RowBlock(NX, NY, rank, world, 4, 3)
    core = rowblock.CoupledCore(forcing_ops(), blk, bt.hx, bt.hy, DT, NSUB, torch.device("cpu"), forcing=series())
    z = np.zeros((2 * NY + 1, 2 * NX + 1))
    core.load_global(H, A, z, z, z, z)
    core.load_column(column_fields())
    core.time = -1800.0
    for _ in range(steps):
        core.step()
    return core


def worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = run(rank, world)
        out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v", "ua", "uo")}
        out["hsnow"] = core.col["hsnow"][core.blk.j0:core.blk.j1].clone()
        torch.save(out, os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_forcing_series_world_two_equals_world_one_bitwise(tmp_path):
    """a time-varying ForcingSeries (records crossed during the run, the wind, the ocean and the column planes from the file) gives the
    same result on two gloo ranks as on one, byte for byte"""
    ref = run(0, 1)
    assert float(ref.u.abs().max()) > 1e-5
    # the series reached the fields: the wind is that of the last step's time, not the box test's
    s = series()
    k0, k1, w = s.bracket(ref.time - DT)
    want = R.forcing_sample("nodes", [s.fields["wind_u"][k0]], [s.fields["wind_u"][k1]], w, NX, NY)[0]
    assert np.array_equal(ref.ua.numpy(), want) and 0 < w < 1
    mp.spawn(worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(2)]
    for key in ("H", "A"):
        assert torch.equal(torch.cat([p[key] for p in parts], dim=1), getattr(ref, key)), key
    for key in ("u", "v", "ua", "uo"):
        assert torch.equal(torch.cat([p[key] for p in parts], dim=0), getattr(ref, key)), key
    assert torch.equal(torch.cat([p["hsnow"] for p in parts], dim=0), ref.col["hsnow"])


def test_coupled_core_needs_the_column_variables():
    s = rowblock.ForcingSeries([0.0, 1.0], {"wind_u": np.zeros((2, 3, 3)), "wind_v": np.zeros((2, 3, 3))})
    bt = synthetic.BoxTest(NX, NY)
    with pytest.raises(ValueError, match="tair, tdew, slp, qsw, qlw, mld, snowfall"):
        rowblock.CoupledCore(forcing_ops(), rowblock.RowBlock(NX, NY), bt.hx, bt.hy, DT, NSUB, torch.device("cpu"), forcing=s)

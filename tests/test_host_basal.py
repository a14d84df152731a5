"""The C++ host's landfast ice (host/include/BathymetryFile.hpp): dynamics.bathymetry_file and the [basal] section.
Without a device: the host's own test program (file checks, keys) and the binary's refusal of bad files before it asks for a device.
On the device: a 128 x 96 box under a loose 3 m cover (A = 0.8: little strength, so the pack moves; T_b = 15 * 2.5 * exp(-4) = 0.69 N m^-2
over the shoal, above a |tau_a| of the box test's cyclone) with a 5 m shoal inside 1000 m of water, an island cutting into the shoal -- 1 row block
against 4 and N steps against N/2 + restart + N/2, the restart files equal byte for byte, both rheologies; and the shoal keeps its ice
below the landfast criterion of Lemieux et al. (2015), 5e-4 m/s, while the deep water beside it moves faster (the box test's wind
does not drive the pack past 5e-4 m/s itself in so short a run: the criterion does not discriminate here, see the test)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import basal_ref as BR
import land_ref
from nextsimdg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST = 128, 96  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
DT, STEPS, NSUB = 120, 8, 24
INIT = "hice = 3.0\ncice = 0.8\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"
LANDFAST = 5e-4  # m/s


@pytest.fixture(scope="module")
def host_dir():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_basal_program(host_dir):
    """the depth file's checks, land stored as 0, the [basal] keys: needs no device"""
    p = subprocess.run([os.path.join(host_dir, "basal_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and re.search(r"host basal tests: \d+ checks, 0 failures", out), out


def test_host_refuses_bad_depth_files_before_any_device(host_dir, tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(host_dir, "nextsim_amd")
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 6\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\nnsub = 4\n" % os.path.join(tmp, "x.nsdg"))
    good = np.full((6, 8), 200.0)
    good[2:4, 3:5] = 8.0
    neg, nan = good.copy(), good.copy()
    neg[2, 3], neg[4, 1] = -3.0, -1.0
    nan[5, 7] = np.nan
    files = {
        "missing.npy": (None, "cannot open"),
        "shape.npy": (np.zeros((8, 6)), "the depth has the shape (8, 6)"),
        "flat.npy": (np.zeros(48), "two-dimensional"),
        "dtype.npy": (good.astype(np.float32), "dtype.npy"),
        "negative.npy": (neg, "value -3 at (2, 3)"),
        "nan.npy": (nan, "at (5, 7)"),
    }
    for name, (a, needle) in files.items():
        path = os.path.join(tmp, name)
        if a is not None:
            np.save(path, a)
        p = subprocess.run([exe, "--config-file", cfg, "--dynamics.bathymetry_file=" + path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=120, cwd=tmp)
        out = p.stdout.decode()
        assert p.returncode != 0 and "dynamics.bathymetry_file" in out and path in out and needle in out, (name, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(tmp, "x.nsdg")), (name, out)
    path = os.path.join(tmp, "good.npy")
    np.save(path, good)
    for args, needle in ((["--basal.k1=0"], "[basal]: basal.k1"), (["--basal.u0=-1"], "[basal]: basal.u0")):
        p = subprocess.run([exe, "--config-file", cfg, "--dynamics.bathymetry_file=" + path] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=120, cwd=tmp)
        assert p.returncode != 0 and needle in p.stdout.decode() and "no HIP device" not in p.stdout.decode(), p.stdout.decode()
    p = subprocess.run([exe, "--config-file", cfg, "--basal.k2=10"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
    assert p.returncode != 0 and "need dynamics.bathymetry_file" in p.stdout.decode(), p.stdout.decode()
    if not torch.cuda.is_available():  # a good file passes every check: the run gets as far as asking for a device
        p = subprocess.run([exe, "--config-file", cfg, "--dynamics.bathymetry_file=" + path, "--basal.k2=10"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()


def mask():
    m = np.zeros((NSLOW, NFAST), dtype=bool)  # [slow, fast]
    m[60:70, 40:46] = True  # an island that cuts into the shoal, across the boundary of the row blocks at row 64
    return m


def depth():
    """a 5 m shoal across the boundaries of four row blocks (rows 32, 64, 96) and the column seams of the passes (57, 63, 64)"""
    return BR.shoal_depth(NFAST, NSLOW, shallow=5.0, box=(20, 110, 30, 75))  # [slow, fast]


@pytest.fixture(scope="module")
def runs(host_dir, tmp_path_factory):
    """run(name, ...) -> (restart bytes, stdout, directory); every configuration runs once per module"""
    base, done = str(tmp_path_factory.mktemp("basal")), {}

    def run(name, dynamics="", start=0, stop=DT * STEPS, init_file=None, bathymetry=True):
        if name in done:
            return done[name]
        tmp = os.path.join(base, name)
        os.makedirs(tmp)
        final, cfg = os.path.join(tmp, "final.nsdg"), os.path.join(tmp, "run.cfg")
        np.save(os.path.join(tmp, "land.npy"), mask())
        np.save(os.path.join(tmp, "depth.npy"), depth()[0])
        with open(cfg, "w") as f:
            f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %d\nstart = %d\nstop = %d\n"
                    "final_file = %s\n%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = 256e3\nland_mask_file = land.npy\n%s%s"
                    % (DT, start, stop, final, ("init_file = %s\n" % init_file) if init_file else "", NSLOW, NFAST, INIT,
                       "bathymetry_file = depth.npy\n" if bathymetry else "", dynamics))
        p = subprocess.run([os.path.join(host_dir, "nextsim_amd"), "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        with open(final, "rb") as f:
            done[name] = (f.read(), p.stdout.decode(), tmp)
        return done[name]

    return run


def velocity(raw):
    """u, v [2X+1, 2Y+1] of the restart file (RectGrid::dump, the .nsdg form)"""
    head, body = raw.split(b"END-HEADER\n", 1)
    keys = dict(line.split("=", 1) for line in head.decode().splitlines() if "=" in line)
    X, Y, NL = int(keys["data.x"]), int(keys["data.y"]), int(keys["data.nLayers"])
    assert (X, Y) == (NSLOW, NFAST) and keys.get("data.dynamics") == "1"
    a = np.frombuffer(body, dtype=np.float64)
    n, nn = X * Y, (2 * X + 1) * (2 * Y + 1)
    sizes = {"hice": n, "cice": n, "hsnow": n, "sst": n, "sss": n, "tice": n * NL, "hice_dg": 5 * n, "cice_dg": 5 * n, "u": nn, "v": nn, "s11": 8 * n,
             "s12": 8 * n, "s22": 8 * n, "newice": n, "damage": 6 * n}
    out, at = {}, 0
    for name in keys["variables"].split(","):
        out[name] = a[at:at + sizes[name]]
        at += sizes[name]
    assert at == a.size and "depth" not in keys["variables"] and "bathymetry" not in keys["variables"]  # the depth is configuration
    return out["u"].reshape(2 * X + 1, 2 * Y + 1), out["v"].reshape(2 * X + 1, 2 * Y + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mevp", "bbm"])
def test_one_row_block_equals_four_a_restarted_run_is_the_whole_run_and_the_shoal_is_landfast(runs, gpu, kind):
    # (the brittle run takes its sub-iteration count from the elastic-wave rule, and the weaker cohesion of tests/test_host_bbm.py)
    dyn = "rheology = bbm\n" if kind == "bbm" else "nsub = %d\n" % NSUB
    tail = "[bbm]\ncohesion_lab = 1e5\n" if kind == "bbm" else ""
    whole, out, _ = runs("whole_" + kind, dyn + tail)
    assert "dynamics bathymetry: the shallowest ocean element has 5 m of water; k1 = 8, k2 = 15 N m^-3, alpha_b = 20, u0 = 5e-05 m/s" in out, out
    assert runs("four_" + kind, dyn + "row_blocks = 4\n" + tail)[0] == whole
    _, _, tmp = runs("first_" + kind, dyn + tail, stop=DT * STEPS // 2)
    second, _, _ = runs("second_" + kind, dyn + "row_blocks = 4\n" + tail, start=DT * STEPS // 2, init_file=os.path.join(tmp, "final.nsdg"))
    assert second == whole
    # the landfast criterion: the ice over the shoal stays below 5e-4 m/s while the deep water beside it moves
    u, v = velocity(whole)
    speed = np.hypot(u, v)
    m, (_, shoal) = mask(), depth()
    ln = land_ref.land_nodes(m)
    fast = BR.shoal_nodes(shoal) & ~ln
    deep = ~land_ref.land_nodes(shoal) & ~ln
    deep[[0, -1]] = deep[:, [0, -1]] = False
    free, _, _ = runs("free_" + kind, dyn + tail, bathymetry=False)
    uf, vf = velocity(free)
    print("%s after %d steps: largest speed over the shoal %.3g m/s (without the depth file %.3g), in deep water %.3g" % (
        kind, STEPS, speed[fast].max(), np.hypot(uf, vf)[fast].max(), speed[deep].max()))
    assert np.all(np.isfinite(speed)) and fast.sum() > 5000
    # Under the box test's own wind the pack reaches ~1.3e-4 m/s in deep water in these 16 minutes (1.9e-5 over the shoal): nothing in this
    # run passes 5e-4 m/s, so the criterion itself does not tell the shoal from the deep water here.  Asserted: the shoal under the
    # criterion, and slower than the deep water beside it and than the same ice without the depth file.  A case whose deep water passes
    # 5e-4 m/s needs a stronger wind than the host's box test has (a forcing file): not built.
    assert speed[fast].max() < LANDFAST
    assert speed[deep].max() > speed[fast].max()
    assert np.hypot(uf, vf)[fast].max() > speed[fast].max()  # without the depth file the same ice moves faster
    # other parameters reach the run: no basal stress at k2 = 0 is the run without the file
    if kind == "mevp":
        off, _, _ = runs("k2_zero", dyn + "[basal]\nk2 = 0\n")
        assert np.array_equal(velocity(off)[0], uf)

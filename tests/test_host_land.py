"""The C++ host's dynamics.land_mask_file (host/include/LandMaskFile.hpp) on the device: a 128 x 96 box with an island, a coast with a
bay and a rock, 1 row block against 4 -- the restart files are equal byte for byte, and the land entries of hice, cice, u and v in the
file are 0; the same with the column thermodynamics."""
import os
import subprocess

import numpy as np
import pytest

import land_ref
from nextsimdg_amd import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST = 128, 96  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
INIT = "hice = 0.3\ncice = 0.9\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"


@pytest.fixture(scope="module")
def host(gpu):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "nextsim_amd")


def mask():
    m = land_ref.shapes_mask(NFAST, NSLOW)  # [slow, fast]
    m[20:110, 40:46] = True  # an island across the boundaries of four row blocks (rows 32, 64, 96)
    m[64, 10] = True
    return m


def run_host(host, tmp, name, mask_file, dynamics=""):
    final = os.path.join(tmp, name + ".nsdg")
    cfg = os.path.join(tmp, name + ".cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 480\n"
                "final_file = %s\n[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = 256e3\nnsub = 24\n%s%s"
                % (final, NSLOW, NFAST, INIT, ("land_mask_file = %s\n" % mask_file) if mask_file else "", dynamics))
    p = subprocess.run([host, "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    with open(final, "rb") as f:
        return f.read(), out


def planes(raw):
    """the restart file (RectGrid::dump, the .nsdg form): {name: array} of hice, cice, hsnow, u, v, newice"""
    head, body = raw.split(b"END-HEADER\n", 1)
    keys = dict(line.split("=", 1) for line in head.decode().splitlines() if "=" in line)
    X, Y, L = int(keys["data.x"]), int(keys["data.y"]), int(keys["data.nLayers"])
    assert (X, Y) == (NSLOW, NFAST) and keys.get("data.dynamics") == "1"
    a = np.frombuffer(body, dtype=np.float64)
    n, nn = X * Y, (2 * X + 1) * (2 * Y + 1)
    out, at = {}, 0
    for name, count, shape in (("hice", n, (X, Y)), ("cice", n, (X, Y)), ("hsnow", n, (X, Y)), ("sst", n, (X, Y)), ("sss", n, (X, Y)), ("tice", n * L, (X, Y, L)),
                               ("hice_dg", 5 * n, (5, X, Y)), ("cice_dg", 5 * n, (5, X, Y)), ("u", nn, (2 * X + 1, 2 * Y + 1)), ("v", nn, (2 * X + 1, 2 * Y + 1)),
                               ("s11", 8 * n, (8, X, Y)), ("s12", 8 * n, (8, X, Y)), ("s22", 8 * n, (8, X, Y)), ("newice", n, (X, Y))):
        out[name] = a[at:at + count].reshape(shape)
        at += count
    assert at == a.size
    return out


@pytest.mark.parametrize("thermo", [False, True])
def test_one_row_block_equals_four_and_land_is_zero_in_the_restart_file(host, tmp_path, thermo):
    tmp = str(tmp_path)
    m = mask()
    path = os.path.join(tmp, "land.npy")
    np.save(path, m.astype(np.uint8))
    dyn = "thermodynamics = true\nforcing = winter\n" if thermo else ""
    one, out = run_host(host, tmp, "one", path, dyn)
    assert "dynamics land mask: %d of %d elements are land" % (m.sum(), m.size) in out, out
    four, _ = run_host(host, tmp, "four", path, dyn + "row_blocks = 4\n")
    assert four == one
    np.save(path, m)  # a bool file is the same mask
    assert run_host(host, tmp, "bool", path, dyn)[0] == one
    f = planes(one)
    ln = land_ref.land_nodes(m)
    for k in ("hice", "cice", "newice") + (("hsnow",) if thermo else ()):
        assert np.all(f[k][m] == 0.0), k
    for k in ("hice_dg", "cice_dg", "s11", "s12", "s22"):
        assert np.all(f[k][:, m] == 0.0), k
    for k in ("u", "v"):
        assert np.all(f[k][ln] == 0.0), k
        assert np.all(np.isfinite(f[k])) and np.max(np.abs(f[k])) > 1e-4, k
    assert np.all(f["hice"][~m] > 0.0)
    plain, _ = run_host(host, tmp, "plain", None, dyn)  # the mask changes the run
    assert plain != one

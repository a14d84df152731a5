"""The C++ host's snow load (host/include/DynamicsStep.hpp "dynamics.snow_load", "dynamics.rho_snow").
Without a device: the host's own test program (keys and refusals) and the binary's refusals before it asks for a device.
On the device: the 128 x 96 box of tests/test_host_basal.py with thermodynamics and 0.3 m of snow -- 1 row block against 4, N steps
against N/2 + restart + N/2 and rho_snow = 0 against a run without snow_load, the restart files equal byte for byte; and the load moves
u, v.  Once with the plane hsnow, once with the DG field S of dynamics.advect_column_state, once with the brittle rheology."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nextsimdg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST = 128, 96  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
DT, STEPS, NSUB = 120, 4, 24
INIT = "hice = 1.0\ncice = 0.9\nsst = -1.76\nhsnow = 0.3\ntice = -8\n"
MODES = {"plane": "nsub = %d\n" % NSUB, "S": "nsub = %d\nadvect_column_state = true\n" % NSUB, "bbm": "rheology = bbm\n"}


@pytest.fixture(scope="module")
def host_dir():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_snow_program(host_dir):
    """the keys, their defaults and their refusals: needs no device"""
    p = subprocess.run([os.path.join(host_dir, "snow_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and re.search(r"host snow tests: \d+ checks, 0 failures", out), out


def test_host_refuses_bad_snow_keys_before_any_device(host_dir, tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(host_dir, "nextsim_amd")
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 6\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\nhsnow = 0.1\n[dynamics]\nnsub = 4\n" % os.path.join(tmp, "x.nsdg"))
    thermo = "--dynamics.thermodynamics=true"
    cases = (
        (["--dynamics.snow_load=true"], "dynamics.snow_load needs dynamics.thermodynamics = true"),
        (["--dynamics.snow_load=true", "--dynamics.thermodynamics=false"], "dynamics.snow_load needs dynamics.thermodynamics = true"),
        ([thermo, "--dynamics.snow_load=true", "--dynamics.rho_snow=-5"], "dynamics.rho_snow = -5"),
        ([thermo, "--dynamics.rho_snow=330"], "dynamics.rho_snow needs dynamics.snow_load = true"),
        ([thermo, "--dynamics.snow_load=false", "--dynamics.rho_snow=100"], "dynamics.rho_snow needs dynamics.snow_load = true"),
    )
    for args, needle in cases:
        p = subprocess.run([exe, "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        out = p.stdout.decode()
        assert p.returncode != 0 and needle in out, (args, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(tmp, "x.nsdg")), (args, out)
    if not torch.cuda.is_available():  # good keys pass every check: the run gets as far as asking for a device
        p = subprocess.run([exe, "--config-file", cfg, thermo, "--dynamics.snow_load=true", "--dynamics.rho_snow=300"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()


@pytest.fixture(scope="module")
def runs(host_dir, tmp_path_factory):
    """run(name, ...) -> (restart bytes, stdout, directory); every configuration runs once per module"""
    base, done = str(tmp_path_factory.mktemp("snow")), {}

    def run(name, dynamics="", start=0, stop=DT * STEPS, init_file=None):
        if name in done:
            return done[name]
        tmp = os.path.join(base, name)
        os.makedirs(tmp)
        final, cfg = os.path.join(tmp, "final.nsdg"), os.path.join(tmp, "run.cfg")
        with open(cfg, "w") as f:
            f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %d\nstart = %d\nstop = %d\n"
                    "final_file = %s\n%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = 256e3\nthermodynamics = true\n%s"
                    % (DT, start, stop, final, ("init_file = %s\n" % init_file) if init_file else "", NSLOW, NFAST, INIT, dynamics))
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
    sizes = {"hice": n, "cice": n, "hsnow": n, "sst": n, "sss": n, "tice": n * NL, "hice_dg": 5 * n, "cice_dg": 5 * n, "hsnow_dg": 5 * n, "u": nn,
             "v": nn, "s11": 8 * n, "s12": 8 * n, "s22": 8 * n, "newice": n, "damage": 6 * n}
    out, at = {}, 0
    for name in keys["variables"].split(","):
        out[name] = a[at:at + sizes[name]]
        at += sizes[name]
    assert at == a.size  # the restart file holds nothing new: the snow was in it already
    return out["u"].reshape(2 * X + 1, 2 * Y + 1), out["v"].reshape(2 * X + 1, 2 * Y + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_one_row_block_equals_four_a_restarted_run_is_the_whole_run_and_the_load_moves_the_ice(runs, gpu, mode):
    # (the brittle run takes its sub-iteration count from the elastic-wave rule, and the weaker cohesion of tests/test_host_bbm.py)
    tail = "[bbm]\ncohesion_lab = 1e5\n" if mode == "bbm" else ""
    dyn = MODES[mode]
    load = dyn + "snow_load = true\n"
    whole, _, _ = runs("whole_" + mode, load + tail)
    assert runs("four_" + mode, load + "row_blocks = 4\n" + tail)[0] == whole
    _, _, tmp = runs("first_" + mode, load + tail, stop=DT * STEPS // 2)
    second, _, _ = runs("second_" + mode, load + "row_blocks = 4\n" + tail, start=DT * STEPS // 2, init_file=os.path.join(tmp, "final.nsdg"))
    assert second == whole
    bare, _, _ = runs("bare_" + mode, dyn + tail)
    assert runs("weightless_" + mode, load + "rho_snow = 0\n" + tail)[0] == bare
    (u, v), (ub, vb) = velocity(whole), velocity(bare)
    print("%s after %d steps: largest speed %.3g m/s with the load, %.3g without; largest difference %.3g" % (
        mode, STEPS, np.hypot(u, v).max(), np.hypot(ub, vb).max(), max(np.abs(u - ub).max(), np.abs(v - vb).max())))
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(v)) and np.abs(ub).max() > 0
    assert not np.array_equal(u, ub) and not np.array_equal(v, vb)

"""The C++ host's dynamics.advect_column_state (include/nsdg.h "column state transport") on the device: row blocks, graphs and
sub-stepping leave the restart file unchanged byte for byte, N steps equal N / 2 steps, a restart and N / 2 more in both file formats
(the restart carries hsnow_dg), a file without hsnow_dg is accepted, and with the mode off nothing changes."""
import os
import subprocess

import pytest

from nextsimdg_amd import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
INIT = "hice = 0.3\ncice = 0.9\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"
MODE = "thermodynamics = true\nforcing = winter\nadvect_column_state = true\n"


@pytest.fixture(scope="module")
def host(gpu):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "nextsim_amd")


def run_host(host, tmp, name, n=128, L=64e3, model="start = 0\nstop = 480\n", dynamics=MODE, ext=".nsdg"):
    """runs nextsim_amd on an n x n box of side L with 120 s steps; returns the restart file's bytes"""
    final = os.path.join(tmp, name + ext)
    cfg = os.path.join(tmp, name + ".cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\n%sfinal_file = %s\n"
                "[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\nnsub = 16\n%s" % (model, final, n, n, INIT, L, dynamics))
    p = subprocess.run([host, "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    with open(final, "rb") as f:
        return f.read()


def test_blocks_graphs_and_mode_off(host, tmp_path):
    tmp = str(tmp_path)
    one = run_host(host, tmp, "one")
    assert b"hsnow_dg" in one.split(b"END-HEADER")[0]
    assert run_host(host, tmp, "four", dynamics=MODE + "row_blocks = 4\n") == one
    assert run_host(host, tmp, "graph", dynamics=MODE + "graph = true\n") == one
    # the mode off, said explicitly, writes what a run without the key writes; the mode changes the run
    plain = "thermodynamics = true\nforcing = winter\n"
    off = run_host(host, tmp, "off", dynamics=plain)
    assert run_host(host, tmp, "off_explicit", dynamics=plain + "advect_column_state = false\n") == off
    assert b"hsnow_dg" not in off
    assert off != one


def test_substeps_auto_one_block_equals_four(host, tmp_path):
    """250 m cells at A0 = 0.9 under the converging sub-cycle: auto splits the step; 1 block == 4 blocks byte for byte"""
    tmp = str(tmp_path)
    dyn = MODE + "substeps = auto\nsubcycle = adaptive_converged\n"
    one = run_host(host, tmp, "one", L=32e3, dynamics=dyn)
    assert run_host(host, tmp, "four", L=32e3, dynamics=dyn + "row_blocks = 4\n") == one


@pytest.mark.parametrize("ext", [".nsdg", ".nc"])
def test_restart_in_both_formats(host, tmp_path, ext):
    """N steps == N / 2 steps, the restart file (hsnow_dg included), N / 2 more -- byte for byte; with 4 row blocks after the restart too"""
    tmp = str(tmp_path)
    full = run_host(host, tmp, "full", ext=ext)
    half = run_host(host, tmp, "half", model="start = 0\nstop = 240\n", ext=ext)
    assert b"hsnow_dg" in half
    resume = "init_file = %s\nstart = 240\nstop = 480\n" % os.path.join(tmp, "half" + ext)
    assert run_host(host, tmp, "resumed", model=resume, ext=ext) == full
    assert run_host(host, tmp, "resumed4", model=resume, dynamics=MODE + "row_blocks = 4\n", ext=ext) == full


def test_a_restart_without_hsnow_dg_is_accepted(host, tmp_path):
    """a file written with the mode off holds no hsnow_dg: a run with the mode on starts the higher snow coefficients at zero"""
    tmp = str(tmp_path)
    plain = "thermodynamics = true\nforcing = winter\n"
    run_host(host, tmp, "half_off", model="start = 0\nstop = 240\n", dynamics=plain)
    resume = "init_file = %s\nstart = 240\nstop = 480\n" % os.path.join(tmp, "half_off.nsdg")
    on = run_host(host, tmp, "resumed_on", model=resume)
    assert b"hsnow_dg" in on
    assert run_host(host, tmp, "resumed_on4", model=resume, dynamics=MODE + "row_blocks = 4\n") == on

"""The C++ host's slab ocean (host/include/DynamicsStep.hpp "dynamics.slab_ocean", "[slabocean]").  Without a
device: the host's own test program (keys, the forcing file's pair, the rows between the ranks) and the binary's refusals before it asks
for a device, message by message.  On the device, a 64 x 48 box with a land strip under the winter forcing: 1 row block against 4 and N
steps against N/2 + restart + N/2, the restart files equal byte for byte; the restart file's sst has left its initial value wherever
there is ocean (10 % open water under cold air everywhere) and holds it on land; a relaxation towards the initial values and towards a
forcing file's pair sst, sss reaches the run; and without the key the run is the run it was."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nextsimdg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST = 64, 48  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
DT, STEPS, NSUB = 120, 6, 16
SST0, SSS0 = -1.76, 32.0
INIT = "hice = 0.3\ncice = 0.9\nsst = %r\nsss = %r\nhsnow = 0.05\ntice = -8\n" % (SST0, SSS0)
THERMO = "nsub = %d\nthermodynamics = true\nforcing = winter\n" % NSUB
SLAB = THERMO + "slab_ocean = true\n"


@pytest.fixture(scope="module")
def host_dir():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_slab_program(host_dir):
    """the keys and their refusals, the forcing file's pair, sst and sss between the ranks: needs no device"""
    p = subprocess.run([os.path.join(host_dir, "slab_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and re.search(r"host slab tests: \d+ checks, 0 failures", out), out


def test_host_refuses_bad_slab_keys_before_any_device(host_dir, tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(host_dir, "nextsim_amd")
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 6\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\nnsub = 4\n" % os.path.join(tmp, "x.nsdg"))
    on = ["--dynamics.thermodynamics=true", "--dynamics.slab_ocean=true"]
    cases = [
        (["--dynamics.slab_ocean=true"], "dynamics.slab_ocean needs dynamics.thermodynamics = true"),
        (["--dynamics.slab_ocean=true", "--dynamics.thermodynamics=false"], "dynamics.slab_ocean needs dynamics.thermodynamics = true"),
        (["--slabocean.relax_t=86400"], "[slabocean]: slabocean.relax_t needs dynamics.slab_ocean = true"),
        (["--dynamics.thermodynamics=true", "--slabocean.relax_s=86400"], "[slabocean]: slabocean.relax_s needs dynamics.slab_ocean = true"),
        (["--dynamics.thermodynamics=true", "--dynamics.slab_ocean=false", "--slabocean.ice_salinity=4"],
         "[slabocean]: slabocean.ice_salinity needs dynamics.slab_ocean = true"),
        (on + ["--slabocean.relax_t=-1"], "[slabocean]: slabocean.relax_t = -1.000000: need relax_t >= 0, relax_s >= 0 and ice_salinity >= 0, all finite"),
        (on + ["--slabocean.relax_s=-2"], "[slabocean]: slabocean.relax_s = -2.000000: need relax_t >= 0"),
        (on + ["--slabocean.ice_salinity=-3"], "[slabocean]: slabocean.ice_salinity = -3.000000: need relax_t >= 0"),
    ]
    for args, needle in cases:
        p = subprocess.run([exe, "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        out = p.stdout.decode()
        assert p.returncode != 0 and needle in out, (args, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(tmp, "x.nsdg")), (args, out)
    if not torch.cuda.is_available():  # good keys pass every check: the run gets as far as asking for a device
        p = subprocess.run([exe, "--config-file", cfg] + on + ["--slabocean.relax_t=86400", "--slabocean.ice_salinity=0"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()


def mask():
    m = np.zeros((NSLOW, NFAST), dtype=bool)  # [slow, fast]
    m[10:54, 20:23] = True  # a strip across the boundaries of four row blocks (rows 16, 32, 48)
    m[32, 5] = True  # and a rock on a boundary row
    return m


@pytest.fixture(scope="module")
def runs(host_dir, tmp_path_factory):
    """run(name, dynamics, ...) -> (restart bytes, stdout, directory); every configuration runs once per module"""
    base, done = str(tmp_path_factory.mktemp("slab")), {}

    def run(name, dynamics, start=0, stop=DT * STEPS, init_file=None):
        if name in done:
            return done[name]
        tmp = os.path.join(base, name)
        os.makedirs(tmp)
        final, cfg = os.path.join(tmp, "final.nsdg"), os.path.join(tmp, "run.cfg")
        np.save(os.path.join(tmp, "land.npy"), mask())
        with open(cfg, "w") as f:
            f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %d\nstart = %d\nstop = %d\n"
                    "final_file = %s\n%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = 256e3\nland_mask_file = land.npy\n%s"
                    % (DT, start, stop, final, ("init_file = %s\n" % init_file) if init_file else "", NSLOW, NFAST, INIT, dynamics))
        p = subprocess.run([os.path.join(host_dir, "nextsim_amd"), "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        with open(final, "rb") as f:
            done[name] = (f.read(), p.stdout.decode(), tmp)
        return done[name]

    return run


def planes(raw):
    """the element planes hice, cice, sst, sss [X, Y] of the restart file (RectGrid::dump, the .nsdg form)"""
    head, body = raw.split(b"END-HEADER\n", 1)
    keys = dict(line.split("=", 1) for line in head.decode().splitlines() if "=" in line)
    X, Y, NL = int(keys["data.x"]), int(keys["data.y"]), int(keys["data.nLayers"])
    assert (X, Y) == (NSLOW, NFAST)
    a = np.frombuffer(body, dtype=np.float64)
    n, nn = X * Y, (2 * X + 1) * (2 * Y + 1)
    sizes = {"hice": n, "cice": n, "hsnow": n, "sst": n, "sss": n, "tice": n * NL, "hice_dg": 5 * n, "cice_dg": 5 * n, "u": nn, "v": nn, "s11": 8 * n,
             "s12": 8 * n, "s22": 8 * n, "newice": n}
    out, at = {}, 0
    for name in keys["variables"].split(","):
        if name in ("hice", "cice", "sst", "sss"):
            out[name] = a[at:at + n].reshape(X, Y)
        at += sizes[name]
    assert at == a.size
    return out


@pytest.mark.gpu
def test_one_row_block_equals_four_and_a_restarted_run_is_the_whole_run(runs, gpu):
    whole, out, _ = runs("whole", SLAB)
    assert "dynamics slab ocean: relax_t = 0 s, relax_s = 0 s, ice_salinity = 5; relaxation targets: none" in out, out
    assert runs("four", SLAB + "row_blocks = 4\n")[0] == whole
    _, _, tmp = runs("first", SLAB, stop=DT * STEPS // 2)
    second, _, _ = runs("second", SLAB + "row_blocks = 4\n", start=DT * STEPS // 2, init_file=os.path.join(tmp, "final.nsdg"))
    assert second == whole
    # the restart file's ocean: evolved wherever there is ocean (open water under cold air in every element), untouched on land
    p, land = planes(whole), mask()
    assert np.all(np.isfinite(p["sst"])) and np.all(np.isfinite(p["sss"]))
    assert np.all(p["sst"][land] == SST0) and np.all(p["sss"][land] == SSS0)
    assert np.all(p["sst"][~land] != SST0) and np.all(p["sss"][~land] != SSS0)
    assert np.all(p["sss"][~land] > SSS0)  # the pack grows under the winter sky: brine
    assert np.all(np.abs(p["sst"][~land] + 0.055 * p["sss"][~land]) < 0.05)  # and the layer stays at its (new) freezing point


@pytest.mark.gpu
def test_without_the_key_the_run_is_the_run_it_was(runs, gpu):
    plain, out, _ = runs("plain", THERMO)
    assert "slab ocean" not in out
    assert runs("key_false", THERMO + "slab_ocean = false\n")[0] == plain
    p, whole = planes(plain), planes(runs("whole", SLAB)[0])
    assert np.all(p["sst"] == SST0) and np.all(p["sss"] == SSS0)  # the reference's ocean: read, never written
    assert not np.array_equal(p["hice"], whole["hice"])  # the mode reaches the ice


RELAX = "[slabocean]\nrelax_t = 1200\nrelax_s = 600\nice_salinity = 4\n"


@pytest.mark.gpu
def test_relaxation_towards_the_initial_values(runs, gpu):
    relax = RELAX
    one, out, tmp = runs("relax", SLAB + relax)
    assert "relax_t = 1200 s, relax_s = 600 s, ice_salinity = 4; relaxation targets: the initial sst, sss" in out, out
    assert runs("relax_four", SLAB + "row_blocks = 4\n" + relax)[0] == one
    whole, land = planes(runs("whole", SLAB)[0]), mask()
    p = planes(one)
    assert np.all(p["sss"][~land] < whole["sss"][~land]) and np.all(p["sss"][~land] > SSS0)  # pulled back towards 32
    assert np.all(p["sst"][land] == SST0) and np.all(p["sss"][land] == SSS0)


@pytest.mark.gpu
def test_relaxation_towards_the_pair_of_a_forcing_file(runs, host_dir, gpu):
    from test_gpu_forcing_file import make_file

    relax, land = RELAX, mask()
    p, tmp = planes(runs("relax", SLAB + relax)[0]), runs("relax", SLAB + relax)[2]
    # a forcing file with the winter constants of the column planes and a warm, fresh pair sst, sss: the targets come from the file, so a
    # restart in the middle is exact
    const = {"tair": -25.0, "tdew": -28.0, "slp": 1.0e5, "qsw": 0.0, "qlw": 180.0, "mld": 20.0, "snowfall": 1e-5}
    fields = {k: np.full((2, 3, 4), v) for k, v in const.items()}
    fields["sst"] = np.stack([np.full((3, 4), 0.0), np.full((3, 4), 2.0)])
    fields["sss"] = np.full((2, 3, 4), 30.0)
    path = make_file(host_dir, tmp, "targets", [0.0, 2.0 * DT * STEPS], fields)
    dyn = "nsub = %d\nthermodynamics = true\nforcing = file\nforcing_file = %s\nslab_ocean = true\n" % (NSUB, path)
    filed, out, _ = runs("file", dyn + relax)
    assert "relaxation targets: the forcing file's sst, sss" in out, out
    assert runs("file_four", dyn + "row_blocks = 4\n" + relax)[0] == filed
    _, _, first = runs("file_first", dyn + relax, stop=DT * STEPS // 2)
    assert runs("file_second", dyn + relax, start=DT * STEPS // 2, init_file=os.path.join(first, "final.nsdg"))[0] == filed
    f = planes(filed)
    assert np.all(f["sss"][~land] < SSS0) and np.all(f["sst"][~land] > p["sst"][~land])  # towards 30 and towards the warm target
    assert np.all(f["sst"][land] == SST0) and np.all(f["sss"][land] == SSS0)

"""Point samples in the C++ host without a device: pytest builds and runs host/test/points_tests.cpp (every refusal of model.drifters_fields
and model.stations_* before any device, the header lines, the reader's 5 + k columns, the clock of the stations' blocks), and the
executable's own refusals leave no file behind."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_point_sample_cases(host_build):
    p = subprocess.run([os.path.join(host_build, "points_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert re.search(r"host point-sample tests: [1-9]\d* checks, 0 failures", out), out


KEYS = ["--model.stations_file=stations.txt", "--model.stations_output=moorings.txt", "--model.stations_fields=hice,shear"]


@pytest.mark.parametrize("step,args,env,why", [
    ("DynamicsStep", KEYS, {"WORLD_SIZE": "2", "RANK": "0"}, "model.stations_file is set in a run of 2 processes"),
    ("DynamicsStep", KEYS + ["--dynamics.loopback_world=3"], {}, "model.stations_file is set with dynamics.loopback_world"),
    ("DynamicsStep", KEYS[:2], {}, "model.stations_fields must list the fields"),
    ("DynamicsStep", KEYS[:2] + ["--model.stations_fields=hice,depth"], {}, "model.stations_fields: unknown field \"depth\""),
    ("DynamicsStep", KEYS[:2] + ["--model.stations_fields=damage"], {}, "the field \"damage\" needs dynamics.rheology = bbm"),
    ("DynamicsStep", KEYS[:2] + ["--model.stations_fields=tice"], {}, "the field \"tice\" is column state"),
    ("DynamicsStep", ["--model.drifters_fields=hice"], {}, "model.drifters_fields is set without model.drifters_file"),
    ("DynamicsStep", ["--model.stations_file=far.txt"] + KEYS[1:], {}, "far.txt, line 1: the station is outside the domain"),
    ("HipStep", KEYS, {}, "Nextsim::HipStep has no dynamics state to sample"),
], ids=["two_processes", "loopback", "no_fields", "unknown", "damage", "tice", "fields_alone", "outside", "hipstep"])
def test_host_refuses_before_any_device(host_build, tmp_path, step, args, env, why):
    """every refusal of the new keys comes from configure(): no device is asked for (there is none here), nothing is written"""
    tmp = str(tmp_path)
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::%s\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 240\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 8000\n"
                % (step, os.path.join(tmp, "x.nsdg")))
    with open(os.path.join(tmp, "stations.txt"), "w") as f:
        f.write("# x y\n100 200\n8000 8000\n")
    with open(os.path.join(tmp, "far.txt"), "w") as f:
        f.write("100 8000.5\n")
    p = subprocess.run([os.path.join(host_build, "nextsim_amd"), "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, cwd=tmp, env=dict(os.environ, **env))
    out = p.stdout.decode()
    assert p.returncode != 0 and why in out and "no HIP device" not in out, out
    assert not [n for n in os.listdir(tmp) if n.startswith("moorings") or n.endswith(".nsdg")]

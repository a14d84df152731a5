"""The C++ host's four outputs switched on at once (host/src/DynamicsOutputs.hpp): the 64 x 48 box of test_host_points.py, 6 steps of
120 s with 24 sub-iterations and the column thermodynamics; a snapshot history of two fields, the time series, five drifters with fields
and the stations of that file.  Every output file and the restart file are compared byte for byte between 1 and 4 row blocks, and each
output file with the file of a run in which it is the only output."""
import glob
import os
import subprocess

import pytest

from nextsimdg_amd import build
from test_host_points import DRIFTER_FIELDS, DT, INIT, L, NFAST, NSLOW, NSUB, STATION_FIELDS, STEPS, lines_of, points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
OUTPUTS = {
    "history": "output_period = 240\noutput_file = ice.nsdg\noutput_fields = hice,hsnow\noutput_kind = snapshot\n",
    "series": "series_file = totals.txt\nseries_fields = area,extent,volume,snow_volume\n",
    "drifters": "drifters_file = seeds.txt\ndrifters_output = track.txt\ndrifters_period = 240\ndrifters_fields = %s\n" % ",".join(DRIFTER_FIELDS),
    "stations": "stations_file = stations.txt\nstations_output = moorings.txt\nstations_fields = %s\n" % ", ".join(STATION_FIELDS),
}
# what each output writes (the history: one record per window of 240 s)
FILES = {
    "history": ["ice.%010d.nsdg" % t for t in (240, 480, 720)],
    "series": ["totals.txt"],
    "drifters": ["track.txt"],
    "stations": ["moorings.txt"],
}


@pytest.fixture(scope="module")
def host(gpu):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "nextsim_amd")


@pytest.fixture(scope="module")
def runs(host, tmp_path_factory):
    """run(name, outputs, dynamics) -> {file name: bytes} of everything the run wrote; every configuration runs once per module"""
    base, done = str(tmp_path_factory.mktemp("together")), {}

    def run(name, outputs, dynamics=""):
        if name in done:
            return done[name]
        tmp = os.path.join(base, name)
        os.makedirs(tmp)
        with open(os.path.join(tmp, "seeds.txt"), "w") as f:
            f.write("\n".join(lines_of(points()[17:22])) + "\n")  # five drifters, some on the boundary of two row blocks
        with open(os.path.join(tmp, "stations.txt"), "w") as f:
            f.write("\n".join(lines_of(points())) + "\n")
        inputs = set(os.listdir(tmp)) | {"run.cfg"}
        with open(os.path.join(tmp, "run.cfg"), "w") as f:
            f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %d\nstart = 0\nstop = %d\n"
                    "final_file = final.nsdg\n%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\nnsub = %d\n"
                    "thermodynamics = true\nforcing = winter\n%s"
                    % (DT, DT * STEPS, "".join(OUTPUTS[o] for o in outputs), NSLOW, NFAST, INIT, L, NSUB, dynamics))
        p = subprocess.run([host, "--config-file", "run.cfg"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        done[name] = {os.path.basename(n): open(n, "rb").read() for n in glob.glob(os.path.join(tmp, "*")) if os.path.basename(n) not in inputs}
        return done[name]

    return run


def test_all_four_outputs_are_the_same_on_one_row_block_and_on_four(runs):
    one = runs("all1", sorted(OUTPUTS))
    assert sorted(one) == sorted(["final.nsdg"] + sum(FILES.values(), []))  # every output wrote its files, and nothing else is there
    assert all(len(raw) > 0 for raw in one.values())
    assert len(one["moorings.txt"].splitlines()) == 1 + STEPS * len(points()) and len(one["track.txt"].splitlines()) == 1 + 3 * 5
    assert len(one["totals.txt"].splitlines()) == 1 + STEPS
    four = runs("all4", sorted(OUTPUTS), dynamics="row_blocks = 4\n")
    assert sorted(four) == sorted(one)
    differ = [n for n in sorted(one) if four[n] != one[n]]
    assert not differ, differ  # byte for byte, the restart file too


@pytest.mark.parametrize("output", sorted(OUTPUTS))
def test_an_output_writes_the_file_it_writes_alone(runs, output):
    together, alone = runs("all1", sorted(OUTPUTS)), runs("only_" + output, [output])
    assert sorted(alone) == sorted(["final.nsdg"] + FILES[output])
    differ = [n for n in sorted(alone) if alone[n] != together[n]]
    assert not differ, differ  # its files, and the restart file: no output changes the run

"""The C++ host's point samples (host/include/Stations.hpp, model.drifters_fields of host/include/Drifters.hpp; include/nsdg.h "point
samples") on the device: a 64 x 48 box, 6 steps of 120 s with 24 sub-iterations.  Both output files are compared byte for byte between 1 and
4 row blocks, across a restart that is fed the last drifter block with its extra columns, and between two sizes of the stations' buffer;
without the new keys the drifters' output and the restart file are what they are without this feature's keys; and the station lines are
the Python driver's merge_stations, digit for digit."""
import os
import subprocess

import numpy as np
import pytest
import torch

from nextsimdg_amd import abi, build, rowblock, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST, L, NSUB, DT, STEPS = 64, 48, 256e3, 24, 120, 6  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
HY = L / NSLOW
INIT = "hice = 0.3\ncice = 0.9\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"
DRIFTER_FIELDS = ("hice", "cice", "shear")
STATION_FIELDS = ("hice", "u", "v", "divergence", "shear", "sigma_n", "sigma_s")


@pytest.fixture(scope="module")
def host(gpu):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "nextsim_amd")


def points():
    """on and next to the boundaries of four row blocks (rows 16, 32, 48), the domain's corners and edges, a few anywhere"""
    xy = []
    for row in (16, 32, 48):
        for k, off in enumerate((0.0, 1e-3, -1e-3, 1.0, -1.0)):
            for fx in (0.15, 0.4, 0.6, 0.85):
                xy.append(((fx + 0.005 * k) * L, row * HY + off))
    rng = np.random.default_rng(9)
    xy += list(zip(rng.uniform(0, L, 20), rng.uniform(0, L, 20)))
    xy += [(L, L), (0.0, 0.0), (0.0, L), (0.5 * L, L), (L, 0.25 * L)]
    return np.array(xy)


def lines_of(xy):
    return ["# x y"] + ["%.17g %.17g" % (x, y) for x, y in xy]


@pytest.fixture(scope="module")
def runs(host, tmp_path_factory):
    """run(name, ...) -> (restart bytes, drifters' output bytes or None, stations' output bytes or None, path of the restart file); every
    configuration runs once per module"""
    base, done = str(tmp_path_factory.mktemp("points")), {}

    def run(name, drifters=None, fields=True, stations=True, buffer=None, dynamics="", start=0, stop=DT * STEPS, init_file=None):
        if name in done:
            return done[name]
        tmp = os.path.join(base, name)
        os.makedirs(tmp)
        final, cfg = os.path.join(tmp, "final.nsdg"), os.path.join(tmp, "run.cfg")
        keys = ""
        if drifters is not None:
            with open(os.path.join(tmp, "seeds.txt"), "w") as f:
                f.write("\n".join(drifters) + "\n")
            keys += "drifters_file = seeds.txt\ndrifters_output = track.txt\ndrifters_period = 240\n"
            if fields:
                keys += "drifters_fields = %s\n" % ",".join(DRIFTER_FIELDS)
        if stations:
            with open(os.path.join(tmp, "stations.txt"), "w") as f:
                f.write("\n".join(lines_of(points())) + "\n")
            keys += "stations_file = stations.txt\nstations_output = moorings.txt\nstations_fields = %s\n" % ", ".join(STATION_FIELDS)
            if buffer is not None:
                keys += "stations_buffer = %d\n" % buffer
        with open(cfg, "w") as f:
            f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %d\nstart = %d\nstop = %d\n"
                    "final_file = %s\n%s%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\nnsub = %d\n%s"
                    % (DT, start, stop, final, ("init_file = %s\n" % init_file) if init_file else "", keys, NSLOW, NFAST, INIT, L, NSUB, dynamics))
        p = subprocess.run([host, "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        read = lambda n: open(os.path.join(tmp, n), "rb").read() if os.path.exists(os.path.join(tmp, n)) else None
        done[name] = (read("final.nsdg"), read("track.txt"), read("moorings.txt"), final)
        return done[name]

    return run


def blocks(raw, header):
    """an output file as {time: [lines]}"""
    lines = raw.decode().splitlines()
    assert lines[0] == header, lines[0]
    by_time = {}
    for line in lines[1:]:
        by_time.setdefault(int(line.split()[0]), []).append(line)
    return by_time


DRIFTER_HEADER = "# time id x y status " + " ".join(DRIFTER_FIELDS)
STATION_HEADER = "# time id x y " + " ".join(STATION_FIELDS)


def test_one_row_block_equals_four_in_both_files(runs):
    restart1, track1, moor1, _ = runs("one", lines_of(points()))
    n = len(points())
    track, moor = blocks(track1, DRIFTER_HEADER), blocks(moor1, STATION_HEADER)
    assert sorted(track) == [240, 480, 720] and all(len(v) == n for v in track.values())
    assert sorted(moor) == [DT * k for k in range(1, STEPS + 1)] and all(len(v) == n for v in moor.values())  # one block per model step
    cols = np.array([[float(c) for c in l.split()] for l in moor[DT * STEPS]])
    assert cols.shape == (n, 4 + len(STATION_FIELDS)) and np.all(np.isfinite(cols)) and list(cols[:, 1]) == list(range(n))
    assert np.array_equal(cols[:, 2:4], points()) and np.abs(cols[:, 5]).max() > 1e-6  # the input order and positions; the ice moves
    dcols = np.array([[float(c) for c in l.split()] for l in track[720]])
    assert dcols.shape == (n, 5 + len(DRIFTER_FIELDS)) and np.all(np.isfinite(dcols))
    restart4, track4, moor4, _ = runs("four", lines_of(points()), dynamics="row_blocks = 4\n")
    assert track4 == track1 and moor4 == moor1 and restart4 == restart1  # byte for byte


def test_a_restart_fed_the_last_block_with_its_extra_columns_continues(runs):
    restart, whole, moor, _ = runs("one", lines_of(points()))
    track, stations = blocks(whole, DRIFTER_HEADER), blocks(moor, STATION_HEADER)
    half = DT * STEPS // 2 + DT  # 480: a multiple of the drifters' period
    _, first_track, first_moor, final = runs("first", lines_of(points()), stop=half)
    first = blocks(first_track, DRIFTER_HEADER)
    assert sorted(first) == [240, 480] and all(first[t] == track[t] for t in first)
    fed = [DRIFTER_HEADER] + first[480]  # output lines of 5 + 3 columns under the header that names the three
    restart2, rest_track, rest_moor, _ = runs("second", fed, start=half, stop=DT * STEPS, init_file=final)
    second = blocks(rest_track, DRIFTER_HEADER)
    assert sorted(second) == [720] and second[720] == track[720]
    a, b = blocks(first_moor, STATION_HEADER), blocks(rest_moor, STATION_HEADER)
    assert sorted(a) + sorted(b) == sorted(stations) and all(stations[t] == {**a, **b}[t] for t in stations)
    assert restart2 == restart


def test_without_the_new_keys_the_files_are_what_they_were(runs):
    restart, track, _, _ = runs("one", lines_of(points()))
    plain_restart, plain_track, none, _ = runs("plain", lines_of(points()), fields=False, stations=False)
    assert none is None and plain_restart == restart
    lines = plain_track.decode().splitlines()
    assert lines[0] == "# time id x y status" and all(len(l.split()) == 5 for l in lines[1:])
    # the bytes of the format the file had before the key existed, restated here: "%ld %zu %.17g %.17g %d" per line under that header
    # (host/test/points_tests.cpp holds formatLine and write() without fields to the same literal strings)
    cols = [l.split() for l in lines[1:]]
    restated = "# time id x y status\n" + "".join("%d %d %.17g %.17g %d\n" % (int(c[0]), int(c[1]), float(c[2]), float(c[3]), int(c[4])) for c in cols)
    assert plain_track == restated.encode()
    assert [int(c[0]) for c in cols] == [t for t in (240, 480, 720) for _ in range(len(points()))] and [int(c[1]) for c in cols] == list(range(len(points()))) * 3
    with_fields = track.decode().splitlines()
    assert [" ".join(l.split()[:5]) for l in with_fields[1:]] == lines[1:]  # the same positions, to the digit
    off_restart, no_track, no_moor, _ = runs("off", stations=False)
    assert no_track is None and no_moor is None and off_restart == restart


def test_a_small_buffer_writes_the_same_file(runs):
    _, _, moor, _ = runs("one", lines_of(points()))
    _, _, small, _ = runs("buffer2", lines_of(points()), buffer=2)
    _, _, large, _ = runs("buffer256", lines_of(points()), buffer=256)
    assert small == moor and large == moor


def test_the_station_lines_are_the_python_drivers(runs, gpu):
    """the same initial state and the same nsdg_boxtest_forcing through DynamicsCore(native=True): the two issue the same calls, so the lines
    agree to the last of their 17 digits"""
    _, _, moor, _ = runs("one", lines_of(points()))
    nx, ny = NFAST, NSLOW  # the dynamics ABI calls the fast dimension nx
    bt = synthetic.BoxTest(nx, ny, L)
    ctx = abi.Context(gpu)
    ctx.set_mevp_params(ctx.mevp_default_params(**bt.subcycle_parameters(float(DT))))  # the hosts' policy
    core = rowblock.DynamicsCore(ctx, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, float(DT), NSUB, torch.device("cuda"), native=True,
                                 stations=points(), station_fields=STATION_FIELDS)
    H = np.zeros((6, ny, nx)); H[0] = 0.3
    A = np.zeros((6, ny, nx)); A[0] = 0.9
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    core.load_global(H, A, uo, vo, ua, va)
    for k in range(STEPS):
        ctx.set_grid(nx, ny, bt.hx, bt.hy)
        ctx.boxtest_forcing(bt.L, float(DT) * k, wind=(core.ua, core.va))  # the cyclone moves with model time
        core.step()
    got = rowblock.DynamicsCore.merge_stations([core.stations_read()])
    core.close()
    ctx.close()
    want = ["%d %d %.17g %.17g " % (DT * (s + 1), p, x, y) + " ".join("%.17g" % got[f][s, p] for f in STATION_FIELDS)
            for s in range(STEPS) for p, (x, y) in enumerate(points())]
    lines = moor.decode().splitlines()
    assert lines[0] == STATION_HEADER and len(lines) == 1 + len(want)
    differ = [k for k, (a, b) in enumerate(zip(lines[1:], want)) if a != b]
    assert not differ, (len(differ), lines[1 + differ[0]], want[differ[0]])

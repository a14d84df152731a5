"""The C++ host's drifters (host/include/Drifters.hpp; include/nsdg.h "drifters") on the device: a 64 x 48 box, 8 steps of 120 s with 24
sub-iterations.  The output file and the restart file are compared byte for byte between 1 and 4 row blocks, across a restart that is fed
the last block of the first half, and with the keys absent."""
import os
import subprocess

import numpy as np
import pytest

from nextsimdg_amd import build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST, L = 64, 48, 256e3  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
HY = L / NSLOW
INIT = "hice = 0.3\ncice = 0.9\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"


@pytest.fixture(scope="module")
def host(gpu):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "nextsim_amd")


def seed_lines():
    """on and next to the boundaries of four row blocks (rows 16, 32, 48), a few anywhere, one stopped, one on the domain's corner"""
    lines = ["# x y [status]"]
    for row in (16, 32, 48):
        for k, off in enumerate((0.0, 1e-3, -1e-3, 1e-2, -1e-2, 0.1, -0.1, 1.0, -1.0)):
            for fx in (0.15, 0.4, 0.6, 0.85):
                lines.append("%.17g %.17g" % ((fx + 0.005 * k) * L, row * HY + off))
    rng = np.random.default_rng(9)
    lines += ["%.17g %.17g 0" % (x, y) for x, y in zip(rng.uniform(0, L, 20), rng.uniform(0, L, 20))]
    lines += ["1000 2000 2", "%.17g %.17g" % (L, L), "", "0 0 0"]
    return lines


@pytest.fixture(scope="module")
def runs(host, tmp_path_factory):
    """run(name, ...) -> (restart bytes, output file bytes or None, path of the restart file); every configuration runs once per module"""
    base, done = str(tmp_path_factory.mktemp("drifters")), {}

    def run(name, drifters=None, period=240, dynamics="", start=0, stop=960, init_file=None, env=None, expect_ok=True):
        if name in done:
            return done[name]
        tmp = os.path.join(base, name)
        os.makedirs(tmp)
        final, cfg, out = os.path.join(tmp, "final.nsdg"), os.path.join(tmp, "run.cfg"), os.path.join(tmp, "track.txt")
        keys = ""
        if drifters is not None:
            with open(os.path.join(tmp, "seeds.txt"), "w") as f:
                f.write("\n".join(drifters) + "\n")
            keys = "drifters_file = seeds.txt\ndrifters_output = track.txt\ndrifters_period = %d\n" % period
        with open(cfg, "w") as f:
            f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = %d\nstop = %d\n"
                    "final_file = %s\n%s%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\nnsub = 24\n%s"
                    % (start, stop, final, ("init_file = %s\n" % init_file) if init_file else "", keys, NSLOW, NFAST, INIT, L, dynamics))
        p = subprocess.run([host, "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=300,
                           env=dict(os.environ, **(env or {})))
        if not expect_ok:
            return p.returncode, p.stdout.decode(), os.listdir(tmp)
        assert p.returncode == 0, p.stdout.decode()
        track = open(out, "rb").read() if os.path.exists(out) else None
        with open(final, "rb") as f:
            done[name] = (f.read(), track, final)
        return done[name]

    return run


def blocks(raw):
    """the output file as {time: [lines]} and {time: array [n, 3] of x, y, status}"""
    lines = raw.decode().splitlines()
    assert lines[0] == "# time id x y status"
    by_time = {}
    for line in lines[1:]:
        by_time.setdefault(int(line.split()[0]), []).append(line)
    values = {}
    for t, ls in by_time.items():
        cols = [l.split() for l in ls]
        assert [int(c[1]) for c in cols] == list(range(len(cols)))
        values[t] = np.array([[float(c[2]), float(c[3]), float(c[4])] for c in cols])
    return by_time, values


def test_one_row_block_equals_four_and_the_keys_change_nothing_else(runs):
    restart1, track1, _ = runs("one", seed_lines())
    lines, values = blocks(track1)
    n = len([l for l in seed_lines() if l and not l.startswith("#")])
    assert sorted(lines) == [240, 480, 720, 960] and all(len(v) == n for v in lines.values())
    first, last = values[240], values[960]
    assert last[-3, 2] == 2 and tuple(last[-3, :2]) == (1000.0, 2000.0)  # the stopped one stayed
    moving = last[:, 2] == 0
    assert moving.sum() > n // 2 and np.abs(last[moving, :2] - first[moving, :2]).max() > 1.0
    start = np.array([[float(c) for c in l.split()[:2]] for l in seed_lines() if l and not l.startswith("#")])
    crossed = (np.floor(start[:, 1] / HY).clip(max=NSLOW - 1) // 16) != (np.floor(last[:, 1] / HY).clip(max=NSLOW - 1) // 16)
    print("%d drifters crossed a block boundary" % crossed.sum())
    assert crossed.sum() >= 1, "no drifter crossed a block boundary: the seeds do not test the hand-over"
    restart4, track4, _ = runs("four", seed_lines(), dynamics="row_blocks = 4\n")
    assert track4 == track1 and restart4 == restart1  # the output file and the restart file, byte for byte
    off, none, _ = runs("off")
    assert none is None and off == restart1  # with the keys absent the restart bytes are what they are with them


def test_a_restart_fed_the_last_block_continues_the_tracks(runs):
    restart, whole, _ = runs("one", seed_lines())
    lines, _ = blocks(whole)
    _, half, final = runs("first", seed_lines(), stop=480)
    first, _ = blocks(half)
    assert sorted(first) == [240, 480] and all(first[t] == lines[t] for t in first)
    restart2, rest, _ = runs("second", ["# the last block of the first half"] + first[480], start=480, stop=960, init_file=final)
    second, _ = blocks(rest)
    assert sorted(second) == [720, 960] and all(second[t] == lines[t] for t in second)  # the lines, byte for byte
    assert restart2 == restart


def test_period_zero_writes_one_block_at_stop(runs):
    _, track, _ = runs("at_stop", seed_lines(), period=0)
    lines, _ = blocks(track)
    assert sorted(lines) == [960] and lines[960] == blocks(runs("one", seed_lines())[1])[0][960]


def test_a_multi_process_run_refuses_the_key_before_any_device_work(runs):
    rc, out, files = runs("world2", seed_lines(), env={"WORLD_SIZE": "2", "RANK": "0"}, expect_ok=False)
    assert rc != 0 and "model.drifters_file is set in a run of 2 processes" in out and "no HIP device" not in out, out
    assert "track.txt" not in files and "final.nsdg" not in files

"""The C++ host of this tree against the host of another build (the parent commit, built in a work tree of its own): the same
configurations on both nextsim_amd binaries with every written file compared byte for byte, and the wall time of iterate()
(model.timing = true) over five alternating runs of each.  profiles/host_blocks.md has a result.
usage: python tools/host_blocks_compare.py --parent <the other build's nextsim_amd> --out <directory> [bytes] [speed]"""
import argparse
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = None
BIN = {"parent": None, "branch": os.path.join(ROOT, "nextsimdg_amd", "host", "build", "nextsim_amd")}
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from test_host_points import INIT, L, lines_of, points  # noqa: E402  (the box, the initial state and the points of that test)

ALL = ("output_period = 240\noutput_file = ice.nsdg\noutput_fields = hice,hsnow\noutput_kind = snapshot\n"
       "series_file = totals.txt\nseries_fields = area,extent,volume,snow_volume\n"
       "drifters_file = seeds.txt\ndrifters_output = track.txt\ndrifters_period = 240\ndrifters_fields = hice,cice,shear\n"
       "stations_file = stations.txt\nstations_output = moorings.txt\nstations_fields = hice, u, v, divergence, shear, sigma_n, sigma_s\n")
BBM_MODEL = "drifters_file = seeds.txt\ndrifters_output = track.txt\ndrifters_period = 240\n"
CASES = {  # name -> (nslow, nfast, stop, [model] keys, [dynamics] keys, tail)
    "all1": (64, 48, 720, ALL, "nsub = 24\nthermodynamics = true\nforcing = winter\n", ""),
    "all4": (64, 48, 720, ALL, "nsub = 24\nthermodynamics = true\nforcing = winter\nrow_blocks = 4\n", ""),
    "bbm4": (128, 96, 480, BBM_MODEL, "rheology = bbm\nrow_blocks = 4\n", "[bbm]\ncohesion_lab = 100000.0\n"),
    "speed": (64, 48, 120 * 200, "timing = true\n", "nsub = 24\nrow_blocks = 4\n", ""),
}


def run(which, case, tag=""):
    nslow, nfast, stop, model, dynamics, tail = CASES[case]
    tmp = os.path.join(OUT, case + tag, which)
    os.makedirs(tmp, exist_ok=True)
    with open(os.path.join(tmp, "seeds.txt"), "w") as f:
        f.write("\n".join(lines_of(points()[17:22] if case != "bbm4" else points())) + "\n")
    with open(os.path.join(tmp, "stations.txt"), "w") as f:
        f.write("\n".join(lines_of(points())) + "\n")
    with open(os.path.join(tmp, "run.cfg"), "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = %d\n"
                "final_file = final.nsdg\n%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\n%s%s"
                % (stop, model, nslow, nfast, INIT, L, dynamics, tail))
    p = subprocess.run(["timeout", "-k", "10", "120", BIN[which], "--config-file", "run.cfg"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp)
    out = p.stdout.decode()
    with open(os.path.join(tmp, "stdout.txt"), "w") as f:
        f.write(out)
    if p.returncode != 0:
        print("STOP: %s %s exit %d\n%s" % (which, case, p.returncode, out[-3000:]), flush=True)
        sys.exit(1)  # nothing more is started on the GPU
    return tmp, out


def compare_bytes():
    bad = 0
    for case in ("all1", "all4", "bbm4"):
        a, outa = run("parent", case)
        b, outb = run("branch", case)
        names = sorted(os.path.basename(n) for n in glob.glob(os.path.join(a, "*")))
        assert names == sorted(os.path.basename(n) for n in glob.glob(os.path.join(b, "*"))), (names, os.listdir(b))
        for n in names:
            same = open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read()
            if n not in ("seeds.txt", "stations.txt", "run.cfg"):
                print("%s %-22s %8d bytes  %s" % (case, n, os.path.getsize(os.path.join(a, n)), "same" if same else "DIFFERENT"), flush=True)
                bad += not same
    print("bytes: %d files differ" % bad, flush=True)
    return bad


def compare_speed():
    times = {"parent": [], "branch": []}
    for k in range(5):
        for which in ("parent", "branch"):
            _, out = run(which, "speed", "_%d" % k)
            m = re.search(r"iterate: ticks = 200 wall time ([0-9.]+) s", out)
            assert m, out[-2000:]
            times[which].append(float(m.group(1)))
            print("speed run %d %s iterate wall %.6f s" % (k, which, times[which][-1]), flush=True)
    for which, t in times.items():
        s = sorted(t)
        print("%s: %s  median %.6f  min %.6f  max %.6f  spread %.6f" % (which, " ".join("%.6f" % x for x in t), s[2], s[0], s[4], s[4] - s[0]))
    sp, sb = sorted(times["parent"]), sorted(times["branch"])
    print("branch median - parent median = %.6f s; parent spread = %.6f s; %s" % (sb[2] - sp[2], sp[4] - sp[0], "within" if sb[2] - sp[2] <= sp[4] - sp[0] else "OUTSIDE"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("what", nargs="*", default=["bytes", "speed"])
    args = ap.parse_args()
    BIN["parent"], OUT, what = os.path.abspath(args.parent), os.path.abspath(args.out), args.what
    if "bytes" in what and compare_bytes():
        sys.exit(2)
    if "speed" in what:
        compare_speed()

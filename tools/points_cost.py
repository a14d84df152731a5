"""What the point samples cost a run that does not use them (profiles/points.md): the step time at 2048^2 through the C++ host with every
new key off against another build of nextsim_amd (the parent commit's), in alternating runs on one box, as the wall-clock difference of a
long and a short run.  Ends at the first failure.  The kernel alone: tools/points_timing.py.

    python tools/points_cost.py --out DIR --parent-exe PATH/nextsim_amd [--reps 3]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="directory for points_cost.log")
ap.add_argument("--parent-exe", required=True, help="nextsim_amd of the build to alternate with")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.makedirs(args.out, exist_ok=True)
EXE = {"this": os.path.join(ROOT, "nextsimdg_amd", "host", "build", "nextsim_amd"), "parent": args.parent_exe}
SHORT, LONG = 20, 120
work = tempfile.mkdtemp(prefix="points_cost_")
log = open(os.path.join(args.out, "points_cost.log"), "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def host(exe, steps):
    cfg = os.path.join(work, "c.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = %d\n"
                "final_file = %s\n[rectgrid]\nnx = 2048\nny = 2048\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 512e3\nnsub = 120\n"
                % (120 * steps, os.path.join(work, "final.nsdg")))
    t0 = time.perf_counter()
    p = subprocess.run([EXE[exe], "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=work, timeout=180)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        say("FAILED rc", p.returncode, p.stdout.decode()[-2000:])
        shutil.rmtree(work, ignore_errors=True)
        sys.exit(1)
    os.remove(os.path.join(work, "final.nsdg"))
    return wall


res = {"this": [], "parent": []}
for rep in range(args.reps):
    for name in ("this", "parent"):  # alternating: each build once per repetition
        ws, wl = host(name, SHORT), host(name, LONG)
        res[name].append(1e3 * (wl - ws) / (LONG - SHORT))
        say("rep %d %-6s wall(%d) %.3f s wall(%d) %.3f s -> %.3f ms/step" % (rep, name, SHORT, ws, LONG, wl, res[name][-1]))
for name, v in res.items():
    say("%-6s ms/step %s mean %.3f spread %.3f" % (name, ", ".join("%.3f" % x for x in v), sum(v) / len(v), max(v) - min(v)))
shutil.rmtree(work, ignore_errors=True)
say("done")

"""Cost of the history statistics and the row totals at 2048^2 (profiles/history_stats.md): the step time through the C++ host with every
new key off against another build of nextsim_amd (the parent commit's), in alternating runs, as the wall-clock difference of a long and a
short run (the method of tools/history_cost.py); and the kernels alone from stream events through the Python binding -- the plain
nsdg_history_accumulate of the default list, nsdg_history_accumulate_stats of that list, of that list with two ice_mean entries and one
max, and nsdg_history_row_totals of all seven quantities, interleaved in one run.  Ends at the first failure.

    python tools/history_stats_cost.py --out DIR [--parent-exe PATH/nextsim_amd] [--reps 4]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="directory for stats_cost.log and stats_cost.json")
ap.add_argument("--parent-exe", default=None, help="nextsim_amd of another build to alternate with")
ap.add_argument("--reps", type=int, default=4)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = args.out
os.makedirs(OUT, exist_ok=True)
EXE = {"this": os.path.join(ROOT, "nextsimdg_amd", "host", "build", "nextsim_amd"), "parent": os.path.abspath(args.parent_exe) if args.parent_exe else None}
REPS, SHORT, LONG = args.reps, 20, 220
work = tempfile.mkdtemp(prefix="hist_stats_cost_")
log = open(os.path.join(OUT, "stats_cost.log"), "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def host(exe, steps, extra=()):
    cfg = os.path.join(work, "c.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = %d\n"
                "final_file = %s\n[rectgrid]\nnx = 2048\nny = 2048\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 512e3\nnsub = 120\n"
                % (120 * steps, os.path.join(work, "final.nsdg")))
    t0 = time.perf_counter()
    p = subprocess.run([EXE[exe], "--config-file", cfg] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=work, timeout=180)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        say("FAILED rc", p.returncode, p.stdout.decode()[-2000:])
        shutil.rmtree(work, ignore_errors=True)
        sys.exit(1)
    for name in os.listdir(work):
        if name.startswith("ice.") or name in ("final.nsdg", "totals.txt"):
            os.remove(os.path.join(work, name))
    return wall


VARIANTS = [("off", "this", []), ("parent", "parent", []),
            ("series", "this", ["--model.series_file=totals.txt", "--model.series_fields=area,extent,volume,drift,speed_max,hice_max"])]
VARIANTS = [v for v in VARIANTS if EXE[v[1]]]
res = {v[0]: [] for v in VARIANTS}
for rep in range(REPS):
    for name, exe, extra in VARIANTS:  # alternating: every variant once per repetition
        ws = host(exe, SHORT, extra)
        wl = host(exe, LONG, extra)
        ms = 1e3 * (wl - ws) / (LONG - SHORT)
        res[name].append(ms)
        say("rep %d %-8s wall(%d) %.3f s wall(%d) %.3f s -> %.3f ms/step" % (rep, name, SHORT, ws, LONG, wl, ms))
for name, v in res.items():
    say("%-8s ms/step %s mean %.3f spread %.3f" % (name, ", ".join("%.3f" % x for x in v), sum(v) / len(v), max(v) - min(v)))

# the kernels alone, interleaved: every configuration once per round, 512 MB through the caches between two calls as a model step would
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nextsimdg_amd import abi  # noqa: E402

ctx = abi.Context(torch.device("cuda:0"))
nx = ny = 2048
ctx.set_grid(nx, ny, 250.0, 250.0)
g = torch.Generator(device="cuda").manual_seed(1)
r = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)
src = {"H": r(6, ny, nx), "A": r(6, ny, nx), "u": r(2 * ny + 1, 2 * nx + 1), "v": r(2 * ny + 1, 2 * nx + 1), "hsnow": r(ny, nx)}
dst = torch.empty(64 * 1024 * 1024, dtype=torch.float64, device="cuda")
DEFAULT = ("hice", "cice", "u", "v")
pairs = lambda entries: [tuple(e.split(":")) if ":" in e else (e, "mean") for e in entries]
WEIGHTED = DEFAULT + ("speed:ice_mean", "hice:ice_mean", "hice:max")
acc4, acc7, wacc = (torch.zeros(n, ny, nx, dtype=torch.float64, device="cuda") for n in (4, 7, 1))
out = torch.zeros(7, ny, dtype=torch.float64, device="cuda")
CALLS = [
    ("accumulate, default list (4 planes)", lambda store: ctx.history_accumulate(0, ny, DEFAULT, src, store, 0, acc4)),
    ("accumulate_stats, default list as means (4)", lambda store: ctx.history_accumulate_stats(0, ny, pairs(DEFAULT), src, store, 0, acc4, None)),
    ("accumulate_stats, + 2 ice_mean + 1 max (7 + weights)", lambda store: ctx.history_accumulate_stats(0, ny, pairs(WEIGHTED), src, store, 0, acc7, wacc[0])),
    ("row_totals, all seven quantities", lambda store: ctx.history_row_totals(0, ny, abi.SERIES_QUANTITIES, src, 0.15, 0, out)),
]
times = {label: [] for label, _ in CALLS}
for it in range(12):
    for label, call in CALLS:
        dst.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(it == 0)
        b.record()
        torch.cuda.synchronize()
        times[label].append(a.elapsed_time(b))
kern = {}
for label, t in times.items():
    t = sorted(t[2:])
    kern[label] = t
    say("kernel %-52s median %.4f ms min %.4f max %.4f (10 calls)" % (label, t[len(t) // 2], t[0], t[-1]))
ctx.close()
json.dump({"ms_per_step": res, "kernel_ms": kern}, open(os.path.join(OUT, "stats_cost.json"), "w"), indent=1)
shutil.rmtree(work, ignore_errors=True)
say("done")

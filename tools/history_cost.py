"""Cost of the history output at 2048^2 (profiles/history_output.md): the step time through the C++ host with the keys off, with the
default field list and with all dynamics fields -- and, with --parent-exe, of another build of nextsim_amd (the parent commit's) -- in
alternating runs, as the wall-clock difference of a long and a short run; the flush per window from the timer tree; the kernel alone
from stream events through the Python binding.  Ends at the first failure.

    python tools/history_cost.py --out DIR [--parent-exe PATH/nextsim_amd] [--reps 4]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True, help="directory for cost.log and cost.json")
ap.add_argument("--parent-exe", default=None, help="nextsim_amd of another build to alternate with")
ap.add_argument("--reps", type=int, default=4)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = args.out
os.makedirs(OUT, exist_ok=True)
EXE = {"this": os.path.join(ROOT, "nextsimdg_amd", "host", "build", "nextsim_amd"), "parent": args.parent_exe}
ALL = "hice,cice,u,v,speed,divergence,shear,sigma_n,sigma_s"
REPS, SHORT, LONG = args.reps, 20, 220
work = tempfile.mkdtemp(prefix="hist_cost_")
log = open(os.path.join(OUT, "cost.log"), "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def host(exe, steps, extra=(), keep_output=False):
    cfg = os.path.join(work, "c.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = %d\n"
                "final_file = %s\n[rectgrid]\nnx = 2048\nny = 2048\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 512e3\nnsub = 120\n"
                % (120 * steps, os.path.join(work, "final.nsdg")))
    t0 = time.perf_counter()
    p = subprocess.run([EXE[exe], "--config-file", cfg] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=work, timeout=180)
    wall = time.perf_counter() - t0
    out = p.stdout.decode()
    if p.returncode != 0:
        say("FAILED rc", p.returncode, out[-2000:])
        shutil.rmtree(work, ignore_errors=True)
        sys.exit(1)
    for name in os.listdir(work):
        if name.startswith("ice.") or name == "final.nsdg":
            os.remove(os.path.join(work, name))
    return wall, out


def on(fields, period=120 * 100000, name="ice.nsdg"):
    return ["--model.output_period=%d" % period, "--model.output_file=" + name, "--model.output_fields=" + fields]


VARIANTS = [("off", "this", []), ("parent", "parent", []), ("default", "this", on("hice,cice,u,v")), ("all", "this", on(ALL))]
VARIANTS = [v for v in VARIANTS if EXE[v[1]]]
res = {v[0]: [] for v in VARIANTS}
for rep in range(REPS):
    for name, exe, extra in VARIANTS:  # alternating: every variant once per repetition
        ws, _ = host(exe, SHORT, extra)
        wl, _ = host(exe, LONG, extra)
        ms = 1e3 * (wl - ws) / (LONG - SHORT)
        res[name].append(ms)
        say("rep %d %-8s wall(%d) %.3f s wall(%d) %.3f s -> %.3f ms/step" % (rep, name, SHORT, ws, LONG, wl, ms))
for name, v in res.items():
    say("%-8s ms/step %s mean %.3f spread %.3f" % (name, ", ".join("%.3f" % x for x in v), sum(v) / len(v), max(v) - min(v)))

# the flush: 40 steps, a window of 10, under model.timing = true (a device synchronisation at every tock: the node holds the flush alone)
for label, fields, fname in (("default .nsdg", "hice,cice,u,v", "ice.nsdg"), ("all .nsdg", ALL, "ice.nsdg"), ("default .nc", "hice,cice,u,v", "ice.nc")):
    _, out = host("this", 40, on(fields, 1200, fname) + ["--model.timing=true"])
    for line in out.splitlines():
        if "history flush" in line or "iterate:" in line:
            say("flush [%s] %s" % (label, line.strip()))

# the kernel alone
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nextsimdg_amd import abi  # noqa: E402

ctx = abi.Context(torch.device("cuda:0"))
nx = ny = 2048
ctx.set_grid(nx, ny, 250.0, 250.0)
g = torch.Generator(device="cuda").manual_seed(1)
r = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=g)
src = {"H": r(6, ny, nx), "A": r(6, ny, nx), "D": r(6, ny, nx), "u": r(2 * ny + 1, 2 * nx + 1), "v": r(2 * ny + 1, 2 * nx + 1),
       "hsnow": r(ny, nx), "tice": r(ny, nx)}
for k in ("s11", "s12", "s22"):
    src[k] = r(ny, (nx + 63) // 64, 8 * 64)
dst = torch.empty(64 * 1024 * 1024, dtype=torch.float64, device="cuda")
kern = {}
for label, fields in (("default (4)", ("hice", "cice", "u", "v")), ("dynamics (9)", tuple(ALL.split(","))), ("all (12)", abi.HISTORY_FIELDS)):
    acc = torch.zeros(len(fields), ny, nx, dtype=torch.float64, device="cuda")
    times = []
    for it in range(12):
        dst.zero_()  # 512 MB through the caches between two samples, as a model step would
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.history_accumulate(0, ny, fields, src, it == 0, 0, acc)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times = sorted(times[2:])
    kern[label] = times
    say("kernel %-13s median %.4f ms min %.4f max %.4f (10 calls, add)" % (label, times[len(times) // 2], times[0], times[-1]))
t0 = time.perf_counter()
host_copy = acc.cpu().numpy() / 3.0
say("download + divide of 12 planes of 2048^2: %.1f ms" % (1e3 * (time.perf_counter() - t0)))
ctx.close()
json.dump({"ms_per_step": res, "kernel_ms": kern}, open(os.path.join(OUT, "cost.json"), "w"), indent=1)
shutil.rmtree(work, ignore_errors=True)
say("done")

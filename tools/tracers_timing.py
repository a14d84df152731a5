"""Ice tracers (include/nsdg.h "ice tracers"): device time of nsdg_tracers_weight for four tracers at order 2 on a 2048 x 2048 grid beside
four calls of nsdg_tracer_weight, in one process and alternating (torch events around 20 launches, after 3 to warm up, 6 rounds each),
with the bytes each form moves and the rate that makes; nsdg_tracers_recover and nsdg_tracers_dilute likewise; then the time of a model
step of a native DynamicsCore with 0, 1 and 4 tracers, alternating (profiles/tracers.md).  Run: python tools/tracers_timing.py [n]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
NT, NC = 4, 6
ctx = abi.Context(torch.device("cuda:0"))
ctx.set_grid(n, n, 250.0, 250.0)
g = torch.Generator(device="cuda").manual_seed(1)
rand = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=g)
H, A = rand(NC, n, n), rand(NC, n, n)
T = [rand(n, n) for _ in range(NT)]
Q = [torch.zeros(NC, n, n, dtype=torch.float64, device="cuda") for _ in range(NT)]
Q1 = [torch.zeros(NC, n, n, dtype=torch.float64, device="cuda") for _ in range(NT)]
hb, ha = rand(n, n), rand(n, n) + 0.5


def window(call, launches=20):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches


def alternate(calls, rounds=6):
    """{name: [ms per call, one per round]}: the forms take turns inside every round"""
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            times[name].append(window(call))
    return times


def four_calls():
    for k in range(NT):
        ctx.tracer_weight(2, 0, n, H, T[k], Q1[k])


fused = lambda: ctx.tracers_weight(2, 0, n, H, T, Q)
fused()
four_calls()
torch.cuda.synchronize()
assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(Q, Q1)), "the two forms differ"
doubles = {"fused": NC + NT + NT * NC, "four calls": NT * (NC + 1 + NC)}  # per element: 34 against 52
for name, t in alternate({"fused": fused, "four calls": four_calls}).items():
    print("weight, %-10s ms per %d tracers: %s; %d doubles per element, %.0f GB/s at the fastest"
          % (name, NT, " ".join("%.4f" % x for x in t), doubles[name], 8 * doubles[name] * n * n / (min(t) * 1e-3) / 1e9))
kinds = (abi.TRACER_AGE, 0, 0, 0)
others = {"recover": (lambda: ctx.tracers_recover(2, 0, n, H, A, Q, kinds, 120.0, 1e-12, 0.01, T), 2 + 2 * NT),
          "dilute": (lambda: ctx.tracers_dilute(0, n, hb, ha, T), 2 + 2 * NT)}
for name, t in alternate({k: v[0] for k, v in others.items()}).items():
    print("%-7s ms per %d tracers: %s; at most %d doubles per element, %.0f GB/s at the fastest"
          % (name, NT, " ".join("%.4f" % x for x in t), others[name][1], 8 * others[name][1] * n * n / (min(t) * 1e-3) / 1e9))

# ---- the model step with 0, 1 and 4 tracers: native DynamicsCore, the box test's cyclone
bt = synthetic.BoxTest(n, n, n * 250.0)
ctx.set_mevp_params(ctx.mevp_default_params(**bt.subcycle_parameters(120.0)))
Hh, Ah = bt.dg_fields()
uo, vo = bt.ocean()
ua, va = bt.wind(0.0)
cores, made = {}, []
for names in ((), ("age",), ("age", "a", "b", "c")):
    core = rowblock.DynamicsCore(ctx, rowblock.RowBlock(n, n), bt.hx, bt.hy, 120.0, 100, torch.device("cuda"), native=True, tracers=names)
    core.load_global(Hh, Ah, uo, vo, ua, va)
    if names:
        core.load_tracers({k: np.full((n, n), 3.0) for k in names if k != "age"})
    made.append(core)
    cores["%d tracers" % len(names)] = core.step
for name, t in alternate(cores, rounds=4).items():
    print("model step (nsub 100), %s: ms per step over 20 steps: %s" % (name, " ".join("%.3f" % x for x in t)))
for core in made:
    core.close()
ctx.close()

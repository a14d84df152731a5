"""nsdg_drifters_advance: device time for 10^6 drifters on a 2048 x 2048 grid (torch events around 20 launches, after 3 to warm up), in
the random order of their seeding and sorted by element (profiles/drifters.md).  Run: python tools/drifters_timing.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextsimdg_amd import abi  # noqa: E402

nx = ny = 2048
h, dt, n = 250.0, 120.0, 1000000
ctx = abi.Context(torch.device("cuda:0"))
ctx.set_grid(nx, ny, h, h)
g = torch.Generator(device="cuda").manual_seed(1)
u = (torch.rand(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda", generator=g) - 0.5) * 0.6
v = (torch.rand(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda", generator=g) - 0.5) * 0.6
A = torch.ones(6, ny, nx, dtype=torch.float64, device="cuda")
d = torch.zeros(3, n, dtype=torch.float64, device="cuda")
d[:2] = torch.rand(2, n, dtype=torch.float64, device="cuda", generator=g) * (nx * h)
e = torch.empty_like(d)
for k in range(3):
    ctx.drifters_advance(0, ny, dt, 0.15, u, v, A, d, e)
    d, e = e, d
torch.cuda.synchronize()
times = []
for rep in range(5):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for k in range(20):
        ctx.drifters_advance(0, ny, dt, 0.15, u, v, A, d, e)
        d, e = e, d
    t1.record()
    torch.cuda.synchronize()
    times.append(t0.elapsed_time(t1) / 20)
print("drifters_advance n=%d on %dx%d: per launch ms, 5 repeats of 20: %s; active after the run: %d"
      % (n, nx, ny, " ".join("%.4f" % t for t in times), int((d[2] == 0).sum())))
# the same drifters sorted by element (what a seeded array looks like): neighbours in the list are neighbours on the mesh
key = torch.floor(d[1] / h) * nx + torch.floor(d[0] / h)
d = d[:, torch.argsort(key)].contiguous()
e = torch.empty_like(d)
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0.record()
for k in range(20):
    ctx.drifters_advance(0, ny, dt, 0.15, u, v, A, d, e)
    d, e = e, d
t1.record()
torch.cuda.synchronize()
print("the same list sorted by element: %.4f ms per launch" % (t0.elapsed_time(t1) / 20))
ctx.close()

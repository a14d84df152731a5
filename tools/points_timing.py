"""nsdg_points_sample: device time for 10^6 points on a 2048 x 2048 grid (torch events around 20 launches, after 3 to warm up), in random
order and sorted by element, with the default three fields (hice cice shear) and with all twelve, beside nsdg_drifters_advance on the same
points in the same run (profiles/points.md).  Prints the bytes a launch asks for and the rate that makes.  Run: python tools/points_timing.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nextsimdg_amd import abi  # noqa: E402

nx = ny = 2048
h, dt, n = 250.0, 120.0, 1000000
ctx = abi.Context(torch.device("cuda:0"))
ctx.set_grid(nx, ny, h, h)
g = torch.Generator(device="cuda").manual_seed(1)
rand = lambda *s: torch.rand(*s, dtype=torch.float64, device="cuda", generator=g)
src = {"u": (rand(2 * ny + 1, 2 * nx + 1) - 0.5) * 0.6, "v": (rand(2 * ny + 1, 2 * nx + 1) - 0.5) * 0.6, "H": rand(6, ny, nx), "A": rand(6, ny, nx),
       "D": rand(6, ny, nx), "hsnow": rand(ny, nx), "tice": rand(ny, nx)}
for name in ("s11", "s12", "s22"):
    src[name] = rand(ny * ((nx + 63) // 64) * 8 * 64)
d = torch.zeros(3, n, dtype=torch.float64, device="cuda")
d[:2] = rand(2, n) * (nx * h)
key = torch.floor(d[1] / h) * nx + torch.floor(d[0] / h)
lists = {"random": d, "sorted by element": d[:, torch.argsort(key)].contiguous()}
# bytes a point asks for: its coordinates, the sources of the list (DG fields 6 planes, 9 nodes, 8 stress coefficients), one store per field
reads = {"hice": 48, "cice": 48, "damage": 48, "u": 72, "v": 72, "s11": 64, "s12": 64, "s22": 64, "hsnow": 8, "tice": 8}
needs = {"hice": ("hice",), "cice": ("cice",), "damage": ("damage",), "u": ("u",), "v": ("v",), "speed": ("u", "v"), "divergence": ("u", "v"),
         "shear": ("u", "v"), "sigma_n": ("s11", "s22"), "sigma_s": ("s11", "s12", "s22"), "hsnow": ("hsnow",), "tice": ("tice",)}


def timed(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            call()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / 20)
    return times


for order, pts in lists.items():
    e = torch.empty_like(pts)
    t = timed(lambda: ctx.drifters_advance(0, ny, dt, 0.15, src["u"], src["v"], src["A"], pts, e))
    print("%s: drifters_advance  ms per launch, 5 repeats of 20: %s" % (order, " ".join("%.4f" % x for x in t)))
    for fields in (("hice", "cice", "shear"), abi.HISTORY_FIELDS):
        out = torch.empty(len(fields), n, dtype=torch.float64, device="cuda")
        t = timed(lambda: ctx.points_sample(0, ny, 2, pts[0], pts[1], fields, src, out))
        asked = 16 + sum(reads[s] for s in {s for f in fields for s in needs[f]}) + 8 * len(fields)
        print("%s: points_sample %2d fields  ms per launch: %s; %d bytes asked per point, %.0f GB/s at the fastest"
              % (order, len(fields), " ".join("%.4f" % x for x in t), asked, asked * n / (min(t) * 1e-3) / 1e9))
ctx.close()

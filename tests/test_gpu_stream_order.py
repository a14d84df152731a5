"""Every ABI call on a stream that is not the null stream (include/nsdg.h "Streams"; the protocol: tests/stream_order.py).

Every other test of the suite binds its contexts to torch's current stream, which is the legacy null stream: the one stream that orders
itself against everything.  There a launch that goes to stream 0 instead of the context's, work left on an internal non-blocking stream
without a join, a blocking null-stream copy and state shared by two contexts all give right answers.  Here

  A. every entry point that touches the device runs between a late producer and an early consumer on a side stream (TABLE; the
     rows and tests/test_stream_order_cpu.py::HOST_ONLY partition the header), and a setter between two enqueued calls acts on the
     second only;
  B. two contexts on two streams, with different grids, parameters, variants, masks and rheologies, interleaved from one host thread;
  C. the Python drivers built and stepped under a side stream;
  D. thread ranks that own their streams (tests/thread_ranks.py own_stream=True) against the single domain on the default stream.

Everything is compared bit for bit: no tolerance anywhere.

The delay of part A is a chain of fp64 torch.mm of 2048^2 on the side stream: ordinary work that ends by itself.  Its length is not fixed
in advance: the module fixture `proto` times one product with events, times the longest warmed host-side stretch of any asynchronous row
(from the enqueue of the producer's copies to the return of the call) and takes at least 10 times that, and never less than 64 products.
Measured on the MI355X (printed by the fixture on every run; two runs):
    one 2048^2 fp64 product                      0.416 ms, 0.433 ms
    longest warmed host-side stretch             0.371 ms (rb_bbm_run[loopback]), 0.321 ms (column_step[1025]: fifteen producer copies);
                                                 the calls alone take 0.01 to 0.18 ms on the host, the blocking ones the delay
    ten times that                               3.7 ms
    chosen delay                                 64 products = 17.9 ms: 48 times the longest stretch
The factor 10 of the rule was never too tight here (with the 16 products = 4.8 ms = 15 times of the first run every row kept its gate
closed); the floor of 64 products is there because 4 ms is less than one scheduling quantum of a shared host.
"""
import math
import threading
import time
import types

import numpy as np
import pytest
import torch

import bbm_cases as Bc
import column_path_cases as Cc
import drifters_cases as Dc
import land_ref
import mevp_cases as Mc
import points_cases as Pc
import stream_order as SO
import transport_cases as Tc
from nextsimdg_amd import abi, rowblock
from stream_order import SENTINEL, Case

pytestmark = pytest.mark.gpu

REAL, DECOY = 12, 13  # seeds of the case builders: the inputs of a row and its decoy, another valid case of the same builder
DELAY_FACTOR = 10  # the delay is at least this many times the longest warmed host-side stretch of an asynchronous row
# never fewer than 64 products (about 20 ms): ten times the longest stretch is 3 ms, less than a scheduling quantum of a shared host -- a
# host thread that loses the processor once between the delay and the gate's query would fail a row that is in order
DELAY_MIN_PRODUCTS, DELAY_MAX_MS, MM = 64, 500.0, 2048
_groups = [52000]  # ids of the in-process communicator groups of this module


def next_group():
    _groups[0] += 1
    return _groups[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tdev(planes):
    return abi.tile(dev(planes))


def sentinel_like(*ts):
    return [torch.full_like(t, SENTINEL) for t in ts]


def work_of(real, decoy, names):
    """work buffers of the named arrays (holding the decoy) and their (work, real, decoy) triples"""
    w = {k: decoy[k].clone() for k in names}
    return w, [(w[k], real[k], decoy[k]) for k in names]


def island(nx, ny):
    """the island across the wave seam and the rock of bbm_cases.island() (70 x 9); at 130 x 5 an island across the tile seam at column
    64 and a rock on the top row"""
    if (nx, ny) == (70, 9):
        return Bc.island()
    assert (nx, ny) == (130, 5)
    land = np.zeros((ny, nx), dtype=bool)
    land[1:4, 60:67] = True
    land[4, 3] = True
    return land


def clear_land(c, land, nodal, planes):
    """no ice, no stress, no motion on land -- and, unlike the case builders' own masks, a finite wind: a decoy is never a NaN"""
    ln = land_ref.land_nodes(land)
    for k in planes:
        for f in (c[k] if isinstance(c[k], list) else [c[k]]):
            f[:, land] = 0.0
    for k in nodal:
        c[k][ln] = 0.0


# ---- the contexts of one side of the comparison: bound to the side stream, or to the default stream -----------------------------------------
class Env:
    def __init__(self, gpu, stream):
        self.gpu, self.stream = gpu, stream
        self.ctx = self.context()
        self.loop = self.context()  # a communicator of one rank whose neighbours are the rank itself
        self.loop.comm_init_local(next_group(), 0, 1)
        self.timed = self.context()
        self.timed.phase_timing(True)
        g = next_group()
        self.pair = (self.context(), self.context(torch.cuda.Stream() if stream is not None else None))  # ranks 0 and 1 of a world of two
        for r, c in enumerate(self.pair):
            c.comm_init_local(g, r, 2)
            c.comm_deadline(20.0)  # a rank that fails must not keep its peer waiting for long
        self.families, self.cases = {}, {}

    def context(self, stream=None):
        stream = stream or self.stream
        return abi.Context(self.gpu) if stream is None else abi.Context(self.gpu, stream=stream)

    def family(self, cls, ctx, *key):
        k = (cls.__name__, id(ctx)) + key
        if k not in self.families:
            torch.cuda.synchronize()
            self.families[k] = cls(ctx, *key)
            torch.cuda.synchronize()
        return self.families[k]

    def close(self):
        for c in self.cases.values():
            for plan in (c.keep or ()):
                plan.close()
        self.cases.clear()
        self.families.clear()
        for c in (self.loop,) + self.pair:
            c.comm_finalize()
        for c in (self.ctx, self.loop, self.timed) + self.pair:
            c.close()


# ---- families: the real and the decoy arrays of one builder on one grid, the derived inputs made by the calls a model step makes ----------
class Mevp:
    """mevp_cases.build(nx, ny, seed, "plastic"): alpha != beta, uniform"""

    def __init__(self, ctx, nx, ny, masked=False):
        self.ctx, self.nx, self.ny = ctx, nx, ny
        land = island(nx, ny) if masked else None
        self.mask = None if land is None else dev(land.astype(np.uint8))
        self.real, self.decoy = self.fields(REAL, land), self.fields(DECOY, land)
        self.tmp = torch.zeros_like(self.real["packed"])

    def fields(self, seed, land):
        self.case = case = Mc.build(self.nx, self.ny, seed, "plastic")
        c, ctx, nx, ny = case["c"], self.ctx, self.nx, self.ny
        if land is not None:
            clear_land(c, land, ("u", "v", "u0", "v0"), ("H", "A", "S"))
        d = {k: dev(c[k]) for k in ("H", "A", "u", "v", "u0", "v0", "ua", "va", "uo", "vo")}
        for k, x in zip(("s11", "s12", "s22"), c["S"]):
            d[k] = tdev(x)
        self.state()
        torch.cuda.synchronize()
        d["pg"] = ctx.private_zeros(9, ny, nx, "cuda")
        d["packed"] = torch.zeros(8 * d["u"].numel(), dtype=torch.float64, device="cuda")
        for k in ("cgh", "cga", "tax", "tay"):
            d[k] = torch.zeros_like(d["u"])
        torch.cuda.synchronize()
        ctx.ice_strength(d["H"], d["A"], d["pg"])
        ctx.mevp_prepare(case["dt"], d["H"], d["A"], (d["ua"], d["va"]), (d["uo"], d["vo"]), (d["u0"], d["v0"]), d["packed"])
        ctx.dg_to_cg(d["H"], d["cgh"])
        ctx.dg_to_cg(d["A"], d["cga"])
        ctx.wind_stress(d["ua"], d["va"], d["tax"], d["tay"])
        torch.cuda.synchronize()
        return d

    def state(self, variant=abi.DEFAULT_MEVP_VARIANT, strip_rows=0):
        ctx, case = self.ctx, self.case
        ctx.set_mevp_params(ctx.mevp_default_params(**case["par"]))
        ctx.set_grid(self.nx, self.ny, case["hx"], case["hy"])
        ctx.set_land_mask(self.mask)
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_strip_rows(strip_rows)

    def setup(self, variant=abi.DEFAULT_MEVP_VARIANT):
        """the setters, and the context's memory of the last packing (time step, parameters, whether it saw a mask)"""
        self.state(variant)
        r = self.real
        self.ctx.mevp_prepare(self.case["dt"], r["H"], r["A"], (r["ua"], r["va"]), (r["uo"], r["vo"]), (r["u0"], r["v0"]), self.tmp)


class Bbm:
    """bbm_cases.build(nx, ny, seed, "branches")"""

    def __init__(self, ctx, nx, ny, masked=False):
        self.ctx, self.nx, self.ny = ctx, nx, ny
        land = island(nx, ny) if masked else None
        self.mask = None if land is None else dev(land.astype(np.uint8))
        self.real, self.decoy = self.fields(REAL, land), self.fields(DECOY, land)
        self.tmp = torch.zeros_like(self.real["packed"])

    def fields(self, seed, land):
        self.case = case = Bc.build(self.nx, self.ny, seed, "branches")
        c, ctx, nx, ny = case["c"], self.ctx, self.nx, self.ny
        if land is not None:
            clear_land(c, land, ("u", "v"), ("H", "A", "D", "S"))
        d = {k: dev(c[k]) for k in ("H", "A", "D", "u", "v", "ua", "va", "uo", "vo")}
        for k, x in zip(("s11", "s12", "s22"), c["S"]):
            d[k] = tdev(x)
        self.zero = torch.zeros_like(d["u"])
        for k in ("hg", "eg", "pm"):
            d[k] = ctx.private_zeros(9, ny, nx, "cuda")
        d["packed"] = torch.zeros(8 * d["u"].numel(), dtype=torch.float64, device="cuda")
        self.state()
        torch.cuda.synchronize()
        ctx.bbm_prepare(d["H"], d["A"], d["hg"], d["eg"], d["pm"])
        ctx.mevp_prepare(case["dts"], d["H"], d["A"], (d["ua"], d["va"]), (d["uo"], d["vo"]), (self.zero, self.zero), d["packed"])
        torch.cuda.synchronize()
        return d

    def state(self):
        ctx, case = self.ctx, self.case
        ctx.set_mevp_params(ctx.mevp_default_params(**case["mevp"]))
        ctx.set_bbm_params(ctx.bbm_default_params(**case["bbm"]))
        ctx.set_grid(self.nx, self.ny, case["hx"], case["hy"])
        ctx.set_land_mask(self.mask)
        ctx.set_mevp_strip_rows(0)

    def setup(self):
        self.state()
        r = self.real
        self.ctx.mevp_prepare(self.case["dts"], r["H"], r["A"], (r["ua"], r["va"]), (r["uo"], r["vo"]), (self.zero, self.zero), self.tmp)


class Transport:
    """transport_cases: four bounded fields and a random velocity with in- and outflow on every side; the time step is the real case's"""

    def __init__(self, ctx, nx, ny, order):
        self.ctx, self.nx, self.ny, self.order = ctx, nx, ny, order
        self.nc = Tc.NCOEF[order]
        self.real, self.decoy = self.fields(REAL), self.fields(DECOY)
        self.dt = self.real.pop("dt")
        self.decoy.pop("dt")

    def fields(self, seed):
        nx, ny, order, ctx = self.nx, self.ny, self.order, self.ctx
        u, v = Tc.velocity(nx, ny, seed)
        d = {"f%d" % f: dev(Tc.bounded_field(nx, ny, order, f, seed)) for f in range(4)}
        d.update(u=dev(u), v=dev(v), dt=Tc.time_step(u, v), T=dev(np.random.default_rng(seed).uniform(-30.0, -1.0, (ny, nx))))
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
        d.update(vx=z(self.nc, ny, nx), vy=z(self.nc, ny, nx), unx=z(order + 1, ny, nx + 1), uny=z(order + 1, ny + 1, nx))
        self.setup()
        torch.cuda.synchronize()
        ctx.prepare_advection(order, d["u"], d["v"], d["vx"], d["vy"], d["unx"], d["uny"])
        torch.cuda.synchronize()
        return d

    def setup(self, bounds=2):
        self.ctx.set_grid(self.nx, self.ny, Tc.HX, Tc.HY)
        self.ctx.set_transport_variant(abi.DEFAULT_TRANSPORT_VARIANT)
        self.ctx.set_transport_bounds(Tc.BOUNDS[:bounds])


ADV = ("vx", "vy", "unx", "uny")


class Samples:
    """points_cases.make: every source of the history, series and point-sample calls, and the points"""

    def __init__(self, ctx, nx, ny, n):
        self.ctx, self.nx, self.ny, self.n = ctx, nx, ny, n
        self.real, self.decoy = self.fields(0), self.fields(1)

    def fields(self, seed):
        c = Pc.make(self.nx, self.ny, self.n, 2, "bbm", seed)
        s = c["src"]
        d = {k: dev(s[k]) for k in ("H", "A", "D", "u", "v", "hsnow", "tice")}
        for k in ("s11", "s12", "s22"):
            d[k] = tdev(s[k + "p"])  # the lanes no element owns are zero, not NaN
        d["x"], d["y"] = dev(c["x"]), dev(c["y"])
        rng = np.random.default_rng(seed + 5)
        d["acc"], d["wacc"] = dev(rng.uniform(0.0, 2.0, (3, self.ny, self.nx))), dev(rng.uniform(0.0, 2.0, (self.ny, self.nx)))
        return d

    def setup(self):
        self.ctx.set_grid(self.nx, self.ny, Pc.HX, Pc.HY)
        self.ctx.set_block(0, self.ny)
        self.ctx.set_land_mask(None)


SOURCES = ("H", "A", "D", "u", "v", "s11", "s12", "s22", "hsnow", "tice")


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------------
def stress_rows_outside(t, k0, k1):
    """the element rows of a tiled array [ny, tiles, 8 * 64] outside [k0, k1)"""
    return [t[:k0], t[k1:]]


def row_mevp_pass(fn, nx, ny, rows, variant=abi.DEFAULT_MEVP_VARIANT, masked=False):
    """nsdg_mevp_iterate* `fn` of abi.Context on the row arguments `rows`"""

    def build(env):
        F = env.family(Mevp, env.ctx, nx, ny, masked)
        w, inputs = work_of(F.real, F.decoy, ("s11", "s12", "s22", "u", "v", "packed", "pg"))
        out = sentinel_like(w["s11"], w["s12"], w["s22"], w["u"], w["v"])
        call = lambda: getattr(env.ctx, fn)(*rows, [w["s11"], w["s12"], w["s22"]], out[:3], (w["u"], w["v"]), (out[3], out[4]), w["packed"], w["pg"])
        untouched = None
        if fn == "mevp_iterate" and rows != (0, 0, ny):
            k0, j0, j1 = rows
            g1 = 2 * j1 + (1 if j1 == ny else 0)
            untouched = lambda seen: [p for t in seen[:3] for p in stress_rows_outside(t, k0, j1)] + [p for t in seen[3:] for p in (t[:2 * j0], t[g1:])]
        return Case(call, inputs, out, fill=out, setup=lambda: F.setup(variant), untouched=untouched)

    return build


def row_mevp_subcycle(nx, ny, nsub):
    def build(env):
        F = env.family(Mevp, env.ctx, nx, ny)
        names = ("s11", "s12", "s22", "u", "v", "u0", "v0", "tax", "tay", "uo", "vo", "cgh", "cga", "pg")
        w, inputs = work_of(F.real, F.decoy, names)
        scratch = torch.zeros(10 * w["u"].numel() + 3 * w["s11"].numel(), dtype=torch.float64, device="cuda")
        call = lambda: env.ctx.mevp_subcycle(F.case["dt"], nsub, [w["s11"], w["s12"], w["s22"]], w["u"], w["v"], w["u0"], w["v0"], w["tax"], w["tay"],
                                             w["uo"], w["vo"], w["cgh"], w["cga"], w["pg"], scratch)
        return Case(call, inputs, [w[k] for k in ("s11", "s12", "s22", "u", "v")], setup=lambda: F.setup(4))

    return build


def row_mevp_helper(name, nx=130, ny=5, masked=False):
    def build(env):
        F, ctx = env.family(Mevp, env.ctx, nx, ny, masked), env.ctx
        dt = F.case["dt"]
        if name == "wind_stress":
            w, inputs = work_of(F.real, F.decoy, ("ua", "va"))
            out = sentinel_like(w["ua"], w["va"])
            call = lambda: ctx.wind_stress(w["ua"], w["va"], out[0], out[1])
        elif name == "ice_strength":
            w, inputs = work_of(F.real, F.decoy, ("H", "A"))
            out = sentinel_like(F.real["pg"])
            call = lambda: ctx.ice_strength(w["H"], w["A"], out[0], 1, ny - 1)
            return Case(call, inputs, out, fill=out, setup=F.setup, untouched=lambda seen: stress_rows_outside(seen[0], 1, ny - 1))
        elif name == "dg_to_cg":
            w, inputs = work_of(F.real, F.decoy, ("H",))
            out = sentinel_like(F.real["cgh"])
            call = lambda: ctx.dg_to_cg(w["H"], out[0])
        elif name == "mevp_stress":
            w, inputs = work_of(F.real, F.decoy, ("u", "v", "pg", "s11", "s12", "s22"))
            call = lambda: ctx.mevp_stress(0, ny, w["u"], w["v"], w["pg"], w["s11"], w["s12"], w["s22"])
            return Case(call, inputs, [w["s11"], w["s12"], w["s22"]], setup=F.setup)
        elif name == "mevp_pack_nodal":
            w, inputs = work_of(F.real, F.decoy, ("u0", "v0", "tax", "tay", "uo", "vo", "cgh", "cga"))
            out = sentinel_like(F.real["packed"])
            call = lambda: ctx.mevp_pack_nodal(dt, (w["u0"], w["v0"]), (w["tax"], w["tay"]), (w["uo"], w["vo"]), w["cgh"], w["cga"], out[0])
        elif name == "mevp_prepare":
            w, inputs = work_of(F.real, F.decoy, ("H", "A", "ua", "va", "uo", "vo", "u0", "v0"))
            out = sentinel_like(F.real["packed"])
            call = lambda: ctx.mevp_prepare(dt, w["H"], w["A"], (w["ua"], w["va"]), (w["uo"], w["vo"]), (w["u0"], w["v0"]), out[0])
        elif name == "mevp_velocity":
            w, inputs = work_of(F.real, F.decoy, ("s11", "s12", "s22", "u", "v", "packed"))
            out = sentinel_like(w["u"], w["v"])
            call = lambda: ctx.mevp_velocity(0, ny, [w["s11"], w["s12"], w["s22"]], (w["u"], w["v"]), (out[0], out[1]), w["packed"])
        elif name == "concentration_max":
            w, inputs = work_of(F.real, F.decoy, ("H", "A"))
            return Case(lambda: ctx.concentration_max(w["H"], w["A"]), inputs, [], setup=F.setup)
        elif name == "land_clear_nodes":
            w, inputs = work_of(F.real, F.decoy, ("ua", "va"))  # the wind is non-zero on land
            other = dev(np.roll(island(nx, ny), 5, axis=1).astype(np.uint8))
            mask = other.clone()
            inputs.append((mask, F.mask, other))  # the mask is an array argument like any other: stream-ordered

            def setup():
                F.setup()
                ctx.set_land_mask(mask)

            return Case(lambda: ctx.land_clear_nodes(w["ua"], w["va"]), inputs, [w["ua"], w["va"]], setup=setup)
        elif name == "land_clear":
            w, inputs = work_of(F.real, F.decoy, ("ua",))
            f = {k: dev(np.random.default_rng(s).uniform(0.5, 1.5, (6, ny, nx))) for k, s in (("real", 1), ("decoy", 2))}
            wf = f["decoy"].clone()
            other = dev(np.roll(island(nx, ny), 5, axis=1).astype(np.uint8))
            mask = other.clone()

            def setup():
                F.setup()
                ctx.set_land_mask(mask)

            return Case(lambda: ctx.land_clear(wf, 1, ny - 1), [(wf, f["real"], f["decoy"]), (mask, F.mask, other)], [wf], setup=setup)
        return Case(call, inputs, out, fill=out, setup=F.setup)

    return build


def row_bbm(name, nx, ny, masked=False):
    def build(env):
        F, ctx = env.family(Bbm, env.ctx, nx, ny, masked), env.ctx
        if name == "bbm_prepare":
            w, inputs = work_of(F.real, F.decoy, ("H", "A"))
            out = sentinel_like(F.real["hg"], F.real["eg"], F.real["pm"])
            j0, j1 = (1, ny - 1) if ny > 2 else (0, ny)
            call = lambda: ctx.bbm_prepare(w["H"], w["A"], out[0], out[1], out[2], j0, j1)
            return Case(call, inputs, out, fill=out, setup=F.setup, untouched=lambda seen: [p for t in seen for p in stress_rows_outside(t, j0, j1)])
        w, inputs = work_of(F.real, F.decoy, ("s11", "s12", "s22", "D", "u", "v", "packed", "hg", "eg", "pm"))
        out = sentinel_like(w["s11"], w["s12"], w["s22"], w["D"], w["u"], w["v"])
        call = lambda: ctx.bbm_iterate(0, 0, ny, [w["s11"], w["s12"], w["s22"]], out[:3], w["D"], out[3], (w["u"], w["v"]), (out[4], out[5]), w["packed"],
                                       (w["hg"], w["eg"], w["pm"]))
        return Case(call, inputs, out, fill=out, setup=F.setup)

    return build


def row_transport(name, nx, ny, order):
    def build(env):
        F, ctx = env.family(Transport, env.ctx, nx, ny, order), env.ctx
        nc, dt = F.nc, F.dt
        outside = lambda seen, j0, j1: [p for t in seen for p in (t[:, :j0], t[:, j1:])]
        if name == "prepare_advection":
            w, inputs = work_of(F.real, F.decoy, ("u", "v"))
            out = sentinel_like(*[F.real[k] for k in ADV])
            return Case(lambda: ctx.prepare_advection(order, w["u"], w["v"], *out), inputs, out, fill=out, setup=F.setup)
        if name == "transport_stage":
            w, inputs = work_of(F.real, F.decoy, ("f0", "f1", "f2", "f3") + ADV)
            out = sentinel_like(w["f0"], w["f1"])
            call = lambda: ctx.transport_stage(order, 1, ny - 1, dt, 0.75, 0.25, [w["f0"], w["f1"]], [w["f2"], w["f3"]], out, [w[k] for k in ADV])
            return Case(call, inputs, out, fill=out, setup=F.setup, untouched=lambda seen: outside(seen, 1, ny - 1))
        if name == "transport_step":
            w, inputs = work_of(F.real, F.decoy, ("f0", "f1") + ADV)
            scratch = torch.zeros(2 * 2 * nc * nx * ny, dtype=torch.float64, device="cuda")
            call = lambda: ctx.transport_step(order, dt, [w["f0"], w["f1"]], [w[k] for k in ADV], scratch)
            return Case(call, inputs, [w["f0"], w["f1"]], setup=F.setup)
        if name == "transport_step_oop":
            w, inputs = work_of(F.real, F.decoy, ("f0", "f1") + ADV)
            out = sentinel_like(w["f0"], w["f1"])
            call = lambda: ctx.transport_step_oop(order, dt, [w["f0"], w["f1"]], out, [w[k] for k in ADV])
            return Case(call, inputs, out, fill=out, setup=F.setup)
        if name == "transport_step_oop_rows":
            w, inputs = work_of(F.real, F.decoy, ("f0", "f1") + ADV)
            out = sentinel_like(w["f0"], w["f1"])
            call = lambda: ctx.transport_step_oop_rows(order, 1, ny - 1, dt, [w["f0"], w["f1"]], out, [w[k] for k in ADV])
            return Case(call, inputs, out, fill=out, setup=F.setup, untouched=lambda seen: outside(seen, 1, ny - 1))
        if name == "transport_limit":
            w, inputs = work_of(F.real, F.decoy, ("f0", "f1"))
            return Case(lambda: ctx.transport_limit(order, 0, ny, [w["f0"], w["f1"]]), inputs, [w["f0"], w["f1"]], setup=F.setup)
        if name == "tracer_weight":
            w, inputs = work_of(F.real, F.decoy, ("f0", "T"))
            out = sentinel_like(w["f0"])
            call = lambda: ctx.tracer_weight(order, 1, ny - 1, w["f0"], w["T"], out[0])
            return Case(call, inputs, out, fill=out, setup=F.setup, untouched=lambda seen: outside(seen, 1, ny - 1))
        if name == "tracer_recover":
            w, inputs = work_of(F.real, F.decoy, ("f0", "f1", "f3", "T"))
            call = lambda: ctx.tracer_recover(order, 0, ny, w["f0"], w["f1"], w["f3"], 0.4, 0.01, w["T"])  # min_conc among the cell means
            return Case(call, inputs, [w["T"]], setup=F.setup)
        raise KeyError(name)

    return build


def row_column_step(n, diag):
    def build(env):
        ctx = env.ctx
        sets = [Cc.tiled(Cc.SETS[0], n, off)[0] for off in (Cc.OFFSET, Cc.OFFSET + 101)]
        real, decoy = ({k: dev(s[k]) for k in Cc.PLANES} for s in sets)
        w, inputs = work_of(real, decoy, Cc.PLANES)
        dg = sentinel_like(torch.zeros(abi.NDIAG * n, dtype=torch.float64, device="cuda")) if diag else []
        call = lambda: ctx.column_step(Cc.DT, {k: w[k] for k in abi.STATE}, {k: w[k] for k in abi.FORCING}, w["newice"], dg[0] if diag else None)
        return Case(call, inputs, [w[k] for k in Cc.OUT] + dg, fill=dg, setup=lambda: ctx.set_column_params(ctx.column_default_params()))

    return build


def row_forcing(name, nx=130, ny=5):
    def build(env):
        ctx = env.ctx
        z = lambda *s: torch.full(s, SENTINEL, dtype=torch.float64, device="cuda")
        nodal = (2 * ny + 1, 2 * nx + 1)

        def setup():
            ctx.set_grid(nx, ny, 1000.0, 1000.0)
            ctx.set_block(0, ny)

        if name == "column_forcing":
            planes = {k: z(ny, nx) for k in ("tair", "tdew", "slp", "qsw", "qlw", "mld", "snowfall")}
            out = list(planes.values())
            return Case(lambda: ctx.column_forcing("winter", 40000.0, planes), [], out, fill=out, setup=setup)
        if name == "boxtest_forcing":
            out = [z(*nodal) for _ in range(4)]
            return Case(lambda: ctx.boxtest_forcing(nx * 1000.0, 7200.0, wind=out[:2], ocean=out[2:]), [], out, fill=out, setup=setup)
        rng = [np.random.default_rng(s) for s in (REAL, DECOY)]
        if name == "column_wind":
            real, decoy = ({k: dev(r.uniform(-10.0, 10.0, nodal)) for k in ("ua", "va")} for r in rng)
            w, inputs = work_of(real, decoy, ("ua", "va"))
            out = [z(ny, nx)]
            return Case(lambda: ctx.column_wind(w["ua"], w["va"], out[0]), inputs, out, fill=out, setup=setup)
        where = name.split("@")[1]
        names = ("a0", "b0", "a1", "b1")
        real, decoy = ({k: dev(r.uniform(-5.0, 5.0, (7, 11))) for k in names} for r in rng)
        w, inputs = work_of(real, decoy, names)
        out = [z(*nodal) if where == "nodes" else z(ny, nx) for _ in range(2)]
        return Case(lambda: ctx.forcing_sample(where, [w["a0"], w["b0"]], [w["a1"], w["b1"]], 0.3, out), inputs, out, fill=out, setup=setup)

    return build


HIST_PAIRS = (("hice", "mean"), ("speed", "ice_mean"), ("hice", "max"))


def row_samples(name, nx=130, ny=5, n=Pc.BLOCK + 1):
    def build(env):
        F, ctx = env.family(Samples, env.ctx, nx, ny, n), env.ctx
        if name == "history_accumulate":
            fields = ("hice", "speed", "sigma_s")
            w, inputs = work_of(F.real, F.decoy, SOURCES + ("acc",))
            call = lambda: ctx.history_accumulate(1, ny - 1, fields, {k: w[k] for k in SOURCES}, False, 0, w["acc"])
            return Case(call, inputs, [w["acc"]], setup=F.setup)
        if name == "history_accumulate_stats":
            w, inputs = work_of(F.real, F.decoy, SOURCES + ("acc", "wacc"))
            call = lambda: ctx.history_accumulate_stats(0, ny, HIST_PAIRS, {k: w[k] for k in SOURCES}, False, 0, w["acc"], w["wacc"])
            return Case(call, inputs, [w["acc"], w["wacc"]], setup=F.setup)
        if name == "history_row_totals":
            w, inputs = work_of(F.real, F.decoy, SOURCES)
            out = [torch.full((len(abi.SERIES_QUANTITIES), ny), SENTINEL, dtype=torch.float64, device="cuda")]
            call = lambda: ctx.history_row_totals(1, ny - 1, abi.SERIES_QUANTITIES, {k: w[k] for k in SOURCES}, 0.15, 0, out[0])
            return Case(call, inputs, out, fill=out, setup=F.setup, untouched=lambda seen: [seen[0][:, :1], seen[0][:, ny - 1:]])
        assert name == "points_sample"
        w, inputs = work_of(F.real, F.decoy, SOURCES + ("x", "y"))
        out = [torch.full((len(abi.HISTORY_FIELDS), n), SENTINEL, dtype=torch.float64, device="cuda")]
        call = lambda: ctx.points_sample(0, ny, 2, w["x"], w["y"], abi.HISTORY_FIELDS, {k: w[k] for k in SOURCES}, out[0])
        return Case(call, inputs, out, fill=out, setup=F.setup)

    return build


def row_drifters(nx=70, ny=9, n=Dc.BLOCK + 1):
    def build(env):
        ctx = env.ctx
        sets = [Dc.make(nx, ny, n, seed) for seed in (0, 1)]
        real, decoy = ({"u": dev(c["u"]), "v": dev(c["v"]), "A": dev(c["A0"][None]), "land": dev(c["land"]), "d": dev(c["d"])} for c in sets)
        w, inputs = work_of(real, decoy, ("u", "v", "A", "land", "d"))
        out = sentinel_like(w["d"])

        def setup():
            ctx.set_grid(nx, ny, Dc.HX, Dc.HY)
            ctx.set_block(0, ny)
            ctx.set_land_mask(w["land"])

        return Case(lambda: ctx.drifters_advance(0, ny, Dc.DT, Dc.MIN_CONC, w["u"], w["v"], w["A"], w["d"], out[0]), inputs, out, fill=out, setup=setup)

    return build


def rnd_pair(shape):
    return tuple(dev(np.random.default_rng(s).uniform(-1.0, 1.0, shape)) for s in (REAL, DECOY))


def row_copy(n):
    def build(env):
        real, decoy = rnd_pair(n)
        w, out = decoy.clone(), sentinel_like(real)
        return Case(lambda: env.ctx.copy_f64(out[0], w), [(w, real, decoy)], out, fill=out)

    return build


def row_blocking(name):
    """calls that block: behind a late producer they must have waited for it"""

    def build(env):
        ctx = env.timed if name == "phase_times" else env.ctx
        real, decoy = rnd_pair(1025)
        w, out = decoy.clone(), sentinel_like(real)

        def call():
            if name == "ctx_synchronize":
                ctx.copy_f64(out[0], w)
                ctx.synchronize()
                return None
            if name == "mevp_pipeline_health":
                ctx.copy_f64(out[0], w)
                return ctx.pipeline_waits_given_up()
            ctx.phase_mark(0)
            ctx.copy_f64(out[0], w)
            ctx.phase_mark(abi.PHASE_END)
            phases, (_, spans) = ctx.phase_times(reset=True)
            assert all(ms > 0.0 for ms, _ in phases.values())
            return {k: count for k, (_, count) in phases.items()}, spans

        return Case(call, [(w, real, decoy)], out, fill=out)

    return build


def halo_arrays():
    """the segments of test_loopback_exchange_delivers_every_block_in_order: odd lengths, odd (8-byte) alignments"""
    shapes = ((40, 257), (9, 3, 512), (1001,))
    real, decoy = zip(*[rnd_pair(s) for s in shapes])
    return real, decoy


def row_halo(stats):
    def build(env):
        ctx = env.loop
        real, decoy = halo_arrays()
        a, b, c = (x.clone() for x in decoy)
        ra, rb, rc = sentinel_like(a, b, c)
        up, down = [a[30:37], b[5:8], c[1:400]], [a[2:3], c[500:503]]
        from_below, from_above = [ra[0:7], rb[0:3], rc[3:402]], [ra[39:40], rc[900:903]]
        plan = ctx.halo_plan(0, 0, up, down, from_above, from_below)

        def call():
            plan.start()
            plan.finish()
            if stats:
                st = plan.stats(reset=True)
                return st["exchanges"], st["untimed"], st["bytes_sent"], st["bytes_received"]

        untouched = lambda seen: [seen[0][7:39], seen[1][3:], seen[2][:3], seen[2][402:900], seen[2][903:]]
        return Case(call, list(zip((a, b, c), real, decoy)), [ra, rb, rc], fill=[ra, rb, rc], untouched=untouched, keep=[plan])

    return build


def row_comm_max_array(n=1025):
    def build(env):
        mine, peer = env.pair
        real, decoy = rnd_pair(n)
        other = dev(np.random.default_rng(3).uniform(-1.0, 1.0, n))
        w, theirs = decoy.clone(), other.clone()
        failed = []

        def peer_main():
            try:
                peer.comm_max_f64_array(theirs)
            except BaseException as e:  # noqa: BLE001
                failed.append(e)

        def call():
            t = threading.Thread(target=peer_main)
            t.start()
            try:
                mine.comm_max_f64_array(w)
            finally:
                t.join()
            assert not failed, failed

        return Case(call, [(w, real, decoy)], [w, theirs], setup=lambda: theirs.copy_(other))

    return build


def blocks_of(env, nx, own, depth, loopback):
    """(context, RowBlock, peers): a single block of `own` rows, or the interior block of three whose neighbours are the rank itself"""
    if not loopback:
        return env.ctx, rowblock.RowBlock(nx, own, 0, 1), (None, None)
    return env.loop, rowblock.RowBlock(nx, 3 * own, 1, 3, *depth), (0, 0)


def row_rb_mevp(loopback, use_graph, stats=False, nx=130, nsub=7):
    def build(env):
        ctx, blk, peers = blocks_of(env, nx, 8 if loopback else 5, (4, 3), loopback)
        F = env.family(Mevp, ctx, nx, blk.ny)
        w, inputs = work_of(F.real, F.decoy, ("s11", "s12", "s22", "u", "v", "packed", "pg"))
        first = [w[k] for k in ("s11", "s12", "s22", "u", "v")]
        second = sentinel_like(*first)
        F.setup()
        run, per_pass, _ = ctx.rb_mevp(blk, peers, nsub, True, use_graph, (first[:3], second[:3]), ((first[3], first[4]), (second[3], second[4])), w["packed"], w["pg"])
        assert per_pass == 4

        def call():
            parity = run(0)
            if stats:
                st = run.stats(reset=True)
                return parity, st["exchanges"], st["untimed"]
            return parity

        return Case(call, inputs, first + second, fill=second, setup=F.setup, keep=[run])

    return build


def row_rb_bbm(loopback, stats=False, nx=130, nsub=3):
    def build(env):
        ctx, blk, peers = blocks_of(env, nx, 8 if loopback else 5, (1, 1), loopback)
        F = env.family(Bbm, ctx, nx, blk.ny)
        w, inputs = work_of(F.real, F.decoy, ("s11", "s12", "s22", "u", "v", "packed", "hg", "eg", "pm", "D"))
        first = [w[k] for k in ("s11", "s12", "s22", "u", "v")]
        second = sentinel_like(*first)
        d1, dwork = sentinel_like(w["D"], w["D"])
        F.setup()
        run = ctx.rb_bbm(blk, peers, nsub, True, (first[:3], second[:3]), ((first[3], first[4]), (second[3], second[4])), w["packed"],
                         (w["hg"], w["eg"], w["pm"]), (w["D"], d1), dwork, complete_nodes=True)

        def call():
            parity = run(0, 0)
            if stats:
                st = run.stats(reset=True)
                return parity, st["exchanges"], st["untimed"]
            return parity

        return Case(call, inputs, first + second + [w["D"], d1, dwork], fill=second + [d1, dwork], setup=F.setup, keep=[run])

    return build


def row_rb_transport(loopback, stats=False, nx=130):
    def build(env):
        ctx, blk, peers = blocks_of(env, nx, 8 if loopback else 5, (3, 2), loopback)
        F = env.family(Transport, ctx, nx, blk.ny, 2)
        w, inputs = work_of(F.real, F.decoy, ("f0", "f1") + ADV)
        phi = [w["f0"], w["f1"]]
        t1, t2 = sentinel_like(*phi), sentinel_like(*phi)
        F.setup()
        run = ctx.rb_transport(blk, peers, phi, t1, t2, [w[k] for k in ADV], bounds=Tc.BOUNDS[:2])

        def call():
            parity = run(F.dt, 0)
            if stats:
                st = run.stats(reset=True)
                return parity, st["exchanges"], st["untimed"]
            return parity

        return Case(call, inputs, phi + t1 + t2, fill=t1 + t2, setup=F.setup, keep=[run])

    return build


class Row:
    def __init__(self, name, build, covers, blocks_host=False):
        self.name, self.build, self.covers, self.blocks_host = name, build, tuple(covers), blocks_host


def table():
    rows = []
    add = lambda name, build, covers=None, blocks_host=False: rows.append(Row(name, build, covers or ["nsdg_" + name.split("[")[0]], blocks_host))
    add("column_step[1025]", row_column_step(1025, False))
    add("column_step[1025-diag]", row_column_step(1025, True))
    for name in ("column_forcing", "column_wind", "boxtest_forcing"):
        add(name, row_forcing(name))
    for where in ("nodes", "elements"):
        add("forcing_sample[%s]" % where, row_forcing("forcing_sample@" + where))
    for name in ("wind_stress", "ice_strength", "dg_to_cg", "mevp_stress", "mevp_pack_nodal", "mevp_prepare", "mevp_velocity"):
        add(name, row_mevp_helper(name))
    add("mevp_prepare[70x9-island]", row_mevp_helper("mevp_prepare", 70, 9, True))
    for order in (0, 1, 2):
        for name in ("prepare_advection", "transport_stage", "transport_step", "transport_step_oop", "transport_step_oop_rows", "transport_limit",
                     "tracer_weight", "tracer_recover"):
            add("%s[130x5-dg%d]" % (name, order), row_transport(name, 130, 5, order))
        for name in ("transport_stage", "transport_step"):  # an odd nx: the pair kernel falls back to one element per lane
            add("%s[65x5-dg%d]" % (name, order), row_transport(name, 65, 5, order))
    for nx, ny in ((130, 5), (65, 3)):
        s = "[%dx%d]" % (nx, ny)
        add("mevp_iterate" + s, row_mevp_pass("mevp_iterate", nx, ny, (0, 0, ny)))
        add("mevp_iterate2" + s, row_mevp_pass("mevp_iterate2", nx, ny, (0, ny)))
        add("mevp_iterate3" + s, row_mevp_pass("mevp_iterate3", nx, ny, (0, ny)))
        add("mevp_iterate4" + s, row_mevp_pass("mevp_iterate4", nx, ny, (0, ny)))
        add("mevp_subcycle%s-nsub7" % s, row_mevp_subcycle(nx, ny, 7), ["nsdg_mevp_subcycle"])  # odd: ends in five hipMemcpyAsync
        add("mevp_subcycle%s-nsub8" % s, row_mevp_subcycle(nx, ny, 8), ["nsdg_mevp_subcycle"])
    add("mevp_iterate[130x5-rows-1-2-4]", row_mevp_pass("mevp_iterate", 130, 5, (1, 2, 4)))
    add("mevp_iterate[130x5-two-kernels]", row_mevp_pass("mevp_iterate", 130, 5, (0, 0, 5), variant=0))
    add("mevp_iterate[70x9-island]", row_mevp_pass("mevp_iterate", 70, 9, (0, 0, 9), masked=True))
    add("mevp_iterate4[70x9-island]", row_mevp_pass("mevp_iterate4", 70, 9, (0, 9), masked=True))
    add("mevp_iterate3_pair[130x5]", row_mevp_pass("mevp_iterate3_pair", 130, 5, ((0, 2), (3, 5))))
    add("mevp_iterate4_pair[130x5]", row_mevp_pass("mevp_iterate4_pair", 130, 5, ((0, 2), (4, 5))))
    for nx, ny, masked in ((130, 5, False), (65, 3, False), (70, 9, True)):
        s = "[%dx%d%s]" % (nx, ny, "-island" if masked else "")
        add("bbm_prepare" + s, row_bbm("bbm_prepare", nx, ny, masked))
        add("bbm_iterate" + s, row_bbm("bbm_iterate", nx, ny, masked))
    add("land_clear[70x9-island]", row_mevp_helper("land_clear", 70, 9, True))
    add("land_clear_nodes[70x9-island]", row_mevp_helper("land_clear_nodes", 70, 9, True))
    for name in ("history_accumulate", "history_accumulate_stats", "history_row_totals", "points_sample"):
        add(name, row_samples(name))
    add("drifters_advance", row_drifters())
    add("copy_f64[1025]", row_copy(1025))
    add("concentration_max", row_mevp_helper("concentration_max"), blocks_host=True)
    add("halo_start+halo_finish[loopback]", row_halo(False), ["nsdg_halo_start", "nsdg_halo_finish"])
    add("comm_max_f64_array[world2]", row_comm_max_array(), ["nsdg_comm_max_f64_array"], blocks_host=True)
    for loopback in (False, True):
        s = "loopback" if loopback else "single"
        for graph in (False, True):
            add("rb_mevp_run[%s%s]" % (s, "-graph" if graph else ""), row_rb_mevp(loopback, graph))
        add("rb_bbm_run[%s]" % s, row_rb_bbm(loopback))
        add("rb_transport_run[%s]" % s, row_rb_transport(loopback))
    add("ctx_synchronize", row_blocking("ctx_synchronize"), blocks_host=True)
    add("mevp_pipeline_health", row_blocking("mevp_pipeline_health"), blocks_host=True)
    add("phase_times", row_blocking("phase_times"), ["nsdg_phase_mark", "nsdg_phase_times"], blocks_host=True)
    add("halo_stats_get[loopback]", row_halo(True), ["nsdg_halo_stats_get"], blocks_host=True)
    add("rb_mevp_stats[loopback]", row_rb_mevp(True, False, stats=True), ["nsdg_rb_mevp_stats"], blocks_host=True)
    add("rb_bbm_stats[loopback]", row_rb_bbm(True, stats=True), ["nsdg_rb_bbm_stats"], blocks_host=True)
    add("rb_transport_stats[loopback]", row_rb_transport(True, stats=True), ["nsdg_rb_transport_stats"], blocks_host=True)
    return rows


TABLE = table()
ROWS = {r.name: r for r in TABLE}
assert len(ROWS) == len(TABLE)


# ---- A. every entry point between a late producer and an early consumer ------------------------------------------------------------------------
class Proto:
    """both sides, every case built and warmed, the plain results, and the delay"""

    def __init__(self, gpu):
        from nextsimdg_amd import build

        build.build_lib(verbose=False)
        self.stream = torch.cuda.Stream()
        assert self.stream.cuda_stream != 0
        self.side, self.default = Env(gpu, self.stream), Env(gpu, None)
        self.x = torch.rand(MM, MM, dtype=torch.float64, device="cuda")
        self.y = torch.empty_like(self.x)
        self.products = 0
        self.backend = SO.CudaBackend(torch, self.stream, self.delay)
        self.plain_backend = SO.CudaBackend(torch, torch.cuda.default_stream(), lambda: None)
        self.references, self.errors = {}, {}
        longest, slow = 0.0, None
        for row in TABLE:
            try:
                for env in (self.side, self.default):
                    torch.cuda.synchronize()
                    env.cases[row.name] = row.build(env)
                    torch.cuda.synchronize()
                refs = [SO.plain(self.side.cases[row.name], self.backend), SO.plain(self.default.cases[row.name], self.plain_backend)]
                SO.compare(row.name + " (side-stream against default-stream context, both plain)", refs[0], refs[1])
                self.references[row.name] = refs
                if not row.blocks_host:  # warmed by the plain call: the protocol's host-side stretch without a delay
                    seconds = self.stretch(self.side.cases[row.name])
                    if seconds > longest:
                        longest, slow = seconds, row.name
            except BaseException as e:  # noqa: BLE001 -- the row's own test reports it
                self.errors[row.name] = e
                torch.cuda.synchronize()
        torch.mm(self.x, self.x, out=self.y)  # loads the product's kernel
        one = self.elapsed_ms(1)
        self.products = max(DELAY_MIN_PRODUCTS, int(math.ceil(1.25 * DELAY_FACTOR * 1e3 * longest / one)))  # (a quarter more: the chain is timed again below)
        assert self.products * one <= DELAY_MAX_MS, "a delay of %d products of %.3f ms is not a quick test: the longest host-side stretch is %.3f ms (%s)" % (
            self.products, one, 1e3 * longest, slow)
        self.delay_ms = self.elapsed_ms(self.products)
        self.longest_ms, self.slowest = 1e3 * longest, slow
        print("stream order: one %d^2 fp64 product %.3f ms; longest warmed host-side stretch %.3f ms (%s); delay = %d products = %.3f ms; ratio %.1f"
              % (MM, one, self.longest_ms, slow, self.products, self.delay_ms, self.delay_ms / max(self.longest_ms, 1e-9)))

    def delay(self):
        for _ in range(self.products):
            torch.mm(self.x, self.x, out=self.y)

    def elapsed_ms(self, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            a.record()
            for _ in range(n):
                torch.mm(self.x, self.x, out=self.y)
            b.record()
        self.stream.synchronize()
        return a.elapsed_time(b)

    def stretch(self, case):
        """host seconds from the enqueue of the producer's copies to the return of the call, everything warm, no delay"""
        torch.cuda.synchronize()
        case.setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for w, real, _ in case.inputs:
            self.backend.copy(w, real)
        for o in case.fill:
            self.backend.fill(o, SENTINEL)
        self.backend.record()
        case.call()
        seconds = time.perf_counter() - t0
        torch.cuda.synchronize()
        return seconds

    def close(self):
        torch.cuda.synchronize()
        self.side.close()
        self.default.close()


@pytest.fixture(scope="module")
def proto(gpu):
    p = Proto(gpu)
    yield p
    p.close()


@pytest.mark.parametrize("name", [r.name for r in TABLE])
def test_call_is_stream_ordered_on_a_side_stream(proto, name):
    """the protocol of tests/stream_order.py for one row: the gate is still closed when an asynchronous call returns and has fired when
    a blocking one does; what the consumer on the stream sees is, bit for bit, the plain call on the side-stream context and on a
    default-stream context; host results are equal; what the call must not write holds the sentinel"""
    row = ROWS[name]
    if name in proto.errors:
        raise proto.errors[name]
    seconds = SO.check(name, proto.side.cases[name], proto.backend, row.blocks_host, proto.references[name])
    assert proto.side.ctx.pipeline_waits_given_up() == 0
    print("%s: the call took %.3f ms on the host under a delay of %.3f ms" % (name, 1e3 * seconds, proto.delay_ms))
    if not row.blocks_host:
        assert proto.delay_ms >= DELAY_FACTOR * proto.longest_ms


def test_setter_between_two_enqueued_calls_acts_on_the_second_only(proto):
    """parameters, a strip height and a mask are host state read when a call is MADE: set between two calls that are both still waiting
    behind the delay, they change the second call only -- both equal the same two calls made one at a time"""
    env = proto.side
    ctx = env.ctx
    F = env.family(Mevp, ctx, 70, 9, True)
    r = F.real
    S = [r["s11"], r["s12"], r["s22"]]
    second_params = ctx.mevp_default_params(**dict(F.case["par"], alpha=520.0, beta=610.0, c_ocean=3e-3))

    def two_calls(synchronous):
        out = [sentinel_like(*S, r["u"], r["v"]) for _ in range(2)]
        packed = sentinel_like(r["packed"], r["packed"])
        torch.cuda.synchronize()
        F.state(variant=1)
        ctx.set_land_mask(None)
        if not synchronous:
            proto.backend.delay()
        gate = proto.backend.record()
        for k in range(2):
            if k == 1:
                ctx.set_mevp_params(second_params)
                ctx.set_mevp_strip_rows(3)
                ctx.set_land_mask(F.mask)
            ctx.mevp_prepare(F.case["dt"], r["H"], r["A"], (r["ua"], r["va"]), (r["uo"], r["vo"]), (r["u0"], r["v0"]), packed[k])
            ctx.mevp_iterate(0, 0, 9, S, out[k][:3], (r["u"], r["v"]), (out[k][3], out[k][4]), packed[k], r["pg"])
            if synchronous:
                torch.cuda.synchronize()
        fired = gate.query()
        torch.cuda.synchronize()
        return out, packed, fired

    (want, want_packed, _), (got, got_packed, fired) = two_calls(True), two_calls(False)
    assert not fired, "delay too short, nothing proven"
    for a, b in zip(want[0] + want[1] + want_packed, got[0] + got[1] + got_packed):
        assert SO.same_bits(a, b)
    assert not SO.same_bits(want_packed[0], want_packed[1]) and not SO.same_bits(want[0][3], want[1][3])  # the setters do act
    ln = dev(land_ref.land_nodes(island(70, 9)))
    assert bool((got[1][3][ln] == 0.0).all()) and not bool((got[0][3][ln] == 0.0).all())  # the mask holds the second call's land nodes only
    assert ctx.pipeline_waits_given_up() == 0


# ---- B. two contexts on two streams from one host thread -----------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_interleaved_equal_their_solo_runs(gpu, proto):
    """context A on s1: 130 x 5, the mEVP passes of variant 4 under a land mask, parameters of mevp_cases' plastic kind; context B on s2:
    65 x 3, the brittle sub-iteration and the DG2 transport, no mask, other parameters, another cell size per call group.  Their calls
    alternate from one host thread and a delay goes to s1 and to s2 in turn, so the kernels of the two streams overlap in time.  Every
    buffer of either context holds the bits of its solo run: no launch constant, scratch or device symbol is shared between contexts"""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    A, B = abi.Context(gpu, stream=s1), abi.Context(gpu, stream=s2)
    torch.cuda.synchronize()
    FA, FB, TB = Mevp(A, 130, 5, True), Bbm(B, 65, 3), Transport(B, 65, 3, 2)
    torch.cuda.synchronize()
    a, b, t = FA.real, FB.real, TB.real
    fresh = lambda *ts: sentinel_like(*ts)
    Sa, Sb = [a["s11"], a["s12"], a["s22"]], [b["s11"], b["s12"], b["s22"]]
    oa = dict(pg=fresh(a["pg"])[0], packed=fresh(a["packed"])[0], p1=fresh(*Sa, a["u"], a["v"]), p2=fresh(*Sa, a["u"], a["v"]), p3=fresh(*Sa, a["u"], a["v"]),
              sub=fresh(*Sa, a["u"], a["v"]), scratch=torch.zeros(10 * a["u"].numel() + 3 * a["s11"].numel(), dtype=torch.float64, device="cuda"))
    ob = dict(gauss=fresh(b["hg"], b["eg"], b["pm"]), packed=fresh(b["packed"])[0], p1=fresh(*Sb, b["D"], b["u"], b["v"]), p2=fresh(*Sb, b["D"], b["u"], b["v"]),
              adv=fresh(*[t[k] for k in ADV]), g=fresh(t["f0"], t["f1"]))
    dta, dtb = FA.case["dt"], FB.case["dts"]

    def pass_a(fn, rows, src, dst):
        getattr(A, fn)(*rows, src[:3], dst[:3], (src[3], src[4]), (dst[3], dst[4]), oa["packed"], oa["pg"])

    def sub_a():
        for dst, src in zip(oa["sub"], Sa + [a["u"], a["v"]]):
            with torch.cuda.stream(s1):
                dst.copy_(src)
        A.mevp_subcycle(dta, 7, oa["sub"][:3], oa["sub"][3], oa["sub"][4], a["u0"], a["v0"], a["tax"], a["tay"], a["uo"], a["vo"], a["cgh"], a["cga"], oa["pg"], oa["scratch"])

    steps_a = [lambda: (FA.state(4), A.ice_strength(a["H"], a["A"], oa["pg"])),
               lambda: A.mevp_prepare(dta, a["H"], a["A"], (a["ua"], a["va"]), (a["uo"], a["vo"]), (a["u0"], a["v0"]), oa["packed"]),
               lambda: pass_a("mevp_iterate4", (0, 5), Sa + [a["u"], a["v"]], oa["p1"]),
               lambda: (A.set_mevp_strip_rows(2), pass_a("mevp_iterate3", (0, 5), oa["p1"], oa["p2"])),
               lambda: (A.set_mevp_variant(1), pass_a("mevp_iterate", (0, 0, 5), oa["p2"], oa["p3"])),
               lambda: (A.set_mevp_variant(4), sub_a())]

    def iterate_b(S, D, uv, dst):
        B.bbm_iterate(0, 0, 3, S, dst[:3], D, dst[3], uv, (dst[4], dst[5]), ob["packed"], ob["gauss"])

    steps_b = [lambda: (FB.state(), B.set_mevp_variant(1), B.bbm_prepare(b["H"], b["A"], *ob["gauss"])),
               lambda: B.mevp_prepare(dtb, b["H"], b["A"], (b["ua"], b["va"]), (b["uo"], b["vo"]), (FB.zero, FB.zero), ob["packed"]),
               lambda: iterate_b(Sb, b["D"], (b["u"], b["v"]), ob["p1"]),
               lambda: iterate_b(ob["p1"][:3], ob["p1"][3], (ob["p1"][4], ob["p1"][5]), ob["p2"]),
               lambda: (TB.setup(), B.prepare_advection(2, t["u"], t["v"], *ob["adv"])),
               lambda: B.transport_step_oop(2, TB.dt, [t["f0"], t["f1"]], ob["g"], ob["adv"])]
    flat = lambda d: [x for v in d.values() for x in (v if isinstance(v, (list, tuple)) else [v])]
    junk = {s: (torch.rand(MM, MM, dtype=torch.float64, device="cuda"), torch.empty(MM, MM, dtype=torch.float64, device="cuda")) for s in (s1, s2)}

    def delay(s):
        with torch.cuda.stream(s):
            for _ in range(max(4, proto.products // 4)):
                torch.mm(junk[s][0], junk[s][0], out=junk[s][1])

    def run(which):
        torch.cuda.synchronize()
        for x in flat(oa) + flat(ob):
            x.fill_(SENTINEL)
        torch.cuda.synchronize()
        for k in range(len(steps_a)):
            if which == "both":
                delay(s1 if k % 2 == 0 else s2)
            if which in ("both", "a"):
                steps_a[k]()
            if which in ("both", "b"):
                steps_b[k]()
        torch.cuda.synchronize()
        return [x.clone() for x in flat(oa)], [x.clone() for x in flat(ob)]

    solo_a, solo_b = run("a")[0], run("b")[1]
    both_a, both_b = run("both")
    for k, (x, y) in enumerate(zip(both_a + both_b, solo_a + solo_b)):
        assert SO.same_bits(x, y), k
    ln = dev(land_ref.land_nodes(island(130, 5)))
    u3 = both_a[next(i for i, x in enumerate(flat(oa)) if x is oa["p3"][3])]
    assert bool((u3[ln] == 0.0).all()) and float(u3.abs().max()) > 1e-5
    assert not any(bool((x == SENTINEL).all()) for x in both_a[:-1] + both_b)  # every step wrote
    assert A.pipeline_waits_given_up() == 0 and B.pipeline_waits_given_up() == 0
    A.close(), B.close()


# ---- C. the Python drivers on a side stream ------------------------------------------------------------------------------------------------------
def same_tree(a, b):
    """bit equality of nested results: dicts, sequences, arrays, tensors, scalars"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_tree(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and SO.same_bits(a.cpu(), b.cpu())
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


DRIVER_NX, DRIVER_NY, DRIVER_NSUB, DRIVER_STEPS = 150, 64, 7, 2


def driver_run(gpu, kind, stream, delay):
    """two steps of one driver with every output on, built and stepped under torch.cuda.stream(stream) (None: the default stream)"""
    import contextlib

    from nextsimdg_amd import synthetic
    from thread_ranks import fields

    nx, ny = DRIVER_NX, DRIVER_NY
    bt, H, A, uo, vo, ua, va = fields(nx, ny)
    land = np.zeros((ny, nx), dtype=bool)
    land[20:30, 60:70] = True
    L = bt.L
    points = [[0.3 * L, 0.3 * L], [0.5 * L, 0.5 * L], [0.7 * L, 0.2 * L], [0.42 * L, 0.39 * L]]  # the last one on the island
    kw = dict(land=land, history=("hice", "speed:ice_mean", "hice:max"), series=("area", "drift", "speed_max"), drifters=points,
              drifter_fields=("hice", "speed"), stations=points, station_fields=("hice", "u", "sigma_n"), phase_timing=True)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        ctx = abi.Context(gpu)
        assert ctx.stream.cuda_stream == (0 if stream is None else stream.cuda_stream)
        ctx.set_mevp_params(ctx.mevp_default_params(alpha=300.0, beta=300.0))
        blk = rowblock.RowBlock(nx, ny)
        if kind == "mevp":
            core = rowblock.DynamicsCore(ctx, blk, bt.hx, bt.hy, 120.0, DRIVER_NSUB, gpu, native=True, use_graph=True, **kw)
            core.load_global(H, A, uo, vo, ua, va)
        elif kind == "bbm":
            core = rowblock.DynamicsCore(ctx, blk, bt.hx, bt.hy, 2.5, DRIVER_NSUB, gpu, native=True, rheology="bbm", **kw)
            core.load_global(H, A, uo, vo, ua, va, D=0.1 * np.ones_like(H) * (np.arange(6) == 0)[:, None, None])
        else:
            core = rowblock.CoupledCore(ctx, blk, bt.hx, bt.hy, 120.0, DRIVER_NSUB, gpu, forcing="winter", advect_column_state=True, **kw)
            core.load_global(H, A, uo, vo, ua, va)
            st, fo, _ = synthetic.column_fields(nx * ny, 5)
            core.load_column({k: v.reshape(ny, nx) for k, v in {**st, **fo}.items()})
        for _ in range(DRIVER_STEPS):
            if stream is not None:
                delay()
            if kind == "coupled":
                core.advance(120.0, substeps="auto")
            else:
                core.step()
        times = core.phase_times()
        res = dict(state=core.state_dict(), history=core.history_read(), series=core.series_read(), drifters=core.drifters_read(),
                   stations=core.stations_read())
        torch.cuda.synchronize()
        given_up = ctx.pipeline_waits_given_up()
        core.close()
        ctx.close()
    return res, times, given_up


@pytest.mark.parametrize("kind", ["mevp", "bbm", "coupled"])
def test_python_driver_on_a_side_stream_equals_the_default_stream(gpu, proto, kind):
    """DynamicsCore (mEVP, native plans with graph replay), DynamicsCore (rheology="bbm", native) and CoupledCore (forcing="winter",
    advect_column_state, advance(substeps="auto")) at 150 x 64 with an island, history, series, drifters with fields, stations and phase
    timing, a delay enqueued on the stream before every step: state and every output bit-equal to the same run on the default stream, the
    same phases with positive times"""
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    buf = (torch.rand(MM, MM, dtype=torch.float64, device="cuda"), torch.empty(MM, MM, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()

    def delay():  # on the current stream: the side stream
        for _ in range(max(4, proto.products // 4)):
            torch.mm(buf[0], buf[0], out=buf[1])

    want, want_times, _ = driver_run(gpu, kind, None, None)
    got, got_times, given_up = driver_run(gpu, kind, s, delay)
    assert given_up == 0
    for k in want:
        assert same_tree(got[k], want[k]), k
    u = want["state"]["u"]
    assert np.isfinite(u).all() and np.abs(u).max() > 1e-6
    assert set(got_times) == set(want_times) and len(got_times) >= 3
    for k in got_times:
        assert got_times[k][0] > 0.0 and got_times[k][1] == want_times[k][1], (k, got_times[k], want_times[k])


# ---- D. thread ranks that own their streams --------------------------------------------------------------------------------------------------------
RANK_NX, RANK_NY, RANK_STEPS = 150, 128, 3


@pytest.fixture(scope="module")
def built(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)


@pytest.fixture(scope="module")
def single_domain(built):
    """the single-domain run on the default stream, once per (coupled, nsub)"""
    from thread_ranks import run_world

    cache = {}

    def get(coupled, nsub, variant=3, **kw):
        key = (coupled, nsub, variant, tuple(sorted(kw)))
        if key not in cache:
            cache[key] = run_world(1, variant, coupled, RANK_NX, RANK_NY, nsub, RANK_STEPS, **kw)[0]
        return cache[key]

    return get


@pytest.mark.parametrize("world,group,nsub,coupled,variant,graph", [(3, 2, 20, False, 3, False), (4, 4, 41, True, 3, True), (4, 5, 31, False, 3, False)])
def test_own_stream_thread_ranks_equal_the_single_domain(single_domain, world, group, nsub, coupled, variant, graph):
    """the worlds of test_native_row_block_driver_equals_single_domain_bitwise with every rank on a stream of its own: nothing orders one
    rank's compute against another's but the exchange, as in production"""
    from thread_ranks import gather, run_world

    ref = single_domain(coupled, nsub, variant)
    assert float(ref["u"].abs().max()) > 1e-5
    parts = run_world(world, variant, coupled, RANK_NX, RANK_NY, nsub, RANK_STEPS, group=group, transport="native", native=True, use_graph=graph,
                      own_stream=True)
    for key in ("H", "A", "u", "v", "s11") + (("hsnow", "tice0") if coupled else ()):
        assert torch.equal(gather(parts, world, key), ref[key]), (key, world, group)


def test_own_stream_thread_ranks_with_winter_forcing_equal_the_single_domain(single_domain):
    from nextsimdg_amd import synthetic
    from thread_ranks import gather, run_world

    nx, ny, nsub = RANK_NX, RANK_NY, 20
    bt = synthetic.BoxTest(nx, ny)
    H, A = bt.dg_fields()
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    cs, cf = synthetic.column_fields_smooth(nx, ny)
    kw = dict(data=(bt, H, A, uo, vo, ua, va), column={**cs, **cf}, alpha=bt.stable_alpha(120.0), core_kw=dict(forcing="winter"))
    ref = single_domain(True, nsub, 3, **kw)
    assert bool(torch.isfinite(ref["u"]).all()) and float(ref["u"].abs().max()) > 1e-5
    parts = run_world(3, 3, True, nx, ny, nsub, RANK_STEPS, group=2, transport="native", native=True, use_graph=True, own_stream=True, **kw)
    for key in ("H", "A", "u", "v", "s11", "tice0", "hsnow"):
        assert torch.equal(gather(parts, 3, key), ref[key]), key


def test_own_stream_needs_the_native_transport(built):
    from thread_ranks import run_world

    with pytest.raises(ValueError, match="own_stream=True needs transport='native'"):
        run_world(2, 1, False, 70, 16, 3, 1, own_stream=True)


def test_own_stream_brittle_blocks_with_an_island_equal_one_block(built):
    """three native brittle row blocks with the island of tests/test_gpu_bbm_native.py across both block boundaries, every rank on a stream
    of its own, against the Python-driven sequence on one block on the default stream"""
    import test_gpu_bbm_native as N
    import thread_ranks

    land = N.island(N.DNY)
    want = N.one_block(N.ODD_NSUB, False, land=land)
    out = {}
    thread_ranks._local_group[0] += 1
    gid = thread_ranks._local_group[0]

    def rank_main(rank):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                c = abi.Context(torch.device("cuda:0"))
                assert c.stream.cuda_stream != 0
                c.comm_deadline(60.0)
                blk = rowblock.RowBlock(N.DNX, N.DNY, rank, 3, 1, 1)
                core = N.run_core(c, torch.device("cuda"), N.ODD_NSUB, True, rank, 3, rowblock.NativeHaloExchanger(c, blk, local_group=gid), land=land)
                out[rank] = N.result(core)
                core.close()
                c.close()
        except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread; the peers' waits end at their deadline
            out[rank] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(3):
        if isinstance(out[r], BaseException):
            raise out[r]
    N.assert_same({k: N.joined(out, k) for k in N.KEYS}, want, "own streams, land")
    assert float(want["u"].abs().max()) > 1e-6

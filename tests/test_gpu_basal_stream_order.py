"""The landfast-ice calls of include/nsdg_basal.h held to stream order on a stream other than the default, by the protocol of
tests/stream_order.py and with the families and the delay of tests/test_gpu_stream_order.py, whose table holds the functions of
include/nsdg.h itself: nsdg_basal.h is a header of its own with a table of its own, TABLE below (the pattern of
tests/test_gpu_tracers_stream_order.py).  Every function that header declares has a row (checked without a GPU); every row passes between
a late producer and an early consumer on a side stream, and what the consumer sees is, bit for bit, the plain call on the side-stream
context and on a default-stream context.  The depth is an array argument like any other: the producer writes it late.  The two setters
and the defaults are host-only: their rows make the call and then the launch that reads what it set."""
import math
import os
import re

import numpy as np
import pytest
import torch

import stream_order as SO
import test_gpu_stream_order as G
from nextsimdg_amd import abi
from stream_order import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 130, 5


def declared_functions():
    src = open(os.path.join(ROOT, "include", "nsdg_basal.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))


def depths():
    """two depth arrays shallow enough for the family's cover to ground on part of them"""
    return {k: G.dev(np.random.default_rng(s).uniform(0.05, 3.0, (NY, NX))) for k, s in (("real", 11), ("decoy", 12))}


def row(name, masked):
    """the call `name` on the mEVP family of tests/test_gpu_stream_order.py (130 x 5, with or without its island)"""
    def build(env):
        ctx = env.ctx
        F = env.family(G.Mevp, ctx, NX, NY, masked)
        d = depths()
        depth = d["decoy"].clone()
        triple = (depth, d["real"], d["decoy"])

        def setup():
            F.setup()
            ctx.set_basal_params(ctx.basal_default_params())
            ctx.set_basal_depth(depth)

        if name == "basal_critical":
            w, inputs = G.work_of(F.real, F.decoy, ("cgh", "cga"))
            out = G.sentinel_like(w["cgh"])
            return Case(lambda: ctx.basal_critical(w["cgh"], w["cga"], out[0]), inputs + [triple], out, fill=out, setup=setup)
        if name == "basal_params_set":  # other parameters, then the launch that reads them
            w, inputs = G.work_of(F.real, F.decoy, ("cgh", "cga"))
            out = G.sentinel_like(w["cgh"])

            def call():
                ctx.set_basal_params(ctx.basal_default_params(k1=5.0, k2=7.0, alpha_b=3.0))
                ctx.basal_critical(w["cgh"], w["cga"], out[0])

            return Case(call, inputs + [triple], out, fill=out, setup=setup)
        if name == "basal_depth_set":  # the array is set inside the call; the packing that follows stores T_b from it as the fourth pair
            w, inputs = G.work_of(F.real, F.decoy, ("H", "A", "ua", "va", "uo", "vo", "u0", "v0"))
            out = G.sentinel_like(F.real["packed"])
            dt = F.case["dt"]

            def setup_without():
                setup()
                ctx.set_basal_depth(None)

            def call():
                ctx.set_basal_depth(depth)
                ctx.mevp_prepare(dt, w["H"], w["A"], (w["ua"], w["va"]), (w["uo"], w["vo"]), (w["u0"], w["v0"]), out[0])

            return Case(call, inputs + [triple], out, fill=out, setup=setup_without)
        raise KeyError(name)

    return build


COVERS = {"basal_critical": ["nsdg_basal_critical"], "basal_params_set": ["nsdg_basal_params_set", "nsdg_basal_default_params"],
          "basal_depth_set": ["nsdg_basal_depth_set"]}
TABLE = [G.Row("%s[%dx%d%s]" % (name, NX, NY, "-island" if masked else ""), row(name, masked), COVERS[name])
         for masked in (False, True) for name in ("basal_critical", "basal_params_set", "basal_depth_set")]
ROWS = {r.name: r for r in TABLE}


def test_every_function_of_the_header_has_a_row_and_a_binding():
    names = declared_functions()
    assert names == ["nsdg_basal_critical", "nsdg_basal_default_params", "nsdg_basal_depth_set", "nsdg_basal_params_set"]
    assert {c for r in TABLE for c in r.covers} == set(names) and len(ROWS) == len(TABLE)
    assert sorted(abi.BASAL_SYMBOLS) == names and not set(abi.BASAL_SYMBOLS) & (set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS))
    assert not any(r.blocks_host for r in TABLE)


class Env:
    """one side of the comparison: a context bound to the side stream, or to the default stream (the part of
    tests/test_gpu_stream_order.py's Env these rows need)"""

    def __init__(self, gpu, stream):
        self.ctx = abi.Context(gpu) if stream is None else abi.Context(gpu, stream=stream)
        self.families, self.cases = {}, {}

    def family(self, cls, ctx, *key):
        k = (cls.__name__, id(ctx)) + key
        if k not in self.families:
            torch.cuda.synchronize()
            self.families[k] = cls(ctx, *key)
            torch.cuda.synchronize()
        return self.families[k]

    def close(self):
        self.cases.clear()
        self.families.clear()
        self.ctx.close()


class Proto(G.Proto):
    """tests/test_gpu_stream_order.py's Proto over the rows of this file: both sides, every case built and warmed, the plain results, and
    a delay of at least DELAY_FACTOR times the longest warmed host-side stretch"""

    def __init__(self, gpu):
        from nextsimdg_amd import build

        build.build_lib(verbose=False)
        self.stream = torch.cuda.Stream()
        assert self.stream.cuda_stream != 0
        self.side, self.default = Env(gpu, self.stream), Env(gpu, None)
        self.x = torch.rand(G.MM, G.MM, dtype=torch.float64, device="cuda")
        self.y = torch.empty_like(self.x)
        self.products = 0
        self.backend = SO.CudaBackend(torch, self.stream, self.delay)
        self.plain_backend = SO.CudaBackend(torch, torch.cuda.default_stream(), lambda: None)
        self.references, self.errors = {}, {}
        longest = 0.0
        for r in TABLE:
            try:
                for env in (self.side, self.default):
                    torch.cuda.synchronize()
                    env.cases[r.name] = r.build(env)
                    torch.cuda.synchronize()
                refs = [SO.plain(self.side.cases[r.name], self.backend), SO.plain(self.default.cases[r.name], self.plain_backend)]
                SO.compare(r.name + " (side-stream against default-stream context, both plain)", refs[0], refs[1])
                self.references[r.name] = refs
                longest = max(longest, self.stretch(self.side.cases[r.name]))
            except BaseException as e:  # noqa: BLE001 -- the row's own test reports it
                self.errors[r.name] = e
                torch.cuda.synchronize()
        torch.mm(self.x, self.x, out=self.y)  # loads the product's kernel
        one = self.elapsed_ms(1)
        self.products = max(G.DELAY_MIN_PRODUCTS, int(math.ceil(1.25 * G.DELAY_FACTOR * 1e3 * longest / one)))
        assert self.products * one <= G.DELAY_MAX_MS
        self.delay_ms = self.elapsed_ms(self.products)
        self.longest_ms = 1e3 * longest


@pytest.fixture(scope="module")
def proto(gpu):
    p = Proto(gpu)
    yield p
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in TABLE])
def test_call_is_stream_ordered_on_a_side_stream(proto, name):
    if name in proto.errors:
        raise proto.errors[name]
    seconds = SO.check(name, proto.side.cases[name], proto.backend, False, proto.references[name])
    print("%s: the call took %.3f ms on the host under a delay of %.3f ms" % (name, 1e3 * seconds, proto.delay_ms))
    assert proto.delay_ms >= G.DELAY_FACTOR * proto.longest_ms
    # the row did something: the outputs are not all sentinel, the plain results on the two contexts were equal (Proto), and part of the
    # cover is grounded: T_b (or the packing's fourth pair) is not zero everywhere
    seen = proto.references[name][0][1][0]
    assert not bool((seen == SO.SENTINEL).all())
    tb = seen if name.startswith(("basal_critical", "basal_params_set")) else seen.view(4, -1)[3]
    assert float(tb.max()) > 0.0 and float(tb.min()) >= 0.0

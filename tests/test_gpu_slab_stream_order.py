"""The slab-ocean calls of include/nsdg_ocean.h held to stream order on a stream other than the default, by the protocol of
tests/stream_order.py and with the delay of tests/test_gpu_stream_order.py, whose table holds the functions of include/nsdg.h itself:
nsdg_ocean.h is a header of its own with a table of its own, TABLE below (the pattern of tests/test_gpu_tracers_stream_order.py).  Every
function that header declares has a row (checked without a GPU); every row passes between a late producer and an early consumer on a
side stream, and what the consumer sees is, bit for bit, the plain call on the side-stream context and on a default-stream context.  The
relaxation targets and the skip mask are array arguments like any other: the producer writes them late.  The setter and the defaults are
host-only: their row makes the call and then the launch that reads what it set."""
import gc
import math
import os
import re

import numpy as np
import pytest
import torch

import column_path_cases as Cc
import stream_order as SO
import test_gpu_stream_order as G
from nextsimdg_amd import abi
from stream_order import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The delay of these rows is four times the least delay of tests/test_gpu_stream_order.py (about 65 ms in place of about 18 ms; its rule of
# DELAY_FACTOR times the longest warmed stretch asks for 3 ms).  The protocol can only prove order while the producer still runs when the
# call returns, and the binding of the fused call makes some forty small Python objects per call: in a process that has run the whole suite
# a full collection of the interpreter, or the host thread losing its processor once, holds such a call for about 20 ms (seen: 21.5 ms
# under a delay of 18 ms, against 0.03 ms warm), and the row then fails with "delay too short, nothing proven" though it is in order.
DELAY_MIN_PRODUCTS = 4 * G.DELAY_MIN_PRODUCTS
OCEAN_OUT = Cc.OUT + ["sst", "sss"]  # what the fused step writes


def declared_functions():
    src = open(os.path.join(ROOT, "include", "nsdg_ocean.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))


def row(name, n):
    """the fused column step on the recorded elements of tests/column_path_cases.py (n odd: the pair kernel and the tail), both
    relaxations on, a mask"""
    def build(env):
        ctx = env.ctx
        sets = [Cc.tiled(Cc.SETS[0], n, off)[0] for off in (Cc.OFFSET, Cc.OFFSET + 101)]
        real, decoy = ({k: G.dev(s[k]) for k in Cc.PLANES} for s in sets)
        for k, seed in (("sst_ext", 21), ("sss_ext", 22)):
            lo, hi = (-1.8, 3.0) if k == "sst_ext" else (30.0, 35.0)
            real[k], decoy[k] = (G.dev(np.random.default_rng(seed + 10 * j).uniform(lo, hi, n)) for j in (0, 1))
        masks = [(np.random.default_rng(31 + j).random(n) < 0.4).astype(np.uint8) for j in (0, 1)]
        masks[0][0], masks[0][-1] = 0, 1  # the real mask skips the last element and not the first, the decoy the other way round
        masks[1][0], masks[1][-1] = 1, 0
        real["skip"], decoy["skip"] = (G.dev(m) for m in masks)
        names = Cc.PLANES + ["sst_ext", "sss_ext", "skip"]
        w, inputs = G.work_of(real, decoy, names)
        base = lambda: ctx.slab_default_params(relax_t=86400.0, relax_s=10 * 86400.0)

        def setup():
            ctx.set_column_params(ctx.column_default_params())
            ctx.set_slab_params(base())

        def launch():
            ctx.column_step_ocean(Cc.DT, {k: w[k] for k in abi.STATE}, {k: w[k] for k in abi.FORCING}, w["newice"],
                                  {"sst": w["sst_ext"], "sss": w["sss_ext"]}, w["skip"])

        if name == "column_step_ocean":
            return Case(launch, inputs, [w[k] for k in OCEAN_OUT], setup=setup)
        if name == "slab_params_set":  # other parameters, then the launch that reads them

            def call():
                ctx.set_slab_params(ctx.slab_default_params(relax_t=7200.0, relax_s=0.0, ice_salinity=8.0))
                launch()

            return Case(call, inputs, [w[k] for k in OCEAN_OUT], setup=setup)
        raise KeyError(name)

    return build


COVERS = {"column_step_ocean": ["nsdg_column_step_ocean"], "slab_params_set": ["nsdg_slab_params_set", "nsdg_slab_default_params"]}
TABLE = [G.Row("%s[%d]" % (name, n), row(name, n), COVERS[name]) for n in (1025, 2) for name in ("column_step_ocean", "slab_params_set")]
ROWS = {r.name: r for r in TABLE}


def test_every_function_of_the_header_has_a_row_and_a_binding():
    names = declared_functions()
    assert names == ["nsdg_column_step_ocean", "nsdg_slab_default_params", "nsdg_slab_params_set"]
    assert {c for r in TABLE for c in r.covers} == set(names) and len(ROWS) == len(TABLE)
    assert sorted(abi.OCEAN_SYMBOLS) == names
    assert not set(abi.OCEAN_SYMBOLS) & (set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS) | set(abi.BASAL_SYMBOLS))
    assert not any(r.blocks_host for r in TABLE)


class Env:
    """one side of the comparison: a context bound to the side stream, or to the default stream (the part of
    tests/test_gpu_stream_order.py's Env these rows need)"""

    def __init__(self, gpu, stream):
        self.ctx = abi.Context(gpu) if stream is None else abi.Context(gpu, stream=stream)
        self.families, self.cases = {}, {}

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
        self.products = max(DELAY_MIN_PRODUCTS, int(math.ceil(1.25 * G.DELAY_FACTOR * 1e3 * longest / one)))
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
    case = proto.side.cases[name]
    gc.collect()  # (a full collection now, not inside the call: see DELAY_MIN_PRODUCTS)
    seconds = SO.check(name, case, proto.backend, False, proto.references[name])
    print("%s: the call took %.3f ms on the host under a delay of %.3f ms" % (name, 1e3 * seconds, proto.delay_ms))
    assert proto.delay_ms >= G.DELAY_FACTOR * proto.longest_ms
    # the row did something: the ocean the consumer saw is neither the real input nor the decoy, except under the mask; and the two
    # rows of one size differ (the setter acted on the launch behind it)
    seen = proto.references[name][0][1]
    real = {k: r for (_, r, _), k in zip(case.inputs, Cc.PLANES + ["sst_ext", "sss_ext", "skip"])}
    free = real["skip"] == 0
    for got, k in zip(seen[-2:], ("sst", "sss")):
        assert bool((got[free] != real[k][free]).any()) and bool((got[~free] == real[k][~free]).all()), k
    other = name.replace("slab_params_set", "X").replace("column_step_ocean", "slab_params_set").replace("X", "column_step_ocean")
    if other in proto.references:
        assert not torch.equal(proto.references[other][0][1][-1], seen[-1])

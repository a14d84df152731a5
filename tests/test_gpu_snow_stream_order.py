"""The snow-load calls of include/nsdg_snow.h held to stream order on a stream other than the default, by the protocol of
tests/stream_order.py and with the families and the delay of tests/test_gpu_stream_order.py, whose table holds the functions of
include/nsdg.h itself: nsdg_snow.h is a header of its own with a table of its own, TABLE below (the pattern of
tests/test_gpu_basal_stream_order.py).  Every function that header declares has a row (checked without a GPU); every row passes between
a late producer and an early consumer on a side stream, and what the consumer sees is, bit for bit, the plain call on the side-stream
context and on a default-stream context.  The snow is an array argument like any other: the producer writes it late.  The setter is
host-only: its row makes the call and then the packing that reads the field."""
import os
import re

import numpy as np
import pytest
import torch

import stream_order as SO
import test_gpu_basal_stream_order as GB
import test_gpu_stream_order as G
from nextsimdg_amd import abi
from stream_order import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 130, 5


def declared_functions():
    src = open(os.path.join(ROOT, "include", "nsdg_snow.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))


def snows():
    """two DG snow fields, 0.1 .. 0.6 m with small slopes"""
    out = {}
    for k, s in (("real", 13), ("decoy", 14)):
        rng = np.random.default_rng(s)
        f = 0.02 * rng.standard_normal((6, NY, NX))
        f[0] = rng.uniform(0.1, 0.6, (NY, NX))
        out[k] = G.dev(f)
    return out


def row(name, masked):
    """the call `name` on the mEVP family of tests/test_gpu_stream_order.py (130 x 5, with or without its island)"""
    def build(env):
        ctx = env.ctx
        F = env.family(G.Mevp, ctx, NX, NY, masked)
        d = snows()
        snow = d["decoy"].clone()
        triple = (snow, d["real"], d["decoy"])

        def setup():
            F.setup()
            ctx.set_snow_load(snow)

        if name == "snow_load_nodal":
            w, inputs = G.work_of(F.real, F.decoy, ("cgh", "cga"))
            out = G.sentinel_like(w["cgh"])
            return Case(lambda: ctx.snow_load_nodal(w["cgh"], w["cga"], out[0]), inputs + [triple], out, fill=out, setup=setup)
        if name == "snow_load_set":  # the field is set inside the call; the packing that follows takes the mass from it
            w, inputs = G.work_of(F.real, F.decoy, ("H", "A", "ua", "va", "uo", "vo", "u0", "v0"))
            out = G.sentinel_like(F.real["packed"])
            dt = F.case["dt"]

            def setup_without():
                setup()
                ctx.set_snow_load(None)

            def call():
                ctx.set_snow_load(snow)
                ctx.mevp_prepare(dt, w["H"], w["A"], (w["ua"], w["va"]), (w["uo"], w["vo"]), (w["u0"], w["v0"]), out[0])

            return Case(call, inputs + [triple], out, fill=out, setup=setup_without)
        raise KeyError(name)

    return build


COVERS = {"snow_load_nodal": ["nsdg_snow_load_nodal"], "snow_load_set": ["nsdg_snow_load_set"]}
TABLE = [G.Row("%s[%dx%d%s]" % (name, NX, NY, "-island" if masked else ""), row(name, masked), COVERS[name])
         for masked in (False, True) for name in ("snow_load_nodal", "snow_load_set")]
ROWS = {r.name: r for r in TABLE}


def test_every_function_of_the_header_has_a_row_and_a_binding():
    names = declared_functions()
    assert names == ["nsdg_snow_load_nodal", "nsdg_snow_load_set"]
    assert {c for r in TABLE for c in r.covers} == set(names) and len(ROWS) == len(TABLE)
    others = set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS) | set(abi.BASAL_SYMBOLS) | set(abi.OCEAN_SYMBOLS)
    assert sorted(abi.SNOW_SYMBOLS) == names and not set(abi.SNOW_SYMBOLS) & others
    assert not any(r.blocks_host for r in TABLE)


class Proto(GB.Proto):
    """tests/test_gpu_basal_stream_order.py's Proto over the rows of this file (its constructor reads the module's TABLE: restated here)"""

    def __init__(self, gpu):
        import math

        from nextsimdg_amd import build

        build.build_lib(verbose=False)
        self.stream = torch.cuda.Stream()
        assert self.stream.cuda_stream != 0
        self.side, self.default = GB.Env(gpu, self.stream), GB.Env(gpu, None)
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
    # the row did something: the outputs are not all sentinel, the plain results on the two contexts were equal (Proto), and the packed
    # c[0] (or the diagnostic h') the consumer sees is larger than the ice-only one somewhere
    seen = proto.references[name][0][1][0]
    assert not bool((seen == SO.SENTINEL).all())
    ctx = proto.side.ctx
    F = proto.side.families[("Mevp", id(ctx), NX, NY, name.endswith("-island]"))]
    r, n = F.real, F.real["cgh"].numel()
    with torch.cuda.stream(proto.stream):
        torch.cuda.synchronize()
        F.setup()
        ctx.set_snow_load(None)
        ice_only = torch.zeros_like(r["packed"])
        ctx.mevp_prepare(F.case["dt"], r["H"], r["A"], (r["ua"], r["va"]), (r["uo"], r["vo"]), (r["u0"], r["v0"]), ice_only)
        torch.cuda.synchronize()
    ice_only = ice_only.view(4, n, 2)[0, :, 0]
    if name.startswith("snow_load_nodal"):  # h' before the scaling of an ice-free node: compared where the packing did not scale
        plain = ice_only < 1e20
        seen, ice_only = seen.reshape(-1)[plain], ice_only[plain]
    else:
        seen = seen.view(4, n, 2)[0, :, 0]
    assert bool((seen >= ice_only).all()) and bool((seen > ice_only).any())

"""The sea-surface tilt calls of include/nsdg_tilt.h held to stream order on a stream other than the default, by the protocol of
tests/stream_order.py and with the families and the delay of tests/test_gpu_stream_order.py, in the manner of
tests/test_gpu_snow_stream_order.py: nsdg_tilt.h is a header of its own with a table of its own, TABLE below.  Every function that header
declares has a row (checked without a GPU); every row passes between a late producer and an early consumer on a side stream, and what the
consumer sees is, bit for bit, the plain call on the side-stream context and on a default-stream context.  The height is an array argument
like any other: the producer writes it late.  The setter is host-only: its row makes the call and then the packing that reads the field."""
import os
import re

import numpy as np
import pytest
import torch

import stream_order as SO
import test_gpu_basal_stream_order as GB
import test_gpu_snow_stream_order as GS
import test_gpu_stream_order as G
from nextsimdg_amd import abi
from stream_order import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 130, 5


def declared_functions():
    src = open(os.path.join(ROOT, "include", "nsdg_tilt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))


def heights():
    """two sea-surface heights on the 261 x 11 lattice: a slope with noise, metres"""
    out = {}
    for k, s in (("real", 17), ("decoy", 18)):
        rng = np.random.default_rng(s)
        out[k] = G.dev(np.linspace(0.0, 1.0, 2 * NX + 1)[None, :] * rng.uniform(0.5, 2.0) + 0.05 * rng.standard_normal((2 * NY + 1, 2 * NX + 1)))
    return out


def row(name, masked):
    """the call `name` on the mEVP family of tests/test_gpu_stream_order.py (130 x 5, with or without its island)"""
    def build(env):
        ctx = env.ctx
        F = env.family(G.Mevp, ctx, NX, NY, masked)
        d = heights()
        ssh = d["decoy"].clone()
        triple = (ssh, d["real"], d["decoy"])

        def setup():
            F.setup()
            ctx.set_block(0, NY)
            ctx.set_tilt(ssh)

        if name == "tilt_nodal":
            out = G.sentinel_like(ssh, ssh)
            return Case(lambda: ctx.tilt_nodal(out[0], out[1]), [triple], out, fill=out, setup=setup)
        if name == "boxtest_ssh":  # no array input: the early consumer is what the row holds
            out = G.sentinel_like(ssh)
            return Case(lambda: ctx.boxtest_ssh(NX * 1000.0, 1.46e-4, abi.GRAVITY, out[0]), [], out, fill=out, setup=setup)
        if name == "tilt_set":  # the field is set inside the call; the packing that follows takes the tilt from it
            w, inputs = G.work_of(F.real, F.decoy, ("H", "A", "ua", "va", "uo", "vo", "u0", "v0"))
            out = G.sentinel_like(F.real["packed"])
            dt = F.case["dt"]

            def setup_without():
                setup()
                ctx.set_tilt(None)

            def call():
                ctx.set_tilt(ssh)
                ctx.mevp_prepare(dt, w["H"], w["A"], (w["ua"], w["va"]), (w["uo"], w["vo"]), (w["u0"], w["v0"]), out[0])

            return Case(call, inputs + [triple], out, fill=out, setup=setup_without)
        raise KeyError(name)

    return build


COVERS = {"tilt_nodal": ["nsdg_tilt_nodal"], "tilt_set": ["nsdg_tilt_set"], "boxtest_ssh": ["nsdg_boxtest_ssh"]}
TABLE = [G.Row("%s[%dx%d%s]" % (name, NX, NY, "-island" if masked else ""), row(name, masked), COVERS[name])
         for masked in (False, True) for name in ("tilt_nodal", "tilt_set", "boxtest_ssh") if not (masked and name == "boxtest_ssh")]
ROWS = {r.name: r for r in TABLE}


def test_every_function_of_the_header_has_a_row_and_a_binding():
    names = declared_functions()
    assert names == ["nsdg_boxtest_ssh", "nsdg_tilt_nodal", "nsdg_tilt_set"]
    assert {c for r in TABLE for c in r.covers} == set(names) and len(ROWS) == len(TABLE)
    others = set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS) | set(abi.BASAL_SYMBOLS) | set(abi.OCEAN_SYMBOLS) | set(abi.SNOW_SYMBOLS)
    assert sorted(abi.TILT_SYMBOLS) == names and not set(abi.TILT_SYMBOLS) & others
    assert not any(r.blocks_host for r in TABLE)


class Proto(GS.Proto):
    """tests/test_gpu_snow_stream_order.py's Proto over the rows of this file (its constructor reads the module's TABLE: restated here)"""

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
    # the row did something: no output is all sentinel, the plain results on the two contexts were equal (Proto), and the packed c2 the
    # consumer sees is not the one of the geostrophic tilt
    seen = proto.references[name][0][1]
    assert not any(bool((s == SO.SENTINEL).all()) for s in seen)
    if name.startswith("tilt_set"):
        ctx = proto.side.ctx
        F = proto.side.families[("Mevp", id(ctx), NX, NY, name.endswith("-island]"))]
        r, n = F.real, F.real["cgh"].numel()
        with torch.cuda.stream(proto.stream):
            torch.cuda.synchronize()
            F.setup()
            ctx.set_tilt(None)
            geo = torch.zeros_like(r["packed"])
            ctx.mevp_prepare(F.case["dt"], r["H"], r["A"], (r["ua"], r["va"]), (r["uo"], r["vo"]), (r["u0"], r["v0"]), geo)
            torch.cuda.synchronize()
        got, geo = seen[0].view(4, n, 2), geo.view(4, n, 2)
        assert torch.equal(got[0], geo[0]) and torch.equal(got[2], geo[2]) and not torch.equal(got[1], geo[1])

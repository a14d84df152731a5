"""nsdg_momentum_budget (include/nsdg_budget.h) held to stream order on a stream other than the default, by the protocol of
tests/stream_order.py and with the families and the delay of tests/test_gpu_stream_order.py, in the manner of
tests/test_gpu_tilt_stream_order.py: nsdg_budget.h is a header of its own with a table of its own, TABLE below.  The launch passes between
a late producer and an early consumer on a side stream, and what the consumer sees -- sixteen planes and the row totals -- is, bit for bit,
the plain call on the side-stream context and on a default-stream context.  nsdg_budget_term_id is host-only and touches no stream."""
import os
import re

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
NAMES = tuple(f[0] for f in abi.BudgetOut._fields_[:16])
INPUTS = ("H", "A", "ua", "va", "s11", "s12", "s22", "u", "v")


def declared_functions():
    src = open(os.path.join(ROOT, "include", "nsdg_budget.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))


def row(masked, totals):
    """the launch on the mEVP family of tests/test_gpu_stream_order.py (130 x 5, with or without its island): the state and the forcing are
    produced late; the packing is the family's own (Mevp.setup packs the real case on the context)"""
    def build(env):
        ctx = env.ctx
        F = env.family(G.Mevp, ctx, NX, NY, masked)
        w, inputs = G.work_of(F.real, F.decoy, INPUTS)
        planes = dict(zip(NAMES, G.sentinel_like(*[F.real["u"]] * 16)))
        power = torch.full((abi.BUDGET_QUANTITIES, NY), SO.SENTINEL, dtype=torch.float64, device="cuda") if totals else None
        out = list(planes.values()) + ([power] if totals else [])

        def call():
            ctx.momentum_budget(0, NY, w["H"], w["A"], (w["ua"], w["va"]), (w["s11"], w["s12"], w["s22"]), (w["u"], w["v"]), F.real["packed"], planes, power)

        return Case(call, inputs, out, fill=out, setup=F.setup)

    return build


TABLE = [G.Row("momentum_budget[%dx%d%s%s]" % (NX, NY, "-island" if masked else "", "-totals" if totals else ""), row(masked, totals), ["nsdg_momentum_budget"])
         for masked in (False, True) for totals in (False, True)]
ROWS = {r.name: r for r in TABLE}


def test_every_function_of_the_header_has_a_row_and_a_binding():
    names = declared_functions()
    assert names == ["nsdg_budget_term_id", "nsdg_momentum_budget"]
    assert {c for r in TABLE for c in r.covers} == set(names) - {"nsdg_budget_term_id"} and len(ROWS) == len(TABLE)  # the other is host-only
    others = set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS) | set(abi.BASAL_SYMBOLS) | set(abi.OCEAN_SYMBOLS) | set(abi.SNOW_SYMBOLS) | set(abi.TILT_SYMBOLS)
    assert sorted(abi.BUDGET_SYMBOLS) == names and not set(abi.BUDGET_SYMBOLS) & others
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
    # the row did something: no output keeps a sentinel, and the forces are felt
    seen = proto.references[name][0][1]
    assert not any(bool((s == SO.SENTINEL).any()) for s in seen)
    assert float(seen[NAMES.index("residual_x")].abs().max()) > 1e-6 and float(seen[NAMES.index("internal_y")].abs().max()) > 1e-6

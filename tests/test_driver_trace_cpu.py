"""The work the Python step driver (nextsimdg_amd/rowblock.py) asks for, pinned call by call.  The other driver tests compare results: a
redundant launch or ghost exchange gives the same bits and passes them all.  Here every call a core makes on its `ops` object and every
exchange it posts is recorded -- names, row ranges, scalars and WHICH buffers (tensors are numbered in the order of their first appearance)
-- and compared with tests/golden/driver_trace_v1.json.  Nothing is computed that matters: the optional calls of the C ABI are do-nothing
stubs on top of the CPU stand-in (tests/oracle_ops.py), the exchanger moves nothing, ghost rows go stale; only the trace is compared.

The golden file was recorded with this file itself, `python tests/test_driver_trace_cpu.py --record`, on the commit BEFORE the driver was
restated as one step frame with its outputs in nextsimdg_amd/outputs.py.  A change of the driver does not re-record it (--record refuses to
overwrite): a trace that differs is a changed sequence of launches or exchanges, which is what this test is there to catch.  The calls made
while a core is constructed are compared as a sorted list -- the order of allocations is not behaviour --, everything after in order.

The coupled case on rank 1 of 3 runs inside a torch.distributed group of ONE rank (gloo, in-process store): advance(substeps="auto") takes
the maximum over the ranks through the exchanger's group, which a core on a multi-block RowBlock cannot do without one.  The reduction
over one rank is the identity and is not part of the trace."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle_ops import OracleOps  # noqa: E402
from nextsimdg_amd import rowblock, synthetic  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "driver_trace_v1.json")
NX = 12


# ---------------------------------------------------------------------------------------------------------------- recording
class Recorder:
    """the trace and the numbering of the tensors, shared by the ops proxy and the exchanger"""

    def __init__(self):
        self.trace, self.ids, self.seen = [], {}, []

    def encode(self, x):
        if isinstance(x, torch.Tensor):
            key = (x.data_ptr(), tuple(x.shape), tuple(x.stride()))
            if key not in self.ids:
                self.ids[key] = "t%d" % len(self.ids)
                self.seen.append(x)  # kept alive: no address is used twice
            return self.ids[key]
        if x is None or isinstance(x, (bool, str)):
            return x
        if isinstance(x, (int, np.integer)):
            return int(x)
        if isinstance(x, float):
            return repr(float(x))
        if isinstance(x, (list, tuple)):
            return [self.encode(v) for v in x]
        if isinstance(x, dict):
            return {str(k): self.encode(v) for k, v in x.items()}
        if isinstance(x, torch.device):
            return str(x)
        return type(x).__name__

    def log(self, name, args=(), kwargs=None):
        self.trace.append([name, self.encode(args), self.encode(kwargs or {})])


class RecordingOps:
    """forwards everything to `ops`; every call is logged first"""

    def __init__(self, ops, rec):
        self.__dict__["_ops"], self.__dict__["_rec"] = ops, rec

    def __getattr__(self, name):
        attr = getattr(self._ops, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            self._rec.log(name, args, kwargs)
            return attr(*args, **kwargs)

        return call

    def __setattr__(self, name, value):
        setattr(self._ops, name, value)


class RecordingExchanger(rowblock.HaloExchanger):
    """the planning of HaloExchanger; the transport logs what would travel and moves nothing"""

    def __init__(self, blk, rec):
        super().__init__(blk)
        self.rec = rec

    def _start(self, plan):
        self.rec.log("exchange_start", (plan.up_send, plan.down_send, plan.from_above, plan.from_below))
        return plan

    def _finish(self, handle):
        self.rec.log("exchange_finish")


class StubOps(OracleOps):
    """the oracle and do-nothing stand-ins for the optional calls of abi.Context it lacks"""

    def concentration_max(self, H, A, j0=0, j1=None):
        return 0.97

    def phase_times(self, reset=False):
        return {}, (0.0, 0)


for _name in ("history_accumulate", "history_accumulate_stats", "history_row_totals", "drifters_advance", "tracer_weight", "tracer_recover",
              "set_land_mask", "land_clear", "land_clear_nodes", "bbm_prepare", "bbm_iterate", "phase_timing", "phase_mark", "column_forcing",
              "column_wind", "forcing_sample"):
    setattr(StubOps, _name, lambda self, *a, **kw: None)


# ---------------------------------------------------------------------------------------------------------------- the cases
def make(cls, rec, ny, nsub, rank=0, world=1, depth=(1, 1), variant=1, overlap=True, **kw):
    bt = synthetic.BoxTest(NX, ny)
    blk = rowblock.RowBlock(NX, ny, rank, world, *depth)
    ops = RecordingOps(StubOps(mevp_variant=variant, alpha=200.0, beta=200.0), rec)
    core = cls(ops, blk, bt.hx, bt.hy, 120.0, nsub, torch.device("cpu"), exchanger=RecordingExchanger(blk, rec) if world > 1 else None,
               overlap=overlap, **kw)
    built = len(rec.trace)
    H, A = bt.dg_fields()
    A[0] -= 0.2
    ua, va = bt.wind(0.0)
    core.load_global(H, A, *bt.ocean(), 3.0 * ua, 3.0 * va, **({"D": np.zeros_like(H)} if kw.get("rheology") == "bbm" else {}))
    return core, bt, built


def dynamics(steps=2, **kw):
    def run(rec):
        core, _, built = make(rowblock.DynamicsCore, rec, **kw)
        for _ in range(steps):
            core.step()
        core.close()
        return built

    return run


def whole_domain_state(core, part):
    """a state of the whole domain with the keys of `part` (one rank's state_dict()): zeros, and the drifter list as it is"""
    b = core.blk
    out = {"rows": (0, b.ny_glob), "ny_global": b.ny_glob, "nx": b.nx}
    for k, a in part.items():
        if k == "drifters":
            out[k] = a
        elif k in ("u", "v"):
            out[k] = np.zeros((2 * b.ny_glob + 1, 2 * b.nx + 1))
        elif k not in out:
            out[k] = np.zeros((a.shape[0], b.ny_glob, b.nx))
    return out


def coupled(ny, drifters, **kw):
    def run(rec):
        L = synthetic.BoxTest(NX, ny).L
        rng = np.random.default_rng(3)
        forcing = rowblock.ForcingSeries([0.0, 3600.0], {k: rng.random((2, 3, 4)) for k in rowblock.ForcingSeries.COLUMN + rowblock.ForcingSeries.WIND})
        land = np.zeros((ny, NX), dtype=bool)
        land[ny // 3:2 * ny // 3, 3:6] = True
        points = {"drifters": [[0.3 * L, 0.3 * L], [0.5 * L, 0.5 * L], [0.7 * L, 0.2 * L]]} if drifters else {}
        core, _, built = make(rowblock.CoupledCore, rec, ny=ny, advect_column_state=True, forcing=forcing, land=land, phase_timing=True,
                              history=("hice", "speed:ice_mean", "hice:max"), series=("area", "drift"), **points, **kw)
        state, planes, _ = synthetic.column_fields(NX * ny, 5)
        core.load_column({k: v.reshape(ny, NX) for k, v in {**state, **planes}.items()})
        core.step()
        core.advance(240.0, substeps=2)
        core.advance(240.0, substeps="auto")
        core.load_state_dict(whole_domain_state(core, core.state_dict()))
        core.step()
        core.history_read(), core.series_read(), core.phase_times()
        if drifters:
            core.drifters_read()
        core.close()
        return built

    return run


def in_a_group_of_one(run):
    def wrapped(rec):
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
        try:
            return run(rec)
        finally:
            dist.destroy_process_group()

    return wrapped


MIDDLE = dict(rank=1, world=3)
CASES = {
    "one_block_v1_nsub7": dynamics(ny=12, nsub=7),
    # the split single-iteration path: 9 launches and 6 exchanges per step
    "rank1of3_depth11_v1_ny30_nsub3_overlap": dynamics(ny=30, nsub=3, **MIDDLE),
    "rank1of3_depth11_v1_ny30_nsub3_no_overlap": dynamics(ny=30, nsub=3, overlap=False, **MIDDLE),
    # a split 4-pass and a 3-pass remainder; 15 owned rows, the split needs depth_below + depth_above + 5 = 12
    "rank1of3_depth43_v4_ny45_nsub7_overlap": dynamics(ny=45, nsub=7, depth=(4, 3), variant=4, **MIDDLE),
    "rank1of3_depth43_v4_ny45_nsub7_no_overlap": dynamics(ny=45, nsub=7, depth=(4, 3), variant=4, overlap=False, **MIDDLE),
    # groups of two passes, a two-iteration remainder and the once-per-step transport exchange: 8 + 3 launches and 4 exchanges
    "rank1of3_depth87_v4_ny60_nsub18": dynamics(ny=60, nsub=18, depth=(8, 7), variant=4, **MIDDLE),
    "bbm_one_block": dynamics(ny=12, nsub=5, rheology="bbm"),
    "bbm_rank1of3_depth11": dynamics(ny=30, nsub=3, rheology="bbm", **MIDDLE),
    "coupled_one_block_everything_on": coupled(ny=12, drifters=True, nsub=4),
    "coupled_rank1of3_depth11_everything_but_drifters": in_a_group_of_one(coupled(ny=30, drifters=False, nsub=3, **MIDDLE)),
    "history_of_bare_names": dynamics(ny=12, nsub=3, history=("hice", "speed")),
}


def record(name):
    rec = Recorder()
    built = CASES[name](rec)
    return {"construction": sorted(rec.trace[:built], key=json.dumps), "run": rec.trace[built:]}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES)
    assert all(g["run"] and g["construction"] for g in golden.values())


def count(calls, prefix):
    return sum(1 for c in calls if c[0].startswith(prefix))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_driver_asks_for_the_same_work(name, golden):
    got, want = json.loads(json.dumps(record(name))), golden[name]
    print("%s: %d calls at construction, %d after (%d mEVP / BBM launches, %d exchanges)"
          % (name, len(got["construction"]), len(got["run"]), count(got["run"], "mevp_iterate") + count(got["run"], "bbm_iterate"),
             count(got["run"], "exchange_start")))
    assert got["construction"] == want["construction"]
    for k, (g, w) in enumerate(zip(got["run"], want["run"])):
        assert g == w, "call %d of %s: the driver asks for %s, recorded was %s" % (k, name, g, w)
    assert len(got["run"]) == len(want["run"])


def test_the_branches_the_cases_are_there_for_are_taken(golden):
    """per step() of two: the launches of the sub-cycle and the exchanges, as the cases' comments say"""
    per_step = lambda name, prefix: count(golden[name]["run"], prefix) / 2
    assert per_step("rank1of3_depth11_v1_ny30_nsub3_overlap", "mevp_iterate") == 9
    assert per_step("rank1of3_depth11_v1_ny30_nsub3_overlap", "exchange_start") == 6
    assert per_step("rank1of3_depth11_v1_ny30_nsub3_no_overlap", "mevp_iterate") == 3
    assert per_step("rank1of3_depth43_v4_ny45_nsub7_overlap", "mevp_iterate4") == 3 and per_step("rank1of3_depth43_v4_ny45_nsub7_overlap", "mevp_iterate3") == 3
    assert per_step("rank1of3_depth43_v4_ny45_nsub7_no_overlap", "mevp_iterate4") == 1
    assert per_step("rank1of3_depth87_v4_ny60_nsub18", "mevp_iterate4") == 8 and per_step("rank1of3_depth87_v4_ny60_nsub18", "mevp_iterate2") == 3
    assert per_step("rank1of3_depth87_v4_ny60_nsub18", "exchange_start") == 4
    assert count(golden["history_of_bare_names"]["run"], "history_accumulate") == 2 and count(golden["history_of_bare_names"]["run"], "history_accumulate_stats") == 0


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/test_driver_trace_cpu.py --record")
    if os.path.exists(GOLDEN):
        raise SystemExit("%s exists: the traces are recorded once, on the commit before a change of the driver" % GOLDEN)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(n), json.dumps(record(n), separators=(",", ":"))) for n in sorted(CASES)) + "\n}\n")
    print("recorded %d cases into %s" % (len(CASES), GOLDEN))

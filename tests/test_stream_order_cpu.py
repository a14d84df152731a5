"""What the stream-order tests (tests/test_gpu_stream_order.py) rest on, without a GPU: the rows of its table and HOST_ONLY below
partition the functions of include/nsdg.h -- a new ABI function cannot be added without deciding which it is --, and the compare logic of
the protocol (tests/stream_order.py) does reject a stale, a decoy-derived and an out-of-rows output, shown on a stand-in call on CPU
tensors with a fake stream that runs nothing before it is synchronised."""
import pytest
import torch

import stream_order as SO
import test_gpu_stream_order as G
from stream_order import SENTINEL, Case
from test_abi_symbols import declared_functions

SETTER = "stores host state in the context; read when a later call is made (test_setter_between_two_enqueued_calls_acts_on_the_second_only)"
HOST = "host only: no context, or nothing but host memory"
PLAN = "builds or frees a plan or a communicator: allocations and host tables, no work ordered against the caller's stream"
HOST_ONLY = {
    "nsdg_abi_version": HOST, "nsdg_last_error": HOST, "nsdg_tiled_len": HOST,
    "nsdg_column_default_params": HOST, "nsdg_mevp_default_params": HOST, "nsdg_bbm_default_params": HOST, "nsdg_bbm_params_check": HOST,
    "nsdg_mevp_stable_params": HOST, "nsdg_mevp_creep_percent_per_day": HOST, "nsdg_substep_count": HOST, "nsdg_bbm_substep_count": HOST,
    "nsdg_history_field_name": HOST, "nsdg_history_field_id": HOST, "nsdg_history_stat_name": HOST, "nsdg_history_stat_id": HOST,
    "nsdg_history_series_name": HOST, "nsdg_history_series_id": HOST,
    "nsdg_grid_set": SETTER, "nsdg_block_set": SETTER, "nsdg_column_params_set": SETTER, "nsdg_mevp_params_set": SETTER, "nsdg_bbm_params_set": SETTER,
    "nsdg_mevp_variant_set": SETTER, "nsdg_transport_variant_set": SETTER, "nsdg_mevp_strip_rows_set": SETTER, "nsdg_mevp_occupancy_set": SETTER,
    "nsdg_transport_bounds_set": SETTER, "nsdg_land_mask_set": SETTER, "nsdg_comm_deadline_set": SETTER, "nsdg_comm_simulate_wire": SETTER,
    "nsdg_phase_timing_set": "allocates or frees the event ring; discards what was pending, records nothing on the stream",
    "nsdg_ctx_create": "allocates the context; its one device operation, the reset of the give-up counter, is enqueued on the context's stream",
    "nsdg_ctx_destroy": "waits for the context's stream, then frees",
    "nsdg_comm_unique_id": HOST, "nsdg_comm_rank": HOST,
    "nsdg_comm_init": PLAN + " (RCCL: needs one process per GPU)", "nsdg_comm_init_local": PLAN, "nsdg_comm_finalize": PLAN + "; drains the communication stream",
    "nsdg_comm_max_f64": "local transport: a host scalar reduced on the host, no stream involved; the RCCL form needs two GPUs",
    "nsdg_halo_plan_create": PLAN, "nsdg_halo_plan_destroy": PLAN, "nsdg_halo_counts": HOST,
    "nsdg_rb_mevp_create": PLAN, "nsdg_rb_mevp_destroy": PLAN, "nsdg_rb_mevp_info": HOST,
    "nsdg_rb_bbm_create": PLAN, "nsdg_rb_bbm_destroy": PLAN, "nsdg_rb_transport_create": PLAN, "nsdg_rb_transport_destroy": PLAN,
}


def test_table_and_host_only_partition_the_header():
    names = set(declared_functions())
    rows = {c for r in G.TABLE for c in r.covers}
    assert not rows & set(HOST_ONLY), sorted(rows & set(HOST_ONLY))
    assert not rows - names and not set(HOST_ONLY) - names, sorted((rows | set(HOST_ONLY)) - names)
    assert rows | set(HOST_ONLY) == names, "neither a row of the table nor HOST_ONLY: %s" % sorted(names - rows - set(HOST_ONLY))
    assert all(isinstance(v, str) and v for v in HOST_ONLY.values())
    assert len({r.name for r in G.TABLE}) == len(G.TABLE)


def test_table_has_the_rows_and_the_shapes_the_kernels_need():
    names = [r.name for r in G.TABLE]
    blocking = {r.name.split("[")[0] for r in G.TABLE if r.blocks_host}
    assert blocking == {"concentration_max", "comm_max_f64_array", "ctx_synchronize", "mevp_pipeline_health", "phase_times", "halo_stats_get",
                        "rb_mevp_stats", "rb_bbm_stats", "rb_transport_stats"}
    for need in ("column_step[1025]", "column_step[1025-diag]", "mevp_subcycle[130x5]-nsub7", "mevp_subcycle[130x5]-nsub8", "transport_step[130x5-dg0]",
                 "transport_step[65x5-dg2]", "bbm_iterate[70x9-island]", "bbm_iterate[65x3]", "rb_mevp_run[single-graph]", "rb_mevp_run[loopback-graph]",
                 "rb_bbm_run[loopback]", "rb_transport_run[single]", "copy_f64[1025]", "land_clear[70x9-island]"):
        assert need in names, need
    for order in (0, 1, 2):
        for call in ("transport_stage", "transport_step", "transport_step_oop", "transport_step_oop_rows", "transport_limit"):
            assert "%s[130x5-dg%d]" % (call, order) in names


# ---- the protocol against a stand-in: CPU tensors, a stream that runs nothing before it is synchronised ----------------------------------------
class FakeEvent:
    def __init__(self, stream, position):
        self.stream, self.position = stream, position

    def query(self):
        return self.stream.done >= self.position


class FakeBackend:
    """every operation is queued and runs in order at the next synchronise -- the latest a real stream may run it"""

    def __init__(self):
        self.queue, self.done = [], 0

    def push(self, fn):
        self.queue.append(fn)

    def copy(self, dst, src):
        self.push(lambda: dst.copy_(src))

    def fill(self, t, value):
        self.push(lambda: t.fill_(value))

    def clone(self, t):
        out = torch.empty_like(t)
        self.push(lambda: out.copy_(t))
        return out

    def delay(self):
        self.push(lambda: None)

    def record(self):
        self.push(lambda: None)
        return FakeEvent(self, self.done + len(self.queue))

    def synchronize(self):
        while self.queue:
            self.queue.pop(0)()
            self.done += 1

    synchronize_all = synchronize


def stand_in(backend, how):
    """out[1:3] = 2 w[1:3] on four-element arrays, made in the ways a library can make it"""
    real, decoy = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), torch.tensor([5.0, 6.0, 7.0, 8.0], dtype=torch.float64)
    w, out = decoy.clone(), torch.full((4,), SENTINEL, dtype=torch.float64)
    work = lambda: out[1:3].copy_(2.0 * w[1:3])

    def call():
        if how == "ordered":
            backend.push(work)
        elif how == "eager":  # a launch on another stream: it runs when the host makes the call and reads what memory holds then
            work()
        elif how == "blocking":
            backend.synchronize()
            work()
        elif how == "late":  # work left on a stream nobody joins: it runs after the consumer has looked
            backend.push(lambda: None)
            call.pending = work
        elif how == "outside":
            backend.push(lambda: out.copy_(2.0 * w))
        return 7 if how != "host" else 8

    return Case(call, [(w, real, decoy)], [out], fill=[out], untouched=lambda seen: [seen[0][:1], seen[0][3:]])


def reference():
    b = FakeBackend()
    ref = SO.plain(stand_in(b, "ordered"), b)
    assert ref[0] == 7 and ref[1][0].tolist() == [SENTINEL, 4.0, 6.0, SENTINEL]
    return ref


def test_protocol_accepts_an_ordered_and_a_blocking_call():
    b = FakeBackend()
    SO.check("ordered", stand_in(b, "ordered"), b, False, [reference()])
    b = FakeBackend()
    SO.check("blocking", stand_in(b, "blocking"), b, True, [reference()])


@pytest.mark.parametrize("how, blocks, message", [
    ("eager", False, "output 0 differs"),  # decoy-derived: 2 * decoy, then lost to the producer's fill
    ("late", False, "output 0 differs"),  # stale: the consumer sees the sentinel
    ("outside", False, "untouched part"),
    ("host", False, "host results"),
    ("blocking", False, "delay too short, nothing proven"),
    ("ordered", True, "documented as host-blocking"),
])
def test_protocol_rejects(how, blocks, message):
    b = FakeBackend()
    case = stand_in(b, how)
    with pytest.raises(AssertionError, match=message):
        want = reference()
        if how == "outside":  # the rows inside are right: only the untouched-rows check can see it
            want = (want[0], [torch.tensor([2.0, 4.0, 6.0, 8.0], dtype=torch.float64)])
        SO.check(how, case, b, blocks, [want])


def test_compare_is_bitwise():
    a = torch.tensor([0.0, float("nan")], dtype=torch.float64)
    assert SO.same_bits(a, a.clone())
    assert not SO.same_bits(a, torch.tensor([-0.0, float("nan")], dtype=torch.float64))
    assert not SO.same_bits(a, a.to(torch.float32))

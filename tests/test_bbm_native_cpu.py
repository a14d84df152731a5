"""The native brittle row-block plan (nsdg_rb_bbm_*) on a machine without a device: the entry points answer with statuses, the binding
matches the header's struct, and the driver refuses what the plan does not do."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bbm_ref as R  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    return abi.load_library()


def test_entry_points_answer_with_statuses_without_a_device(lib):
    d, h, out, st = abi.RbBbmDesc(), C.c_void_p(), abi.I32(-7), abi.HaloStats()
    assert lib.nsdg_rb_bbm_create(None, C.byref(d), C.byref(h)) == -1 and not h.value
    assert lib.nsdg_rb_bbm_create(None, None, None) == -1
    assert lib.nsdg_rb_bbm_run(None, None, 0, 0, C.byref(out)) == -1 and out.value == -7
    assert lib.nsdg_rb_bbm_stats(None, None, C.byref(st), 0) == -1
    assert lib.nsdg_rb_bbm_destroy(None) == 0


def test_the_binding_has_the_members_of_the_header_in_order():
    src = open(os.path.join(ROOT, "include", "nsdg.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} nsdg_rb_bbm_desc;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [re.sub(r"[\s*]|\[\d+\]", "", n) for n in re.sub(r"^\s*(const\s+)?(int32_t|double)", "", decl.strip()).split(",") if n.strip()]
    assert names == [n for n, _ in abi.RbBbmDesc._fields_]
    # 12 int32, 5 ping-pong pairs, packed + 3 Gauss arrays, D[2] and D_work: no padding
    assert C.sizeof(abi.RbBbmDesc) == 12 * 4 + (5 * 2 + 4 + 2 + 1) * 8


def test_the_driver_refuses_graphs_and_ops_without_the_native_calls():
    bt = synthetic.BoxTest(8, 8)
    mk = lambda **kw: rowblock.DynamicsCore(R.make_ops(), rowblock.RowBlock(8, 8), bt.hx, bt.hy, 8.0, 4, torch.device("cpu"), rheology="bbm", **kw)
    with pytest.raises(ValueError, match="use_graph"):
        mk(use_graph=True)
    with pytest.raises(ValueError, match="use_graph"):
        mk(use_graph=True, native=True)
    with pytest.raises(ValueError, match="rb_bbm"):
        mk(native=True)
    assert mk().native is False


def test_the_odd_count_keeps_the_margins_of_the_reference_run():
    """tests/test_gpu_bbm_native.py runs section 6 of tests/test_gpu_bbm.py with nsub = 7 as well, sub-steps of 2.5 / 7 s where that section
    used 0.25 s: the reference run must stay clear of the scheme's two discontinuities just the same (assert_driver_margins, for 7)"""
    import numpy as np

    import test_gpu_bbm as G

    nsub, record, f = 7, [], G.driver_fields()
    core = rowblock.DynamicsCore(R.make_ops(record=record), rowblock.RowBlock(G.DNX, G.DNY), G.HX, G.HY, G.DDT, nsub, torch.device("cpu"), rheology="bbm")
    core.load_global(f["H"], f["A"], f["uo"], f["vo"], f["ua"], f["va"])
    core.load_state_dict(G.start_state(f))
    for _ in range(G.DNSTEPS):
        core.step()
    assert len(record) == G.DNSTEPS * nsub
    N = R.bbm_par()["compr_strength"]
    worst = min(float(np.min(np.abs(d["sn_old"])) / d["smax"]) for d in record)
    shares = [float(np.mean(d["failing"])) for d in record]
    print("nsub %d: min |sigma_n| / max |sigma| %.3e; failing share first %.3f, max %.3f, last %.3f" % (nsub, worst, shares[0], max(shares), shares[-1]))
    assert worst >= 1e-6 and all(np.min(d["sn_new"]) > -0.5 * N for d in record)
    assert all(0.1 <= x <= 0.9 for x in shares)

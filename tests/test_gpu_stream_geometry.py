"""The streaming kernels past one pass of their grid (csrc/history.hip, csrc/tracer.hip): history_accumulate_kernel<false> and <true>,
history_row_totals_kernel, tracer_weight_kernel<1 / 3 / 6> and tracer_recover_kernel at the smallest shapes that turn their grid-stride
loop round, against the references their small-shape tests use and under the same rules -- tests/test_gpu_history.py,
tests/test_gpu_history_stats.py and tests/test_gpu_column_transport.py, where a launch is at most four workgroups or a fifth of a pass.
Shapes, inputs and comparisons are those of tests/stream_geometry_cases.py; tests/test_stream_geometry_cpu.py shows that they fail on what
a broken loop would leave behind.

The grid is min(ceil(n / 256), 8 CUs) workgroups of 256 lanes (of four rows for the row totals) and the CU count is the device's own
(ctx.num_cus()), so the shapes follow the device: the owned rows [3, ny - 2) hold 1.25 passes.  Every family runs with row0 = 0 into
arrays of all ny rows, where the rows outside the range must stay NaN, and with row0 = j0 into an accumulator of exactly the owned rows
between guards of NaN, as both hosts call it (the statistics with seven spare rows per plane on top: a plane_stride larger than the
owned rows).  Every comparison is made over the whole range, on the first trip alone and on the later trips alone.

On an MI355X (256 CUs):
  element kernels   130 x 5047, rows [3, 5045): 655 460 elements, 2048 workgroups, 524 288 elements a trip, 2 trips, 131 172 in the last
                    (512 whole workgroups and 100 lanes of one more)
  row totals         65 x 10246, rows [3, 10244): 10 241 rows, 2048 workgroups, 8192 rows a trip, 2 trips, 2049 rows in the last
Largest observed error / bound of the rounded comparisons there (printed by the tests; every other comparison is bit for bit):
  sums         speed 0.075, shear 0.034 (all twelve fields, and alone); divergence and sigma_s came out equal to the reference
  statistics   speed 0.075, speed:max 0.037, speed:ice_mean 0.060, shear:ice_mean 0.027, shear:min 0.017
  row totals   drift 0.016, speed_max 0.001
the same over the whole range, on the first trip and on the later trips, with row0 = 0 and with row0 = j0 (drift: 0.008 on the later trips)."""
import numpy as np
import pytest
import torch

import history_ref as R
import history_stats_ref as S
import stream_geometry_cases as cases
import test_gpu_history as G
import test_gpu_history_stats as GS
from nextsimdg_amd import abi

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 1024  # doubles of NaN on either side of an array that is exactly what the call owns


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # a copy: the arrays of a case are read-only


def full(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def guarded(*shape):
    """(buffer, view): an array of NaN of this shape with GUARD doubles of NaN before and behind it"""
    n = int(np.prod(shape))
    buf = full(n + 2 * GUARD)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def two_trips(ctx, case, grid, what):
    """the launch of this case on this device: at least two trips, asserted from the device's own CU count"""
    cus = ctx.num_cus()
    owned = (case["j1"] - case["j0"]) * (case["nx"] if grid is cases.element_grid else 1)
    wgs, per, trips = grid(cus, owned)
    print("%s: %d CUs, %d x %d, rows [%d, %d): %d %s, %d workgroups, %d a trip, %d trips, %d in the last" % (
        what, cus, case["nx"], case["ny"], case["j0"], case["j1"], owned, "elements" if grid is cases.element_grid else "rows", wgs, per, trips,
        owned - (trips - 1) * per))
    assert trips >= 2 and wgs == 8 * cus and int(case["trip"].max()) == trips - 1


@pytest.fixture(scope="module")
def history(ctx):
    """the case of the plain sums and the statistics, its states on the device"""
    case = cases.history_case(ctx.num_cus())
    return case, [G.to_device(st) for st in case["states"]]


# ------------------------------------------------------------------------------------------------ nsdg_history_accumulate
@pytest.mark.parametrize("own", [False, True], ids=["row0=0", "row0=j0"])
def test_sums_of_two_samples(ctx, history, own):
    case, states = history
    two_trips(ctx, case, cases.element_grid, "history_accumulate")
    nx, ny, j0, j1 = (case[k] for k in ("nx", "ny", "j0", "j1"))
    ctx.set_grid(nx, ny, G.HX, G.HY)
    for fields in (R.FIELDS, ("shear",)):
        buf, acc = guarded(len(fields), j1 - j0, nx) if own else (None, full(len(fields), ny, nx))
        for k, d in enumerate(states):
            ctx.history_accumulate(j0, j1, fields, d, k == 0, j0 if own else 0, acc)
        torch.cuda.synchronize()
        got = acc.cpu().numpy()
        if own:
            assert guards_intact(buf)
        else:
            assert np.all(np.isnan(got[:, :j0])) and np.all(np.isnan(got[:, j1:]))
            got = got[:, j0:j1]
        want = cases.history_want(case, fields)
        for mode in cases.MODES:
            cases.compare_history(case, fields, got, want, mode, "%d fields, row0 = %d" % (len(fields), j0 if own else 0))


# ------------------------------------------------------------------------------------------------ nsdg_history_accumulate_stats
@pytest.mark.parametrize("own", [False, True], ids=["row0=0", "row0=j0"])
def test_statistics_of_two_samples(ctx, history, own):
    case, states = history
    two_trips(ctx, case, cases.element_grid, "history_accumulate_stats")
    nx, ny, j0, j1 = (case[k] for k in ("nx", "ny", "j0", "j1"))
    ctx.set_grid(nx, ny, G.HX, G.HY)
    pairs = [S.parse(e) for e in GS.PAIRS]
    spare = 7  # rows of a plane behind the owned ones: plane_stride = (j1 - j0 + spare) nx
    if own:
        (buf, acc), (wbuf, wacc) = guarded(len(pairs), j1 - j0 + spare, nx), guarded(j1 - j0 + spare, nx)
    else:
        acc, wacc = full(len(pairs), ny, nx), full(ny, nx)
    for k, d in enumerate(states):
        ctx.history_accumulate_stats(j0, j1, pairs, d, k == 0, j0 if own else 0, acc, wacc)
    torch.cuda.synchronize()
    got, wgot = acc.cpu().numpy(), wacc.cpu().numpy()
    if own:
        assert guards_intact(buf) and guards_intact(wbuf)
        assert np.all(np.isnan(got[:, j1 - j0:])) and np.all(np.isnan(wgot[j1 - j0:]))
        got, wgot = got[:, :j1 - j0], wgot[:j1 - j0]
    else:
        assert np.all(np.isnan(got[:, :j0])) and np.all(np.isnan(got[:, j1:])) and np.all(np.isnan(wgot[:j0])) and np.all(np.isnan(wgot[j1:]))
        got, wgot = got[:, j0:j1], wgot[j0:j1]
    want, wwant = cases.stats_want(case)
    for mode in cases.MODES:
        cases.compare_stats(case, got, wgot, want, wwant, mode, "row0 = %d" % (j0 if own else 0))


# ------------------------------------------------------------------------------------------------ nsdg_history_row_totals
@pytest.mark.parametrize("own", [False, True], ids=["row0=0", "row0=j0"])
def test_row_totals(ctx, own):
    case = cases.series_case(ctx.num_cus())
    two_trips(ctx, case, cases.row_grid, "history_row_totals")
    nx, ny, j0, j1 = (case[k] for k in ("nx", "ny", "j0", "j1"))
    ctx.set_grid(nx, ny, G.HX, G.HY)
    d = {k: dev(case["state"][k]) for k in ("H", "A", "u", "v", "hsnow")}
    buf, out = guarded(7, j1 - j0) if own else (None, full(7, ny))
    ctx.history_row_totals(j0, j1, S.QUANTITIES, d, cases.EXTENT, j0 if own else 0, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if own:
        assert guards_intact(buf)
    else:
        assert np.all(np.isnan(got[:, :j0])) and np.all(np.isnan(got[:, j1:]))
        got = got[:, j0:j1]
    for mode in cases.MODES:
        cases.compare_series(case, got, mode, "row0 = %d" % (j0 if own else 0))


# ------------------------------------------------------------------------------------------------ nsdg_tracer_weight, nsdg_tracer_recover
@pytest.mark.parametrize("order", [0, 1, 2])
def test_tracer_weight(ctx, order):
    case = cases.weight_case(ctx.num_cus(), order)
    two_trips(ctx, case, cases.element_grid, "tracer_weight, order %d" % order)
    nx, ny, j0, j1 = (case[k] for k in ("nx", "ny", "j0", "j1"))
    ctx.set_grid(nx, ny, 250.0, 250.0)
    buf, Q = guarded(*case["Q0"].shape)  # all ny rows: the rows outside [j0, j1) keep what Q held
    Q.copy_(dev(case["Q0"]))
    ctx.tracer_weight(order, j0, j1, dev(case["H"]), dev(case["T"]), Q)
    torch.cuda.synchronize()
    assert guards_intact(buf)
    got = Q.cpu().numpy()
    for mode in cases.MODES:
        cases.compare_tracer(case, got, case["want"], mode, "weight, order %d" % order)


def test_tracer_recover(ctx):
    case = cases.recover_case(ctx.num_cus())
    two_trips(ctx, case, cases.element_grid, "tracer_recover")
    nx, ny, j0, j1 = (case[k] for k in ("nx", "ny", "j0", "j1"))
    ctx.set_grid(nx, ny, 250.0, 250.0)
    H, A, Q = dev(case["H"]), dev(case["A"]), dev(case["Q"])
    for (mc, mt), want in zip(cases.RECOVER_PARAMS, case["want"]):
        buf, T = guarded(ny, nx)
        T.copy_(dev(case["T"]))
        ctx.tracer_recover(2, j0, j1, H, A, Q, mc, mt, T)
        torch.cuda.synchronize()
        assert guards_intact(buf)
        got = T.cpu().numpy()
        for mode in cases.MODES:
            cases.compare_tracer(case, got, want, mode, "recover, min_conc %g, min_thick %g" % (mc, mt))

"""History statistics and series without a GPU (include/nsdg.h "history output"): the numpy statement
(tests/history_stats_ref.py) held to known answers -- the normative row order is exact on integers and is NOT the order of np.sum or of a
sequential sum --, DynamicsCore.merge_series over any split of the rows, the driver's "name:stat" entries and series= on the CPU stand-in
with everything they refuse, and the host-only calls of the C ABI."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import history_ref as R  # noqa: E402
import history_stats_ref as S  # noqa: E402
from nextsimdg_amd import abi, build, rowblock, synthetic  # noqa: E402

NX, NY, NSUB = 20, 9, 3


# ------------------------------------------------------------------------------------------------ a. the reference
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 257])
def test_the_row_reduction_of_small_integers_is_the_exact_sum(n):
    x = np.random.default_rng(n).integers(-1000, 1000, n).astype(np.float64)
    assert S.reduce_row(x) == float(np.sum(x.astype(np.int64)))
    assert S.reduce_row(x, S.op_max) == x.max()
    assert S.reduce_row(np.zeros(0)) == 0.0 and S.reduce_row(np.zeros(0), S.op_max) == -np.inf


def test_the_normative_order_is_neither_numpys_nor_sequential():
    """the input the GPU tests reuse: a kernel that adds in another order gives other bits"""
    x = S.many_magnitudes(257)
    got = S.reduce_row(x)
    assert got != np.sum(x) and got != np.add.accumulate(x)[-1]
    assert abs(got - np.sum(x)) <= 257 * S.EPS * np.sum(x)  # and still the sum


def test_the_maximum_keeps_a_nan_wherever_it_sits():
    for at in (0, 5, 64, 129):
        x = np.arange(130, dtype=np.float64)
        x[at] = np.nan
        with np.errstate(invalid="ignore"):
            assert np.isnan(S.reduce_row(x, S.op_max)) and np.isnan(S.reduce_row(x))


def test_row_terms():
    A = np.array([[-0.5, 0.1, 0.15, 0.7, 1.5]])
    H = np.array([[-1.0, 0.0, 2.0, 3.0, 0.5]])
    u = np.zeros((3, 11))
    v = np.zeros((3, 11))
    u[1, 1::2], v[1, 1::2] = 3.0, 4.0
    src = dict(H=H, A=A, u=u, v=v, hsnow=-H)
    want = {"area": [0, 0.1, 0.15, 0.7, 1], "extent": [0, 0, 1, 1, 1], "volume": [0, 0, 2, 3, 0.5], "snow_volume": [1, 0, 0, 0, 0],
            "drift": [0, 0.5, 0.75, 3.5, 5], "speed_max": [5] * 5, "hice_max": H[0]}
    for name in S.QUANTITIES:
        assert np.array_equal(S.row_terms(name, 1.0, 1.0, 0.15, **src)[0], np.array(want[name], dtype=np.float64)), name
    tot = S.row_totals(S.QUANTITIES, 1.0, 1.0, 0.15, **src)
    assert tot.shape == (7, 1) and tot[1, 0] == 3.0 and tot[5, 0] == 5.0 and tot[6, 0] == 3.0


def stat_case(nx=7, ny=3, nsamples=3, seed=11):
    rng = np.random.default_rng(seed)
    states = []
    for _ in range(nsamples):
        st = {"H": rng.standard_normal((6, ny, nx)), "A": rng.standard_normal((6, ny, nx))}
        st["A"][0, 1, 2] = -1.0  # never any ice here
        states.append(st)
    return states


def test_ice_mean_is_nan_exactly_where_the_window_saw_no_ice():
    states = stat_case()
    pairs = ("hice:mean", "hice:ice_mean", "cice:min", "cice:max")
    names, stats = zip(*[S.parse(e) for e in pairs])
    weights = np.stack([S.weight(st["A"]) for st in states])
    no_ice = np.all(weights <= 0, axis=0)
    assert no_ice[1, 2] and not no_ice.all()  # the reference first: the fixed element has no ice, others do
    acc, wacc = np.full((4, 3, 7), np.nan), np.full((3, 7), np.nan)
    for k, st in enumerate(states):
        S.accumulate_stats(acc, wacc, R.samples(names, 1.0, 1.0, **st), S.weight(st["A"]), stats, 0, 3, k == 0)
    out = S.finalise(acc, wacc, stats, len(states))
    assert np.array_equal(np.isnan(out[1]), no_ice) and not np.isnan(out[[0, 2, 3]]).any()
    H = np.stack([st["H"][0] for st in states])
    A = np.stack([st["A"][0] for st in states])
    assert np.array_equal(out[0], (H[0] + H[1] + H[2]) / 3)
    assert np.array_equal(out[2], A.min(axis=0)) and np.array_equal(out[3], A.max(axis=0))
    iced = ~no_ice
    assert np.allclose(out[1][iced], np.sum(weights * H, axis=0)[iced] / np.sum(weights, axis=0)[iced], rtol=1e-13)


def test_a_nan_sample_is_sticky_in_the_extremes():
    acc = np.full((2, 1, 3), np.nan)
    stats = ("min", "max")
    for k, row in enumerate(([1.0, 2.0, 3.0], [np.nan, 5.0, 0.0], [0.0, 9.0, -1.0])):
        x = np.array([[row], [row]])
        S.accumulate_stats(acc, None, x, None, stats, 0, 1, k == 0)
    assert np.isnan(acc[:, 0, 0]).all() and np.array_equal(acc[:, 0, 1:], [[2.0, -1.0], [9.0, 3.0]])


# ------------------------------------------------------------------------------------------------ b. merge_series
def test_merge_series_of_any_split_of_the_rows_is_bit_identical():
    rng = np.random.default_rng(5)
    count, rows = 4, 9
    whole = {"rows": (0, rows), "count": count}
    for name in ("area", "extent", "volume", "drift"):
        whole[name] = 10.0 ** rng.uniform(-8, 8, (count, rows))
    whole["speed_max"] = rng.random((count, rows))
    hx, hy = 1300.0, 700.0
    one = rowblock.DynamicsCore.merge_series([whole], hx, hy)
    assert one["count"] == count and one["rows"] == (0, rows)
    for k in range(count):  # the rows one after the other, in row order
        t = 0.0
        for r in range(rows):
            t = t + whole["volume"][k, r]
        assert one["volume"][k] == t * (hx * hy)
    assert np.any(one["volume"] != np.sum(whole["volume"], axis=1) * (hx * hy))  # pairwise numpy is another order
    assert np.array_equal(one["speed_max"], whole["speed_max"].max(axis=1))
    assert np.array_equal(one["drift"], np.add.accumulate(whole["drift"], axis=1)[:, -1] / np.add.accumulate(whole["area"], axis=1)[:, -1])
    for ways in (3, 9):
        step = rows // ways
        parts = [{k: (v[:, r:r + step] if isinstance(v, np.ndarray) else v) for k, v in whole.items()} for r in range(0, rows, step)]
        for p, r in zip(parts, range(0, rows, step)):
            p["rows"] = (r, r + step)
        got = rowblock.DynamicsCore.merge_series(parts[::-1], hx, hy)
        for name in ("area", "extent", "volume", "drift", "speed_max"):
            assert np.array_equal(got[name], one[name]), (ways, name)
    nothing = dict(whole, area=np.zeros((count, rows)))
    assert np.isnan(rowblock.DynamicsCore.merge_series([nothing], hx, hy)["drift"]).all()
    with pytest.raises(ValueError, match="do not join"):
        rowblock.DynamicsCore.merge_series([{"rows": (0, 2), "count": 1, "area": np.zeros((1, 2))},
                                            {"rows": (3, 4), "count": 1, "area": np.zeros((1, 1))}], hx, hy)


# ------------------------------------------------------------------------------------------------ c. the driver on the CPU stand-in
def make_core(history=None, ops=None, coupled=False, **kw):
    bt = synthetic.BoxTest(NX, NY)
    H, A = bt.dg_fields()
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    cls = rowblock.CoupledCore if coupled else rowblock.DynamicsCore
    ops = S.StatsOps(alpha=200.0, beta=200.0) if ops is None else ops
    core = cls(ops, rowblock.RowBlock(NX, NY), bt.hx, bt.hy, 120.0, NSUB, torch.device("cpu"), history=history, **kw)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    return core, bt


class Recording(S.StatsOps):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def history_accumulate(self, *a):
        self.calls.append("history_accumulate")
        super().history_accumulate(*a)

    def history_accumulate_stats(self, *a):
        self.calls.append("history_accumulate_stats")
        super().history_accumulate_stats(*a)

    def history_row_totals(self, *a):
        self.calls.append("history_row_totals")
        super().history_row_totals(*a)


def test_bare_names_take_the_plain_call_and_need_nothing_new():
    ops = Recording(alpha=200.0, beta=200.0)
    core, _ = make_core(("hice", "speed"), ops=ops)
    core.step()
    assert ops.calls == ["history_accumulate"] and core._history.with_stats is False and core._history.wacc is None and core.series is None
    assert core._series is None
    assert sorted(core.history_read()) == ["count", "hice", "rows", "speed"]
    core, _ = make_core(("hice",), ops=R.HistoryOps(alpha=200.0, beta=200.0))  # a test double without the new methods keeps working
    core.step()
    assert core.history_read()["count"] == 1


def test_stats_and_series_through_the_driver():
    ops = Recording(alpha=200.0, beta=200.0)
    entries = ("hice", "speed:ice_mean", "hice:max", "hice:min", "cice:mean")
    series = ("area", "extent", "volume", "drift", "speed_max", "hice_max")
    core, bt = make_core(entries, ops=ops, series=series, series_capacity=2)
    acc, wacc = np.full((5, NY, NX), np.nan), np.full((NY, NX), np.nan)
    names, stats = zip(*[S.parse(e) for e in entries])
    want_rows = []
    for k in range(2):
        core.step()
        src = dict(H=core.H.numpy(), A=core.A.numpy(), u=core.u.numpy(), v=core.v.numpy())
        S.accumulate_stats(acc, wacc, R.samples(names, bt.hx, bt.hy, **src), S.weight(src["A"]), stats, 0, NY, k == 0)
        want_rows.append(S.row_totals(series, bt.hx, bt.hy, 0.15, **src))
    assert ops.calls == ["history_row_totals", "history_accumulate_stats"] * 2
    with pytest.raises(ValueError, match="series buffer is full"):
        core.step()
    with pytest.raises(ValueError, match="series buffer is full"):
        core.advance(120.0, substeps=2)
    rec = core.history_read()
    want = S.finalise(acc, wacc, stats, 2)
    assert sorted(k for k in rec if k not in ("rows", "count")) == sorted(entries)
    for k, e in enumerate(entries):
        assert np.array_equal(rec[e], want[k], equal_nan=True), e
    assert np.array_equal(rec["hice:max"], np.maximum(rec["hice:max"], rec["hice:min"]))
    ser = core.series_read()
    assert ser["count"] == 2 and ser["rows"] == (0, NY) and core.series_read()["count"] == 0
    for k, name in enumerate(series):
        assert ser[name].shape == (2, NY) and np.array_equal(ser[name], np.stack([w[k] for w in want_rows])), name
    tot = rowblock.DynamicsCore.merge_series([ser], bt.hx, bt.hy)
    assert np.all(tot["extent"] >= tot["area"]) and np.all(tot["area"] > 0) and np.all(tot["volume"] > 0)
    assert np.all(tot["drift"] <= tot["speed_max"]) and np.all(tot["drift"] >= 0)
    assert np.all(tot["extent"] == np.round(tot["extent"] / (bt.hx * bt.hy)) * (bt.hx * bt.hy))  # whole cells
    core.step()  # the read made room
    assert core.series_read(reset=False)["count"] == 1


def test_construction_refuses_what_it_cannot_do():
    plain = lambda: R.HistoryOps(alpha=200.0, beta=200.0)
    with pytest.raises(ValueError, match="unknown history statistic in 'hice:median'"):
        make_core(("hice", "hice:median"))
    with pytest.raises(ValueError, match="unknown history field 'thickness'"):
        make_core(("thickness:max",))
    with pytest.raises(ValueError, match="'hice:max' is listed twice"):
        make_core(("hice:max", "u", "hice:max"))
    with pytest.raises(ValueError, match="listed twice"):
        make_core(("hice", "hice:mean"))  # the bare name IS the mean
    make_core(("hice", "hice:max", "hice:min", "hice:ice_mean"))  # one field under several statistics is fine
    with pytest.raises(ValueError, match="HistoryOps has no history_accumulate_stats"):
        make_core(("hice:max",), ops=plain())
    with pytest.raises(ValueError, match="HistoryOps has no history_row_totals"):
        make_core(("hice",), ops=plain(), series=("area",))
    with pytest.raises(ValueError, match="'hsnow'.*needs a CoupledCore"):
        make_core(("hsnow:max",))
    with pytest.raises(ValueError, match="'damage' needs rheology='bbm'"):
        make_core(("damage:max",))

    class NoConcentration(rowblock.DynamicsCore):
        TRANSPORTED = ("H",)

    bt = synthetic.BoxTest(NX, NY)
    with pytest.raises(ValueError, match="'speed:ice_mean' weights by the concentration: this core has no A"):
        NoConcentration(S.StatsOps(alpha=200.0, beta=200.0), rowblock.RowBlock(NX, NY), bt.hx, bt.hy, 120.0, NSUB, torch.device("cpu"),
                        history=("speed:ice_mean",))
    with pytest.raises(ValueError, match="unknown series quantity 'mass'"):
        make_core(series=("area", "mass"))
    with pytest.raises(ValueError, match="'area' is listed twice"):
        make_core(series=("area", "area"))
    with pytest.raises(ValueError, match="'drift'.*needs 'area'"):
        make_core(series=("drift", "volume"))
    with pytest.raises(ValueError, match="'snow_volume'.*needs a CoupledCore"):
        make_core(series=("snow_volume",))
    with pytest.raises(ValueError, match="at least one quantity"):
        make_core(series=())
    with pytest.raises(ValueError, match="series_capacity"):
        make_core(series=("area",), series_capacity=0)
    with pytest.raises(ValueError, match="extent_conc must be finite"):
        make_core(series=("area",), extent_conc=float("nan"))
    core, _ = make_core()
    with pytest.raises(ValueError, match="series="):
        core.series_read()


# ------------------------------------------------------------------------------------------------ d. the C ABI on the host
def test_stat_and_series_names_agree_with_the_binding():
    build.build_lib(verbose=False)
    lib = abi.load_library()
    assert abi.HISTORY_STATS == S.STATS and abi.SERIES_QUANTITIES == S.QUANTITIES and set(abi.SERIES_SOURCES) == set(S.QUANTITIES)
    for k, name in enumerate(S.STATS):
        assert lib.nsdg_history_stat_name(k) == name.encode() and lib.nsdg_history_stat_id(name.encode()) == k
    for k, name in enumerate(S.QUANTITIES):
        assert lib.nsdg_history_series_name(k) == name.encode() and lib.nsdg_history_series_id(name.encode()) == k
    assert lib.nsdg_history_stat_name(4) is None and lib.nsdg_history_stat_name(-1) is None and lib.nsdg_history_series_name(7) is None
    assert lib.nsdg_history_stat_id(b"median") == -1 and lib.nsdg_history_stat_id(None) == -1
    assert lib.nsdg_history_series_id(b"mass") == -1 and lib.nsdg_history_series_id(None) == -1
    # no context: an argument error, never a crash
    assert lib.nsdg_history_accumulate_stats(None, 0, 0, 1, None, None, None, 1, 0, 0, None, None) == -1
    assert lib.nsdg_history_row_totals(None, 0, 0, 1, None, None, 0.15, 0, 0, None) == -1
    assert lib.nsdg_abi_version() == 6 and lib.nsdg_history_field_name(12) is None


# ------------------------------------------------------------------------------------------------ e. the C++ host
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    import subprocess

    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_output_stats_tests_program(host_build, tmp_path):
    """host/test/output_stats_tests.cpp: the field:stat entries and the series keys with their refusals, the dataset names, the window
    per statistic, the series lines written and read back"""
    import subprocess

    p = subprocess.run([os.path.join(host_build, "output_stats_tests"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert "output stats tests:" in out and " 0 failures" in out, out


@pytest.mark.parametrize("step,args,env,why", [
    ("DynamicsStep", ["--model.output_period=240", "--model.output_file=ice.nsdg", "--model.output_fields=hice,hice:median"], {}, "unknown statistic"),
    ("DynamicsStep", ["--model.output_period=240", "--model.output_file=ice.nsdg", "--model.output_fields=hice:max", "--model.output_kind=snapshot"],
     {}, "names a statistic of a window"),
    ("DynamicsStep", ["--model.series_file=totals.txt", "--model.series_fields=drift"], {}, "it needs \"area\""),
    ("DynamicsStep", ["--model.series_file=totals.txt", "--model.series_fields=snow_volume"], {}, "needs dynamics.thermodynamics"),
    ("DynamicsStep", ["--model.series_file=totals.txt"], {"WORLD_SIZE": "2", "RANK": "0"}, "there is no gather"),
    ("HipStep", ["--model.series_file=totals.txt"], {}, "Nextsim::HipStep writes no time series"),
])
def test_host_refuses_the_new_keys_before_any_device(host_build, tmp_path, step, args, env, why):
    import subprocess

    tmp = str(tmp_path)
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::%s\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 240\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n" % (step, os.path.join(tmp, "x.nsdg")))
    p = subprocess.run([os.path.join(host_build, "nextsim_amd"), "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=120, cwd=tmp, env=dict(os.environ, **env))
    out = p.stdout.decode()
    assert p.returncode != 0 and why in out and "no HIP device" not in out, out
    assert not [n for n in os.listdir(tmp) if n.startswith("ice.") or n.startswith("totals")]

"""History statistics and row totals on the device (csrc/history.hip; include/nsdg.h "history output"):
nsdg_history_accumulate_stats and nsdg_history_row_totals against their numpy statement (tests/history_stats_ref.py), their row ranges,
guards and checks, and the Python driver's "name:stat" entries and series=.

Shapes: those of tests/test_gpu_history.py (nx = 63, 64, 65 around the seam of the 64-element stress tiles and of the 64 lanes of a row's
wave, 130 two folds per lane and a remainder, 1 the smallest row; ny = 1 and 3: one row, and fewer rows than the four of a workgroup), and
for the row totals nx = 257: five folds in lane 0, four in the others.  What is a source value, clamped, compared or (a + b) / 2, must
match bit for bit, the weighted products included -- the product is rounded in a statement of its own, so numpy reproduces it; what goes
through a square root or a strain rate matches within n_samples * 16 * 2^-53 * scale (history_ref.rounding_scale), with 16 + 4 for a
weighted sample (history_stats_ref.WEIGHTED_FACTOR: the derivation)."""
import os
import sys
import threading

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
import test_gpu_history as G  # noqa: E402  (its states, shapes and driver set-up: the plain means are tested there)
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
HX, HY, NSAMPLES, ALL = G.HX, G.HY, G.NSAMPLES, G.ALL
I32 = abi.I32
NAN = float("nan")
# one field under mean, min and max, three weighted fields of which two are rounded, and the extremes of exact and of rounded fields
PAIRS = ("hice", "hice:min", "hice:max", "hice:ice_mean", "speed:ice_mean", "shear:ice_mean", "sigma_n", "sigma_n:min", "sigma_n:max",
         "sigma_n:ice_mean", "speed", "speed:max", "shear:min", "u:ice_mean", "damage:max", "tice:min")
EXTENT = 0.15


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def split(entries):
    names, stats = zip(*[S.parse(e) for e in entries])
    return names, stats


def full(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def reference_stats(states, ref, entries):
    """(acc, wacc) of the normative update over the samples of G.case"""
    names, stats = split(entries)
    idx = [ALL.index(n) for n in names]
    acc, wacc = np.full((len(entries),) + ref.shape[2:], np.nan), np.full(ref.shape[2:], np.nan)
    for k, st in enumerate(states):
        S.accumulate_stats(acc, wacc, ref[k][idx], S.weight(st["A"]), stats, 0, ref.shape[2], k == 0)
    return acc, wacc


def compare(got, want, entries, scale, nsamples, what):
    for k, e in enumerate(entries):
        name, stat = S.parse(e)
        if name in R.EXACT_FIELDS:
            assert np.array_equal(got[k], want[k], equal_nan=True), (what, e, float(np.nanmax(np.abs(got[k] - want[k]))))
        else:
            factor = S.WEIGHTED_FACTOR if stat == "ice_mean" else S.SAMPLE_FACTOR
            bound = nsamples * factor * R.EPS * scale[name]
            err = float(np.max(np.abs(got[k] - want[k])))
            print("%s %-16s largest error %.3e, bound %.3e (%.3f of it)" % (what, e, err, bound, err / bound))
            assert err <= bound, (what, e, err, bound)


def device_stats(ctx, nx, ny, states, entries, ranges=None, row0=0):
    ctx.set_grid(nx, ny, HX, HY)
    acc, wacc = full(len(entries), ny - row0, nx), full(ny - row0, nx)  # the first sample stores
    pairs = [S.parse(e) for e in entries]
    for k, st in enumerate(states):
        d = G.to_device(st)
        for (j0, j1) in ranges or [(0, ny)]:
            ctx.history_accumulate_stats(j0, j1, pairs, d, k == 0, row0, acc, wacc)
    torch.cuda.synchronize()
    return acc, wacc


# ------------------------------------------------------------------------------------------------ a. the statistics against the reference
@pytest.mark.parametrize("ny", [1, 3])
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130])
def test_three_samples_of_every_statistic_match_the_reference(ctx, nx, ny):
    states, ref, scale = G.case(nx, ny)
    acc, wacc = device_stats(ctx, nx, ny, states, PAIRS)
    want, wwant = reference_stats(states, ref, PAIRS)
    A = np.stack([st["A"][0] for st in states])
    if nx * ny >= 63:
        assert (A < 0).any() and (A > 1).any()  # both clamps act
    assert np.array_equal(wacc.cpu().numpy(), wwant)
    compare(acc.cpu().numpy(), want, PAIRS, scale, NSAMPLES, "%dx%d:" % (nx, ny))


def test_a_list_of_means_equals_the_plain_call_bitwise(ctx):
    nx, ny = 130, 3
    states, _, _ = G.case(nx, ny)
    plain = G.device_sum(ctx, nx, ny, states, ALL)
    acc, wacc = device_stats(ctx, nx, ny, states, tuple(n + ":mean" for n in ALL))
    assert not bool(torch.isnan(plain).any()) and torch.equal(acc, plain)
    assert bool(torch.isnan(wacc).all())  # no weighted pair: the weight plane is not touched
    ctx.history_accumulate_stats(0, ny, [("hice", "mean"), ("speed", "max")], G.to_device(states[0]), True, 0, acc[:2], None)  # and may be NULL
    torch.cuda.synchronize()


def test_a_nan_sample_is_sticky_in_the_extremes_and_the_sums(ctx):
    nx, ny = 65, 3
    states, ref, _ = G.case(nx, ny)
    states = [dict(st) for st in states]
    states[1] = dict(states[1], H=states[1]["H"].copy(), u=states[1]["u"].copy())
    states[1]["H"][0, 1, 7] = np.nan  # the second sample of element (1, 7), and of the speed of element (2, 64)
    states[1]["u"][2 * 2 + 1, 2 * 64 + 1] = np.nan
    entries = ("hice:min", "hice:max", "hice", "speed:min", "speed:max", "hice:ice_mean")
    acc, _ = device_stats(ctx, nx, ny, states, entries)
    got = acc.cpu().numpy()
    nan = np.isnan(got)
    hit = np.zeros((ny, nx), dtype=bool)
    hit[1, 7] = True
    for k in (0, 1, 2, 5):
        assert np.array_equal(nan[k], hit), entries[k]
    hit[:] = False
    hit[2, 64] = True
    for k in (3, 4):
        assert np.array_equal(nan[k], hit), entries[k]
    H = np.stack([st["H"][0] for st in G.case(nx, ny)[0]])
    keep = ~nan[0]
    assert np.array_equal(got[0][keep], H.min(axis=0)[keep]) and np.array_equal(got[1][keep], H.max(axis=0)[keep])


def test_a_row_range_between_nan_neighbours_writes_nothing_else(ctx):
    nx, ny = 65, 3
    states, ref, scale = G.case(nx, ny)
    d = G.to_device(states[0])
    pairs = [S.parse(e) for e in PAIRS]
    idx = [ALL.index(n) for n, _ in pairs]
    ctx.set_grid(nx, ny, HX, HY)
    acc, wacc = full(len(PAIRS), ny, nx), full(ny, nx)
    ctx.history_accumulate_stats(1, 2, pairs, d, True, 0, acc, wacc)
    got, wgot = acc.cpu().numpy(), wacc.cpu().numpy()
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isnan(got[:, 2])) and np.all(np.isnan(wgot[0])) and np.all(np.isnan(wgot[2]))
    want, wwant = np.full_like(got, np.nan), np.full_like(wgot, np.nan)
    S.accumulate_stats(want, wwant, ref[0][idx], S.weight(states[0]["A"]), split(PAIRS)[1], 1, 2, True)
    assert np.array_equal(wgot[1], wwant[1])
    compare(got[:, 1:2], want[:, 1:2], PAIRS, scale, 1, "row 1 stored:")
    ctx.history_accumulate_stats(0, 1, pairs, d, False, 0, acc, wacc)  # store = 0 keeps a NaN, in every statistic
    assert bool(torch.isnan(acc[:, 0]).all()) and bool(torch.isnan(wacc[0]).all())
    # planes of ONE row (row0 = 1) between guards of NaN, the weight plane as well
    guard = 4 * nx
    buf, wbuf = full(2 * guard + len(PAIRS) * nx), full(2 * guard + nx)
    own, wown = buf[guard:guard + len(PAIRS) * nx].view(len(PAIRS), 1, nx), wbuf[guard:guard + nx].view(1, nx)
    ctx.history_accumulate_stats(1, 2, pairs, d, True, 1, own, wown)
    ctx.history_accumulate_stats(1, 2, pairs, d, False, 1, own, wown)
    torch.cuda.synchronize()
    for b in (buf, wbuf):
        assert bool(torch.isnan(b[:guard]).all()) and bool(torch.isnan(b[-guard:]).all())
    S.accumulate_stats(want, wwant, ref[0][idx], S.weight(states[0]["A"]), split(PAIRS)[1], 1, 2, False)
    assert np.array_equal(wown.cpu().numpy(), wwant[1:2])
    compare(own.cpu().numpy(), want[:, 1:2], PAIRS, scale, 2, "row 1 of its own plane, twice:")
    # the row totals: one row of three, and a slot between guards
    out = full(3, ny)
    ctx.history_row_totals(1, 2, ("area", "volume", "hice_max"), d, EXTENT, 0, out)
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isnan(got[:, 2]))
    assert np.array_equal(got[:, 1], S.row_totals(("area", "volume", "hice_max"), HX, HY, EXTENT, **states[0])[:, 1])
    buf = full(2 * guard + 3)
    ctx.history_row_totals(1, 2, ("area", "volume", "hice_max"), d, EXTENT, 1, buf[guard:guard + 3].view(3, 1))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())
    assert np.array_equal(buf[guard:guard + 3].cpu().numpy(), got[:, 1])


def test_two_row_ranges_equal_one_call_bitwise(ctx):
    nx, ny = 130, 3
    states, _, _ = G.case(nx, ny)
    one, wone = device_stats(ctx, nx, ny, states, PAIRS)
    two, wtwo = device_stats(ctx, nx, ny, states, PAIRS, ranges=[(0, 1), (1, 3)])
    assert not bool(torch.isnan(one).any()) and torch.equal(one, two) and torch.equal(wone, wtwo)
    d = G.to_device(states[0])
    a, b = full(7, ny), full(7, ny)
    ctx.history_row_totals(0, ny, S.QUANTITIES, d, EXTENT, 0, a)
    ctx.history_row_totals(2, 3, S.QUANTITIES, d, EXTENT, 0, b)
    ctx.history_row_totals(0, 2, S.QUANTITIES, d, EXTENT, 0, b)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(a).any()) and torch.equal(a, b)


def test_the_calls_check_their_arguments(gpu):
    c = abi.Context(gpu)
    lib, nx, ny = c.lib, 8, 4
    st = G.to_device(G.random_state(nx, ny, np.random.default_rng(1)))
    acc = torch.full((2, ny, nx), 7.0, dtype=torch.float64, device="cuda")
    wacc = torch.full((ny, nx), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((7, ny), 7.0, dtype=torch.float64, device="cuda")
    ids = lambda *a: (I32 * len(a))(*a)
    src = lambda **drop: abi.HistorySources(*[None if n in drop else st[n].data_ptr() for n in abi.HISTORY_SOURCES])
    err = lib.nsdg_last_error

    def stats(j0, j1, n, f, s, sources, store, row0, stride, w=wacc):
        return lib.nsdg_history_accumulate_stats(c.h, j0, j1, n, f, s, abi.C.byref(sources), store, row0, stride, acc.data_ptr(),
                                                 None if w is None else w.data_ptr())

    def totals(j0, j1, n, q, sources, conc, row0, stride):
        return lib.nsdg_history_row_totals(c.h, j0, j1, n, q, abi.C.byref(sources), conc, row0, stride, out.data_ptr())

    assert stats(0, ny, 1, ids(0), ids(0), src(), 1, 0, nx * ny) == -3 and b"nsdg_grid_set" in err()  # NSDG_ERR_STATE
    assert totals(0, ny, 1, ids(0), src(), EXTENT, 0, ny) == -3 and b"nsdg_grid_set" in err()
    c.set_grid(nx, ny, HX, HY)
    # 1a: the checks of nsdg_history_accumulate ...
    for j0, j1 in ((-1, 2), (3, 2), (0, ny + 1)):
        assert stats(j0, j1, 1, ids(0), ids(0), src(), 1, 0, nx * ny) == -1, (j0, j1)
        assert totals(j0, j1, 1, ids(0), src(), EXTENT, 0, ny) == -1, (j0, j1)
    assert stats(0, ny, 0, ids(0), ids(0), src(), 1, 0, nx * ny) == -1 and stats(0, ny, 17, ids(*[0] * 17), ids(*[0] * 17), src(), 1, 0, nx * ny) == -1
    assert stats(0, ny, 1, ids(12), ids(0), src(), 1, 0, nx * ny) == -1 and b"unknown field id 12" in err()
    assert stats(0, ny, 2, ids(0, 11), ids(2, 3), src(D=1), 1, 0, nx * ny) == -1 and b"'damage'" in err()
    assert stats(1, ny, 1, ids(0), ids(0), src(), 1, 2, nx * ny) == -1 and b"row0" in err()
    assert stats(0, ny, 1, ids(0), ids(0), src(), 1, 0, nx * ny - 1) == -1 and b"plane_stride" in err()
    assert lib.nsdg_history_accumulate_stats(c.h, 0, ny, 1, ids(0), None, abi.C.byref(src()), 1, 0, nx * ny, acc.data_ptr(), None) == -1
    assert lib.nsdg_history_accumulate_stats(c.h, 0, ny, 1, None, ids(0), abi.C.byref(src()), 1, 0, nx * ny, acc.data_ptr(), None) == -1
    assert lib.nsdg_history_accumulate_stats(c.h, 0, ny, 1, ids(0), ids(0), None, 1, 0, nx * ny, acc.data_ptr(), None) == -1
    assert lib.nsdg_history_accumulate_stats(c.h, 0, ny, 1, ids(0), ids(0), abi.C.byref(src()), 1, 0, nx * ny, None, None) == -1
    # ... and its own
    assert stats(0, ny, 1, ids(0), ids(4), src(), 1, 0, nx * ny) == -1 and b"unknown stat id 4" in err()
    assert stats(0, ny, 1, ids(0), ids(-1), src(), 1, 0, nx * ny) == -1
    assert stats(0, ny, 2, ids(3, 3), ids(2, 2), src(), 1, 0, nx * ny) == -1 and b"'v:min' is listed twice" in err()
    assert stats(0, ny, 2, ids(3, 3), ids(2, 3), src(), 1, 0, nx * ny) == 0  # one field, two statistics
    assert stats(0, ny, 1, ids(4), ids(1), src(A=1), 1, 0, nx * ny) == -1 and b"'speed'" in err() and b"source A" in err()
    assert stats(0, ny, 1, ids(4), ids(1), src(), 1, 0, nx * ny, w=None) == -1 and b"'speed'" in err() and b"wacc" in err()
    assert stats(0, ny, 1, ids(4), ids(3), src(A=1, H=1), 1, 0, nx * ny, w=None) == 0  # no weighted pair: neither A nor wacc is needed
    assert stats(1, ny, 1, ids(0), ids(1), src(), 1, 1, nx * (ny - 1)) == 0
    # 1b
    assert totals(0, ny, 0, ids(0), src(), EXTENT, 0, ny) == -1 and totals(0, ny, 8, ids(*range(7), 0), src(), EXTENT, 0, ny) == -1
    assert totals(0, ny, 1, ids(7), src(), EXTENT, 0, ny) == -1 and b"unknown quantity id 7" in err()
    assert totals(0, ny, 1, ids(-1), src(), EXTENT, 0, ny) == -1
    assert totals(0, ny, 2, ids(2, 2), src(), EXTENT, 0, ny) == -1 and b"'volume' is listed twice" in err()
    for q, name, drop in ((0, "area", "A"), (1, "extent", "A"), (2, "volume", "H"), (3, "snow_volume", "hsnow"), (4, "drift", "A"),
                          (4, "drift", "u"), (5, "speed_max", "v"), (6, "hice_max", "H")):
        assert totals(0, ny, 1, ids(q), src(**{drop: 1}), EXTENT, 0, ny) == -1, name
        assert ("'%s'" % name).encode() in err() and ("source %s" % drop).encode() in err(), err()
    assert totals(0, ny, 1, ids(2), src(A=1, u=1, v=1, hsnow=1, s11=1, s12=1, s22=1, tice=1, D=1), EXTENT, 0, ny) == 0  # volume reads H alone
    for bad in (NAN, float("inf"), -float("inf")):
        assert totals(0, ny, 1, ids(1), src(), bad, 0, ny) == -1 and b"extent_conc" in err()
    assert totals(1, ny, 1, ids(0), src(), EXTENT, 2, ny) == -1 and b"row0" in err()
    assert totals(0, ny, 1, ids(0), src(), EXTENT, 0, ny - 1) == -1 and b"q_stride" in err()
    assert totals(1, ny, 7, ids(*range(7)), src(), EXTENT, 1, ny - 1) == 0
    assert lib.nsdg_history_row_totals(c.h, 0, ny, 1, None, abi.C.byref(src()), EXTENT, 0, ny, out.data_ptr()) == -1
    assert lib.nsdg_history_row_totals(c.h, 0, ny, 1, ids(0), None, EXTENT, 0, ny, out.data_ptr()) == -1
    assert lib.nsdg_history_row_totals(c.h, 0, ny, 1, ids(0), abi.C.byref(src()), EXTENT, 0, ny, None) == -1
    torch.cuda.synchronize()
    acc.fill_(7.0), wacc.fill_(7.0), out.fill_(7.0)
    assert stats(2, 2, 1, ids(0), ids(1), src(), 1, 0, nx * ny) == 0 and totals(2, 2, 1, ids(0), src(), EXTENT, 0, ny) == 0  # empty: nothing
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all()) and bool((wacc == 7.0).all()) and bool((out == 7.0).all())
    with pytest.raises(abi.NsdgError, match="unknown history statistic"):
        c.history_accumulate_stats(0, ny, [("hice", "median")], st, True, 0, acc[:1], wacc)
    with pytest.raises(abi.NsdgError, match="wacc has shape"):
        c.history_accumulate_stats(0, ny, [("hice", "ice_mean")], st, True, 0, acc[:1], wacc[:1])
    with pytest.raises(abi.NsdgError, match="unknown series quantity"):
        c.history_row_totals(0, ny, ("mass",), st, EXTENT, 0, out[:1])
    with pytest.raises(abi.NsdgError, match="out has shape"):
        c.history_row_totals(0, ny, ("area",), st, EXTENT, 0, out)
    with pytest.raises(abi.NsdgError, match="source u has"):
        c.history_row_totals(0, ny, ("speed_max",), dict(st, u=st["u"][:-1]), EXTENT, 0, out[:1])
    c.close()


# ------------------------------------------------------------------------------------------------ b. the row totals against the reference
def magnitudes_state(nx, ny):
    """a state whose rows span sixteen decades: a row total of it remembers the order of its additions (row 0 of H at nx = 257 is the
    vector tests/test_history_stats_cpu.py holds against np.sum and a sequential sum)"""
    st = G.random_state(nx, ny, np.random.default_rng(nx + ny))
    n = nx * ny
    st["H"][0] = S.many_magnitudes(n).reshape(ny, nx)
    st["hsnow"] = S.many_magnitudes(n, seed=8).reshape(ny, nx)
    st["A"][0] = 1e-8 * S.many_magnitudes(n, seed=9).reshape(ny, nx)  # in (1e-16, 1): the area and the drift weights
    st["A"][0, 0, 0] = 0.5
    for k, seed in (("u", 17), ("v", 18)):
        st[k] = 1e-8 * S.many_magnitudes(st[k].size, seed=seed).reshape(st[k].shape)
    return st


_series_cases = {}


def series_case(nx, ny):
    if (nx, ny) not in _series_cases:
        out = []
        for st in (G.random_state(nx, ny, np.random.default_rng(7000 * nx + ny)), magnitudes_state(nx, ny)):
            want = S.row_totals(S.QUANTITIES, HX, HY, EXTENT, **st)
            bound = {q: S.row_total_bound(q, HX, HY, EXTENT, **st) for q in S.QUANTITIES if q not in S.EXACT_QUANTITIES}
            want.setflags(write=False)
            out.append((st, want, bound))
        _series_cases[(nx, ny)] = out
    return _series_cases[(nx, ny)]


@pytest.mark.parametrize("ny", [1, 3])
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130, 257])
def test_row_totals_match_the_reference(ctx, nx, ny):
    ctx.set_grid(nx, ny, HX, HY)
    order = ("drift", "hice_max", "area", "snow_volume", "extent", "speed_max", "volume")  # the list's order, not the id's
    for which, (st, want, bound) in zip(("random", "magnitudes"), series_case(nx, ny)):
        d = G.to_device(st)
        out = full(7, ny)
        ctx.history_row_totals(0, ny, order, d, EXTENT, 0, out)
        got = out.cpu().numpy()
        for k, q in enumerate(order):
            w = want[S.QUANTITIES.index(q)]
            if q in S.EXACT_QUANTITIES:
                assert np.array_equal(got[k], w), (which, q, got[k], w)
            else:
                err = np.abs(got[k] - w)
                print("%dx%d %-10s %-9s largest error %.3e, bound %.3e" % (nx, ny, which, q, err.max(), bound[q][np.argmax(err)]))
                assert np.all(err <= bound[q]), (which, q, err, bound[q])
        # a strided slot of a larger buffer, and a list that reads H alone
        big = full(2, ny + 3)
        ctx.history_row_totals(0, ny, ("volume", "hice_max"), {"H": d["H"]}, EXTENT, 0, big[:, :ny])
        assert np.array_equal(big[:, :ny].cpu().numpy(), want[[2, 6]]) and bool(torch.isnan(big[:, ny:]).all())
    if nx == 257:  # the property the CPU test establishes for this vector: another order of additions gives other bits
        H0 = series_case(nx, ny)[1][0]["H"][0, 0]
        assert want[2, 0] != np.sum(H0) and want[2, 0] != np.add.accumulate(H0)[-1]


def test_a_nan_in_a_row_reaches_its_totals_and_no_other_row(ctx):
    nx, ny = 130, 3
    st = dict(series_case(nx, ny)[0][0])
    st["H"] = st["H"].copy()
    st["H"][0, 1, 129] = np.nan
    ctx.set_grid(nx, ny, HX, HY)
    out = full(7, ny)
    ctx.history_row_totals(0, ny, S.QUANTITIES, G.to_device(st), EXTENT, 0, out)
    nan = np.isnan(out.cpu().numpy())
    want = np.zeros((7, ny), dtype=bool)
    want[[2, 6], 1] = True  # volume and hice_max of row 1
    assert np.array_equal(nan, want)


# ------------------------------------------------------------------------------------------------ c. the driver
DNX, DNY, DSTEPS = G.DNX, G.DNY, G.DSTEPS
ENTRIES = ("hice", "hice:min", "hice:max", "speed:ice_mean", "shear:ice_mean", "cice:ice_mean", "sigma_s:max", "divergence:min", "u")
SERIES = ("area", "extent", "volume", "drift", "speed_max", "hice_max")


def run_steps(core, nsteps=DSTEPS):
    for _ in range(nsteps):
        core.step()
    return core.history_read(), core.series_read()


def restore(ctx):
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


@pytest.fixture(scope="module")
def one_block(ctx):
    core, bt = G.make_core(ctx, ENTRIES, series=SERIES)
    rec, ser = run_steps(core)
    core.close()
    restore(ctx)
    return rec, ser, bt


def same(a, b, keys):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_driver_record_and_series_make_sense(one_block):
    rec, ser, bt = one_block
    assert rec["count"] == DSTEPS and ser["count"] == DSTEPS and ser["rows"] == (0, DNY)
    assert sorted(k for k in rec if k not in ("rows", "count")) == sorted(ENTRIES)
    land = G.rock()
    assert np.all(rec["hice:min"] <= rec["hice"]) and np.all(rec["hice"] <= rec["hice:max"]) and np.any(rec["hice:min"] < rec["hice:max"])
    assert np.array_equal(np.isnan(rec["speed:ice_mean"]), land) and np.array_equal(np.isnan(rec["cice:ice_mean"]), land)  # no ice on the rock
    assert np.all(rec["speed:ice_mean"][~land] >= 0) and np.max(rec["speed:ice_mean"][~land]) > 1e-4
    tot = rowblock.DynamicsCore.merge_series([ser], bt.hx, bt.hy)
    cells = (DNX * DNY - land.sum()) * (bt.hx * bt.hy)  # the association of merge_series: the count times the cell
    assert np.all(tot["area"] > 0) and np.all(tot["area"] <= tot["extent"]) and np.all(tot["extent"] <= cells)
    assert np.all(tot["drift"] > 0) and np.all(tot["drift"] <= tot["speed_max"])
    assert tot["hice_max"].max() == rec["hice:max"].max()  # the largest cell mean of the window, by either road
    # a closed box and positive thicknesses: the transport moves ice and creates none
    assert np.all(ser["volume"] > 0)
    drift = np.abs(tot["volume"] - tot["volume"][0]) / tot["volume"][0]
    print("volume over %d steps: %r, relative change %r" % (DSTEPS, tot["volume"], drift))
    assert np.all(drift <= 1e-13)


def thread_world(world, nsteps=DSTEPS):
    from thread_ranks import Mailbox, ThreadExchanger

    mailbox, out = Mailbox(), {}

    def rank_main(rank):
        try:
            c = abi.Context(torch.device("cuda:0"))
            blk = rowblock.RowBlock(DNX, DNY, rank, world, 1, 1)
            core, _ = G.make_core(c, ENTRIES, rank, world, ThreadExchanger(blk, mailbox), series=SERIES)
            out[rank] = run_steps(core, nsteps)
            core.close()
            c.close()
        except BaseException as e:  # noqa: BLE001 -- wake the peers up, then re-raise in the main thread
            with mailbox.cv:
                mailbox.error = e
                mailbox.cv.notify_all()
            out[rank] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return [out[r] for r in range(world)]


def test_one_block_equals_three_blocks_bitwise(one_block):
    rec, ser, bt = one_block
    parts = thread_world(3)
    assert [p[1]["rows"] for p in parts] == [(0, 3), (3, 6), (6, 9)]
    same(rowblock.DynamicsCore.merge_history([p[0] for p in parts]), rec, ENTRIES)
    got = rowblock.DynamicsCore.merge_series([p[1] for p in parts], bt.hx, bt.hy)
    assert got["count"] == DSTEPS
    same(got, rowblock.DynamicsCore.merge_series([ser], bt.hx, bt.hy), SERIES)
    joined = {q: np.concatenate([p[1][q] for p in parts], axis=1) for q in SERIES}
    same(joined, ser, SERIES)  # and every row total by itself


def test_graphs_equal_no_graphs_under_the_native_plan(gpu, one_block):
    rec, ser, _ = one_block
    for use_graph in (False, True):
        c = abi.Context(gpu)
        core, _ = G.make_core(c, ENTRIES, variant=4, native=True, use_graph=use_graph, series=SERIES)
        assert core.per_pass == 4
        got, gser = run_steps(core)
        core.close()
        c.close()
        same(got, rec, ENTRIES)
        same(gser, ser, SERIES)


def test_windows_reset_and_a_full_buffer_is_refused(ctx):
    core, _ = G.make_core(ctx, ("hice:max", "speed:ice_mean"), series=("volume",), series_capacity=2)
    core._history.acc.fill_(NAN), core._history.wacc.fill_(NAN), core._series.buf.fill_(NAN)
    assert core.advance(120.0, substeps=2) == 2
    rec = core.history_read()
    assert rec["count"] == 1 and np.array_equal(rec["hice:max"], core.H[0].cpu().numpy())  # the first sample stores: no NaN survives
    assert not np.isnan(rec["speed:ice_mean"][~G.rock()]).any()
    core.step()
    assert core.series_read(reset=False)["count"] == 2
    with pytest.raises(ValueError, match="series buffer is full"):
        core.step()  # the third
    ser = core.series_read()
    assert ser["count"] == 2 and ser["volume"].shape == (2, DNY) and not np.isnan(ser["volume"]).any()
    core.step()
    assert core.series_read()["count"] == 1 and core.history_read()["count"] == 2
    with pytest.raises(ValueError, match="no sample"):
        core.history_read()
    core.close()
    restore(ctx)


def test_coupled_core_totals_the_snow(ctx):
    ctx.set_column_params(ctx.column_default_params())
    core, bt = G.make_core(ctx, ("hsnow:max", "hsnow:ice_mean"), cls=rowblock.CoupledCore, advect_column_state=True,
                           series=("snow_volume", "volume", "area"))
    st, fo, _ = synthetic.column_fields(DNX * DNY, 5)
    column = {k: v.reshape(DNY, DNX) for k, v in {**st, **fo}.items()}
    column["wind"] = 0.2 * column["wind"]
    core.load_column(column)
    core.step()
    want = S.row_totals(("snow_volume",), bt.hx, bt.hy, 0.15, hsnow=core.col["hsnow"].cpu().numpy())
    core.step()
    rec, ser = core.history_read(), core.series_read()
    assert np.array_equal(ser["snow_volume"][0], want[0])
    tot = rowblock.DynamicsCore.merge_series([ser], bt.hx, bt.hy)
    assert np.all(tot["snow_volume"] > 0) and np.all(tot["volume"] > 0) and np.nanmax(rec["hsnow:max"]) > 0
    core.close()
    restore(ctx)
    with pytest.raises(ValueError, match="'snow_volume'.*needs a CoupledCore"):
        G.make_core(ctx, None, series=("snow_volume",))
    restore(ctx)


def test_brittle_rheology_with_the_largest_damage(ctx):
    import test_gpu_bbm as B

    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_bbm_params(ctx.bbm_default_params())
    f = B.driver_fields()
    core = rowblock.DynamicsCore(ctx, rowblock.RowBlock(B.DNX, B.DNY), B.HX, B.HY, B.DDT, B.DNSUB, torch.device("cuda"), rheology="bbm",
                                 history=("damage:max", "damage:min", "damage"), series=("area", "drift"))
    core.load_global(f["H"], f["A"], f["uo"], f["vo"], f["ua"], f["va"])
    core.load_state_dict(B.start_state(f))
    seen = []
    for _ in range(2):
        core.step()
        seen.append(core.state_dict()["D"][0])
    rec, ser = core.history_read(), core.series_read()
    core.close()
    assert np.array_equal(rec["damage:max"], np.maximum(seen[0], seen[1])) and np.array_equal(rec["damage:min"], np.minimum(seen[0], seen[1]))
    assert np.array_equal(rec["damage"], (seen[0] + seen[1]) / 2) and 0.0 < rec["damage:min"].min() and rec["damage:max"].max() < 1.0
    assert ser["count"] == 2 and np.all(rowblock.DynamicsCore.merge_series([ser], B.HX, B.HY)["drift"] > 0)

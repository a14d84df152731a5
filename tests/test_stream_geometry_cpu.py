"""The streaming kernels past one pass of their grid, without a GPU: what tests/test_gpu_stream_geometry.py relies on, held on the
references alone (tests/stream_geometry_cases.py).  The shapes turn the grid-stride loop round for every CU count the project has met;
the vectorised row reduction is the normative one, bit for bit; and the comparisons the device test makes fail on what a launch with a
broken loop would leave behind -- the later trips left out, made one workgroup further on, or reading one workgroup further on --, for
every call, over the whole range and on the later trips, while the first trip still passes."""
import numpy as np
import pytest

import history_stats_ref as S
import stream_geometry_cases as cases

CUS = 256  # the references of the comparisons below: the shapes of an MI355X


# ------------------------------------------------------------------------------------------------ 1. the shapes
@pytest.mark.parametrize("cus", cases.CU_COUNTS)
def test_the_shapes_turn_the_loop_round(cus):
    for shape, grid, step, nx in ((cases.element_shape, cases.element_grid, cases.LANES, 130), (cases.row_shape, cases.row_grid, cases.ROWS, 65)):
        sx, ny, j0, j1 = shape(cus)
        assert sx == nx and j0 == 3 and j1 == ny - 2 and j0 >= 1 and j1 < ny
        owned = (j1 - j0) * nx if step == cases.LANES else j1 - j0
        wgs, per, trips = grid(cus, owned)
        assert wgs == 8 * cus and per == wgs * step  # the cap acts
        assert trips >= 2 and owned - per >= 0.2 * per, (owned, per)
        assert owned % step != 0  # the last workgroup is ragged
        assert nx * ny < 1000000
    assert cases.element_grid(256, 2048 * 2048) == (2048, 524288, 8) and cases.row_grid(256, 2048) == (512, 2048, 1)
    assert cases.element_grid(256, 257) == (2, 512, 1) and cases.row_grid(304, 9) == (3, 12, 1)


def test_the_trips_of_the_selections():
    nx, ny, j0, j1 = cases.element_shape(CUS)
    trip = cases.element_trips(CUS, nx, j0, j1)
    assert trip.shape == (j1 - j0, nx) and trip.reshape(-1)[524287] == 0 and trip.reshape(-1)[524288] == 1 and trip.max() == 1
    assert int(np.sum(trip == 1)) == (j1 - j0) * nx - 524288 == 131172
    nx, ny, j0, j1 = cases.row_shape(CUS)
    trip = cases.row_trips(CUS, j0, j1)
    assert trip[8191] == 0 and trip[8192] == 1 and trip.max() == 1 and int(np.sum(trip == 1)) == 2049
    for mode, n in zip(cases.MODES, (10241, 8192, 2049)):
        assert int(np.sum(cases.selection(trip, mode))) == n


# ------------------------------------------------------------------------------------------------ 2. the vectorised row reduction
def rows_to_reduce(nx):
    rng = np.random.default_rng(nx)
    x = np.stack([rng.standard_normal(nx), S.many_magnitudes(nx), S.many_magnitudes(nx, seed=9), -S.many_magnitudes(nx, seed=8),
                  rng.standard_normal(nx), rng.standard_normal(nx), rng.standard_normal(nx), np.zeros(nx), -np.zeros(nx), rng.standard_normal(nx)])
    x[4, nx // 2] = np.nan
    x[5, nx - 1] = np.inf
    x[6, 0] = -np.inf
    x[9, 0], x[9, nx - 1] = -np.inf, np.inf  # both in one row (nx > 1): the sum is a NaN
    return x


@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130, 257])
def test_reduce_rows_is_reduce_row_bit_for_bit(nx):
    x = rows_to_reduce(nx)
    for op in (S.op_sum, S.op_max):
        with np.errstate(invalid="ignore"):
            want = np.array([S.reduce_row(row, op) for row in x])
        got = S.reduce_rows(x, op)
        assert cases.same_bits(got, want), (nx, op.__name__, got, want)
        assert np.isnan(got[4]) and got[5] == np.inf and got[6] == (-np.inf if op is S.op_sum else x[6].max())
        assert op is S.op_max or nx == 1 or np.isnan(got[9])
    assert cases.same_bits(S.reduce_rows(np.zeros((2, 0))), np.zeros(2)) and np.all(S.reduce_rows(np.zeros((2, 0)), S.op_max) == -np.inf)


def test_row_totals_of_many_rows_are_the_row_totals():
    G = cases.history_tests()
    for nx in (65, 130):
        st = G.random_state(nx, 5, np.random.default_rng(nx))
        st["H"][0, 2] = S.many_magnitudes(nx)
        st["A"][0, 3, 7] = np.nan
        with np.errstate(invalid="ignore"):
            want = S.row_totals(S.QUANTITIES, G.HX, G.HY, cases.EXTENT, **st)
        assert cases.same_bits(S.row_totals_of_many_rows(S.QUANTITIES, G.HX, G.HY, cases.EXTENT, **st), want)


# ------------------------------------------------------------------------------------------------ 3. the inputs can tell
def tells(compare, want, untouched, trip, step):
    """compare(got, mode) passes on the reference itself; on each wrong reference it fails over the whole range and on the later trips
    and passes on the first trip"""
    for mode in cases.MODES:
        compare(want, mode)
    for kind, name in enumerate(cases.WRONG):
        bad = cases.wrong(kind, want, untouched, trip, step)
        compare(bad, cases.MODES[1])
        for mode in (cases.MODES[0], cases.MODES[2]):
            with pytest.raises(AssertionError):
                compare(bad, mode)
                print("NOT NOTICED: %s, %s" % (name, mode))


def test_wrong_later_trips_fail_the_comparison_of_the_sums():
    case = cases.history_case(CUS)
    for fields in (cases.R.FIELDS, ("shear",)):
        want = cases.history_want(case, fields)
        tells(lambda got, mode: cases.compare_history(case, fields, got, want, mode, "sums"), want, np.nan, case["trip"], cases.LANES)


def test_wrong_later_trips_fail_the_comparison_of_the_statistics():
    case = cases.history_case(CUS)
    want, wwant = cases.stats_want(case)
    assert not np.isnan(want).any() and not np.isnan(wwant).any()
    tells(lambda got, mode: cases.compare_stats(case, got, wwant, want, wwant, mode, "stats"), want, np.nan, case["trip"], cases.LANES)
    tells(lambda wgot, mode: cases.compare_stats(case, want, wgot, want, wwant, mode, "stats"), wwant, np.nan, case["trip"], cases.LANES)
    # every plane by itself: no pair is carried by the others
    pairs = cases.stats_tests().PAIRS
    for kind in range(len(cases.WRONG)):
        bad = cases.wrong(kind, want, np.nan, case["trip"], cases.LANES)
        one = want.copy()
        for k, e in enumerate(pairs):
            one[k] = bad[k]
            with pytest.raises(AssertionError):
                cases.compare_stats(case, one, wwant, want, wwant, cases.MODES[2], e)
            one[k] = want[k]


def test_wrong_later_trips_fail_the_comparison_of_the_row_totals():
    case = cases.series_case(CUS)
    j0, j1 = case["j0"], case["j1"]
    want = case["want"][:, j0:j1]
    tells(lambda got, mode: cases.compare_series(case, got, mode, "totals"), want, np.nan, case["trip"], cases.ROWS)
    for kind in range(len(cases.WRONG)):  # every quantity by itself
        bad = cases.wrong(kind, want, np.nan, case["trip"], cases.ROWS)
        for k, q in enumerate(S.QUANTITIES):
            one = want.copy()
            one[k] = bad[k]
            with pytest.raises(AssertionError):
                cases.compare_series(case, one, cases.MODES[2], q)
    # the rows of many magnitudes sit one in each trip, away from both ends, and remember the order of their additions
    first, later = case["magnitude_rows"]
    assert case["trip"][first - j0] == 0 and case["trip"][later - j0] == 1 and j0 + 4 < first and later < j1 - 4
    volume, area = S.QUANTITIES.index("volume"), S.QUANTITIES.index("area")
    for r in (first, later):
        for k, x in ((volume, case["state"]["H"][0, r]), (area, case["state"]["A"][0, r])):
            assert case["want"][k, r] == S.reduce_row(x)
            assert case["want"][k, r] != np.add.accumulate(x)[-1] and case["want"][k, r] != np.sum(x)


def test_wrong_later_trips_fail_the_comparison_of_the_column_state_transport():
    for order in (0, 1, 2):
        case = cases.weight_case(CUS, order)
        j0, j1 = case["j0"], case["j1"]
        later = np.zeros(case["T"].shape, dtype=bool)
        later[j0:j1] = case["trip"] > 0
        assert np.isnan(case["H"][:, later]).any() and np.isinf(case["T"][later]).any() and np.signbit(case["T"][later]).any()

        def whole(owned, full=case["want"]):
            out = full.copy()
            out[..., j0:j1, :] = owned
            return out

        tells(lambda got, mode: cases.compare_tracer(case, whole(got), case["want"], mode, "weight"), case["want"][:, j0:j1],
              case["Q0"][:, j0:j1], case["trip"], cases.LANES)
    case = cases.recover_case(CUS)
    j0, j1 = case["j0"], case["j1"]
    for want in case["want"]:
        def whole(owned, full=want):
            out = full.copy()
            out[j0:j1] = owned
            return out

        assert np.sum(want[j0:j1][case["trip"] > 0] != case["T"][j0:j1][case["trip"] > 0]) > 50000  # ice in the later trips
        tells(lambda got, mode: cases.compare_tracer(case, whole(got), want, mode, "recover"), want[j0:j1], case["T"][j0:j1], case["trip"],
              cases.LANES)
    # a row outside the range that was written fails the whole range
    bad = case["want"][0].copy()
    bad[j1, 5] += 1.0
    with pytest.raises(AssertionError):
        cases.compare_tracer(case, bad, case["want"][0], cases.MODES[0], "recover")

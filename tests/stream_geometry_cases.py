"""Shapes, inputs, references and comparisons for the streaming kernels past one pass of their grid (csrc/history.hip, csrc/tracer.hip):
what tests/test_gpu_stream_geometry.py runs on the device and tests/test_stream_geometry_cpu.py holds to its conditions without one.

The five kernels share one launch shape: one lane per element (history_accumulate_kernel<false / true>, tracer_weight_kernel<1 / 3 / 6>,
tracer_recover_kernel) or one wave per row (history_row_totals_kernel), a grid capped at 8 workgroups per CU, and a grid-stride loop for
the rest.  element_grid and row_grid restate the two rules as functions of the CU count; element_shape and row_shape give the smallest
arrays whose owned rows hold about 1.25 passes of that grid, so that the loop turns round once and the second trip is a ragged fifth of
the first.  Everything here is numpy: the modules of the GPU tests whose inputs and comparisons are reused are imported where they are
needed."""
import numpy as np

import column_transport_ref as CT
import history_ref as R
import history_stats_ref as S

LANES, ROWS, PER_CU = 256, 4, 8  # lanes and rows of a workgroup; workgroups per CU at which the grid is capped
CU_COUNTS = (64, 256, 304)  # the CPU test holds the shapes to their conditions at each of them
PASSES = 1.25
J0, TOP = 3, 2  # the owned rows are [J0, ny - TOP)
ELEMENT_NX, ROW_NX = 130, 65  # three stress tiles and a remainder of two; lane 0 of a row's wave folds two elements, the others one
NSAMPLES = 2  # the first stores into an accumulator of NaN, the second adds
EXTENT = 0.15
MAGNITUDES_SEEDS = (17, 117)  # of H and A: seeds at which 65 of them remember the order of their sum (the CPU test asserts it)
MODES = ("the whole range", "the first trip", "the later trips")
# what a launch with a broken loop leaves behind: the later trips never made; their lanes one workgroup further on (the first
# workgroup's worth of the later trips is then never visited); their lanes reading one workgroup further on and writing their own slot
WRONG = ("later trips left out", "later trips work one workgroup on", "later trips read one workgroup on")


def div_up(a, b):
    return -(-a // b)


def element_grid(cus, n):
    """(workgroups, elements of one pass, trips) of a launch over n elements: min(ceil(n / 256), 8 CUs) workgroups of 256 lanes"""
    wgs = min(div_up(n, LANES), PER_CU * cus)
    return wgs, wgs * LANES, div_up(n, wgs * LANES)


def row_grid(cus, rows):
    """(workgroups, rows of one pass, trips) of a launch over `rows` rows: min(ceil(rows / 4), 8 CUs) workgroups of four waves"""
    wgs = min(div_up(rows, ROWS), PER_CU * cus)
    return wgs, wgs * ROWS, div_up(rows, wgs * ROWS)


def element_shape(cus):
    """(nx, ny, j0, j1): the owned rows hold 1.25 passes of the element grid, rounded up to whole rows, and no multiple of 256"""
    rows = div_up(int(PASSES * PER_CU * cus * LANES), ELEMENT_NX)
    while (rows * ELEMENT_NX) % LANES == 0:
        rows += 1
    return ELEMENT_NX, rows + J0 + TOP, J0, rows + J0


def row_shape(cus):
    """(nx, ny, j0, j1): 1.25 passes of the row grid, and no multiple of the four rows of a workgroup"""
    rows = int(PASSES * PER_CU * cus * ROWS)
    while rows % ROWS == 0:
        rows += 1
    return ROW_NX, rows + J0 + TOP, J0, rows + J0


def element_trips(cus, nx, j0, j1):
    """[j1 - j0, nx]: the trip of the loop in which the element is visited"""
    n = (j1 - j0) * nx
    return (np.arange(n) // element_grid(cus, n)[1]).reshape(j1 - j0, nx)


def row_trips(cus, j0, j1):
    return np.arange(j1 - j0) // row_grid(cus, j1 - j0)[1]


def selection(trip, mode):
    return {MODES[0]: trip >= 0, MODES[1]: trip == 0, MODES[2]: trip > 0}[mode]


def wrong(kind, want, untouched, trip, step):
    """`want` [..., *trip.shape] as a launch with the broken loop WRONG[kind] would leave it; untouched: what the output held before the
    launch; step: a workgroup's worth, 256 elements or 4 rows.  (Written for the two trips these shapes take.)"""
    lead = want.shape[:want.ndim - trip.ndim]
    w = want.reshape(lead + (-1,))
    u = np.broadcast_to(untouched, want.shape).reshape(w.shape)
    later = np.nonzero(trip.reshape(-1) > 0)[0]
    out = w.copy()
    if kind == 0:
        out[..., later] = u[..., later]
    elif kind == 1:
        out[..., later[:step]] = u[..., later[:step]]
    else:
        ok = later + step < w.shape[-1]
        out[..., later[ok]] = w[..., later[ok] + step]
        out[..., later[~ok]] = u[..., later[~ok]]
    return out.reshape(want.shape)


def history_tests():
    import test_gpu_history as G

    return G


def stats_tests():
    import test_gpu_history_stats as GS

    return GS


_cases = {}


def cached(key, make):
    """every case is computed once per process and left unchanged"""
    if key not in _cases:
        _cases[key] = make()
    return _cases[key]


def frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ history: the plain sums and the statistics
def history_case(cus):
    """NSAMPLES states of test_gpu_history.random_state on the element shape, the reference samples of all twelve fields
    [NSAMPLES, 12, ny, nx] and the scale of every rounded field"""
    def make():
        G = history_tests()
        nx, ny, j0, j1 = element_shape(cus)
        rng = np.random.default_rng(1000 * nx + ny)
        states = [G.random_state(nx, ny, rng) for _ in range(NSAMPLES)]
        ref = frozen(np.stack([R.samples(R.FIELDS, G.HX, G.HY, **st) for st in states]))
        scale = {n: max(R.rounding_scale(n, G.HX, G.HY, **{k: st[k] for k in ("u", "v", "s11", "s12", "s22")}) for st in states)
                 for n in R.FIELDS if n not in R.EXACT_FIELDS}
        return dict(nx=nx, ny=ny, j0=j0, j1=j1, states=states, ref=ref, scale=scale, trip=element_trips(cus, nx, j0, j1))
    return cached(("history", cus), make)


def history_want(case, fields):
    """[len(fields), j1 - j0, nx]: history_ref.accumulate of the NSAMPLES samples on the rows [j0, j1) of planes of NaN.  (The planes of
    all ny rows are accumulated, and the rows outside the range must still be NaN.)"""
    idx = [R.FIELDS.index(n) for n in fields]
    acc = np.full((len(fields), case["ny"], case["nx"]), np.nan)
    for k in range(NSAMPLES):
        R.accumulate(acc, case["ref"][k][idx], case["j0"], case["j1"], k == 0)
    outside = np.ones(case["ny"], dtype=bool)
    outside[case["j0"]:case["j1"]] = False
    assert np.all(np.isnan(acc[:, outside])) and not np.any(np.isnan(acc[:, ~outside]))
    return acc[:, case["j0"]:case["j1"]]


def compare_history(case, fields, got, want, mode, what):
    """the rule of tests/test_gpu_history.py on the owned rows [k, j1 - j0, nx], restricted to the elements of `mode`"""
    sel = selection(case["trip"], mode)
    history_tests().compare(got[:, sel], want[:, sel], fields, case["scale"], NSAMPLES, "%s, %s:" % (what, mode))


def stats_want(case):
    """(acc [16, j1 - j0, nx], wacc [j1 - j0, nx]): history_stats_ref.accumulate_stats of the sixteen PAIRS over the NSAMPLES samples"""
    pairs = stats_tests().PAIRS
    names, stats = zip(*[S.parse(e) for e in pairs])
    idx = [R.FIELDS.index(n) for n in names]
    acc, wacc = np.full((len(pairs), case["ny"], case["nx"]), np.nan), np.full((case["ny"], case["nx"]), np.nan)
    for k, st in enumerate(case["states"]):
        S.accumulate_stats(acc, wacc, case["ref"][k][idx], S.weight(st["A"]), stats, case["j0"], case["j1"], k == 0)
    return acc[:, case["j0"]:case["j1"]], wacc[case["j0"]:case["j1"]]


def compare_stats(case, got, wgot, want, wwant, mode, what):
    """the rule of tests/test_gpu_history_stats.py: the weight plane bit for bit, every pair under that file's compare"""
    GS = stats_tests()
    sel = selection(case["trip"], mode)
    assert np.array_equal(wgot[sel], wwant[sel]), (what, mode, "wacc")
    GS.compare(got[:, sel], want[:, sel], GS.PAIRS, case["scale"], NSAMPLES, "%s, %s:" % (what, mode))


# ------------------------------------------------------------------------------------------------ the row totals
def series_case(cus):
    """one random state on the row shape; the middle row of each trip holds many_magnitudes in H and A, so that the order of a row's
    additions shows in its totals.  want [7, ny] in the order of S.QUANTITIES, bound[q] [ny] for the rounded ones"""
    def make():
        G = history_tests()
        nx, ny, j0, j1 = row_shape(cus)
        per = row_grid(cus, j1 - j0)[1]
        st = G.random_state(nx, ny, np.random.default_rng(7000 * nx + ny))
        rows = (j0 + per // 2, j0 + per + (j1 - j0 - per) // 2)
        for r in rows:
            st["H"][0, r] = S.many_magnitudes(nx, seed=MAGNITUDES_SEEDS[0])
            st["A"][0, r] = 1e-8 * S.many_magnitudes(nx, seed=MAGNITUDES_SEEDS[1])  # in (1e-16, 1): the area and the drift weights
        want = frozen(S.row_totals_of_many_rows(S.QUANTITIES, G.HX, G.HY, EXTENT, **st))
        bound = {q: frozen(S.row_total_bound(q, G.HX, G.HY, EXTENT, **st)) for q in S.QUANTITIES if q not in S.EXACT_QUANTITIES}
        return dict(nx=nx, ny=ny, j0=j0, j1=j1, state=st, want=want, bound=bound, magnitude_rows=rows, trip=row_trips(cus, j0, j1))
    return cached(("series", cus), make)


def compare_series(case, got, mode, what):
    """the rule of test_row_totals_match_the_reference on got [7, j1 - j0] in the order of S.QUANTITIES"""
    sel = selection(case["trip"], mode)
    rows = slice(case["j0"], case["j1"])
    for k, q in enumerate(S.QUANTITIES):
        g, w = got[k][sel], case["want"][k, rows][sel]
        if q in S.EXACT_QUANTITIES:
            assert np.array_equal(g, w), (what, mode, q, int(np.sum(g != w)))
        else:
            err, bound = np.abs(g - w), case["bound"][q][rows][sel]
            print("%s, %s: %-9s largest error / bound %.3f" % (what, mode, q, float(np.max(err / bound))))
            assert np.all(err <= bound), (what, mode, q, float(np.max(err / bound)))  # (a NaN is not below its bound)


# ------------------------------------------------------------------------------------------------ the column state transport
def sprinkle(a, value, first, count):
    """`count` values spread evenly over a, the rows of the later trips included"""
    a.reshape(-1)[first::max(1, a.size // count)] = value


def weight_case(cus, order):
    """the recipe of test_weight_matches_numpy_bit_for_bit: NaN in H, inf and -0 in T, Q filled beforehand"""
    def make():
        nx, ny, j0, j1 = element_shape(cus)
        nc = {0: 1, 1: 3, 2: 6}[order]
        rng = np.random.default_rng(nx * 31 + ny + order)
        H = rng.standard_normal((nc, ny, nx)) * rng.uniform(0.0, 3.0, (nc, ny, nx))
        T = rng.uniform(-30.0, 5.0, (ny, nx))
        sprinkle(H, np.nan, 0, 97 * nc)
        sprinkle(T, np.inf, 3, 89)
        sprinkle(T, -0.0, 0, 83)
        Q0 = rng.standard_normal((nc, ny, nx))
        want = CT.weight(H, T, j0, j1, Q=Q0)
        return dict(nx=nx, ny=ny, j0=j0, j1=j1, order=order, H=frozen(H), T=frozen(T), Q0=frozen(Q0), want=frozen(want),
                    trip=element_trips(cus, nx, j0, j1))
    return cached(("weight", cus, order), make)


RECOVER_PARAMS = ((CT.MIN_CONC, CT.MIN_THICK), (0.3, 0.5))


def recover_case(cus):
    """the recipe of test_recover_matches_numpy_bit_for_bit_on_random_inputs, with NaN, inf and -0 among the cell means"""
    def make():
        nx, ny, j0, j1 = element_shape(cus)
        rng = np.random.default_rng(nx + 7 * ny)
        H, A, Q = (rng.standard_normal((6, ny, nx)) for _ in range(3))
        H[0] = rng.uniform(-0.2, 2.0, (ny, nx))
        A[0] = rng.uniform(-0.1, 1.1, (ny, nx))
        A[0][rng.random((ny, nx)) < 0.1] = 1e-13
        H[0][rng.random((ny, nx)) < 0.1] = 0.0
        Q[0] = -8.0 * H[0] + rng.standard_normal((ny, nx))
        sprinkle(H[0], np.nan, 1, 97)
        sprinkle(H[0], np.inf, 2, 89)
        sprinkle(A[0], np.nan, 5, 83)
        sprinkle(Q[0], np.nan, 7, 79)
        sprinkle(Q[0], np.inf, 11, 73)
        sprinkle(Q[0], -0.0, 13, 71)
        T = rng.uniform(-20.0, 0.0, (ny, nx))
        want = [frozen(CT.recover(H, A, Q, T, mc, mt, j0, j1)) for mc, mt in RECOVER_PARAMS]
        return dict(nx=nx, ny=ny, j0=j0, j1=j1, H=frozen(H), A=frozen(A), Q=frozen(Q), T=frozen(T), want=want,
                    trip=element_trips(cus, nx, j0, j1))
    return cached(("recover", cus), make)


def same_bits(got, want):
    from test_gpu_column_transport import same_bits as same

    return same(got, want)


def compare_tracer(case, got, want, mode, what):
    """bit for bit, on arrays of all ny rows [..., ny, nx]: the whole range is the whole array, so the rows outside [j0, j1) must hold
    what they held"""
    if mode == MODES[0]:
        assert same_bits(got, want), (what, mode)
        return
    sel = np.zeros((case["ny"], case["nx"]), dtype=bool)
    sel[case["j0"]:case["j1"]] = selection(case["trip"], mode)
    assert same_bits(got[..., sel], want[..., sel]), (what, mode)

"""Independent numpy statement of the history statistics and the row totals (include/nsdg.h "history output":
nsdg_history_accumulate_stats, nsdg_history_row_totals), and their CPU stand-in for the driver tests without a GPU.

The samples are those of tests/history_ref.py, by import.  The row reduction is written with explicit lane and tree loops -- one Python
float per lane, one addition per line of the header's order -- and shares no code with csrc/history.hip."""
import numpy as np

import history_ref as R

STATS = ("mean", "ice_mean", "min", "max")
QUANTITIES = ("area", "extent", "volume", "snow_volume", "drift", "speed_max", "hice_max")
EXACT_QUANTITIES = ("area", "extent", "volume", "snow_volume", "hice_max")  # the terms are source values, clamped or compared: no rounding
MAX_QUANTITIES = ("speed_max", "hice_max")
LANES = 64
EPS = R.EPS
# A rounded sample x is within 16 eps scale of any other correct evaluation (history_ref.rounding_scale).  The weighted sample t = w x
# has 0 <= w <= 1 exact and one more rounding on either side: |t_a - t_b| <= w |x_a - x_b| + 2 eps |w x| <= (16 + 2 c) eps scale with
# |x| <= c scale; c = 1 for speed (the scale is the largest speed) and c = 2 for shear (|e11 - e22| + |g| <= 2 scale): 16 + 4 covers both.
SAMPLE_FACTOR = 16
WEIGHTED_FACTOR = 16 + 4


def weight(A):
    """w = min(max(A, 0), 1) of the cell mean; a NaN stays a NaN"""
    return np.minimum(np.maximum(R.plane0(A), 0.0), 1.0)


def parse(entry):
    """"name" or "name:stat" -> (name, stat)"""
    name, _, stat = entry.partition(":")
    return name, stat or "mean"


def accumulate_stats(acc, wacc, x, w, stats, j0, j1, store, row0=0):
    """the normative update of every plane k with statistic stats[k] on the rows [j0, j1); x: [k, ny, nx] samples, w: [ny, nx]"""
    rows = slice(j0 - row0, j1 - row0)
    for k, stat in enumerate(stats):
        xk, old = x[k, j0:j1], acc[k, rows]
        if stat == "mean":
            acc[k, rows] = xk if store else old + xk
        elif stat == "ice_mean":
            t = w[j0:j1] * xk  # rounded on its own
            acc[k, rows] = t if store else old + t
        elif stat == "min":
            acc[k, rows] = xk if store else np.where((xk < old) | (xk != xk), xk, old)
        elif stat == "max":
            acc[k, rows] = xk if store else np.where((xk > old) | (xk != xk), xk, old)
        else:
            raise ValueError("unknown statistic %r" % (stat,))
    if "ice_mean" in stats:
        wacc[rows] = w[j0:j1] if store else wacc[rows] + w[j0:j1]


def finalise(acc, wacc, stats, n):
    """what a host makes of a window of n samples: [k, rows, nx]"""
    out = np.empty_like(acc)
    for k, stat in enumerate(stats):
        if stat == "mean":
            out[k] = acc[k] / n
        elif stat == "ice_mean":
            out[k] = np.nan
            iced = wacc > 0
            out[k][iced] = acc[k][iced] / wacc[iced]
        else:
            out[k] = acc[k]
    return out


def row_terms(name, hx, hy, extent_conc, H=None, A=None, u=None, v=None, hsnow=None, **_):
    """the terms x(iy, ix) of one quantity, [ny, nx]"""
    if name == "area":
        return weight(A)
    if name == "extent":
        return np.where(R.plane0(A) >= extent_conc, 1.0, 0.0)
    if name == "volume":
        return np.maximum(R.plane0(H), 0.0)
    if name == "snow_volume":
        return np.maximum(np.asarray(hsnow, dtype=np.float64), 0.0)
    if name == "drift":
        return weight(A) * R.sample("speed", hx, hy, u=u, v=v)
    if name == "speed_max":
        return R.sample("speed", hx, hy, u=u, v=v)
    if name == "hice_max":
        return R.plane0(H).copy()
    raise ValueError("unknown series quantity %r" % (name,))


def op_sum(a, b):
    return a + b


def op_max(a, b):
    return b if (b > a or b != b) else a


def reduce_row(x, op=op_sum):
    """the normative order: lane l folds ix = l, l + 64, ... in ascending order from the identity; then s = 32 ... 1: p_l = op(p_l, p_(l+s))
    for l < s; the result is p_0"""
    p = [np.float64(0.0) if op is op_sum else np.float64(-np.inf) for _ in range(LANES)]
    for lane in range(LANES):
        for ix in range(lane, len(x), LANES):
            p[lane] = op(p[lane], np.float64(x[ix]))
    s = LANES // 2
    while s >= 1:
        for lane in range(s):
            p[lane] = op(p[lane], p[lane + s])
        s //= 2
    return p[0]


def reduce_rows(x, op=op_sum):
    """reduce_row of every row of x [rows, nx] at once, for arrays of thousands of rows: the same operations in the same sequence, each
    of them on a vector over the rows (tests/test_stream_geometry_cpu.py holds it to reduce_row bit for bit)"""
    x = np.asarray(x, dtype=np.float64)
    if op is op_sum:
        vop = lambda a, b: a + b
    else:
        vop = lambda a, b: np.where((b > a) | (b != b), b, a)
    p = np.full((x.shape[0], LANES), 0.0 if op is op_sum else -np.inf)
    with np.errstate(invalid="ignore"):
        for first in range(0, x.shape[1], LANES):  # lane l folds ix = l, l + 64, ... in ascending order
            fold = x[:, first:first + LANES]
            p[:, :fold.shape[1]] = vop(p[:, :fold.shape[1]], fold)
        s = LANES // 2
        while s >= 1:
            p[:, :s] = vop(p[:, :s], p[:, s:2 * s])
            s //= 2
    return p[:, 0].copy()


def row_totals_of_many_rows(quantities, hx, hy, extent_conc, **src):
    """row_totals by reduce_rows"""
    return np.stack([reduce_rows(row_terms(name, hx, hy, extent_conc, **src), op_max if name in MAX_QUANTITIES else op_sum)
                     for name in quantities])


def row_totals(quantities, hx, hy, extent_conc, **src):
    """[nq, ny]: R_k(iy) of every row"""
    out = []
    for name in quantities:
        t = row_terms(name, hx, hy, extent_conc, **src)
        op = op_max if name in MAX_QUANTITIES else op_sum
        with np.errstate(invalid="ignore"):
            out.append([reduce_row(row, op) for row in t])
    return np.array(out, dtype=np.float64)


def row_total_bound(name, hx, hy, extent_conc, **src):
    """[ny]: how far a correct row total of a rounded quantity may sit from row_totals: the bound of every term (SAMPLE_FACTOR or
    WEIGHTED_FACTOR eps scale of the speed), summed over the row, and the roundings of the reduction itself -- at most nx / 64 folds and
    six tree levels on the way of any term, on both sides: (nx / 64 + 7) eps sum |terms|"""
    t = row_terms(name, hx, hy, extent_conc, **src)
    nx = t.shape[1]
    scale = R.rounding_scale("speed", hx, hy, u=src["u"], v=src["v"])
    factor = WEIGHTED_FACTOR if name == "drift" else SAMPLE_FACTOR
    return nx * factor * EPS * scale + (nx / 64 + 7) * EPS * np.sum(np.abs(t), axis=1)


def many_magnitudes(n, seed=6):
    """positive numbers over sixteen decades: a sum of them remembers the order it was taken in (the default seed is one at which 257 of
    them do: tests/test_history_stats_cpu.py asserts it)"""
    return 10.0 ** np.random.default_rng(seed).uniform(-8.0, 8.0, n)


class StatsOps(R.HistoryOps):
    """HistoryOps and the two new calls of abi.Context, on CPU torch tensors"""

    def history_accumulate_stats(self, j0, j1, pairs, sources, store, row0, acc, wacc=None):
        src = {k: t.numpy() for k, t in sources.items() if t is not None}
        x = R.samples([f for f, _ in pairs], self.hx, self.hy, **src)
        w = weight(src["A"]) if "A" in src else None
        accumulate_stats(acc.numpy(), None if wacc is None else wacc.numpy(), x, w, [s for _, s in pairs], j0, j1, store, row0)

    def history_row_totals(self, j0, j1, quantities, sources, extent_conc, row0, out):
        src = {k: t.numpy() for k, t in sources.items() if t is not None}
        out.numpy()[:, j0 - row0:j1 - row0] = row_totals(quantities, self.hx, self.hy, extent_conc, **src)[:, j0:j1]

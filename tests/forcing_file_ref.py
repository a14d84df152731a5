"""numpy restatement of nsdg_forcing_sample (include/nsdg.h "forcing from a file"): records on a cell-centred lattice over the square
domain, sampled bilinearly onto the CG2 nodes or the element centres of a row block and interpolated linearly in time.  The index-space
coordinate is num / den in integers, divided once, exactly as the kernel computes it."""
import numpy as np


def axis(num, den, n):
    """(i0, i1, f) arrays for integer numerators `num` over `den` on an axis of n lattice points, clamped with weight 0 at both ends"""
    num = np.asarray(num, dtype=np.int64)
    low, high = num <= 0, num >= (n - 1) * den
    q = np.where(low, 0, np.where(high, n - 1, num // den))
    f = np.where(low | high, 0.0, (num - q * den).astype(np.float64) / float(den))
    i1 = np.where(low | high, q, q + 1)
    return q, i1, f


def coordinates(where, nx, ny, row0=0, ny_global=None, nxr=1, nyr=1):
    """the (i0, i1, fx) of the columns and (j0, j1, fy) of the rows of the local array's targets"""
    ny_global = ny if ny_global is None else ny_global
    if where == "nodes":
        gx = np.arange(2 * nx + 1, dtype=np.int64)
        gy = np.arange(2 * ny + 1, dtype=np.int64) + 2 * row0
        numx, numy = gx * nxr - nx, gy * nyr - ny_global
    elif where == "elements":
        ix = np.arange(nx, dtype=np.int64)
        iy = np.arange(ny, dtype=np.int64) + row0
        numx, numy = (2 * ix + 1) * nxr - nx, (2 * iy + 1) * nyr - ny_global
    else:
        raise ValueError(where)
    return axis(numx, 2 * nx, nxr), axis(numy, 2 * ny_global, nyr)


def lerp(a, b, f):
    return a + f * (b - a)


def sample(rec, where, nx, ny, row0=0, ny_global=None):
    """one record plane [nyr, nxr] sampled onto the targets: [2 ny + 1, 2 nx + 1] (nodes) or [ny, nx] (elements)"""
    rec = np.asarray(rec, dtype=np.float64)
    nyr, nxr = rec.shape
    (i0, i1, fx), (j0, j1, fy) = coordinates(where, nx, ny, row0, ny_global, nxr, nyr)
    fx, fy = fx[None, :], fy[:, None]
    lo = lerp(rec[j0][:, i0], rec[j0][:, i1], fx)
    hi = lerp(rec[j1][:, i0], rec[j1][:, i1], fx)
    return lerp(lo, hi, fy)


def forcing_sample(where, rec0, rec1, w, nx, ny, row0=0, ny_global=None):
    """the list of output planes of nsdg_forcing_sample for the record planes rec0[k], rec1[k] and time weight w"""
    return [lerp(sample(a, where, nx, ny, row0, ny_global), sample(b, where, nx, ny, row0, ny_global), w) for a, b in zip(rec0, rec1)]


def bracket(times, t):
    """(k0, k1, w) of the records around model time t: k0 the last record with times[k0] <= t, k1 = k0 + 1 and
    w = (t - times[k0]) / (times[k1] - times[k0]); at the last record itself k1 = k0 and w = 0.  Outside [times[0], times[-1]]: ValueError"""
    times = np.asarray(times, dtype=np.float64)
    if not (times[0] <= t <= times[-1]):
        raise ValueError("model time %r s is outside the forcing records [%r, %r] s" % (t, times[0], times[-1]))
    k0 = int(np.searchsorted(times, t, side="right")) - 1
    if k0 == len(times) - 1:
        return k0, k0, 0.0
    return k0, k0 + 1, (t - times[k0]) / (times[k0 + 1] - times[k0])

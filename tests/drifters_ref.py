"""Independent numpy restatement of nsdg_drifters_advance, written from the text of include/nsdg.h "drifters" (not from csrc/drifters.hip).

The Lagrange weights are built from the node positions -1/2, 0, +1/2 of the reference element by the product formula, not from the closed
forms of the header.  dtype: the arithmetic of the step (np.float64, or np.longdouble to measure the rounding of the float64 run).  The
DECISIONS the header states as IEEE double operations -- the element of a coordinate -- are taken in float64 whatever the dtype, so that both
runs follow the same drifter through the same elements."""
import numpy as np

NODES = (-0.5, 0.0, 0.5)
ACTIVE, LEFT, NO_ICE, LAND = 0.0, 1.0, 2.0, 3.0


def lagrange(t, dtype):
    """the weights of the three nodes at the local coordinate t: L_k(t) = prod_{m != k} (t - t_m) / (t_k - t_m)"""
    w = []
    for k, tk in enumerate(NODES):
        p = dtype(1.0)
        for m, tm in enumerate(NODES):
            if m != k:
                p = p * (t - dtype(tm)) / (dtype(tk) - dtype(tm))
        w.append(p)
    return w


def locate(x, h, n):
    """rule 1: min(n - 1, floor(x / h)) by IEEE double division, never below 0"""
    f = np.floor(np.float64(x) / np.float64(h))
    if not f > 0:
        return 0
    return int(min(f, n - 1))


def velocity(u, v, ix, iy, iyg, x, y, hx, hy, dtype):
    """rule 5: the biquadratic velocity of the local element (ix, iy), global row iyg, at (x, y)"""
    lx = lagrange(x / hx - dtype(ix) - dtype(0.5), dtype)
    ly = lagrange(y / hy - dtype(iyg) - dtype(0.5), dtype)
    out = []
    for w in (u, v):
        s = dtype(0.0)
        for r in range(3):
            row = dtype(0.0)
            for c in range(3):
                row = row + lx[c] * dtype(w[2 * iy + r, 2 * ix + c])
            s = s + ly[r] * row
        out.append(s)
    return out


def advance(u, v, A0, d, hx, hy, dt, min_conc, land=None, row0=0, ny_global=None, j0=0, j1=None, dtype=np.float64):
    """one call of nsdg_drifters_advance.  u, v: [2 ny + 1, 2 nx + 1] of the local array; A0: [ny, nx], the cell means of the concentration;
    land: [ny, nx] or None; d: [3, n].  Returns d_out [3, n] in `dtype`"""
    ny, nx = A0.shape
    ny_global = ny if ny_global is None else ny_global
    j1 = ny if j1 is None else j1
    hx, hy, dt = dtype(hx), dtype(hy), dtype(dt)
    Lx, Ly = dtype(nx) * hx, dtype(ny_global) * hy
    n = d.shape[1]
    out = np.full((3, n), -np.inf, dtype=dtype)
    for i in range(n):
        x, y, s = dtype(d[0, i]), dtype(d[1, i]), float(d[2, i])
        ix, iyg = locate(x, hx, nx), locate(y, hy, ny_global)
        iy = iyg - row0
        if not (j0 <= iy < j1):
            continue
        out[:, i] = (x, y, s)
        if s != ACTIVE:
            continue
        if land is not None and land[iy, ix]:
            out[2, i] = LAND
            continue
        if A0[iy, ix] < min_conc:
            out[2, i] = NO_ICE
            continue
        u1, v1 = velocity(u, v, ix, iy, iyg, x, y, hx, hy, dtype)
        ixa, ixb = max(ix - 1, 0), min(ix + 1, nx - 1)
        iya, iyb = max(iyg - 1, 0), min(iyg + 1, ny_global - 1)
        xp, yp = x + dt * u1, y + dt * v1
        xp = min(max(xp, dtype(ixa) * hx), dtype(ixb + 1) * hx) if xp == xp else x
        yp = min(max(yp, dtype(iya) * hy), dtype(iyb + 1) * hy) if yp == yp else y
        ix2 = min(max(locate(xp, hx, nx), ixa), ixb)
        iyg2 = min(max(locate(yp, hy, ny_global), iya), iyb)
        u2, v2 = velocity(u, v, ix2, iyg2 - row0, iyg2, xp, yp, hx, hy, dtype)
        xn = x + dtype(0.5) * dt * (u1 + u2)
        yn = y + dtype(0.5) * dt * (v1 + v2)
        if not (0 <= xn <= Lx and 0 <= yn <= Ly):
            out[2, i] = LEFT
        else:
            out[0, i], out[1, i] = xn, yn
    return out


def bound(Lx, Ly):
    """the position tolerance of a float64 run of one step against another (tests/test_gpu_drifters.py states where it comes from)"""
    return 64 * 2.0 ** -52 * max(Lx, Ly)

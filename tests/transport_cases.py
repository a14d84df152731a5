"""Inputs of the tests that hold the DG transport to tests/transport_independent.py (numpy only; shared by the CPU test of the oracle and
the device test, so that what the device test needs of its inputs is asserted without a GPU as well).

Velocities are random at every node, the boundary included, with both signs of the normal component forced on all four sides: the
open boundary -- outflow, and 'nothing flows in' against a non-zero inflow velocity -- is part of every case.  Fields for the closure
are a quiet background with elements that the closure must cap, elements it must scale and elements it must leave alone placed on
BOTH sides of every column-window seam and every strip seam of the marching kernel."""
import numpy as np

NCOEF = {0: 1, 1: 3, 2: 6}
OWN = {0: 62, 1: 60, 2: 58}  # columns a wave of the marching kernel owns: 64 - 2 (order + 1)
STRIP = 4  # rows of a strip of the march on any small grid
HX, HY = 700.0, 900.0
CFL = 0.05  # largest nodal speed times dt over the smaller mesh width: three steps keep a field of O(1) at O(1)

# the closure of the fields of a multi-field step, all different: (lo, hi, cap_mean)
BOUNDS = ((0.0, np.inf, False), (0.0, 1.0, True), (-0.25, 0.75, True), (0.1, 2.0, False))
BACKGROUND = (0.45, 0.45, 0.3, 0.5)  # cell means well inside the bounds
UNTOUCHED, CAPPED, SCALED = 0, 1, 2


def shapes(order):
    """the smallest grids at which each kernel of csrc/transport.hip can go wrong (nx, ny)"""
    own = OWN[order]
    return [(own + 1, 9),  # one column-window seam, two strip seams, a one-row last strip
            (own, 5),  # no ragged column
            (own - 1, 4),
            (2 * own + 1, 5),  # three windows
            (64, 9), (130, 5),  # the 64-lane block edge of the pair kernel (even nx) and of the stage kernel
            (65, 5),  # odd nx: variant 2 falls back to the stage kernel
            (2, 3), (1, 1), (1, 7), (7, 1)]


def velocity(nx, ny, seed):
    """CG2 nodal velocity, non-zero on the whole boundary, inflow and outflow on each of the four sides"""
    rng = np.random.default_rng(seed)
    u = 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1))
    v = 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1))
    for side in (u[:, 0], u[:, -1], v[0, :], v[-1, :]):  # the normal component on the left / right / bottom / top side
        side[0], side[-1] = abs(side[0]) + 0.05, -abs(side[-1]) - 0.05
    return u, v


def time_step(u, v):
    return CFL * min(HX, HY) / max(np.abs(u).max(), np.abs(v).max())


def random_field(nx, ny, order, seed):
    """a field of O(1) with every coefficient random"""
    rng = np.random.default_rng(seed)
    nc = NCOEF[order]
    return np.concatenate([0.6 + 0.2 * rng.standard_normal((1, ny, nx)), 0.1 * rng.standard_normal((nc - 1, ny, nx))])


def seams(nx, ny, order):
    """(window seams, strip seams) of the march on the whole array: a seam s lies between the columns (rows) s - 1 and s"""
    return list(range(OWN[order], nx, OWN[order])), list(range(STRIP, ny, STRIP))


def marks(nx, ny, order):
    """what the closure is meant to do with each element [ny, nx]: sparse over the grid, and all three kinds in every column and row
    next to a seam"""
    iy, ix = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    k = (3 * ix + 5 * iy) % 11
    m = np.where(k == 0, CAPPED, np.where(k == 1, SCALED, UNTOUCHED))
    cols, rows = seams(nx, ny, order)
    near = np.zeros((ny, nx), dtype=bool)
    for s in cols:
        near[:, s - 1:s + 1] = True
    for r in rows:
        near[r - 1:r + 1, :] = True
    dense = np.array([CAPPED, SCALED, UNTOUCHED])[(ix + iy) % 3]
    return np.where(near, dense, m)


def bounded_field(nx, ny, order, f, seed):
    """field f of a multi-field step under BOUNDS[f]: background + the marked elements.  A CAPPED mark puts the cell mean above hi
    where the mean is capped (elsewhere it asks for a scaling from above, or from below where there is no upper bound); a SCALED mark
    puts the mean just above lo with a slope that takes the left edge below lo"""
    lo, hi, cap = BOUNDS[f]
    rng = np.random.default_rng(seed + 101 * f)
    nc = NCOEF[order]
    F = np.concatenate([BACKGROUND[f] + 0.03 * rng.standard_normal((1, ny, nx)), 0.02 * rng.standard_normal((nc - 1, ny, nx))])
    m = marks(nx, ny, order)
    if cap:
        F[0][m == CAPPED] = hi + 0.3
    elif nc > 1:
        if np.isfinite(hi):
            F[0][m == CAPPED], F[2][m == CAPPED] = hi - 0.05, 0.4
        else:
            F[0][m == CAPPED], F[2][m == CAPPED] = lo + 0.05, -0.4
    F[0][m == SCALED] = lo + 0.05
    if nc > 1:
        F[1][m == SCALED] = 0.4
    return F


def classify(before, after):
    """what the closure did to each element, from a step's result before and after it: [ny, nx] of UNTOUCHED / CAPPED / SCALED"""
    capped = after[0] != before[0]
    scaled = np.any(after[1:] != before[1:], axis=0) & ~capped
    return np.where(capped, CAPPED, np.where(scaled, SCALED, UNTOUCHED))


def seam_sides(nx, ny, order):
    """[(name, mask of the elements on one side, mask of the elements on the other side)] for every seam of the march whose sides --
    the column or row next to it -- hold at least three elements, one for each kind (the 1 x 7 grid has strip seams of one element)"""
    cols, rows = seams(nx, ny, order)
    if ny < 3:
        cols = []
    if nx < 3:
        rows = []
    out = []
    for s in cols:
        a, b = np.zeros((ny, nx), dtype=bool), np.zeros((ny, nx), dtype=bool)
        a[:, s - 1], b[:, s] = True, True
        out.append(("window seam at column %d" % s, a, b))
    for r in rows:
        a, b = np.zeros((ny, nx), dtype=bool), np.zeros((ny, nx), dtype=bool)
        a[r - 1, :], b[r, :] = True, True
        out.append(("strip seam at row %d" % r, a, b))
    return out


def kinds_expected(order, f):
    """the kinds of closure action field f can show at this order: order 0 has only the cap, an uncapped field only the scaling"""
    kinds = [UNTOUCHED]
    if BOUNDS[f][2]:
        kinds.append(CAPPED)
    if order > 0:
        kinds.append(SCALED)
    return kinds


def assert_closure_active_at_the_seams(nx, ny, order, f, before, after):
    """every kind of action the field can show is present on both sides of every seam"""
    got = classify(before, after)
    for name, a, b in seam_sides(nx, ny, order):
        for side in (a, b):
            for kind in kinds_expected(order, f):
                assert np.any(got[side] == kind), (name, "field %d" % f, "order %d" % order, "kind %d missing" % kind)


# ------------------------------------------------------------------------------------------------ polynomial exactness
POLY = (0.7, 1.1e-4, -0.8e-4, 2.3e-8, -1.7e-8, 1.9e-8)  # a00, a10, a01, a20, a02, a11 of phi = sum a_mn x^m y^n (metres)
SIGNS = ((1, 1), (-1, -1), (1, -1), (-1, 1))


def poly_coefficients(order, nx, ny, sx=0.0, sy=0.0):
    """the DG(order) coefficients of the global polynomial phi(x - sx, y - sy), total degree <= order, in every element -- written out by
    hand from x = xc + hx xi, x^2 = (xc^2 + hx^2 / 12) + 2 xc hx xi + hx^2 (xi^2 - 1/12): no quadrature, no table.  A polynomial of
    the space is its own L2 projection"""
    a00, a10, a01, a20, a02, a11 = POLY
    if order < 2:
        a20 = a02 = a11 = 0.0
    if order < 1:
        a10 = a01 = 0.0
    yc, xc = np.meshgrid((np.arange(ny) + 0.5) * HY - sy, (np.arange(nx) + 0.5) * HX - sx, indexing="ij")
    c = [a00 + a10 * xc + a01 * yc + a20 * (xc * xc + HX * HX / 12.0) + a02 * (yc * yc + HY * HY / 12.0) + a11 * xc * yc,
         HX * (a10 + 2.0 * a20 * xc + a11 * yc), HY * (a01 + 2.0 * a02 * yc + a11 * xc),
         a20 * HX * HX + 0.0 * xc, a02 * HY * HY + 0.0 * xc, a11 * HX * HY + 0.0 * xc]
    return np.ascontiguousarray(np.array(c[:NCOEF[order]]))


def uniform_velocity(nx, ny, sign):
    """nodal fields of a uniform velocity with the given signs of (u_x, v_y), and the time step of a Courant number of 0.2"""
    ux, vy = 0.31 * sign[0], 0.23 * sign[1]
    shape = (2 * ny + 1, 2 * nx + 1)
    return np.full(shape, ux), np.full(shape, vy), ux, vy, 0.2 * HX / 0.31


def exact_zone(nx, ny, order, nsteps, sign):
    """the elements further than nsteps (order + 1) cells from the inflow sides [ny, nx]: every stage carries the 'nothing flows in'
    of the open boundary one cell further"""
    d = nsteps * (order + 1)
    z = np.zeros((ny, nx), dtype=bool)
    z[(d if sign[1] > 0 else 0):(ny if sign[1] > 0 else ny - d), (d if sign[0] > 0 else 0):(nx if sign[0] > 0 else nx - d)] = True
    return z


# ------------------------------------------------------------------------------------------------ the comparison
RTOL, ATOL_OF_MAX = 1e-12, 1e-13  # the bound of the device against the oracle on three transport steps (tests/test_gpu_parity.py)


def ratio(got, want):
    """largest |got - want| / (ATOL_OF_MAX max|want| + RTOL |want|) over the array: <= 1 meets the bound"""
    got, want = np.asarray(got), np.asarray(want)
    lim = ATOL_OF_MAX * np.max(np.abs(want)) + RTOL * np.abs(want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(lim > 0, np.abs(got - want) / lim, np.where(got == want, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0

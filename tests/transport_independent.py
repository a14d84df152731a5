"""INDEPENDENT restatement of the DG transport at EVERY order (DESIGN.md sections 3.1 and 3.3), TEST INFRASTRUCTURE, numpy only.

Why it exists.  The reference snapshot holds no dynamics code, so `oracle/dyn_oracle.c` and the kernels of `csrc/transport.hip` can
only be held to each other -- and an error they share passes every such comparison.  `tests/dyn_independent.py` removes that common
mode for ONE DG2 stage on a closed 6 x 5 box.  This file does it for the whole transport: DG0, DG1 and DG2, the advecting velocity,
the bare stage, the full Runge-Kutta step, the closure, the open boundary, and a step on a row range -- on grids of any size.

It is written from the FORMULAS of DESIGN.md only: it imports nothing from nextsimdg_amd (no basis tables, no generated constants),
nothing from the oracle and nothing from dyn_independent.py, and it takes a different route wherever the mathematics allows one:

  * the basis is the products of 1, t, t^2 - 1/12 evaluated where they are needed, derivatives analytic; nothing is tabulated;
  * every L2 projection solves with the FULL mass matrix of a 6-point Gauss rule (orthogonality of the basis is not assumed);
  * the CG2 velocity is projected with that 6-point rule from Lagrange functions built from their nodes (the kernels use one
    precomputed 9-column matrix PV);
  * the volume term is integrated with a 5-point rule (the scheme's (p+1)-point rule is exact for it); only the edge term uses the
    scheme's own p+1 points, where the quadrature IS the definition of the flux;
  * the upwind value is chosen by the sign of v.n (the kernels add a max(v.n, 0) and a min(v.n, 0) term), a neighbour outside the
    array is a zero field;
  * the time step is written in BUTCHER form -- slopes k1, k2, k3 -- not as the Shu-Osher pairs (a, b) of the kernels' RK table;
  * the closure finds theta as the minimum over the points, each from its own value (the kernels take the extrema first);
  * a step on a row range is computed on the WINDOW of those rows and p+1 ghost rows on either side, cut out of the array -- what a
    row block does -- not by a full step restricted afterwards.

Arrays: DG fields [nc, ny, nx] (coefficient planes), CG2 nodal fields [2 ny + 1, 2 nx + 1], edge-normal velocities
un_x [p+1, ny, nx + 1] and un_y [p+1, ny + 1, nx].  Vectorised over the elements: loops run over quadrature points and coefficients
only, so a 125 x 9 case takes well under a second."""
import numpy as np
from numpy.polynomial.legendre import leggauss

NCOEF = {0: 1, 1: 3, 2: 6}
# basis function i is P[KX[i]](xi) * P[KY[i]](eta) with P = 1, t, t^2 - 1/12: 1, xi, eta, xi^2 - 1/12, eta^2 - 1/12, xi eta
KX = (0, 1, 0, 2, 0, 1)
KY = (0, 0, 1, 0, 2, 1)
NODES = (-0.5, 0.0, 0.5)  # the CG2 nodes of the reference interval


def gauss(n):
    """n-point Gauss-Legendre rule on [-1/2, 1/2]"""
    x, w = leggauss(n)
    return 0.5 * x, 0.5 * w


def tensor_rule(n):
    """the n x n rule on the reference square as flat arrays x, y, w"""
    g, w = gauss(n)
    x, y = np.meshgrid(g, g)
    return x.ravel(), y.ravel(), np.outer(w, w).ravel()


def _p(k, t):
    return (np.ones_like(t), t, t * t - 1.0 / 12.0)[k]


def _dp(k, t):
    return (np.zeros_like(t), np.ones_like(t), 2.0 * t)[k]


def _pts(x, y):
    return np.atleast_1d(np.asarray(x, dtype=float)), np.atleast_1d(np.asarray(y, dtype=float))


def basis(order, x, y):
    """values of the DG(order) basis at the points (x[q], y[q]): [nc, nq]"""
    x, y = _pts(x, y)
    return np.array([_p(KX[i], x) * _p(KY[i], y) for i in range(NCOEF[order])])


def basis_dx(order, x, y):
    x, y = _pts(x, y)
    return np.array([_dp(KX[i], x) * _p(KY[i], y) for i in range(NCOEF[order])])


def basis_dy(order, x, y):
    x, y = _pts(x, y)
    return np.array([_p(KX[i], x) * _dp(KY[i], y) for i in range(NCOEF[order])])


def mass_inverse(order):
    """inverse of the FULL mass matrix of the reference square, 6-point rule"""
    x, y, w = tensor_rule(6)
    B = basis(order, x, y)
    return np.linalg.inv((B * w) @ B.T)


def lagrange(k, t):
    """the quadratic Lagrange function of node k, from the nodes"""
    t = np.asarray(t, dtype=float)
    out = np.ones_like(t)
    for j in range(3):
        if j != k:
            out = out * (t - NODES[j]) / (NODES[k] - NODES[j])
    return out


def evaluate(F, order, x, y):
    """the DG field F at the reference point(s) (x, y) of every element: [nq, ny, nx]"""
    return np.tensordot(basis(order, x, y).T, F, axes=1)


# ------------------------------------------------------------------------------------------------ the advecting velocity
def advection(u, v, nx, ny, order):
    """(vx, vy, un_x, un_y): the L2 projection of the CG2 velocity (u, v) on DG(order), and its normal component at the order + 1 Gauss
    points of every x-edge (u) and y-edge (v), from the three Lagrange nodes of that edge"""
    x, y, w = tensor_rule(6)
    P = mass_inverse(order) @ (basis(order, x, y) * w)  # [nc, 36]: point values -> coefficients
    LX = np.array([lagrange(a, x) for a in range(3)])
    LY = np.array([lagrange(a, y) for a in range(3)])

    def project(f):
        val = np.zeros((x.size, ny, nx))  # the biquadratic velocity at the 36 points of every element
        for ay in range(3):
            for ax in range(3):
                val += (LY[ay] * LX[ax])[:, None, None] * f[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2][None]
        return np.tensordot(P, val, axes=1)

    s, _ = gauss(order + 1)
    unx = np.zeros((order + 1, ny, nx + 1))
    uny = np.zeros((order + 1, ny + 1, nx))
    for g in range(order + 1):
        for a in range(3):
            unx[g] += lagrange(a, s[g]) * u[a:a + 2 * ny:2, ::2]  # the nodes (2 iy + a, 2 ex) of the x-edge (iy, ex)
            uny[g] += lagrange(a, s[g]) * v[::2, a:a + 2 * nx:2]  # the nodes (2 ey, 2 ix + a) of the y-edge (ey, ix)
    return project(u), project(v), unx, uny


# ------------------------------------------------------------------------------------------------ the operator
def _neighbour(F, dx, dy):
    """G[:, iy, ix] = F[:, iy + dy, ix + dx], a zero field outside the array (nothing flows in)"""
    _, ny, nx = F.shape
    G = np.zeros_like(F)
    ys, yd = (slice(dy, ny), slice(0, ny - dy)) if dy >= 0 else (slice(0, ny + dy), slice(-dy, ny))
    xs, xd = (slice(dx, nx), slice(0, nx - dx)) if dx >= 0 else (slice(0, nx + dx), slice(-dx, nx))
    G[:, yd, xd] = F[:, ys, xs]
    return G


def L(phi, adv, hx, hy, order):
    """d phi / dt of the upwind DG scheme: M^-1 [ int phi v . grad psi_i  -  sum over the edges int (v.n) phi^up psi_i ]"""
    vx, vy, unx, uny = adv
    x, y, w = tensor_rule(5)
    f = evaluate(phi, order, x, y)
    fx, fy = f * evaluate(vx, order, x, y), f * evaluate(vy, order, x, y)
    rhs = (np.tensordot(basis_dx(order, x, y) * w, fx, axes=1) / hx + np.tensordot(basis_dy(order, x, y) * w, fy, axes=1) / hy)
    s, ws = gauss(order + 1)
    for g in range(order + 1):
        t = s[g]
        # outward normal velocity, own point, the neighbour across the edge and its point, the mesh width along the normal
        for vn, own, (dx, dy), other, h in (
                (unx[g][:, 1:], (0.5, t), (1, 0), (-0.5, t), hx),
                (-unx[g][:, :-1], (-0.5, t), (-1, 0), (0.5, t), hx),
                (uny[g][1:, :], (t, 0.5), (0, 1), (t, -0.5), hy),
                (-uny[g][:-1, :], (t, -0.5), (0, -1), (t, 0.5), hy)):
            inner = evaluate(phi, order, *own)[0]
            outer = evaluate(_neighbour(phi, dx, dy), order, *other)[0]
            up = np.where(vn >= 0.0, inner, outer)
            rhs -= (ws[g] / h) * basis(order, *own)[:, 0][:, None, None] * (vn * up)[None]
    return np.tensordot(mass_inverse(order), rhs, axes=1)


def stage(phi0, phis, adv, hx, hy, dt, a, b, order):
    """one stage in the form of the bare-stage entry point: a phi0 + b (phis + dt L(phis))"""
    return a * phi0 + b * (phis + dt * L(phis, adv, hx, hy, order))


def step(phi, adv, hx, hy, dt, order):
    """one step of the SSP Runge-Kutta scheme of order + 1 stages in Butcher form: Euler, Heun, the third-order scheme of Shu and Osher"""
    k1 = L(phi, adv, hx, hy, order)
    if order == 0:
        return phi + dt * k1
    k2 = L(phi + dt * k1, adv, hx, hy, order)
    if order == 1:
        return phi + 0.5 * dt * (k1 + k2)
    k3 = L(phi + 0.25 * dt * (k1 + k2), adv, hx, hy, order)
    return phi + dt * (k1 / 6.0 + k2 / 6.0 + 2.0 * k3 / 3.0)


# ------------------------------------------------------------------------------------------------ the closure
def limit_points(order):
    """where the closure looks: the (p+1)^2 volume Gauss points, the p+1 Gauss points of each of the four edges, the four corners"""
    g, _ = gauss(order + 1)
    pts = [(a, b) for b in g for a in g]
    pts += [(0.5, t) for t in g] + [(-0.5, t) for t in g] + [(t, 0.5) for t in g] + [(t, -0.5) for t in g]
    pts += [(a, b) for b in (-0.5, 0.5) for a in (-0.5, 0.5)]
    return pts


def limit(F, lo, hi, cap, order):
    """DESIGN.md section 3.3, returns a new array: a cell mean above hi becomes hi (cap), then the higher coefficients are scaled by the
    largest theta <= 1 that keeps every point of limit_points() inside [lo, hi].  Order 0 has only the cap"""
    out = np.array(F, dtype=float, copy=True)
    if cap:
        out[0] = np.minimum(out[0], hi)
    if order == 0:
        return out
    mean = out[0]
    theta = np.ones_like(mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        for (x, y) in limit_points(order):
            dev = evaluate(out, order, x, y)[0] - mean  # what theta scales
            below, above = mean + dev < lo, mean + dev > hi
            theta = np.where(below, np.minimum(theta, np.where(mean > lo, (mean - lo) / -dev, 0.0)), theta)
            theta = np.where(above, np.minimum(theta, np.where(mean < hi, (hi - mean) / dev, 0.0)), theta)
    out[1:] *= theta
    return out


# ------------------------------------------------------------------------------------------------ a step on a row range
def step_rows(phi, adv, hx, hy, dt, order, j0, j1, out, closure=None):
    """a step (and its closure (lo, hi, cap), if one is given) whose result is defined on the rows [j0, j1) only: returns a copy of `out`
    with those rows replaced; the rows outside keep the caller's values.  The rows are advanced on the window [j0 - S, j1 + S) of the
    array, S = order + 1 the number of stages: every stage carries the false 'nothing flows in' of a cut one row further into the
    window, so after S stages exactly the S ghost rows are wrong and the rows [j0, j1) are the step of the whole array"""
    vx, vy, unx, uny = adv
    ny = phi.shape[1]
    S = order + 1
    r0, r1 = max(j0 - S, 0), min(j1 + S, ny)
    window = (vx[:, r0:r1], vy[:, r0:r1], unx[:, r0:r1], uny[:, r0:r1 + 1])
    new = step(phi[:, r0:r1], window, hx, hy, dt, order)
    if closure is not None:
        new = limit(new, closure[0], closure[1], closure[2], order)
    res = np.array(out, dtype=float, copy=True)
    res[:, j0:j1] = new[:, j0 - r0:j1 - r0]
    return res

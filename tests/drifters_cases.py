"""The inputs the drifter kernel is held to its reference on, shared by tests/test_drifters_cpu.py (float64 against longdouble reference) and
tests/test_gpu_drifters.py (device against float64 reference): random velocity fields with |u| dt up to 0.9 h, random concentrations and land,
and drifters seeded where an index or a clamp can go wrong."""
import numpy as np

import drifters_ref as R

BLOCK = 256  # abi.DRIFTERS_BLOCK, the lanes per workgroup of the launch (asserted equal in the GPU test)
# (nx, ny, n): the large grid at every count around the block size; the small grids make the clamps and the min / max of the neighbourhood
# degenerate
CASES = [(70, 9, 1), (70, 9, BLOCK - 1), (70, 9, BLOCK), (70, 9, BLOCK + 1), (70, 9, 1000), (1, 1, 257), (3, 1, 257), (1, 3, 257)]
HX, HY, DT, MIN_CONC = 1000.0, 800.0, 120.0, 0.15


def make(nx, ny, n, seed=0):
    """dict(u, v [2 ny + 1, 2 nx + 1]; A0 [ny, nx]; land [ny, nx] uint8; d [3, n]; hx, hy, dt, min_conc)"""
    rng = np.random.default_rng(1000 * nx + 10 * ny + n + seed)
    Lx, Ly = nx * HX, ny * HY
    u = rng.uniform(-0.9, 0.9, (2 * ny + 1, 2 * nx + 1)) * HX / DT
    v = rng.uniform(-0.9, 0.9, (2 * ny + 1, 2 * nx + 1)) * HY / DT
    A0 = rng.random((ny, nx))
    land = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    if nx * ny <= 3:  # something must move on the small grids
        land[:] = 0
        A0[0, 0] = 0.9
    x, y = rng.uniform(0, Lx, n), rng.uniform(0, Ly, n)
    kind = rng.integers(0, 10, n)
    ex, ey = rng.integers(0, nx + 1, n) * HX, rng.integers(0, ny + 1, n) * HY
    x = np.where((kind == 1) | (kind == 3), ex, x)  # on a vertical element edge (the domain's own among them)
    y = np.where((kind == 2) | (kind == 3), ey, y)  # on a horizontal edge; kind 3: on a corner
    x = np.where(kind == 4, Lx, np.where(kind == 5, 0.0, x))  # on the domain edge
    y = np.where(kind == 6, Ly, np.where(kind == 7, 0.0, y))
    for target, k in ((land != 0, 8), ((A0 < MIN_CONC) & (land == 0), 9)):  # inside a land element / an ice-free element
        cells = np.argwhere(target)
        for i in np.flatnonzero(kind == k):
            if len(cells):
                iy, ix = cells[rng.integers(len(cells))]
                x[i], y[i] = (ix + rng.random()) * HX, (iy + rng.random()) * HY
    if n == 1:
        x[0], y[0] = 0.37 * Lx, 0.61 * Ly
        A0[R.locate(y[0], HY, ny), R.locate(x[0], HX, nx)] = 0.8
        land[R.locate(y[0], HY, ny), R.locate(x[0], HX, nx)] = 0
    status = np.where(rng.random(n) < 0.1, rng.integers(1, 4, n), 0).astype(np.float64) if n > 1 else np.zeros(1)
    return dict(u=u, v=v, A0=A0, land=land, d=np.stack([x, y, status]), hx=HX, hy=HY, dt=DT, min_conc=MIN_CONC)


def reference(c, dtype=np.float64, **kw):
    return R.advance(c["u"], c["v"], c["A0"], c["d"], c["hx"], c["hy"], c["dt"], c["min_conc"], land=c["land"], dtype=dtype, **kw)


def rotation(nx=70, ny=9, h=1000.0, theta=0.05, dt=100.0, centre=(6.3, 4.4), radius=3.0):
    """solid-body rotation u = -w (y - yc), v = w (x - xc) by its nodal values, which CG2 reproduces exactly; w dt = theta.  Returns
    (u, v, h, dt, (xc, yc), r0)"""
    w = theta / dt
    xc, yc = centre[0] * h, centre[1] * h
    X, Y = np.meshgrid(np.arange(2 * nx + 1) * (h / 2), np.arange(2 * ny + 1) * (h / 2))
    return -w * (Y - yc), w * (X - xc), h, dt, (xc, yc), radius * h


def rotation_check(x, y, x0, y0, centre, theta, nsteps):
    """Heun on a linear field: z' = z (1 - theta^2 / 2 + i theta) about the centre.  Returns the relative errors of r_n / r_0 against
    (1 + theta^4 / 4)^(n / 2) and of the angle against n atan2(theta, 1 - theta^2 / 2)"""
    z0 = complex(x0 - centre[0], y0 - centre[1])
    z = complex(x - centre[0], y - centre[1])
    ratio = abs(z) / abs(z0)
    want = (1 + theta ** 4 / 4) ** (nsteps / 2)
    turn = nsteps * np.arctan2(theta, 1 - theta * theta / 2)
    dphi = np.angle(z / z0 * np.exp(-1j * turn))  # what is left after the expected turn is taken out
    return abs(ratio / want - 1), abs(dphi) / turn

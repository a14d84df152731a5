"""The inputs the point-sample kernel is held to its reference on, stated once for tests/test_points_cpu.py (float64 against longdouble
reference) and tests/test_gpu_points.py (device against float64 reference): random DG fields, velocities and stresses on grids around the
64-lane tile seams of the stress, and points seeded where an index or a weight can go wrong."""
import numpy as np

import points_ref as R

BLOCK = 256  # abi.POINTS_BLOCK, the lanes per workgroup of the launch (asserted equal in the GPU test)
HX, HY = 1000.0, 800.0  # hx != hy; both make the element centres (i + 1/2) h and their quotients by h exact
# (nx, ny, n, order, rheology): every grid of the tile seams (one tile less one, one tile, one more, two and a partial third) and the one-row
# and one-column arrays with n straddling the block; 70 x 9 at every count around the block size, every order and both rheologies
GRIDS = [(nx, ny) for nx in (1, 63, 64, 65, 130) for ny in (1, 3)]
CASES = [(nx, ny, BLOCK + 1, 2, ("mevp", "bbm")[k % 2]) for k, (nx, ny) in enumerate(GRIDS)]
CASES += [(70, 9, n, 2, "bbm") for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 1000)]
CASES += [(70, 9, 1000, 2, "mevp"), (70, 9, 1000, 1, "mevp"), (70, 9, 1000, 0, "bbm"), (65, 3, BLOCK, 1, "bbm"), (64, 1, BLOCK, 0, "mevp")]


def fields_of(rheology):
    """every field the rheology has: the mEVP sub-cycle carries no damage"""
    return tuple(f for f in R.FIELDS if f != "damage" or rheology == "bbm")


def tile(planes):
    """coefficient planes [8, ny, nx] -> the tiled array of include/nsdg.h "Data layout", the lanes no element owns left NaN"""
    nc, ny, nx = planes.shape
    ntx = -(-nx // 64)
    a = np.full(ny * ntx * nc * 64, np.nan)
    for c in range(nc):
        for iy in range(ny):
            ix = np.arange(nx)
            a[((iy * ntx + ix // 64) * nc) * 64 + (c // 2) * 128 + 2 * (ix % 64) + c % 2] = planes[c, iy]
    return a


def points(nx, ny, n, rng):
    """x, y [n]: random, on element centres, on element edges and corners, on the four edges and corners of the domain"""
    Lx, Ly = nx * HX, ny * HY
    x, y = rng.uniform(0, Lx, n), rng.uniform(0, Ly, n)
    kind = rng.integers(0, 12, n)
    cx, cy = (rng.integers(0, nx, n) + 0.5) * HX, (rng.integers(0, ny, n) + 0.5) * HY
    ex, ey = rng.integers(0, nx + 1, n) * HX, rng.integers(0, ny + 1, n) * HY
    x = np.where(kind == 1, cx, x)  # an element centre
    y = np.where(kind == 1, cy, y)
    x = np.where((kind == 2) | (kind == 4), ex, x)  # on a vertical element edge (the domain's own among them)
    y = np.where((kind == 3) | (kind == 4), ey, y)  # on a horizontal edge; kind 4: on a corner
    x = np.where(kind == 5, Lx, np.where(kind == 6, 0.0, x))  # on the domain's edges
    y = np.where(kind == 7, Ly, np.where(kind == 8, 0.0, y))
    corner = kind == 9  # the domain's corners
    x = np.where(corner, np.where(rng.random(n) < 0.5, 0.0, Lx), x)
    y = np.where(corner, np.where(rng.random(n) < 0.5, 0.0, Ly), y)
    if n >= 16:  # every special position is there whatever the draw
        x[:8] = [Lx, Lx, 0.0, 0.0, Lx, 0.5 * HX, (nx - 0.5) * HX, 0.0]
        y[:8] = [Ly, 0.0, Ly, 0.0, 0.5 * HY, Ly, (ny - 0.5) * HY, (ny - 0.5) * HY]
    return x, y


def make(nx, ny, n, order=2, rheology="bbm", seed=0):
    """dict(nx, ny, hx, hy, order, fields, x, y [n], src): src holds H, A (and D under "bbm") [nc(order), ny, nx], u, v [2 ny + 1, 2 nx + 1],
    s11, s12, s22 tiled (and planes s11p ... [8, ny, nx]), hsnow, tice [ny, nx]"""
    rng = np.random.default_rng(100000 * nx + 1000 * ny + 10 * n + order + seed + (7 if rheology == "bbm" else 0))
    nc = R.NC[order]
    dgf = lambda mean, spread: np.concatenate([rng.uniform(0, mean, (1, ny, nx)), spread * rng.standard_normal((nc - 1, ny, nx))])
    src = {"H": dgf(3.0, 0.3), "A": dgf(1.0, 0.1)}
    if rheology == "bbm":
        src["D"] = dgf(1.0, 0.1)
    src["u"] = rng.uniform(-0.5, 0.5, (2 * ny + 1, 2 * nx + 1))
    src["v"] = rng.uniform(-0.5, 0.5, (2 * ny + 1, 2 * nx + 1))
    scale = 2.0e3 if rheology == "bbm" else 1.5e4  # Pa of the brittle sub-cycle, N/m of mEVP
    for name in ("s11", "s12", "s22"):
        planes = scale * rng.standard_normal((8, ny, nx))
        src[name + "p"], src[name] = planes, tile(planes)
    src["hsnow"], src["tice"] = rng.uniform(0, 0.4, (ny, nx)), rng.uniform(-30, 0, (ny, nx))
    x, y = points(nx, ny, n, rng)
    return dict(nx=nx, ny=ny, hx=HX, hy=HY, order=order, rheology=rheology, fields=fields_of(rheology), x=x, y=y, src=src)


def reference(c, fields=None, dtype=np.float64, rows=None, **kw):
    """(values, M) of case c; rows = (lo, hi): the local array of those rows placed in the domain (row0 = lo, ny_global = ny)"""
    src, ny = c["src"], c["ny"]
    if rows is not None:
        lo, hi = rows
        src = local_sources(c, lo, hi)
        kw.update(row0=lo, ny_global=c["ny"])
        ny = hi - lo
    return R.sample(fields or c["fields"], c["x"], c["y"], c["nx"], ny, c["hx"], c["hy"], c["order"], src, dtype=dtype, **kw)


def local_sources(c, lo, hi):
    """the sources of the element rows [lo, hi) of case c as a local array of their own"""
    out = {}
    for k, a in c["src"].items():
        if k in ("u", "v"):
            out[k] = a[2 * lo:2 * hi + 1].copy()
        elif k in ("s11", "s12", "s22"):
            out[k] = tile(c["src"][k + "p"][:, lo:hi])
        elif k in ("hsnow", "tice"):
            out[k] = a[lo:hi].copy()
        else:
            out[k] = a[:, lo:hi].copy()
    return out

"""Inputs of the symmetry tests (tests/test_symmetry_cpu.py, tests/test_gpu_symmetry.py): rough random states on small grids, built
from numpy.random.default_rng with the seeds below.  numpy only.

The states are deliberately rough: noise in every DG coefficient, ice-free elements on both sides of a window seam, a tile seam and a
strip seam of the marching kernels in both orientations, a land mask that no element of the symmetry group maps onto itself, hx != hy
and fc != 0.  image(case, M) is the same problem seen through the map M of tests/symmetry_maps.py.

Mesh widths are fixed (not a fixed domain divided by the grid): with HX x HY = 1000 m x 1300 m, velocities of 1e-3 m/s per node and
P* h exp(-20 (1 - A)) between 70 Pa m and 5e4 Pa m the adaptive alpha_e = sqrt(c zeta dt / (rho h hx hy)) lies between its floor of 50
and several hundred on every grid, the 7 x 5 one included."""
import numpy as np

HX, HY = 1000.0, 1300.0
DT = 120.0
AD = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=50.0)
UNIFORM = dict(alpha=300.0, beta=300.0)
FORMS = {"uniform": UNIFORM, "adaptive": AD}
SPEED = {"uniform": 0.05, "adaptive": 1e-3}
FC = 1.46e-4

MEVP_GRIDS = ((130, 23), (58, 13), (7, 5))  # (nx, ny); the transposes are their images under T
TRANSPORT_GRIDS = MEVP_GRIDS + ((2, 3), (1, 7))
# the seeds the cases were accepted with (tests/test_symmetry_cpu.py holds the conditions: decision masks map exactly, every threshold
# decision >= 1e-6 relative from its threshold in every orientation, alpha_e spread by more than a factor 2 in the adaptive cases)
SEEDS = dict(mevp=20261, transport=20269, bbm=20263, history=20264, coupled=20265)

H_A_BOUNDS = ((0.0, float("inf"), False), (0.0, 1.0, True))
BOUNDS4 = H_A_BOUNDS + H_A_BOUNDS


def land_mask(nx, ny):
    """an island, a peninsula from the left side and one from the bottom side, and a block on the top side cut by a one-element channel;
    scaled to the array.  No element of the symmetry group maps it onto itself (asserted in tests/test_symmetry_cpu.py)"""
    m = np.zeros((ny, nx), dtype=bool)
    if nx < 5 or ny < 5:
        return m
    m[ny // 2:ny // 2 + max(ny // 8, 1), (2 * nx) // 3:(2 * nx) // 3 + max(nx // 10, 1)] = True  # island
    m[(3 * ny) // 5:(3 * ny) // 5 + max(ny // 10, 1), 0:max(nx // 5, 1)] = True  # peninsula from the left side
    m[0:max(ny // 3, 1), nx // 3:nx // 3 + max(nx // 16, 1)] = True  # peninsula from the bottom side
    c0, w = nx // 2, max(nx // 20, 1)
    m[ny - max(ny // 5, 1):, c0 - w:c0 + w + 1] = True  # a block on the top side ...
    m[ny - max(ny // 5, 1):, c0] = False  # ... with a one-element channel through it
    return m


def land_nodes(land):
    ny, nx = land.shape
    out = np.zeros((2 * ny + 1, 2 * nx + 1), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out[dy:dy + 2 * ny:2, dx:dx + 2 * nx:2] |= land
    return out


def ice_free_elements(nx, ny):
    """(iy, ix) of the ice-free elements: 2 x 2 blocks (their shared corner node is ice-free too) and single elements on both sides of the
    window seam at column 57, the tile seams at 64 and 128, the strip seam at row 5, and of the same seams of the transposed array
    (its columns are these rows, its strip seams at these columns 5, 10, 15 ...)"""
    want = [(4, 56), (4, 57), (5, 56), (5, 57),  # window seam x strip seam
            (9, 63), (10, 64), (4, 4), (5, 5), (4, 5), (14, 113), (15, 114), (9, 127), (10, 128), (2, 9), (2, 10),
            (ny // 2, nx // 2), (1, 1)]
    return sorted({(iy, ix) for iy, ix in want if iy < ny and ix < nx})


def _zero_rim(a):
    a[0] = a[-1] = 0.0
    a[:, 0] = a[:, -1] = 0.0
    return a


def mevp_case(nx, ny, form, land=False, seed=None):
    """the inputs of mEVP sub-iterations on the nx x ny grid: dict(nx, ny, hx, hy, dt, form, params, H, A, u, v, u0, v0, s, ua, va, uo,
    vo, land)"""
    rng = np.random.default_rng([SEEDS["mevp"] if seed is None else seed, nx, ny])
    shape = (2 * ny + 1, 2 * nx + 1)
    H = 0.03 * rng.standard_normal((6, ny, nx))
    A = 0.003 * rng.standard_normal((6, ny, nx))
    H[0] = rng.uniform(0.5, 2.0, (ny, nx))
    A[0] = rng.uniform(0.7, 0.99, (ny, nx))
    for iy, ix in ice_free_elements(nx, ny):
        H[:, iy, ix], A[:, iy, ix] = 0.0, 0.0
        H[0, iy, ix], A[0, iy, ix] = 1e-3, 1e-14
    sp = SPEED[form]
    u, v = _zero_rim(sp * rng.standard_normal(shape)), _zero_rim(sp * rng.standard_normal(shape))
    u0, v0 = _zero_rim(u + 0.1 * sp * rng.standard_normal(shape)), _zero_rim(v + 0.1 * sp * rng.standard_normal(shape))
    s = [1e3 * rng.standard_normal((8, ny, nx)) for _ in range(3)]
    ua, va = 8.0 * rng.standard_normal(shape), 8.0 * rng.standard_normal(shape)
    uo, vo = 0.05 * rng.standard_normal(shape), 0.05 * rng.standard_normal(shape)
    mask = land_mask(nx, ny) if land else None
    if mask is not None:  # no ice, no stress, no motion on land
        ln = land_nodes(mask)
        for f in [H, A] + s:
            f[:, mask] = 0.0
        for f in (u, v, u0, v0):
            f[ln] = 0.0
    return dict(nx=nx, ny=ny, hx=HX, hy=HY, dt=DT, form=form, params=dict(FORMS[form], fc=FC), H=H, A=A, u=u, v=v, u0=u0, v0=v0, s=s,
                ua=ua, va=va, uo=uo, vo=vo, land=mask)


STATE_KEYS = ("H", "A", "D", "u", "v", "u0", "v0", "s", "ua", "va", "uo", "vo", "land")


def image(case, M):
    """the case seen through the map M: every array mapped by its kind, fc with its sign, hx and hy swapped under T"""
    out = dict(case)
    out.update(M.state({k: case[k] for k in STATE_KEYS if case.get(k) is not None}))
    out["nx"], out["ny"], out["hx"], out["hy"] = M.grid(case["nx"], case["ny"], case["hx"], case["hy"])
    if "params" in case:
        out["params"] = M.params(case["params"])
    if "fields" in case:
        out["fields"] = [M.dg(f) for f in case["fields"]]
    if "hsnow" in case:
        out["hsnow"], out["tice"] = M.elem(case["hsnow"]), M.elem(case["tice"])
    return out


# ------------------------------------------------------------------------------------------------ transport
NCOEF = {0: 1, 1: 3, 2: 6}
TRANSPORT_HX, TRANSPORT_HY = 700.0, 900.0
CFL = 0.05


def transport_case(nx, ny, order, nfields=2, seed=None):
    """velocity random at every node with inflow and outflow on all four sides, nfields fields with cell means in [0.6, 1.1] and slopes
    of 0.2 under the bounds BOUNDS4[:nfields]: the cap and the limiter of the concentration-like fields both act"""
    rng = np.random.default_rng([SEEDS["transport"] if seed is None else seed, nx, ny, order])
    shape = (2 * ny + 1, 2 * nx + 1)
    u, v = 0.3 * rng.standard_normal(shape), 0.3 * rng.standard_normal(shape)
    for side in (u[:, 0], u[:, -1], v[0, :], v[-1, :]):  # the normal component on each side: both signs
        side[0], side[-1] = abs(side[0]) + 0.05, -abs(side[-1]) - 0.05
    nc = NCOEF[order]
    fields = []
    for f in range(4):
        F = 0.2 * rng.uniform(-1.0, 1.0, (nc, ny, nx))
        F[0] = rng.uniform(0.6, 1.1, (ny, nx))
        fields.append(F)
    dt = CFL * min(TRANSPORT_HX, TRANSPORT_HY) / max(np.abs(u).max(), np.abs(v).max())
    return dict(nx=nx, ny=ny, hx=TRANSPORT_HX, hy=TRANSPORT_HY, dt=dt, order=order, u=u, v=v, fields=fields[:nfields], bounds=BOUNDS4[:nfields])


_G = {1: np.array([0.0]), 2: np.array([-0.5, 0.5]) / np.sqrt(3.0), 3: np.array([-0.5, 0.0, 0.5]) * np.sqrt(0.6)}
_PSI = (lambda x, y: 1.0 + 0 * x, lambda x, y: x, lambda x, y: y, lambda x, y: x * x - 1.0 / 12, lambda x, y: y * y - 1.0 / 12, lambda x, y: x * y)


def closure_decisions(phi, order, lo, hi, cap):
    """what the closure decides for a field before it acts, and how far each decision is from its threshold: (capped [ny, nx],
    limited [ny, nx], margin) -- margin = the smallest relative distance |value - threshold| / max(|threshold|, 1) over the cell means
    (cap) and the extreme point values (limiter) of every element"""
    mean = phi[0].copy()
    capped = (mean > hi) if cap else np.zeros(mean.shape, dtype=bool)
    margin = float(np.min(np.abs(mean - hi))) / max(abs(hi), 1.0) if (cap and np.isfinite(hi)) else np.inf
    mean = np.where(capped, hi, mean)
    if order == 0:
        return capped, np.zeros(mean.shape, dtype=bool), margin
    g = _G[order + 1]
    pts = [(x, y) for y in g for x in g] + [(e, t) for t in g for e in (-0.5, 0.5)] + [(t, e) for t in g for e in (-0.5, 0.5)]
    pts += [(x, y) for x in (-0.5, 0.5) for y in (-0.5, 0.5)]
    vals = np.array([mean + sum(phi[c] * _PSI[c](x, y) for c in range(1, phi.shape[0])) for x, y in pts])
    mn, mx = vals.min(axis=0), vals.max(axis=0)
    limited = (mn < lo) | (mx > hi)
    margin = min(margin, float(np.min(np.abs(mn - lo))) / max(abs(lo), 1.0))
    if np.isfinite(hi):
        margin = min(margin, float(np.min(np.abs(mx - hi))) / max(abs(hi), 1.0))
    return capped, limited, margin


# ------------------------------------------------------------------------------------------------ brittle rheology, history, coupled steps
def bbm_case(nx, ny, seed=None):
    """one BBM sub-iteration: the fields of tests/bbm_cases.random_case (|sigma_n| >= 1.5e3 Pa with both signs, far from -N; damage cell
    means in [0.05, 0.85], inside (0, d_max)) on a mesh with hx != hy"""
    from bbm_cases import random_case

    c = random_case(nx, ny, seed=SEEDS["bbm"] if seed is None else seed)
    c = {("s" if k == "S" else k): v for k, v in c.items()}
    c.update(hx=HX, hy=HY, dts=1.0, params=dict(fc=FC))
    return c


def history_case(nx, ny, seed=None):
    """the sources of one history sample of every field: the rough mEVP state plus snow, surface temperature and damage"""
    c = mevp_case(nx, ny, "uniform", seed=SEEDS["history"] if seed is None else seed)
    rng = np.random.default_rng([SEEDS["history"], 7])
    c["hsnow"], c["tice"] = rng.uniform(0.0, 0.3, (ny, nx)), rng.uniform(-20.0, -1.0, (ny, nx))
    c["D"] = 0.01 * rng.standard_normal((6, ny, nx))
    c["D"][0] = rng.uniform(0.0, 0.9, (ny, nx))
    return c


def coupled_case(nx, ny, seed=None):
    """three coupled model steps (sub-cycle + transport with the closure): moderate fields under a strong wind, land mask, adaptive form"""
    rng = np.random.default_rng([SEEDS["coupled"] if seed is None else seed, nx, ny])
    shape = (2 * ny + 1, 2 * nx + 1)
    H = 0.02 * rng.standard_normal((6, ny, nx))
    A = 0.01 * rng.standard_normal((6, ny, nx))
    H[0], A[0] = rng.uniform(0.5, 1.5, (ny, nx)), rng.uniform(0.8, 0.99, (ny, nx))
    y, x = np.meshgrid(np.linspace(0, 1, shape[0]), np.linspace(0, 1, shape[1]), indexing="ij")
    ua = 12.0 * np.sin(2.3 * x + 0.4) * np.cos(1.7 * y) + rng.standard_normal(shape)
    va = 9.0 * np.cos(1.9 * x) * np.sin(2.9 * y + 0.3) + rng.standard_normal(shape)
    uo, vo = 0.05 * rng.standard_normal(shape), 0.05 * rng.standard_normal(shape)
    return dict(nx=nx, ny=ny, hx=4000.0, hy=5000.0, dt=DT, nsub=24, params=dict(AD, fc=FC), H=H, A=A, ua=ua, va=va, uo=uo, vo=vo, land=land_mask(nx, ny))

"""Independent numpy statement of the history samples (include/nsdg.h "history output"), and the CPU stand-in of
nsdg_history_accumulate for the multi-rank CPU tests: HistoryOps wraps tests/oracle_ops.py, which stays as it is.

Everything here works on whole arrays with strided slices of the CG2 lattice -- no element loop, no index arithmetic shared with
csrc/history.hip."""
import numpy as np

from oracle_ops import OracleOps

FIELDS = ("hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s", "hsnow", "tice", "damage")
COPY_FIELDS = ("hice", "cice", "u", "v", "hsnow", "tice", "damage")  # a sample is a source value: bit for bit on any machine
EXACT_FIELDS = COPY_FIELDS + ("sigma_n",)  # (a + b) / 2: one rounding, the same everywhere
EPS = 2.0 ** -53


def plane0(f):
    """the cell mean of a DG field given as coefficient planes [nc, ny, nx], or the plane itself"""
    f = np.asarray(f)
    return f[0] if f.ndim == 3 else f


def centre(u):
    """a nodal field [2 ny + 1, 2 nx + 1] at the centre nodes of the elements"""
    return u[1::2, 1::2]


def strain_rates(u, v, hx, hy):
    """(e11, e22, g) at the element centres from the mid-edge nodes: E / W = (2 iy + 1, 2 ix + 2) / (2 iy + 1, 2 ix), N / S = (2 iy + 2,
    2 ix + 1) / (2 iy, 2 ix + 1) -- the exact derivatives of the biquadratic velocity there"""
    uE, uW, vE, vW = u[1::2, 2::2], u[1::2, 0:-1:2], v[1::2, 2::2], v[1::2, 0:-1:2]
    uN, uS, vN, vS = u[2::2, 1::2], u[0:-1:2, 1::2], v[2::2, 1::2], v[0:-1:2, 1::2]
    return (uE - uW) / hx, (vN - vS) / hy, (uN - uS) / hy + (vE - vW) / hx


def sample(name, hx, hy, H=None, A=None, u=None, v=None, s11=None, s12=None, s22=None, hsnow=None, tice=None, D=None):
    """one field [ny, nx] of one state.  H, A, D: coefficient planes or the cell-mean plane; u, v: the CG2 lattice; s11, s12, s22:
    coefficient planes [8, ny, nx] or coefficient 0 alone; hsnow, tice: one plane"""
    if name == "hice":
        return plane0(H).copy()
    if name == "cice":
        return plane0(A).copy()
    if name == "hsnow":
        return np.array(hsnow, dtype=np.float64)
    if name == "tice":
        return np.array(tice, dtype=np.float64)
    if name == "damage":
        return plane0(D).copy()
    if name == "u":
        return centre(u).copy()
    if name == "v":
        return centre(v).copy()
    if name == "speed":
        return np.sqrt(centre(u) * centre(u) + centre(v) * centre(v))
    if name in ("divergence", "shear"):
        e11, e22, g = strain_rates(u, v, hx, hy)
        return e11 + e22 if name == "divergence" else np.sqrt((e11 - e22) ** 2 + g * g)
    if name == "sigma_n":
        return (plane0(s11) + plane0(s22)) / 2
    if name == "sigma_s":
        return np.sqrt((plane0(s11) - plane0(s22)) ** 2 / 4 + plane0(s12) ** 2)
    raise ValueError("unknown history field %r" % (name,))


def samples(fields, hx, hy, **src):
    return np.stack([sample(n, hx, hy, **src) for n in fields])


def accumulate(acc, x, j0, j1, store, row0=0):
    """acc[k, iy - row0] (store ? = : +=) x[k, iy] on the rows [j0, j1): the sequential sum per element"""
    rows = slice(j0 - row0, j1 - row0)
    if store:
        acc[:, rows] = x[:, j0:j1]
    else:
        acc[:, rows] = acc[:, rows] + x[:, j0:j1]


def rounding_scale(name, hx, hy, u=None, v=None, s11=None, s12=None, s22=None):
    """the size of the numbers a non-exact field is rounded at: a sample of it is within 16 * 2^-53 * scale of any other correct
    evaluation (under ten roundings, FMA contraction either way)"""
    if name in ("divergence", "shear"):
        return (np.max(np.abs(u)) + np.max(np.abs(v))) * (1.0 / hx + 1.0 / hy)
    if name == "sigma_s":
        return max(np.max(np.abs(plane0(s))) for s in (s11, s12, s22))
    if name == "speed":
        return np.max(np.hypot(centre(u), centre(v)))
    raise ValueError("%r is exact" % (name,))


class HistoryOps(OracleOps):
    """OracleOps and the history call of abi.Context, on CPU torch tensors (the oracle keeps the stress as coefficient planes)"""

    def history_accumulate(self, j0, j1, fields, sources, store, row0, acc):
        src = {k: t.numpy() for k, t in sources.items() if t is not None}
        accumulate(acc.numpy(), samples(fields, self.hx, self.hy, **src), j0, j1, store, row0)

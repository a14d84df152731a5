"""Independent numpy restatement of nsdg_points_sample, written from the text of include/nsdg.h "point samples" (not from csrc/points.hip),
by another route: the Lagrange weights and their derivatives by the product formula over the node positions, the DG basis from its
definition as a list of functions, the tiled address of a stress coefficient by its own index arithmetic.

dtype: the arithmetic of the samples.  np.float64: float64 operations only, every sum and product COMPENSATED (the class DD: a value is
an unevaluated sum hi + lo of two doubles, built with the error-free transformations TwoSum and Dekker's TwoProduct), and ONE rounding to
float64 at the end -- the reference is then within about one rounding of the exact sample wherever a long double is a double.
np.longdouble: the same expressions in the platform's extended precision, to measure the float64 route.  What the header states as
IEEE double operations is done in plain float64 whatever the dtype: the element of a coordinate (rule 1), and the local coordinates (rule
3) -- xi = x / hx - ix - 1/2 is ONE rounding, of the quotient (both subtractions are exact: they remove leading bits), and that rounding
moves the point by less than half an ulp of its own coordinate.  The sample is DEFINED at that float64 (xi, eta); the device and both
routes start from the same bits.

Besides every sample the reference returns M, the size of the numbers it is rounded at: the value of the same expression with every
coefficient, every source value and every monomial of a weight or basis function replaced by its absolute value (|L-| -> 2 t^2 + |t|,
|L0| -> 1 + 4 t^2, |xi^2 - 1/12| -> xi^2 + 1/12, ...), so cancellation inside a weight is covered.  A square root sqrt(a^2 + b^2) takes
M_a + M_b, by |d sqrt(a^2 + b^2)| <= |da| + |db|.  The bound of a comparison is K[field] * 2^-53 * M (K: tests/test_gpu_points.py derives it)."""
import numpy as np

FIELDS = ("hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s", "hsnow", "tice", "damage")
NODES = (-0.5, 0.0, 0.5)
TILE = 64
EPS = 2.0 ** -53
# the roundings on the longest path of the DEVICE's evaluation of a sample (tests/test_gpu_points.py: the derivation).  0: a copy, bit for bit
K = {"hice": 7, "cice": 7, "damage": 7, "u": 10, "v": 10, "speed": 12, "divergence": 11, "shear": 13, "sigma_n": 10, "sigma_s": 12, "hsnow": 0, "tice": 0}
NC = (1, 3, 6)


# ---------------------------------------------------------------------------------------------------- compensated float64 arithmetic
def _two_sum(a, b):
    """s + e = a + b exactly (Knuth)"""
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _two_prod(a, b):
    """p + e = a b exactly (Dekker, with Veltkamp's split at 27 bits; no overflow at the sizes of a sea-ice state)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class DD:
    """arrays of double-double numbers hi + lo, |lo| <= ulp(hi) / 2: about 106 bits from float64 operations alone.  A NaN or an infinity
    in hi makes the value NaN (the error terms are not finite then), which is all a sample of a NaN source has to be"""

    def __init__(self, hi, lo=None):
        self.hi = np.asarray(hi, dtype=np.float64)
        self.lo = np.zeros_like(self.hi) if lo is None else np.asarray(lo, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, DD) else DD(x)

    @staticmethod
    def _norm(s, e):
        hi = s + e
        return DD(hi, e - (hi - s))

    def __add__(self, o):
        o = DD.of(o)
        s, e = _two_sum(self.hi, o.hi)
        return DD._norm(s, e + (self.lo + o.lo))

    __radd__ = __add__

    def __neg__(self):
        return DD(-self.hi, -self.lo)

    def __sub__(self, o):
        return self + (-DD.of(o))

    def __rsub__(self, o):
        return DD.of(o) + (-self)

    def __mul__(self, o):
        o = DD.of(o)
        p, e = _two_prod(self.hi, o.hi)
        return DD._norm(p, e + (self.hi * o.lo + self.lo * o.hi))

    __rmul__ = __mul__

    def __truediv__(self, h):
        """by a plain double (a mesh width, a power of two)"""
        h = np.float64(h)
        q = self.hi / h
        p, e = _two_prod(q, h)
        return DD._norm(q, (((self.hi - p) - e) + self.lo) / h)

    def sqrt(self):
        s = np.sqrt(self.hi)
        p, e = _two_prod(s, s)
        safe = np.where(s > 0, s, 1.0)
        return DD._norm(s, np.where(s > 0, (((self.hi - p) - e) + self.lo) / (2.0 * safe), 0.0))

    def round(self):
        """the one rounding to float64"""
        return self.hi + self.lo


def _lift(a, dtype):
    """an array of source values or coordinates in the arithmetic of the route"""
    return DD(a) if dtype is np.float64 else np.asarray(a).astype(dtype)


def _sqrt(v):
    return v.sqrt() if isinstance(v, DD) else np.sqrt(v)


def locate(x, h, n):
    """rule 1 for an array of coordinates: min(n - 1, floor(x / h)) by IEEE double division, never below 0 (a NaN gives 0)"""
    f = np.floor(np.asarray(x, dtype=np.float64) / np.float64(h))
    return np.where(f > 0, np.minimum(f, n - 1), 0).astype(np.int64)


def lagrange(t, dtype):
    """L_k(t) = prod_{m != k} (t - t_m) / (t_k - t_m) and L_k'(t) = sum_{m != k} prod_{j != k, m} (t - t_j) / prod_{m != k} (t_k - t_m); the
    denominators are powers of two.  t: a value of the route (a float64 scalar or array is lifted)"""
    if not isinstance(t, DD):
        t = _lift(t, dtype)
    w, d = [], []
    for k, tk in enumerate(NODES):
        others = [np.float64(tm) for m, tm in enumerate(NODES) if m != k]
        den = (np.float64(tk) - others[0]) * (np.float64(tk) - others[1])
        w.append((t - others[0]) * (t - others[1]) / den)
        d.append(((t - others[0]) + (t - others[1])) / den)
    return w, d


def lagrange_sizes(t):
    """the sums of the absolute monomials of the weights 2 t^2 - t, 1 - 4 t^2, 2 t^2 + t and of their derivatives 4 t - 1, -8 t, 4 t + 1"""
    a = np.abs(t)
    return [2 * a * a + a, 1 + 4 * a * a, 2 * a * a + a], [4 * a + 1, 8 * a, 4 * a + 1]


def basis(xi64, eta64, dtype):
    """the eight functions of DESIGN.md section 3 at the float64 (xi, eta), in the arithmetic of the route, and the sums of their absolute
    monomials in float64"""
    xi, eta = _lift(xi64, dtype), _lift(eta64, dtype)
    c = _lift(np.ones_like(xi64), dtype) / 12.0 if dtype is np.float64 else dtype(1) / dtype(12)
    one = _lift(np.ones_like(xi64), dtype)
    val = [one, xi, eta, xi * xi - c, eta * eta - c, xi * eta, eta * (xi * xi - c), xi * (eta * eta - c)]
    ax, ay, c64 = np.abs(xi64), np.abs(eta64), 1.0 / 12.0
    size = [np.ones(xi64.shape), ax, ay, ax * ax + c64, ay * ay + c64, ax * ay, ay * (ax * ax + c64), ax * (ay * ay + c64)]
    return val, size


def tiled_coefficient(a, c, iy, ix, nx):
    """coefficient c of the elements (iy, ix) of a tiled 8-coefficient array: a[T + (c / 2) 128 + 2 l + c % 2], T = ((iy ntx + ix / 64) 8) 64"""
    ntx = -(-nx // TILE)
    tile, lane = ix // TILE, ix % TILE
    return np.asarray(a).reshape(-1)[((iy * ntx + tile) * 8) * TILE + (c // 2) * (2 * TILE) + 2 * lane + (c % 2)]


def sample(fields, x, y, nx, ny, hx, hy, order, src, row0=0, ny_global=None, j0=0, j1=None, dtype=np.float64, tiled=True):
    """one call of nsdg_points_sample on a local array of nx x ny elements.  x, y: [n]; src: H, A, D [nc, ny, nx]; u, v [2 ny + 1, 2 nx + 1];
    s11, s12, s22 tiled (flat) or, with tiled=False, coefficient planes [8, ny, nx]; hsnow, tice [ny, nx] -- of the LOCAL array, only what
    the fields read.  Returns (values, M), both [len(fields), n]: values in `dtype` with -inf where the launch does not own the point, M in
    float64 (0 there)"""
    ny_global = ny if ny_global is None else ny_global
    j1 = ny if j1 is None else j1
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    ix, iyg = locate(x, hx, nx), locate(y, hy, ny_global)
    iy = iyg - row0
    own = (iy >= j0) & (iy < j1)
    val = np.full((len(fields), n), -np.inf, dtype=dtype)
    M = np.zeros((len(fields), n))
    if not own.any():
        return val, M
    p = np.flatnonzero(own)
    ix, iy, iyg = ix[p], iy[p], iyg[p]
    xi64, eta64 = x[p] / np.float64(hx) - ix - 0.5, y[p] / np.float64(hy) - iyg - 0.5  # rule 3, in float64 by definition
    compensated = dtype is np.float64
    hxd, hyd = (np.float64(hx), np.float64(hy)) if compensated else (dtype(hx), dtype(hy))  # (DD divides by a plain double)
    zero = lambda: _lift(np.zeros(len(p)), dtype)
    bas, bas_size = basis(xi64, eta64, dtype)

    def dg(f):
        f = np.asarray(f)
        v, m = zero(), np.zeros(len(p))
        for c in range(NC[order]):
            coeff = f[c, iy, ix]
            v = v + _lift(coeff, dtype) * bas[c]
            m = m + np.abs(coeff) * bas_size[c]
        return v, m

    def stress(a):
        v, m = zero(), np.zeros(len(p))
        for c in range(8):
            coeff = tiled_coefficient(a, c, iy, ix, nx) if tiled else np.asarray(a)[c, iy, ix]
            v = v + _lift(coeff, dtype) * bas[c]
            m = m + np.abs(coeff) * bas_size[c]
        return v, m

    (lx, dlx), (ly, dly) = lagrange(xi64, dtype), lagrange(eta64, dtype)
    (sx, dsx), (sy, dsy) = lagrange_sizes(xi64), lagrange_sizes(eta64)

    def nodal(w, wy, wx, zy, zx):
        """sum_r wy_r sum_c wx_c w_rc over the 3 x 3 nodes of the element, and the same with the sizes zy, zx and |w|"""
        w = np.asarray(w)
        v, m = zero(), np.zeros(len(p))
        for r in range(3):
            for c in range(3):
                node = w[2 * iy + r, 2 * ix + c]
                v = v + wy[r] * wx[c] * _lift(node, dtype)
                m = m + zy[r] * zx[c] * np.abs(node)
        return v, m

    cache = {}

    def get(key):
        if key not in cache:
            if key in ("H", "A", "D"):
                cache[key] = dg(src[key])
            elif key in ("s11", "s12", "s22"):
                cache[key] = stress(src[key])
            elif key in ("u", "v"):
                cache[key] = nodal(src[key], ly, lx, sy, sx)
            elif key == "e11":
                v, m = nodal(src["u"], ly, dlx, sy, dsx)
                cache[key] = (v / hxd, m / hx)
            elif key == "e22":
                v, m = nodal(src["v"], dly, lx, dsy, sx)
                cache[key] = (v / hyd, m / hy)
            elif key == "g":
                (a, ma), (b, mb) = nodal(src["u"], dly, lx, dsy, sx), nodal(src["v"], ly, dlx, sy, dsx)
                cache[key] = (a / hyd + b / hxd, ma / hy + mb / hx)
        return cache[key]

    for k, name in enumerate(fields):
        if name in ("hice", "cice", "damage"):
            v, m = get({"hice": "H", "cice": "A", "damage": "D"}[name])
        elif name in ("hsnow", "tice"):
            v, m = _lift(np.asarray(src[name])[iy, ix], dtype), np.zeros(len(p))
        elif name in ("u", "v"):
            v, m = get(name)
        elif name == "speed":
            (a, ma), (b, mb) = get("u"), get("v")
            v, m = _sqrt(a * a + b * b), ma + mb
        elif name == "divergence":
            (a, ma), (b, mb) = get("e11"), get("e22")
            v, m = a + b, ma + mb
        elif name == "shear":
            (a, ma), (b, mb), (g, mg) = get("e11"), get("e22"), get("g")
            v, m = _sqrt((a - b) * (a - b) + g * g), ma + mb + mg
        elif name == "sigma_n":
            (a, ma), (b, mb) = get("s11"), get("s22")
            v, m = (a + b) / 2.0, (ma + mb) / 2
        elif name == "sigma_s":
            (a, ma), (b, mb), (s, ms) = get("s11"), get("s22"), get("s12")
            v, m = _sqrt((a - b) * (a - b) / 4.0 + s * s), (ma + mb) / 2 + ms
        else:
            raise ValueError("unknown field %r" % (name,))
        val[k, p], M[k, p] = (v.round() if isinstance(v, DD) else v), m
    return val, M


def bound(fields, M):
    """K * 2^-53 * M per sample: [len(fields), n]"""
    return np.array([K[f] for f in fields], dtype=np.float64)[:, None] * EPS * M


class PointsOps:
    """CPU ops with the point-sample call of abi.Context (and the drifter call, which the driver's drifter_fields needs) added to an ops object
    of tests/oracle_ops.py by composition: everything else is the inner object's.  The oracle keeps the stress as coefficient planes"""

    def __init__(self, inner):
        self.inner, self.row0, self.ny_glob = inner, 0, None

    def __getattr__(self, name):  # whatever this class does not define
        return getattr(self.inner, name)

    def set_block(self, row0, ny_global):
        self.row0, self.ny_glob = row0, ny_global
        if callable(getattr(self.inner, "set_block", None)):
            self.inner.set_block(row0, ny_global)

    def drifters_advance(self, j0, j1, dt, min_conc, u, v, A, d_in, d_out):
        import drifters_ref

        assert d_in.data_ptr() != d_out.data_ptr()
        d_out.numpy()[:] = drifters_ref.advance(u.numpy(), v.numpy(), A.numpy()[0], d_in.numpy(), self.inner.hx, self.inner.hy, dt, min_conc,
                                                row0=self.row0, ny_global=self.ny_glob, j0=j0, j1=j1)

    def points_sample(self, j0, j1, order, x, y, fields, sources, out):
        src = {k: t.numpy() for k, t in sources.items() if t is not None}
        val, _ = sample(tuple(fields), x.numpy(), y.numpy(), self.inner.nx, self.inner.ny, self.inner.hx, self.inner.hy, order, src, row0=self.row0, ny_global=self.ny_glob,
                        j0=j0, j1=j1, tiled=False)
        out.numpy()[:] = val

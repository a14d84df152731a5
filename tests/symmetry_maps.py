"""The symmetry group of the square acting on every array kind of the dynamics (numpy only; nothing of the package is imported).

Generators: T (x <-> y) and X (x -> L - x); Y (y -> L - y) is written out on its own and must equal T o X o T bit for bit
(tests/test_symmetry_cpu.py).  A map object answers, per array kind, "what does the mirrored / transposed problem hold where the
original holds a":

    node(a)            CG2 node array [2ny+1, 2nx+1] of a scalar
    vec(ax, ay)        pair of arrays of one kind (default: node arrays) holding a vector's x and y member
    dg(a)              DG coefficient planes [nc, ny, nx], nc in 1, 3, 6, 8
    stress(s11, s12, s22)  three 8-coefficient plane sets of the symmetric tensor
    gauss(a)           [9, ny, nx] values at the 3 x 3 Gauss points, q = 3 qy + qx
    elem(a)            [..., ny, nx] scalars per element (land mask, decision masks, history samples, alpha_e)
    edges(unx, uny)    the edge-normal velocities un_x [ng, ny, nx+1], un_y [ng, ny+1, nx] (Gauss index along the edge)
    params(d)          dict of scalar parameters: fc changes sign under every reflection, T swaps hx and hy
    grid(nx, ny, hx, hy)

Every map is an involution.  The keyword arguments of Map() switch single ingredients off: the sensitivity tests need maps that are
wrong in exactly one place."""
import numpy as np

# T on the coefficients: psi = 1, x, y, x^2 - 1/12, y^2 - 1/12, x y, (x^2 - 1/12) y, x (y^2 - 1/12)  (and the first 6, 3, 1 of them)
T_PERM = {8: [0, 2, 1, 4, 3, 5, 7, 6], 6: [0, 2, 1, 4, 3, 5], 3: [0, 2, 1], 1: [0]}
X_ODD = {8: [1, 5, 7], 6: [1, 5], 3: [1], 1: []}  # coefficients odd in xi
Y_ODD = {8: [2, 5, 6], 6: [2, 5], 3: [2], 1: []}  # coefficients odd in eta
VECTOR_PAIRS = (("u", "v"), ("u0", "v0"), ("ua", "va"), ("uo", "vo"), ("tax", "tay"))
KINDS = ("T", "X", "Y")


def _c(a):
    return np.ascontiguousarray(a)


class Map:
    def __init__(self, kind, fc_sign=True, permute8=True, s12_sign=True):
        assert kind in KINDS
        self.kind, self.fc_sign, self.permute8, self.s12_sign = kind, fc_sign, permute8, s12_sign

    def __repr__(self):
        return self.kind

    # ---- the lattice
    def grid(self, nx, ny, hx, hy):
        return (ny, nx, hy, hx) if self.kind == "T" else (nx, ny, hx, hy)

    def _space(self, a):
        """the last two axes [.., y, x] of any array"""
        if self.kind == "T":
            return np.swapaxes(a, -1, -2)
        return a[..., ::-1] if self.kind == "X" else a[..., ::-1, :]

    def node(self, a):
        return _c(self._space(a))

    def elem(self, a):
        return _c(self._space(a))

    # ---- vectors: T swaps the members, X negates the x member, Y the y member
    def vec(self, ax, ay, scalar=None):
        f = scalar or self.node
        if self.kind == "T":
            return f(ay), f(ax)
        return (-f(ax), f(ay)) if self.kind == "X" else (f(ax), -f(ay))

    # ---- DG coefficient planes
    def dg(self, a):
        nc = a.shape[0]
        b = self._space(a)
        if self.kind == "T":
            return _c(b[T_PERM[nc]] if (self.permute8 or nc != 8) else b)
        b = b.copy()
        b[(X_ODD if self.kind == "X" else Y_ODD)[nc]] *= -1.0
        return b

    def dgvec(self, ax, ay):
        return self.vec(ax, ay, scalar=self.dg)

    def stress(self, s11, s12, s22):
        if self.kind == "T":
            return self.dg(s22), self.dg(s12), self.dg(s11)
        return self.dg(s11), (-self.dg(s12) if self.s12_sign else self.dg(s12)), self.dg(s22)

    # ---- values at the 3 x 3 Gauss points
    def gauss(self, a):
        b = self._space(a)
        b = b.reshape(3, 3, *b.shape[-2:])  # [qy, qx, ., .]
        if self.kind == "T":
            b = b.transpose(1, 0, 2, 3)
        else:
            b = b[:, ::-1] if self.kind == "X" else b[::-1]
        return _c(b).reshape(9, *b.shape[-2:])

    # ---- edge-normal velocities: un_x = u on the vertical edges (Gauss points along y), un_y = v on the horizontal ones (along x)
    def edges(self, unx, uny):
        if self.kind == "T":
            return _c(uny.transpose(0, 2, 1)), _c(unx.transpose(0, 2, 1))
        if self.kind == "X":
            return _c(-unx[:, :, ::-1]), _c(uny[::-1, :, ::-1])
        return _c(unx[::-1, ::-1, :]), _c(-uny[:, ::-1, :])

    # ---- parameters (nsdg_mevp_params, nsdg_bbm_params, the grid spacings): scalars
    def params(self, d):
        d = dict(d)
        if "fc" in d and self.fc_sign:
            d["fc"] = -d["fc"]  # a reflection reverses the sense of rotation
        if self.kind == "T" and "hx" in d:
            d["hx"], d["hy"] = d["hy"], d["hx"]
        return d

    # ---- a whole named state: dict of arrays, the kind of each told by its name
    def state(self, st):
        out = {}
        done = set()
        for a, b in VECTOR_PAIRS:
            if a in st:
                out[a], out[b] = self.vec(st[a], st[b])
                done |= {a, b}
        if "s" in st:
            out["s"] = list(self.stress(*st["s"]))
            done.add("s")
        for k, v in st.items():
            if k in done:
                continue
            if k in ("H", "A", "D"):
                out[k] = self.dg(v)
            elif k in ("pg", "hg", "eg", "pm"):
                out[k] = self.gauss(v)
            elif k in ("cgh", "cga"):
                out[k] = self.node(v)
            elif k == "land":
                out[k] = self.elem(v)
            else:
                raise KeyError(k)
        return out


T, X, Y = Map("T"), Map("X"), Map("Y")
MAPS = {"T": T, "X": X, "Y": Y}


"""CPU reference of landfast ice (include/nsdg_basal.h): grounding on shoals as a basal stress in the momentum
update, after Lemieux et al. (2015).  numpy only.

The construction.  The seabed stress is one more IMPLICIT term in the denominator of the velocity update,
    u_b = N / (D + C_b),   u_oracle = N / D,   D = (m / dt)(1 + beta_n) + c,   C_b = T_b / (|u_old| + u0),
so the velocity with the term is the velocity without it times D / (D + C_b) -- an exact identity, node by node.  The UNCHANGED oracle
(oracle_lib) therefore runs every sub-iteration, and every node is corrected by that factor, with D restated here in numpy from DESIGN.md
sections 3.2 / 3.5 (beta_n of the adaptive form from the oracle's alpha_e) and T_b restated here from the formula.  Land nodes are zeroed
as tests/land_ref.py does.  The same factor applied to tests/dyn_independent.py's mevp_velocity and to tests/bbm_ref.py's velocity gives
the pure-Python form and the brittle form.

Parameters are read by name from an oracle_lib.MevpParams or from the dict the pure-Python references take (get()).
It lives under tests/ because it calls the oracle; the product never imports it."""
import numpy as np

import land_ref
import oracle_lib as O
from land_ref import LandOracleOps

DEFAULTS = dict(k1=8.0, k2=15.0, alpha_b=20.0, u0=5e-5)  # Lemieux et al. 2015


def basal_par(**kw):
    bp = dict(DEFAULTS)
    for k in kw:
        assert k in bp, k
    bp.update(kw)
    return bp


def get(p, name, default=None):
    """a parameter by name from a ctypes structure or a dict"""
    if isinstance(p, dict):
        return p.get(name, default)
    return getattr(p, name)


def nodal_depth(depth):
    """[2ny+1, 2nx+1]: at every CG2 node the mean of the element-wise depth [ny, nx] over the elements adjacent to it inside the array"""
    depth = np.asarray(depth, dtype=np.float64)
    ny, nx = depth.shape
    out, cnt = np.zeros((2 * ny + 1, 2 * nx + 1)), np.zeros((2 * ny + 1, 2 * nx + 1))
    for dy in range(3):
        for dx in range(3):
            out[dy:dy + 2 * ny:2, dx:dx + 2 * nx:2] += depth
            cnt[dy:dy + 2 * ny:2, dx:dx + 2 * nx:2] += 1.0
    return out / cnt


def ice_free(p, cgh, cga):
    """the ice-free-node rule of DESIGN.md section 3.3 (both thresholds 0: off)"""
    if not (get(p, "min_conc", 0.0) > 0.0 or get(p, "min_thick", 0.0) > 0.0):
        return np.zeros(np.shape(cgh), dtype=bool)
    return (cga < get(p, "min_conc")) | (cgh < get(p, "min_thick") * cga) | (cgh <= get(p, "h_min"))


def critical_stress(p, bp, cgh, cga, depth, land=None):
    """T_b [N m^-2] at every node: k2 max(0, h - a h_wn / k1) exp(-alpha_b (1 - a)), 0 at land nodes and at ice-free nodes.
    h = cgH itself (not raised to h_min), a = clamp(cgA, 0, 1); land: the ELEMENT mask or None"""
    a = np.clip(cga, 0.0, 1.0)
    hc = a * nodal_depth(depth) / bp["k1"]
    tb = bp["k2"] * np.maximum(0.0, cgh - hc) * np.exp(-bp["alpha_b"] * (1.0 - a))
    tb[ice_free(p, cgh, cga)] = 0.0
    if land is not None:
        tb[land_ref.land_nodes(land)] = 0.0
    return tb


def node_beta(p, cgh, cga, alpha_e):
    """beta_n of every node: the launch constant, or -- adaptive form, DESIGN.md section 3.5 -- the largest alpha_e h'_c(e) / h'_n of the
    adjacent elements, at least alpha_min, and alpha_min at an ice-free node"""
    if not get(p, "aevp_c", 0.0) > 0.0:
        return np.full(cgh.shape, float(get(p, "beta")))
    ny, nx = alpha_e.shape
    hn = np.maximum(cgh, get(p, "h_min"))
    offer = np.zeros(cgh.shape)
    q = alpha_e * hn[1::2, 1::2]  # alpha_e times the element's own mass (at its centre node)
    for dy in range(3):
        for dx in range(3):
            blk = offer[dy:dy + 2 * ny:2, dx:dx + 2 * nx:2]
            np.maximum(blk, q, out=blk)
    beta = np.maximum(offer / hn, get(p, "aevp_alpha_min"))
    beta[ice_free(p, cgh, cga)] = get(p, "aevp_alpha_min")
    return beta


def denominator(p, dt, cgh, cga, u, v, uo, vo, beta):
    """D = (m / dt)(1 + beta_n) + c of the update without the seabed stress (beta: an array, or 0 for the brittle momentum step)"""
    free = ice_free(p, cgh, cga)
    m = get(p, "rho_ice") * np.maximum(cgh, get(p, "h_min"))
    a = np.where(free, 1.0, np.clip(cga, 0.0, 1.0))
    c = a * get(p, "c_ocean") * get(p, "rho_ocean") * np.sqrt((uo - u) ** 2 + (vo - v) ** 2)
    return (m / dt) * (1.0 + beta) + c


def factor(D, tb, u, v, u0):
    """D / (D + C_b), C_b = T_b / (|u| + u0) with the speed of the ice itself"""
    cb = tb / (np.sqrt(u * u + v * v) + u0)
    return D / (D + cb)


def subcycle(nx, ny, hx, hy, dt, nsub, p, bp, depth, land, s, u, v, u0, v0, tax, tay, uo, vo, cgh, cga, pg, basal=True, omp=False):
    """nsub sub-iterations in place on s (3 x [8, ny, nx]), u, v: oracle stress + velocity, every node corrected by D / (D + C_b), land
    nodes (land: the element mask or None) zeroed after each.  basal=False: the same without the correction -- the reference that lost
    the term.  Returns T_b"""
    ln = land_ref.land_nodes(land) if land is not None else None
    tb = critical_stress(p, bp, cgh, cga, depth, land)
    ad = p.aevp_c > 0
    alpha_e = np.zeros((ny, nx)) if ad else None
    u0, v0 = u0.copy(), v0.copy()
    for _ in range(nsub):
        O.mevp_stress(nx, ny, 0, ny, hx, hy, p, u, v, pg, *s, **(dict(dt=dt, cgh=cgh, cga=cga, alpha_e=alpha_e) if ad else {}), omp=omp)
        un, vn = np.zeros_like(u), np.zeros_like(v)
        O.mevp_velocity(nx, ny, 0, ny, hx, hy, dt, p, s, (u, v), (un, vn), (u0, v0), (tax, tay), (uo, vo), cgh, cga,
                        **(dict(alpha_e=alpha_e) if ad else {}), omp=omp)
        if basal:
            f = factor(denominator(p, dt, cgh, cga, u, v, uo, vo, node_beta(p, cgh, cga, alpha_e)), tb, u, v, bp["u0"])
            un *= f
            vn *= f
        if ln is not None:
            un[ln] = 0.0
            vn[ln] = 0.0
        u[:], v[:] = un, vn
    return tb


def python_subcycle(par, bp, hx, hy, dt, nsub, depth, S, u, v, u0, v0, tax, tay, uo, vo, cgh, cga, P):
    """the pure-Python form: tests/dyn_independent.py per sub-iteration with the same correction (par: its parameter dict; no land).
    Returns (S, u, v)"""
    import dyn_independent as DI

    tb = critical_stress(par, bp, cgh, cga, depth)
    ad = par.get("aevp_c", 0.0) > 0.0
    for _ in range(nsub):
        if ad:
            S, alpha_e = DI.mevp_stress(par, hx, hy, u, v, P, S, dt=dt, cgh=cgh, cga=cga)
        else:
            S, alpha_e = DI.mevp_stress(par, hx, hy, u, v, P, S), None
        un, vn = DI.mevp_velocity(par, hx, hy, dt, S, u, v, u0, v0, tax, tay, uo, vo, cgh, cga, alpha_e=alpha_e)
        f = factor(denominator(par, dt, cgh, cga, u, v, uo, vo, node_beta(par, cgh, cga, alpha_e)), tb, u, v, bp["u0"])
        u, v = un * f, vn * f
    return S, u, v


def bbm_iterate(mp, bbm, bp, hx, hy, dts, depth, S, D, u, v, gauss, nod, land=None):
    """the brittle form: one sub-iteration of tests/bbm_ref.py on a whole array with the same correction (beta = 0: the brittle momentum
    step is the node update with K1 = K2 = rho_i / dt_s).  land: the element mask or None.  Returns new (S, D, u, v)"""
    import bbm_ref as B

    ln = B.land_nodes(land) if land is not None else None
    tb = critical_stress(mp, bp, nod["cgh"], nod["cga"], depth, land)
    So, Do, un, vn = B.iterate(mp, bbm, hx, hy, dts, S, D, u, v, gauss, nod, land=ln)
    f = factor(denominator(mp, dts, nod["cgh"], nod["cga"], u, v, nod["uo"], nod["vo"], 0.0), tb, u, v, bp["u0"])
    return So, Do, un * f, vn * f


def shoal_depth(nx, ny, deep=1000.0, shallow=10.0, box=None):
    """the shoal case: `shallow` metres inside the element box (iy0, iy1, ix0, ix1) -- by default the middle third of the rows and the
    columns nx // 3 .. 2 nx // 3 + 1 -- inside `deep` metres of water.  Returns (depth [ny, nx], shoal element mask)"""
    iy0, iy1, ix0, ix1 = box if box is not None else (ny // 3, 2 * ny // 3 + 1, nx // 3, 2 * nx // 3 + 1)
    shoal = np.zeros((ny, nx), dtype=bool)
    shoal[iy0:iy1, ix0:ix1] = True
    return np.where(shoal, shallow, deep), shoal


def thick_cover(H, A, seed=23):
    """the cover of the shoal case, in place on DG fields [6, ny, nx]: cell means H ~ 2 m and A ~ 0.95 (the higher coefficients stay):
    over 10 m of water h_c = a h_w / k1 ~ 1.2 m < h, the keels ground; over 1000 m h_c ~ 119 m, T_b = 0"""
    rng = np.random.default_rng(seed)
    H[0] = 2.0 + 0.05 * rng.standard_normal(H[0].shape)
    A[0] = 0.95 - 0.04 * rng.random(A[0].shape)
    return H, A


def shoal_nodes(shoal):
    """the nodes all of whose adjacent elements are shoal elements: the interior of the shoal on the CG2 lattice"""
    return ~land_ref.land_nodes(~shoal)


class BasalOracleOps(LandOracleOps):
    """LandOracleOps with the landfast-ice calls of abi.Context: the depth and the parameters are remembered, T_b is formed at every
    packing, and every sub-iteration's velocity is corrected by D / (D + C_b) on the node rows it wrote"""

    def __init__(self, **mevp):
        super().__init__(**mevp)
        self.depth, self.bp, self._tb = None, basal_par(), None

    def set_grid(self, nx, ny, hx, hy):
        if (nx, ny) != (getattr(self, "nx", None), getattr(self, "ny", None)):
            self.depth = None  # nsdg_grid_set: a new shape drops the depth array
        super().set_grid(nx, ny, hx, hy)

    def set_basal_params(self, bp):
        self.bp = basal_par(**({k: getattr(bp, k) for k in DEFAULTS} if not isinstance(bp, dict) else bp))

    def set_basal_depth(self, depth):
        if depth is None:
            self.depth = None
            return
        d = depth.numpy()
        assert d.shape == (self.ny, self.nx)
        self.depth = d

    def basal_critical(self, cgh, cga, tb):
        assert self.depth is not None
        tb.numpy()[:] = critical_stress(self.p, self.bp, cgh.numpy(), cga.numpy(), self.depth, self.land)

    def _pack_basal(self):
        _, _, _, _, cgh, cga = self.nodal
        self._tb = None if self.depth is None else critical_stress(self.p, self.bp, cgh, cga, self.depth, self.land)

    def mevp_prepare(self, *a):
        super().mevp_prepare(*a)
        self._pack_basal()

    def mevp_pack_nodal(self, *a):
        super().mevp_pack_nodal(*a)
        self._pack_basal()

    def mevp_iterate(self, k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        super().mevp_iterate(k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg)
        if self._tb is None:
            return
        dt, _, _, ocean, cgh, cga = self.nodal
        u, v = uv_old[0].numpy(), uv_old[1].numpy()
        f = factor(denominator(self.p, dt, cgh, cga, u, v, ocean[0], ocean[1], node_beta(self.p, cgh, cga, self._alpha_e)), self._tb, u, v, self.bp["u0"])
        rows = slice(2 * j0, 2 * j1 + (1 if j1 == self.ny else 0))
        for x in uv_new:
            x.numpy()[rows] *= f[rows]

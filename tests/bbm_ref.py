"""INDEPENDENT dense numpy restatement of the brittle Bingham-Maxwell sub-cycle (include/nsdg.h "brittle rheology", DESIGN.md section
3.8), TEST INFRASTRUCTURE.  Written from the formulas, not from the kernel: it imports nothing from nextsimdg_amd, and takes other routes
wherever the mathematics allows one --

  * the basis functions are numpy Polynomial objects and every operator is built from them by quadrature;
  * the strain rate at a Gauss point is the derivative of the biquadratic velocity THERE (the kernel projects the derivative on the
    8-coefficient space and evaluates the projection; the space contains the derivatives);
  * the L2 projections solve with the full mass matrix of a 6-point rule; the damage is projected on the 6-function DG2 space directly
    (the kernel takes coefficients 0..5 of the 8-function projection);
  * the stress divergence at a node is the weak form -(h sigma, grad phi_n) summed over the Gauss points: the gradient of a CG2 function
    lies in the 8-function space, so the projection of step 9 drops out of the integral;
  * exp, sqrt, true division and ** where the kernel uses Newton-refined reciprocals and repeated multiplication;
  * the ice-free-node rule is decided on the true thickness and a free-drift node simply has no stress term.

Sums over basis functions and Gauss points run in a fixed order with elementwise array operations, so that a row block computes what the
whole domain computes, bit for bit.  It also holds an ops stand-in (BbmRefOps) with which rowblock.DynamicsCore(rheology="bbm") runs on the
CPU."""
import numpy as np
from numpy.polynomial import Polynomial as Poly
from numpy.polynomial.legendre import leggauss


def gauss_unit(n):
    x, w = leggauss(n)
    return 0.5 * x, 0.5 * w


NODES = (-0.5, 0.0, 0.5)


def _lagrange(k):
    p = Poly([1.0])
    for j in range(3):
        if j != k:
            p = p * Poly([-NODES[j], 1.0]) / (NODES[k] - NODES[j])
    return p


LAG = [_lagrange(k) for k in range(3)]
DLAG = [p.deriv() for p in LAG]
_P0, _P1, _P2 = Poly([1.0]), Poly([0.0, 1.0]), Poly([-1.0 / 12.0, 0.0, 1.0])
PSI = [(_P0, _P0), (_P1, _P0), (_P0, _P1), (_P2, _P0), (_P0, _P2), (_P1, _P1), (_P2, _P1), (_P1, _P2)]


def psi(i, x, y):
    return PSI[i][0](x) * PSI[i][1](y)


G3, W3 = gauss_unit(3)
GQ = [(G3[q % 3], G3[q // 3]) for q in range(9)]  # q = 3 qy + qx
WQ = np.array([W3[q % 3] * W3[q // 3] for q in range(9)])
PSI_Q = np.array([[psi(i, x, y) for i in range(8)] for (x, y) in GQ])  # [q, i]
PHI_Q = np.array([[LAG[a % 3](x) * LAG[a // 3](y) for a in range(9)] for (x, y) in GQ])  # [q, a], a = 3 ay + ax
PHIX_Q = np.array([[DLAG[a % 3](x) * LAG[a // 3](y) for a in range(9)] for (x, y) in GQ])
PHIY_Q = np.array([[LAG[a % 3](x) * DLAG[a // 3](y) for a in range(9)] for (x, y) in GQ])


def _mass(n):
    x, w = gauss_unit(6)
    return np.array([[sum(w[a] * w[b] * psi(i, x[a], x[b]) * psi(j, x[a], x[b]) for a in range(6) for b in range(6)) for j in range(n)]
                     for i in range(n)])


PROJ8 = np.linalg.solve(_mass(8), (PSI_Q * WQ[:, None]).T)  # [i, q]: coefficients from Gauss-point values
PROJ6 = np.linalg.solve(_mass(6), (PSI_Q[:, :6] * WQ[:, None]).T)
LUMP = np.array([sum(WQ[q] * PHI_Q[q, a] for q in range(9)) for a in range(9)])  # int phi_a over the reference element (exact)


def apply(M, X):
    """out[r] = sum_c M[r, c] X[c] with the sum in the order of c, elementwise on the trailing axes"""
    out = []
    for r in range(M.shape[0]):
        acc = M[r, 0] * X[0]
        for c in range(1, M.shape[1]):
            acc = acc + M[r, c] * X[c]
        out.append(acc)
    return np.array(out)


def mevp_par(**kw):
    p = dict(rho_ice=900.0, rho_atm=1.3, rho_ocean=1026.0, c_atm=1.2e-3, c_ocean=5.5e-3, compaction=20.0, fc=1.46e-4, h_min=1e-4,
             min_conc=1e-12, min_thick=0.01)
    p.update(kw)
    return p


def bbm_par(**kw):
    p = dict(young=5.9605e8, nu=1.0 / 3.0, p0=1e4, lambda0=1e7, relax_exponent=5, tan_phi=0.7, cohesion_lab=2e6, compr_strength=1e10,
             t_heal=1e5, d_max=1.0 - 1e-6)
    p.update(kw)
    return p


def substep_count(bp, rho_ice, h, dt, courant):
    c = np.sqrt(bp["young"] / (rho_ice * (1.0 - bp["nu"] ** 2)))
    return max(1, int(np.ceil(dt * c / (courant * h))))


# ------------------------------------------------------------------------------------------------ per model step
def prepare(mp, bp, H, A):
    """hg, eg, pm at the 3 x 3 Gauss points: [9, ny, nx] each"""
    h = np.maximum(apply(PSI_Q[:, :6], H), 0.0)
    a = np.minimum(np.maximum(apply(PSI_Q[:, :6], A), 0.0), 1.0)
    eg = np.exp(np.ascontiguousarray(-mp["compaction"] * (1.0 - a)))
    return h, eg, bp["p0"] * h ** 1.5 * eg


def nodal_mean(F):
    _, ny, nx = F.shape
    out, cnt = np.zeros((2 * ny + 1, 2 * nx + 1)), np.zeros((2 * ny + 1, 2 * nx + 1))
    for a in range(9):
        ay, ax = divmod(a, 3)
        val = apply(np.array([[psi(i, NODES[ax], NODES[ay]) for i in range(F.shape[0])]]), F)[0]
        out[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] += val
        cnt[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] += 1.0
    return out / cnt


def wind_stress(mp, ua, va):
    mag = np.sqrt(ua * ua + va * va)
    return mp["c_atm"] * mp["rho_atm"] * mag * ua, mp["c_atm"] * mp["rho_atm"] * mag * va


def land_nodes(mask):
    ny, nx = mask.shape
    out = np.zeros((2 * ny + 1, 2 * nx + 1), dtype=bool)
    for ay in range(3):
        for ax in range(3):
            out[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] |= mask
    return out


def ice_free(mp, cgh, cga):
    if mp["min_conc"] <= 0.0 and mp["min_thick"] <= 0.0:
        return np.zeros(cgh.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        thin = cgh / cga < mp["min_thick"]
    return (cga < mp["min_conc"]) | (cgh <= mp["h_min"]) | thin


# ------------------------------------------------------------------------------------------------ one sub-iteration
def local_nodal(f, r0, r1):
    """the 9 nodal values of the elements of rows [r0, r1): [a, rows, nx], a = 3 ay + ax"""
    nx = (f.shape[1] - 1) // 2
    return np.array([f[2 * r0 + a // 3:2 * r1 + a // 3:2, a % 3:a % 3 + 2 * nx:2] for a in range(9)])


def element_step(mp, bp, hx, hy, dts, S, D, u, v, hg, eg, pm, r0, r1, diag=None):
    """steps 1-8 on the element rows [r0, r1).  S = [3][8, ny, nx] (s11, s12, s22), D = [6, ny, nx].  Returns (S' [3][8, rows, nx],
    D' [6, rows, nx], T [3][9, rows, nx] = hg sigma at the Gauss points).  diag: a dict that receives the Gauss-point values the tests'
    branch-margin conditions are stated on"""
    h = min(hx, hy)
    sl = slice(r0, r1)
    ul, vl = local_nodal(u, r0, r1), local_nodal(v, r0, r1)
    e11 = apply(PHIX_Q, ul) / hx
    e22 = apply(PHIY_Q, vl) / hy
    e12 = 0.5 * (apply(PHIY_Q, ul) / hy + apply(PHIX_Q, vl) / hx)
    s11, s12, s22 = (apply(PSI_Q, c[:, sl]) for c in S)
    d = apply(PSI_Q[:, :6], D[:, sl])
    egq, hgq, pmq = eg[:, sl], hg[:, sl], pm[:, sl]
    # 1
    d = np.minimum(np.maximum(d, 0.0), bp["d_max"])
    d = np.maximum(0.0, d - dts / bp["t_heal"])
    # 2
    x = (1.0 - d) * egq
    E = bp["young"] * x
    lam = bp["lambda0"] * x ** (bp["relax_exponent"] - 1)
    # 3
    sn_old = 0.5 * (s11 + s22)
    with np.errstate(divide="ignore", invalid="ignore"):
        Pt = np.where(sn_old < 0.0, np.minimum(1.0, -pmq / sn_old), 0.0)
    # 4
    m = np.minimum(1.0 - 1e-12, lam / (lam + dts * (1.0 - Pt)))
    # 5
    nu = bp["nu"]
    k1, k2 = 1.0 / (1.0 + nu), nu / (1.0 - nu ** 2)
    tr = e11 + e22
    s11 = (s11 + dts * E * (k1 * e11 + k2 * tr)) * m
    s22 = (s22 + dts * E * (k1 * e22 + k2 * tr)) * m
    s12 = (s12 + dts * E * k1 * e12) * m
    # 6
    sn = 0.5 * (s11 + s22)
    ss = np.sqrt(0.25 * (s11 - s22) ** 2 + s12 ** 2)
    den = ss + bp["tan_phi"] * sn
    coh = bp["cohesion_lab"] * np.sqrt(0.1 / h)
    N = bp["compr_strength"]
    with np.errstate(divide="ignore", invalid="ignore"):
        dc = np.where(sn < -N, -N / sn, np.where(den > coh, coh / den, 1.0))
    # 7
    r = np.minimum(1.0, dts * np.sqrt(E) / (h * np.sqrt(2.0 * (1.0 + nu) * mp["rho_ice"])))
    f = (1.0 - dc) * r
    dh = d
    d = np.minimum(bp["d_max"], d + (1.0 - d) * f)
    s11, s12, s22 = s11 * (1.0 - f), s12 * (1.0 - f), s22 * (1.0 - f)
    if diag is not None:
        diag.update(sn_old=sn_old, sn_new=sn, failing=den > coh, r=r, d_healed=dh, d_c=dc, Pt_used=sn_old < 0.0,
                    smax=max(np.max(np.abs(s11)), np.max(np.abs(s12)), np.max(np.abs(s22))), emax=max(np.max(np.abs(e11)), np.max(np.abs(e12)), np.max(np.abs(e22))), s11=s11, s12=s12, s22=s22, d=d, coh=coh)
    # 8
    Sn = [apply(PROJ8, t) for t in (s11, s12, s22)]
    Dn = apply(PROJ6, d)
    return Sn, Dn, [hgq * s11, hgq * s12, hgq * s22]


def velocity(mp, hx, hy, dts, T, r0, u, v, nod, j0, j1, land=None):
    """step 9: the new velocity on the node rows owned by element rows [j0, j1) (the top row of the array too when j1 is its last row).
    T = hg sigma at the Gauss points of the element rows [r0, r0 + rows) (r0 <= j0 - 1, or r0 = j0 = 0); nod = dict(cgh, cga, tax, tay,
    uo, vo) on the local lattice; land = bool array of land NODES.  Returns (un, vn, g0, g1): the rows [g0, g1) of the lattice"""
    nm, nn = u.shape
    ny, nx = (nm - 1) // 2, (nn - 1) // 2
    rows = T[0].shape[1]
    divx, divy = np.zeros((nm, nn)), np.zeros((nm, nn))
    lump = np.zeros((nm, nn))
    area = hx * hy
    for a in range(9):
        ay, ax = divmod(a, 3)
        cx = cy = 0.0
        for q in range(9):
            gx, gy = PHIX_Q[q, a] / hx, PHIY_Q[q, a] / hy
            cx = cx - WQ[q] * (T[0][q] * gx + T[1][q] * gy)
            cy = cy - WQ[q] * (T[1][q] * gx + T[2][q] * gy)
        divx[2 * r0 + ay:2 * (r0 + rows) + ay:2, ax:ax + 2 * nx:2] += area * cx
        divy[2 * r0 + ay:2 * (r0 + rows) + ay:2, ax:ax + 2 * nx:2] += area * cy
        lump[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] += area * LUMP[a]
    g0, g1 = 2 * j0, 2 * j1 + (1 if j1 == ny else 0)
    sl = slice(g0, g1)
    cgh, cga = nod["cgh"][sl], nod["cga"][sl]
    free = ice_free(mp, cgh, cga)
    m = mp["rho_ice"] * np.maximum(cgh, mp["h_min"])
    a = np.where(free, 1.0, np.minimum(np.maximum(cga, 0.0), 1.0))
    fx = np.where(free, 0.0, divx[sl] / lump[sl])
    fy = np.where(free, 0.0, divy[sl] / lump[sl])
    uo, vo, uu, vv = nod["uo"][sl], nod["vo"][sl], u[sl], v[sl]
    c = a * mp["c_ocean"] * mp["rho_ocean"] * np.sqrt((uo - uu) ** 2 + (vo - vv) ** 2)
    den = m / dts + c
    un = ((m / dts) * uu + a * nod["tax"][sl] + c * uo + m * mp["fc"] * (vv - vo) + fx) / den
    vn = ((m / dts) * vv + a * nod["tay"][sl] + c * vo - m * mp["fc"] * (uu - uo) + fy) / den
    edge = np.zeros((g1 - g0, nn), dtype=bool)
    edge[:, 0] = edge[:, -1] = True
    if g0 == 0:
        edge[0] = True
    if g1 == nm:
        edge[-1] = True
    if land is not None:
        edge |= land[sl]
    un[edge] = 0.0
    vn[edge] = 0.0
    return un, vn, g0, g1


def iterate(mp, bp, hx, hy, dts, S, D, u, v, gauss, nod, k0=0, j0=0, j1=None, land=None, diag=None):
    """one sub-iteration on a whole local array (or the row ranges of nsdg_bbm_iterate): returns new (S, D, u, v); rows that the call does
    not cover keep the input's values"""
    ny = D.shape[1]
    j1 = ny if j1 is None else j1
    hg, eg, pm = gauss
    Sn, Dn, T = element_step(mp, bp, hx, hy, dts, S, D, u, v, hg, eg, pm, k0, j1, diag)
    So, Do = [c.copy() for c in S], D.copy()
    for o, n in zip(So, Sn):
        o[:, k0:j1] = n
    Do[:, k0:j1] = Dn
    un, vn = u.copy(), v.copy()
    a, b, g0, g1 = velocity(mp, hx, hy, dts, T, k0, u, v, nod, j0, j1, land)
    un[g0:g1], vn[g0:g1] = a, b
    return So, Do, un, vn


def nodal_fields(mp, H, A, ua, va, uo, vo):
    tax, tay = wind_stress(mp, ua, va)
    return dict(cgh=nodal_mean(H), cga=nodal_mean(A), tax=tax, tay=tay, uo=uo, vo=vo)


# ------------------------------------------------------------------------------------------------ ops stand-in for the row-block driver
def _ops_base():
    from land_ref import LandOracleOps  # OracleOps (the stand-in of tests/test_rowblock_gloo.py) with the land calls

    return LandOracleOps


def make_ops(bbm=None, record=None, **mevp):
    """BbmRefOps(bbm parameters dict, **mEVP parameters): the CPU stand-in of tests/test_rowblock_gloo.py with bbm_prepare / bbm_iterate
    from this file (and the packing's nodal fields from this file too); transport, limiter and land calls are the stand-in's.  record: a
    list that receives the diag dict of every bbm_iterate call"""
    Base = _ops_base()

    class BbmRefOps(Base):
        def __init__(self):
            super().__init__()
            self.bp = bbm_par(**(bbm or {}))
            self.mp = mevp_par(**mevp)
            self.record = record

        def mevp_prepare(self, dt, H, A, wind, ocean, u0v0, packed):
            assert not u0v0[0].numpy().any() and not u0v0[1].numpy().any()  # the BBM packing takes u0 = v0 = 0
            self.bbm_dts = dt
            self.bbm_nod = nodal_fields(self.mp, H.numpy(), A.numpy(), wind[0].numpy(), wind[1].numpy(), ocean[0].numpy(), ocean[1].numpy())
            self.bbm_land = land_nodes(self.land) if self.land is not None else None
            if self.bbm_land is not None:  # land nodes are packed with constants: a NaN forcing there never enters
                for k in ("tax", "tay"):
                    self.bbm_nod[k] = np.where(self.bbm_land, 0.0, self.bbm_nod[k])

        def bbm_prepare(self, H, A, hg, eg, pm, j0=0, j1=None):
            j1 = self.ny if j1 is None else j1
            for dst, src in zip((hg, eg, pm), prepare(self.mp, self.bp, H.numpy(), A.numpy())):
                dst.numpy()[:, j0:j1] = src[:, j0:j1]

        def bbm_iterate(self, k0, j0, j1, s_in, s_out, d_in, d_out, uv_old, uv_new, packed, gauss):
            diag = {} if self.record is not None else None
            u, v = uv_old[0].numpy(), uv_old[1].numpy()
            Sn, Dn, T = element_step(self.mp, self.bp, self.hx, self.hy, self.bbm_dts, [x.numpy() for x in s_in], d_in.numpy(), u, v,
                                     *[g.numpy() for g in gauss], k0, j1, diag)
            for o, n in zip(s_out, Sn):
                o.numpy()[:, k0:j1] = n
            d_out.numpy()[:, k0:j1] = Dn
            a, b, g0, g1 = velocity(self.mp, self.hx, self.hy, self.bbm_dts, T, k0, u, v, self.bbm_nod, j0, j1, self.bbm_land)
            uv_new[0].numpy()[g0:g1], uv_new[1].numpy()[g0:g1] = a, b
            if diag is not None:
                diag["rows"] = (k0, j1)
                self.record.append(diag)

    return BbmRefOps()

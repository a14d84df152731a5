"""numpy restatement of the momentum budget (include/nsdg_budget.h), TEST INFRASTRUCTURE: the sixteen nodal
forces and the nine row totals of nsdg_momentum_budget, operation for operation as the header states them -- every product a statement of
its own -- from the packed coefficients, the state (u, v, S) and the forcing.  What the header takes from other code is taken from that
code's restatement: the stress divergence by the weak form and the tables of tests/mevp_ref.py (a rule of its own, not the kernels'
sum-factorised operators), the nodal mean of A by mevp_ref.nodal_mean, the gradient of the height by tilt_ref.gradient; sqrt and true
division stand where the kernels use Newton-refined reciprocals.  It imports nothing from nextsimdg_amd.

BudgetOracleOps: the CPU twin of abi.Context.momentum_budget for rowblock.DynamicsCore(..., budget=...), composed with the land, basal,
snow and tilt twins."""
import numpy as np

import mevp_ref as MR
import tilt_ref as TR

TERMS = ("wind", "water", "coriolis", "tilt", "internal", "basal", "inertia", "residual")  # in id order: nsdg_budget_term_id
KE = 8
PLANES = tuple(t + "_" + c for t in TERMS for c in "xy")
OWNED = ((0, 0), (0, 1), (1, 0), (1, 1))  # (oy, ox) of the vertex, bottom edge, left edge, centre of an element


def _p(p, name):
    return p[name] if isinstance(p, dict) else getattr(p, name)


def divergence(S, hx, hy):
    """(div_x / M, div_y / M) on the [2ny+1, 2nx+1] lattice from the stress S = [3][8, ny, nx]: the weak form -(sigma, grad phi_n) summed
    over the elements round a node, over the lumped mass of the node -- the loops of mevp_ref.velocity"""
    ny, nx = S[0].shape[1:]
    nm, nn = 2 * ny + 1, 2 * nx + 1
    divx, divy, lump = np.zeros((nm, nn)), np.zeros((nm, nn)), np.zeros((nm, nn))
    s11, s12, s22 = (MR.apply(MR.PSI_4, c) for c in S)
    area = hx * hy
    for a in range(9):
        ay, ax = divmod(a, 3)
        cx = cy = 0.0
        for q in range(16):
            gx, gy = MR.PHIX_4[q, a] / hx, MR.PHIY_4[q, a] / hy
            cx = cx - MR.W4[q] * (s11[q] * gx + s12[q] * gy)
            cy = cy - MR.W4[q] * (s12[q] * gx + s22[q] * gy)
        divx[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] += area * cx
        divy[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] += area * cy
        lump[ay:ay + 2 * ny:2, ax:ax + 2 * nx:2] += area * MR.LUMP[a]
    return divx / lump, divy / lump


def unpack(packed, shape):
    """the device's packed buffer (4 pair planes of [n, 2]) as (c [6, nm, nn], tb [nm, nn])"""
    n = shape[0] * shape[1]
    q = np.asarray(packed)[:8 * n].reshape(4, n, 2)
    c = np.array([q[k // 2, :, k % 2].reshape(shape) for k in range(6)])
    return c, q[3, :, 0].reshape(shape)


def fixed_nodes(c):
    """land nodes (c[1] < 0) and the Dirichlet nodes of the lattice edge"""
    fixed = c[1] < 0.0
    fixed[0] = fixed[-1] = True
    fixed[:, 0] = fixed[:, -1] = True
    return fixed


def forces(p, dt, hx, hy, c, A, ua, va, S, u, v, tb=None, u0=0.0, eta=None, g=TR.GRAVITY):
    """{"<term>_x", "<term>_y": [nm, nn]} and "m", the nodal mass per area; c = the packed coefficients [6, nm, nn], tb = the seventh (None:
    no depth was packed), eta = the sea-surface height (None: the tilt of the geostrophic current)"""
    with np.errstate(invalid="ignore", over="ignore"):
        land = c[1] < 0.0
        fixed = fixed_nodes(c)
        free = c[0] > 2.0 ** 50
        s = np.where(free, 2.0 ** -100, 1.0)
        hp, cd, c2, c3 = s * c[0], s * c[1], s * c[2], s * c[3]
        uo, vo = c[4], c[5]
        rho = _p(p, "rho_ice")
        m = rho * hp
        a = np.where(free, 1.0, np.minimum(np.maximum(MR.nodal_mean(A), 0.0), 1.0))
        f_atm = _p(p, "c_atm") * _p(p, "rho_atm")
        wm = np.sqrt(ua * ua + va * va)
        tax, tay = f_atm * wm * ua, f_atm * wm * va
        F = {}
        F["wind_x"], F["wind_y"] = a * tax, a * tay
        du, dv = uo - u, vo - v
        drag = cd * np.sqrt(du * du + dv * dv)
        F["water_x"], F["water_y"] = drag * du, drag * dv
        cor = (rho * _p(p, "fc")) * hp
        F["coriolis_x"], F["coriolis_y"] = cor * v, -(cor * u)
        if eta is None:
            F["tilt_x"], F["tilt_y"] = -(cor * vo), cor * uo
        else:
            sx, sy = TR.gradient(np.where(np.isnan(eta), 0.0, eta), hx, hy)  # a land node reads nothing of eta; ocean nodes never meet a NaN
            m_g = m * g
            F["tilt_x"], F["tilt_y"] = -(m_g * sx), -(m_g * sy)
        dx, dy = divergence(S, hx, hy)
        F["internal_x"], F["internal_y"] = np.where(free, 0.0, dx), np.where(free, 0.0, dy)
        if tb is None:
            F["basal_x"], F["basal_y"] = np.zeros_like(u), np.zeros_like(v)
        else:
            cb = tb / (np.sqrt(u * u + v * v) + u0)
            F["basal_x"], F["basal_y"] = -(cb * u), -(cb * v)
        mdt = m / dt
        mu, mv = mdt * u, mdt * v
        F["inertia_x"] = (c2 - F["wind_x"] - F["tilt_x"]) - mu
        F["inertia_y"] = (c3 - F["wind_y"] - F["tilt_y"]) - mv
        F["residual_x"] = ((((c2 - mu) + F["water_x"]) + F["coriolis_x"]) + F["internal_x"]) + F["basal_x"]
        F["residual_y"] = ((((c3 - mv) + F["water_y"]) + F["coriolis_y"]) + F["internal_y"]) + F["basal_y"]
    for k in PLANES:
        F[k] = np.where(fixed, 0.0, F[k])
    F["m"] = m
    F["fixed"] = fixed
    F["land"] = land
    return F


def scale(F):
    """sum over the eight terms of |F_x| + |F_y| per node: what the tolerances of the tests are relative to"""
    return sum(np.abs(F[k]) for k in PLANES)


def fold(acc):
    """the lanes folded by halves: p_l = p_l + p_(l + s), s = 32 ... 1; acc = [rows, 64]"""
    s = 32
    while s >= 1:
        acc = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    return acc[:, 0]


def row_totals(F, u, v, hx, hy, j0, j1):
    """[9, j1 - j0]: per element row the power of the eight terms and the kinetic energy over the nodes the row owns, in the header's order"""
    nx = (u.shape[1] - 1) // 2
    area = hx * hy
    ml = {(0, 0): area / 9.0, (0, 1): area / 4.5, (1, 0): area / 4.5, (1, 1): area / 2.25}
    uu, vv = np.where(F["fixed"], 0.0, u), np.where(F["fixed"], 0.0, v)
    out = np.zeros((9, j1 - j0))
    own = lambda f, oy, ox: f[2 * j0 + oy:2 * j1 + oy:2, ox:ox + 2 * nx:2]
    for q in range(9):
        acc = np.zeros((j1 - j0, 64))
        for i0 in range(0, nx, 64):
            w = min(64, nx - i0)
            for oy, ox in OWNED:
                un, vn = own(uu, oy, ox)[:, i0:i0 + w], own(vv, oy, ox)[:, i0:i0 + w]
                if q < KE:
                    pa = un * own(F[TERMS[q] + "_x"], oy, ox)[:, i0:i0 + w]
                    pb = vn * own(F[TERMS[q] + "_y"], oy, ox)[:, i0:i0 + w]
                    p = ml[(oy, ox)] * (pa + pb)
                else:
                    e = own(F["m"], oy, ox)[:, i0:i0 + w] * (un * un + vn * vn)
                    p = ml[(oy, ox)] * (0.5 * e)
                acc[:, :w] = acc[:, :w] + p
        out[q] = fold(acc)
    return out


# ------------------------------------------------------------------------------------------------ the CPU twin of the driver's call
def coefficients(p, dt, u0, v0, tax, tay, uo, vo, cgh, cga, land=None):
    """c [6, nm, nn]: what the packing holds per node (csrc/mevp_common.h), from the nodal fields a CPU twin remembers of its last packing:
    h', a C_o rho_o, mdt u0 + a tau_x - m f_c v_o, mdt v0 + a tau_y + m f_c u_o, u_o, v_o; the first four scaled by 2^100 at an ice-free
    node (with a = 1); a land node (land: bool [nm, nn]) holds (h_min, -1, 0, 0, 0, 0)"""
    from basal_ref import ice_free

    free = ice_free(p, cgh, cga)
    hn = np.maximum(cgh, _p(p, "h_min"))
    m = _p(p, "rho_ice") * hn
    a = np.where(free, 1.0, np.minimum(np.maximum(cga, 0.0), 1.0))
    w = np.where(free, 2.0 ** 100, 1.0)
    cor = m * _p(p, "fc")
    c = np.array([w * hn, w * (a * (_p(p, "c_ocean") * _p(p, "rho_ocean"))), w * ((m / dt) * u0 + a * tax - cor * vo),
                  w * ((m / dt) * v0 + a * tay + cor * uo), uo + 0.0 * hn, vo + 0.0 * hn])
    if land is not None:
        c[:, land] = np.array([_p(p, "h_min"), -1.0, 0.0, 0.0, 0.0, 0.0])[:, None]
    return c


class BudgetCalls:
    """abi.Context.momentum_budget on top of an OracleOps (and the land, basal, snow and tilt twins it is composed with): the forces of
    forces() from the nodal fields the last packing remembered -- under a height those carry the tilt in the start velocity
    (tilt_ref.start_velocity), so c2 = mdt u0' + a tau_x - m f_c v_o is the c2 of the packing with the height, to rounding -- and the row
    totals of row_totals().  Only the owned node rows of the planes asked for are written"""

    def momentum_budget(self, j0, j1, H, A, wind, s, uv, packed, planes=None, power=None, row0=0):
        import land_ref

        dt, (u0, v0), (tax, tay), (uo, vo), cgh, cga = self.nodal
        land = getattr(self, "land", None)
        ln = land_ref.land_nodes(land) if land is not None else None
        c = coefficients(self.p, dt, u0, v0, tax, tay, uo, vo, cgh, cga, ln)
        tb = getattr(self, "_tb", None)
        ssh = getattr(self, "ssh", None)
        u, v = uv[0].numpy(), uv[1].numpy()
        F = forces(self.p, dt, self.hx, self.hy, c, A.numpy(), wind[0].numpy(), wind[1].numpy(), [x.numpy() for x in s], u, v, tb=tb,
                   u0=self.bp["u0"] if tb is not None else 0.0, eta=None if ssh is None else ssh.numpy(), g=getattr(self, "gravity", TR.GRAVITY))
        rows = slice(2 * j0, 2 * j1 + (1 if j1 == self.ny else 0))
        for k, t in (planes or {}).items():
            t.numpy()[rows] = F[k][rows]
        if power is not None:
            power.numpy()[:, j0 - row0:j1 - row0] = row_totals(F, u, v, self.hx, self.hy, j0, j1)


def make_ops(land=False, basal=False, snow=False, tilt=False, **mevp):
    """the twin composed as the setting needs it, in the order tilt_ref.TiltLandOracleOps composes its own"""
    import basal_ref
    import land_ref
    import snow_ref
    from oracle_ops import OracleOps

    base = basal_ref.BasalOracleOps if basal else (land_ref.LandOracleOps if land else OracleOps)
    bases = (BudgetCalls,) + ((TR.TiltCalls,) if tilt else ()) + ((snow_ref.SnowCalls,) if snow else ()) + (base,)
    return type("BudgetOracleOps", bases, {})(**mevp)


def BudgetOracleOps(**mevp):
    """the twin with every call: land mask, depth, snow load and sea-surface height beside the budget"""
    return make_ops(land=True, basal=True, snow=True, tilt=True, **mevp)

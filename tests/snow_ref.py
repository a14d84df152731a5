"""CPU reference of the snow load (include/nsdg_snow.h): the momentum equation feels the snow's weight.  numpy plus
the UNCHANGED oracle.

The construction is the substitution the header states.  The load enters the packing only through the thickness behind the nodal mass,
    hl = cgH + r max(cgS, 0),   r = rho_snow / rho_ice,
at the nodes that are neither land nor ice-free; hl >= cgH, so such a node is not ice-free on (hl, cgA) either.  Everything packed WITH a
snow field therefore equals what is packed WITHOUT one from the nodal thickness
    cgH_ref = where(ice_free(cgH, cgA), cgH, hl),
and the oracle (oracle_lib), which takes the nodal thickness as an argument, runs every sub-iteration on cgH_ref.  The seabed stress of a
depth array keeps reading cgH itself: with one the reference is composed from tests/basal_ref.py's pieces (basal_subcycle).

SnowOracleOps / SnowLandOracleOps / make_bbm_ops: the CPU twins of abi.Context for rowblock.CoupledCore(..., snow_load=True).
It lives under tests/ because it calls the oracle; the product never imports it."""
import numpy as np

import basal_ref
import land_ref
import oracle_lib as O
from basal_ref import get, ice_free
from oracle_ops import OracleOps

RHO_SNOW = 330.0  # NSDG_SNOW_DENSITY: the column step's rho_s


def loaded_thickness(p, rho_snow, cgh, cga, cgs):
    """cgH_ref: the nodal thickness that carries the snow's weight where the node is not ice-free on (cgH, cgA).  Two separately rounded
    operations and the where; r is one IEEE division"""
    r = rho_snow / get(p, "rho_ice")
    load = r * np.maximum(cgs, 0.0)
    hl = cgh + load
    return np.where(ice_free(p, cgh, cga), cgh, hl)


def load_nodal(p, rho_snow, cgh, cga, cgs, land=None):
    """what nsdg_snow_load_nodal writes: h' = max(cgH_ref, h_min), h_min at a land node (land: the ELEMENT mask or None)"""
    h = np.maximum(loaded_thickness(p, rho_snow, cgh, cga, cgs), get(p, "h_min"))
    if land is not None:
        h[land_ref.land_nodes(land)] = get(p, "h_min")
    return h


def nodal_snow(nx, ny, snow):
    """cgS: the oracle's nodal mean of the snow, [ny, nx] (the plane hsnow) or [nc, ny, nx] (the DG field S)"""
    snow = np.ascontiguousarray(snow, dtype=np.float64)
    return O.dg_to_cg(nx, ny, snow.reshape((-1, ny, nx)))


def basal_subcycle(nx, ny, hx, hy, dt, nsub, p, bp, depth, land, rho_snow, cgs, s, u, v, u0, v0, tax, tay, uo, vo, cgh, cga, pg):
    """basal_ref.subcycle under a snow load: T_b from cgH, the oracle, the denominator D and beta_n from cgH_ref.  Returns T_b"""
    href = loaded_thickness(p, rho_snow, cgh, cga, cgs)
    ln = land_ref.land_nodes(land) if land is not None else None
    tb = basal_ref.critical_stress(p, bp, cgh, cga, depth, land)
    ad = p.aevp_c > 0
    alpha_e = np.zeros((ny, nx)) if ad else None
    u0, v0 = u0.copy(), v0.copy()
    for _ in range(nsub):
        O.mevp_stress(nx, ny, 0, ny, hx, hy, p, u, v, pg, *s, **(dict(dt=dt, cgh=href, cga=cga, alpha_e=alpha_e) if ad else {}))
        un, vn = np.zeros_like(u), np.zeros_like(v)
        O.mevp_velocity(nx, ny, 0, ny, hx, hy, dt, p, s, (u, v), (un, vn), (u0, v0), (tax, tay), (uo, vo), href, cga, **(dict(alpha_e=alpha_e) if ad else {}))
        f = basal_ref.factor(basal_ref.denominator(p, dt, href, cga, u, v, uo, vo, basal_ref.node_beta(p, href, cga, alpha_e)), tb, u, v, bp["u0"])
        un *= f
        vn *= f
        if ln is not None:
            un[ln] = 0.0
            vn[ln] = 0.0
        u[:], v[:] = un, vn
    return tb


class SnowCalls:
    """the snow-load calls of abi.Context on top of an OracleOps: the field is remembered, and the nodal thickness every packing remembers
    is cgH_ref"""

    snow, rho_snow = None, RHO_SNOW

    def set_grid(self, nx, ny, hx, hy):
        if (nx, ny) != (getattr(self, "nx", None), getattr(self, "ny", None)):
            self.snow = None  # nsdg_grid_set: a new shape drops the field
        super().set_grid(nx, ny, hx, hy)

    def set_snow_load(self, snow, rho_snow=RHO_SNOW):
        if snow is None:
            self.snow = None
            return
        assert tuple(snow.shape[-2:]) == (self.ny, self.nx) and (snow.dim() == 2 or snow.shape[0] in (1, 3, 6))
        assert np.isfinite(rho_snow) and rho_snow >= 0.0
        self.snow, self.rho_snow = snow, float(rho_snow)  # the tensor itself: read at the packing, as the device reads the pointer

    def _cgs(self):
        return nodal_snow(self.nx, self.ny, self.snow.numpy())

    def snow_load_nodal(self, cgh, cga, out):
        assert self.snow is not None
        out.numpy()[:] = load_nodal(self.p, self.rho_snow, cgh.numpy(), cga.numpy(), self._cgs(), getattr(self, "land", None))

    def _load(self):
        if self.snow is None:
            return
        dt, u0v0, tau, ocean, cgh, cga = self.nodal
        self.nodal = (dt, u0v0, tau, ocean, loaded_thickness(self.p, self.rho_snow, cgh, cga, self._cgs()), cga)

    def mevp_prepare(self, *a):
        super().mevp_prepare(*a)
        self._load()

    def mevp_pack_nodal(self, *a):
        super().mevp_pack_nodal(*a)
        self._load()


class SnowOracleOps(SnowCalls, OracleOps):
    pass


class SnowLandOracleOps(SnowCalls, land_ref.LandOracleOps):
    """the masked twin: land nodes are packed with constants whatever the thickness, and zeroed after every sub-iteration"""


def make_bbm_ops(bbm=None, **mevp):
    """tests/bbm_ref.py's stand-in with the snow-load calls: its packing forms the nodal fields itself, and the thickness among them is
    replaced by cgH_ref"""
    import bbm_ref as B

    base = type(B.make_ops(bbm=bbm, **mevp))

    class SnowBbmRefOps(SnowCalls, base):
        def _load(self):
            if self.snow is None:
                return
            nod = self.bbm_nod
            nod["cgh"] = loaded_thickness(self.mp, self.rho_snow, nod["cgh"], nod["cga"], self._cgs())

        def snow_load_nodal(self, cgh, cga, out):
            assert self.snow is not None
            out.numpy()[:] = load_nodal(self.mp, self.rho_snow, cgh.numpy(), cga.numpy(), self._cgs(), self.land)

    return SnowBbmRefOps()

"""CPU reference of the land mask: coastlines as fixed nodes of the mEVP sub-cycle.

The construction is the one the scheme was checked with: the UNCHANGED oracle (oracle_lib: oracle_mevp_stress / oracle_mevp_velocity per
sub-iteration, the oracle's transport, limiter and cap) with the land nodes zeroed after every sub-iteration.  A CG2 node is a land node
if any element adjacent to it inside the array is land.  Nothing else knows about land.

coupled_steps(): the model steps of one domain written out against oracle_lib directly (no driver).
LandOracleOps:   the CPU twin of abi.Context for rowblock.DynamicsCore(..., land=mask): OracleOps plus the three land calls, variant 1
                 only (one sub-iteration per pass; the device's passes of 2, 3 and 4 are pinned to its single sub-iterations bit for bit).
It lives under tests/ because it calls the oracle; the product never imports it."""
import numpy as np

import oracle_lib as O
from oracle_ops import OracleOps

H_A_BOUNDS = ((0.0, float("inf"), False), (0.0, 1.0, True))  # the closure of the dynamics' transported fields (abi.H_A_BOUNDS)


def land_nodes(land):
    """[2ny+1, 2nx+1] bool: the CG2 nodes with a land element next to them (element (iy, ix) touches the nodes [2iy:2iy+3, 2ix:2ix+3])"""
    land = np.asarray(land) != 0
    ny, nx = land.shape
    out = np.zeros((2 * ny + 1, 2 * nx + 1), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out[dy:dy + 2 * ny:2, dx:dx + 2 * nx:2] |= land
    return out


def subcycle(nx, ny, hx, hy, dt, nsub, p, land, s, u, v, u0, v0, tax, tay, uo, vo, cgh, cga, pg, omp=False):
    """nsub sub-iterations in place on s (3 x [8, ny, nx]), u, v: oracle stress + velocity, land nodes zeroed after each
    (omp: the oracle's OpenMP build, bit-identical to the serial one)"""
    ln = land_nodes(land)
    ad = p.aevp_c > 0
    alpha_e = np.zeros((ny, nx)) if ad else None
    u0, v0 = u0.copy(), v0.copy()
    for _ in range(nsub):
        O.mevp_stress(nx, ny, 0, ny, hx, hy, p, u, v, pg, *s, **(dict(dt=dt, cgh=cgh, cga=cga, alpha_e=alpha_e) if ad else {}), omp=omp)
        un, vn = np.zeros_like(u), np.zeros_like(v)
        O.mevp_velocity(nx, ny, 0, ny, hx, hy, dt, p, s, (u, v), (un, vn), (u0, v0), (tax, tay), (uo, vo), cgh, cga,
                        **(dict(alpha_e=alpha_e) if ad else {}), omp=omp)
        un[ln] = 0.0
        vn[ln] = 0.0
        u[:], v[:] = un, vn


def coupled_steps(nx, ny, hx, hy, dt, nsub, nsteps, p, land, H, A, uo, vo, ua, va, u=None, v=None, each=None, omp=False):
    """nsteps model steps of the dynamics (sub-cycle + SSP-RK3 DG2 transport of H, A with the closure) on one domain with the element
    mask `land` ([ny, nx], None = no land).  The inputs are not modified; land elements of H, A and land nodes of u, v are cleared first
    (what DynamicsCore.load_global does).  Returns dict(H, A, u, v, s); each(step, state) is called after every step"""
    land = np.zeros((ny, nx), dtype=bool) if land is None else np.asarray(land) != 0
    ln = land_nodes(land)
    H, A = H.copy(), A.copy()
    H[:, land] = 0.0
    A[:, land] = 0.0
    shape = (2 * ny + 1, 2 * nx + 1)
    u = np.zeros(shape) if u is None else u.copy()
    v = np.zeros(shape) if v is None else v.copy()
    u[ln] = 0.0
    v[ln] = 0.0
    uo, vo, ua, va = (np.ascontiguousarray(a) for a in (uo, vo, ua, va))
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    for step in range(nsteps):
        pg = O.ice_strength(nx, ny, p, H, A, omp=omp)
        cgh, cga = O.dg_to_cg(nx, ny, H, omp=omp), O.dg_to_cg(nx, ny, A, omp=omp)
        tax, tay = O.wind_stress(p, ua, va, omp=omp)
        subcycle(nx, ny, hx, hy, dt, nsub, p, land, s, u, v, u, v, tax, tay, uo, vo, cgh, cga, pg, omp=omp)
        adv = O.prepare_advection(nx, ny, 2, u, v, omp=omp)
        new = []
        for f, (lo, hi, cap) in zip((H, A), H_A_BOUNDS):
            t1, t2 = np.zeros_like(f), np.zeros_like(f)
            O.transport_stage(nx, ny, 0, ny, hx, hy, 2, dt, 0.0, 1.0, f, f, t1, adv, omp=omp)
            O.transport_stage(nx, ny, 0, ny, hx, hy, 2, dt, 0.75, 0.25, f, t1, t2, adv, omp=omp)
            O.transport_stage(nx, ny, 0, ny, hx, hy, 2, dt, 1.0 / 3.0, 2.0 / 3.0, f, t2, t1, adv, omp=omp)
            O.transport_limit(nx, ny, 2, t1, lo, hi, cap, omp=omp)
            new.append(t1)
        H, A = new
        if each is not None:
            each(step, dict(H=H, A=A, u=u, v=v, s=s))
    return dict(H=H, A=A, u=u, v=v, s=s)


class LandOracleOps(OracleOps):
    """OracleOps with the land calls of abi.Context: the mask is remembered, land nodes are zeroed after every sub-iteration"""

    def __init__(self, **mevp):
        super().__init__(mevp_variant=1, **mevp)
        self.land = None

    def set_grid(self, nx, ny, hx, hy):
        if (nx, ny) != (getattr(self, "nx", None), getattr(self, "ny", None)):
            self.land = None  # nsdg_grid_set: a new shape drops the mask
        super().set_grid(nx, ny, hx, hy)

    def set_land_mask(self, land):
        if land is None:
            self.land = self._nodes = None
            return
        m = land.numpy() != 0
        assert m.shape == (self.ny, self.nx)
        self.land, self._nodes = m, land_nodes(m)

    def land_clear(self, f, j0=0, j1=None):
        if self.land is None:
            return
        j1 = self.ny if j1 is None else j1
        a = f.numpy().reshape(-1, self.ny, self.nx)
        a[:, j0:j1][:, self.land[j0:j1]] = 0.0

    def land_clear_nodes(self, u, v):
        if self.land is None:
            return
        u.numpy()[self._nodes] = 0.0
        v.numpy()[self._nodes] = 0.0

    def mevp_iterate(self, k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg):
        super().mevp_iterate(k0, j0, j1, s_in, s_out, uv_old, uv_new, packed, pg)
        self.land_clear_nodes(*uv_new)


def shapes_mask(nx, ny):
    """an island, a bay cut into a coast and a single-element rock, scaled to the array (the issue's shape case)"""
    m = np.zeros((ny, nx), dtype=bool)
    m[ny // 3:ny // 3 + max(ny // 6, 2), nx // 4:nx // 4 + max(nx // 5, 2)] = True  # island
    m[:, nx - max(nx // 8, 2):] = True  # a coast along the right edge ...
    m[ny // 2:ny // 2 + max(ny // 5, 2), nx - max(nx // 8, 2):nx - max(nx // 16, 1)] = False  # ... with a bay cut into it
    m[(3 * ny) // 4, nx // 2] = True  # rock
    return m

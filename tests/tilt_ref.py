"""CPU reference of the sea-surface tilt (include/nsdg_tilt.h): the tilt force -m g grad(eta) from a sea-surface
height on the CG2 lattice.  numpy plus the UNCHANGED oracle.

The gradient and the box test's height are restated here in numpy, operation for operation.  The sub-cycle is not restated: the term
(m / dt) u^n enters only the coefficient c2 (c3), and the mass cancels, so the packing WITH a height equals the packing WITHOUT one started
from
    u0' = u0 + dt (fc vo - g sx),     v0' = v0 - dt (fc uo + g sy)
(the first term takes the geostrophic tilt -m fc k x u_o out, the second puts -m g grad(eta) in).  The oracle, which takes u0, v0 as
arguments, runs every sub-iteration from (u0', v0').

TiltOracleOps / TiltLandOracleOps: the CPU twins of abi.Context for rowblock.DynamicsCore(..., tilt="ssh").
It lives under tests/ because it calls the oracle; the product never imports it."""
import numpy as np

import land_ref
from oracle_ops import OracleOps

GRAVITY = 9.81  # NSDG_GRAVITY


def gradient(eta, hx, hy):
    """(sx, sy) on the [2ny+1, 2nx+1] lattice whose nodes are hx/2, hy/2 apart: the centred difference over hx (hy), on the outermost
    column (row) twice the one-sided difference over the same divisor.  A difference and one division per value, as the device"""
    eta = np.asarray(eta, dtype=np.float64)
    dx, dy = np.empty_like(eta), np.empty_like(eta)
    dx[:, 1:-1] = eta[:, 2:] - eta[:, :-2]
    dx[:, 0] = 2.0 * (eta[:, 1] - eta[:, 0])
    dx[:, -1] = 2.0 * (eta[:, -1] - eta[:, -2])
    dy[1:-1] = eta[2:] - eta[:-2]
    dy[0] = 2.0 * (eta[1] - eta[0])
    dy[-1] = 2.0 * (eta[-1] - eta[-2])
    return dx / hx, dy / hy


def box_xy(nx, ny, L, row0=0, ny_glob=None):
    """x, y of nsdg_boxtest_forcing at the nodes of a local array of ny rows placed at element row row0 of ny_glob"""
    ny_glob = ny if ny_glob is None else ny_glob
    x = np.arange(2 * nx + 1) * (L / (2 * nx))
    y = (np.arange(2 * ny + 1) + 2 * row0) * (L / (2 * ny_glob))
    return x[None, :], y[:, None]


def box_ssh(nx, ny, L, fc, g=GRAVITY, row0=0, ny_glob=None):
    """eta = -(fc / g) (0.01 / L) [x (x - L) + y (y - L)]: the height whose geostrophic current is the box test's gyre"""
    x, y = box_xy(nx, ny, L, row0, ny_glob)
    k = -(fc / g) * (0.01 / L)
    return k * (x * (x - L) + y * (y - L))


def box_ocean(nx, ny, L, row0=0, ny_glob=None):
    """(uo, vo) of nsdg_boxtest_forcing"""
    x, y = box_xy(nx, ny, L, row0, ny_glob)
    return 0.01 * (2 * y - L) / L + 0.0 * x, 0.01 * (L - 2 * x) / L + 0.0 * y


def start_velocity(dt, fc, g, u0, v0, uo, vo, sx, sy):
    """(u0', v0'): the start of the step from which the unchanged sub-cycle computes what the tilt of the height computes"""
    return u0 + dt * (fc * vo - g * sx), v0 - dt * (fc * uo + g * sy)


class TiltCalls:
    """the tilt calls of abi.Context on top of an OracleOps: the field is remembered, and the start velocity every packing remembers is
    (u0', v0')"""

    ssh, gravity, row0, ny_glob = None, GRAVITY, 0, None

    def set_grid(self, nx, ny, hx, hy):
        if (nx, ny) != (getattr(self, "nx", None), getattr(self, "ny", None)):
            self.ssh = None  # nsdg_grid_set: a new shape drops the field
        super().set_grid(nx, ny, hx, hy)

    def set_block(self, row0, ny_glob):
        self.row0, self.ny_glob = int(row0), int(ny_glob)

    def set_tilt(self, ssh, gravity=GRAVITY):
        if ssh is None:
            self.ssh = None
            return
        assert tuple(ssh.shape) == (2 * self.ny + 1, 2 * self.nx + 1)
        assert np.isfinite(gravity) and gravity > 0.0
        self.ssh, self.gravity = ssh, float(gravity)  # the tensor itself: read at the packing, as the device reads the pointer

    def tilt_nodal(self, sx, sy):
        assert self.ssh is not None
        sx.numpy()[:], sy.numpy()[:] = gradient(self.ssh.numpy(), self.hx, self.hy)

    def boxtest_ssh(self, domain_size, fc, gravity, ssh):
        ssh.numpy()[:] = box_ssh(self.nx, self.ny, domain_size, fc, gravity, self.row0, self.ny_glob or self.ny)

    def _tilt(self):
        if self.ssh is None:
            return
        dt, (u0, v0), tau, (uo, vo), cgh, cga = self.nodal
        sx, sy = gradient(self.ssh.numpy(), self.hx, self.hy)
        nodes = getattr(self, "_nodes", None) if getattr(self, "land", None) is not None else None
        if nodes is not None:  # a land node reads nothing of eta and is held at rest whatever it starts from
            sx, sy = np.where(nodes, 0.0, sx), np.where(nodes, 0.0, sy)
        self.nodal = (dt, list(start_velocity(dt, self.p.fc, self.gravity, u0, v0, uo, vo, sx, sy)), tau, [uo, vo], cgh, cga)

    def mevp_prepare(self, *a):
        super().mevp_prepare(*a)
        self._tilt()

    def mevp_pack_nodal(self, *a):
        super().mevp_pack_nodal(*a)
        self._tilt()


class TiltOracleOps(TiltCalls, OracleOps):
    pass


class TiltLandOracleOps(TiltCalls, land_ref.LandOracleOps):
    """the masked twin: land nodes are zeroed after every sub-iteration, whatever eta holds inside land"""

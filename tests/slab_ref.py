"""The slab ocean of include/nsdg_ocean.h restated in numpy, operation for operation (TEST INFRASTRUCTURE): every
line of update() is one IEEE fp64 operation on arrays, in the header's order, so the device's sst and sss are held to it bit for bit.  It
takes what a plain column step took and gave -- the planes before, hice and hsnow after, and the diagnostic planes -- and returns the new
sst and sss.  SlabOps is the CPU stand-in on tests/tracers_ops.py::TracersOps whose column_step_ocean is the oracle's column step with
diagnostics plus the restatement, so that a CoupledCore(slab_ocean=True) runs without a device."""
import numpy as np

import oracle_lib as O
from tracers_ops import TracersOps

# the column step's constants (csrc/column_step.hip; core/src/include/constants.hpp of the reference)
RHO_W, C_P, RHO_I, RHO_S, L_F, ICE_S = 1025.0, 4186.84, 917.0, 330.0, 333.55e3, 5.0
MU = 0.055  # linear freezing point: T_f = -MU sss


class SlabParams:
    """nsdg_slab_params without the library"""

    def __init__(self, relax_t=0.0, relax_s=0.0, ice_salinity=ICE_S):
        self.relax_t, self.relax_s, self.ice_salinity = float(relax_t), float(relax_s), float(ice_salinity)


def check_params(p):
    """the rule of nsdg_slab_params_set"""
    for k in ("relax_t", "relax_s", "ice_salinity"):
        v = getattr(p, k)
        if not (np.isfinite(v) and v >= 0):
            raise ValueError("nsdg_slab_params_set: %s must be finite and >= 0" % k)


def evaporation(drag_ocean_q, rho, wind, qw, qa):
    """evap as the kernel writes it: drag_ocean_q * rho * wind * (q_w - q_a), left to right (no product-sum to fuse)"""
    return ((drag_ocean_q * rho) * wind) * (qw - qa)


def update(dt, before, after, diag, params=None, drag_ocean_q=1.5e-3, ext=None, skip=None):
    """(sst, sss) after the step.  before: cice, hice, hsnow, sst, sss, mld, snowfall, wind before the step; after: hice, hsnow after it;
    diag: the planes rho, qa, qw, qio, qow, subl of that step by name; ext: {"sst", "sss"} targets (read only under their relaxation)"""
    p = params or SlabParams()
    dt = np.float64(dt)
    c, T, S, mld = before["cice"], before["sst"], before["sss"], before["mld"]
    evap = evaporation(np.float64(drag_ocean_q), diag["rho"], before["wind"], diag["qw"], diag["qa"])
    with np.errstate(all="ignore"):
        m1 = mld * RHO_W
        mlbhc = m1 * C_P
        oc = 1.0 - c
        a = c * diag["qio"]
        b = oc * diag["qow"]
        qnet = a + b
        e = qnet * dt
        q = e / mlbhc
        T1 = T - q
        if p.relax_t > 0:
            g = dt / np.float64(p.relax_t)
            d = ext["sst"] - T
            r = g * d
            T1 = T1 + r
        dh = after["hice"] - before["hice"]
        dMi = RHO_I * dh
        ds = after["hsnow"] - before["hsnow"]
        dMs = RHO_S * ds
        f = c * diag["subl"]
        g = oc * evap
        v = f + g
        pw = before["snowfall"] - v
        w = pw * dt
        w = w - dMi
        W = w - dMs
        M = RHO_W * mld
        x = M * S
        y = np.float64(p.ice_salinity) * dMi
        z = x - y
        D = M + W
        S1 = z / D
        if p.relax_s > 0:
            g = dt / np.float64(p.relax_s)
            d = ext["sss"] - S
            r = g * d
            S1 = S1 + r
    if skip is not None:
        keep = np.asarray(skip).reshape(np.shape(T)) != 0
        T1, S1 = np.where(keep, T, T1), np.where(keep, S, S1)
    return T1, S1


def water(dt, before, after, diag, drag_ocean_q=1.5e-3):
    """(M, W, dMi) of update(), for the salt identity"""
    c = before["cice"]
    evap = evaporation(np.float64(drag_ocean_q), diag["rho"], before["wind"], diag["qw"], diag["qa"])
    dMi = RHO_I * (after["hice"] - before["hice"])
    dMs = RHO_S * (after["hsnow"] - before["hsnow"])
    W = ((before["snowfall"] - (c * diag["subl"] + (1.0 - c) * evap)) * np.float64(dt) - dMi) - dMs
    return RHO_W * before["mld"], W, dMi


BEFORE = ("cice", "hice", "hsnow", "sst", "sss", "mld", "snowfall", "wind")


def column_step_ocean(cp, dt, state, forcing, newice, params=None, ext=None, skip=None, omp=False):
    """the oracle's column step with diagnostics plus update(), in place on numpy planes (sst, sss of `forcing` included)"""
    before = {k: (state[k] if k in state else forcing[k]).copy() for k in BEFORE}
    diag = O.column_step(cp, dt, state, forcing, newice, want_diag=True, omp=omp)
    T1, S1 = update(dt, before, state, diag, params, cp.drag_ocean_q, ext, skip)
    forcing["sst"][...] = T1
    forcing["sss"][...] = S1
    return diag


class SlabOps(TracersOps):
    """TracersOps and the slab-ocean calls of abi.Context"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.slab = SlabParams()

    def slab_default_params(self, **kw):
        return SlabParams(**kw)

    def set_slab_params(self, p):
        check_params(p)
        self.slab = SlabParams(p.relax_t, p.relax_s, p.ice_salinity)

    def column_step_ocean(self, dt, state, forcing, newice, ext=None, skip=None):
        st = {k: v.numpy().reshape(-1) for k, v in state.items()}
        fo = {k: v.numpy().reshape(-1) for k, v in forcing.items()}
        ex = {k: v.numpy().reshape(-1) for k, v in (ext or {}).items() if v is not None}
        if (self.slab.relax_t > 0 and "sst" not in ex) or (self.slab.relax_s > 0 and "sss" not in ex):
            raise ValueError("nsdg_column_step_ocean: null relaxation target while its relaxation is on")
        column_step_ocean(self.cp, dt, st, fo, newice.numpy().reshape(-1), self.slab, ex, None if skip is None else skip.numpy().reshape(-1), self.omp)


def slab_ops(**mevp):
    """the stand-in with uniform alpha = beta = 200 unless told otherwise (the single-iteration sub-cycle: ghost depth (1, 1))"""
    mevp.setdefault("alpha", 200.0)
    mevp.setdefault("beta", 200.0)
    return SlabOps(**mevp)

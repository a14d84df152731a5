"""numpy restatements of the sub-stepping rule (include/nsdg.h "sub-stepping"): the strength wave speed, the number of sub-steps and the
largest clamped concentration at the 3x3 Gauss points -- what nsdg_substep_count and nsdg_concentration_max compute."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def psi_g3():
    """the kernels' table of the DG2 basis at the 3x3 Gauss points (csrc/dg_tables.h PSI_G3), first 6 coefficients: [9, 6]"""
    src = open(os.path.join(ROOT, "nextsimdg_amd", "csrc", "dg_tables.h")).read()
    body = re.search(r"PSI_G3\[9\]\[8\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = re.findall(r"\{([^{}]*)\}", body)
    return np.array([[float(x) for x in r.split(",")] for r in rows])[:, :6]


def wave_speed(amax, pstar=27.5e3, compaction=20.0, rho_ice=900.0):
    return np.sqrt((1.0 + compaction * amax) * pstar * np.exp(-compaction * (1.0 - amax)) / (2.0 * rho_ice))


def substep_count(amax, h, dt, courant=1.5, **kw):
    """(n, c, ratio): n = max(1, ceil(c dt / (courant h)))"""
    c = wave_speed(amax, **kw)
    ratio = c * dt / (courant * h)
    return max(1, int(np.ceil(ratio))), c, ratio


def concentration_max(H, A, j0=0, j1=None):
    """largest clamp(A, 0, 1) at the Gauss points of rows [j0, j1) where max(H, 0) > 0 (0 if none); H, A: [6, ny, nx].  ValueError on a
    non-finite coefficient or point value"""
    H, A = np.asarray(H)[:6], np.asarray(A)[:6]
    j1 = H.shape[1] if j1 is None else j1
    h, a = H[:, j0:j1], A[:, j0:j1]
    if not (np.isfinite(h).all() and np.isfinite(a).all()):
        raise ValueError("non-finite H or A")
    P = psi_g3()
    hq = np.einsum("qc,cyx->qyx", P, h)
    aq = np.einsum("qc,cyx->qyx", P, a)
    if not (np.isfinite(hq).all() and np.isfinite(aq).all()):
        raise ValueError("non-finite H or A at a Gauss point")
    aq = np.clip(aq, 0.0, 1.0)
    sel = np.maximum(hq, 0.0) > 0.0
    return float(aq[sel].max()) if sel.any() else 0.0

"""numpy restatement of the ice tracers (include/nsdg.h "ice tracers"), written from the formulas of the header: up to four intensive
planes T_k ride on the ice as Q_k = H T_k, are divided back where the element holds ice (the tracer of the kind AGE grows by dt there) and
are zero where it does not; thermodynamic growth dilutes them with ice of the value 0.  The GPU tests hold nsdg_tracers_weight /
nsdg_tracers_recover / nsdg_tracers_dilute to these bit for bit.  Every operation is one IEEE fp64 operation, as in the header."""
import numpy as np

from column_transport_ref import MIN_CONC, MIN_THICK, holds_ice  # the ice test is the one of nsdg_tracer_recover

PASSIVE, AGE = 0, 1
TRACERS_MAX = 4


def _rows(shape, j0, j1):
    rows = np.zeros(shape, dtype=bool)
    rows[j0:shape[0] if j1 is None else j1] = True
    return rows


def weight(H, T, j0=0, j1=None, Q=None):
    """Q[k][c, j, i] = T[k][j, i] * H[c, j, i] on the rows [j0, j1); other rows: as given in Q (zeros if Q is None).  Returns a list"""
    H = np.asarray(H, dtype=np.float64)
    j1 = H.shape[1] if j1 is None else j1
    out = []
    for k, t in enumerate(T):
        q = np.zeros_like(H) if Q is None else np.array(Q[k], dtype=np.float64, copy=True)
        q[:, j0:j1] = np.asarray(t, dtype=np.float64)[None, j0:j1] * H[:, j0:j1]
        out.append(q)
    return out


def recover(H, A, Q, kinds, dt, T, min_conc=MIN_CONC, min_thick=MIN_THICK, j0=0, j1=None):
    """on the rows [j0, j1): where the element holds ice T[k] = Q[k][0] / H[0], plus dt for kinds[k] == AGE; where it does not, 0.  Other
    rows: as given in T.  Returns a list of new arrays"""
    H0, A0 = np.asarray(H, dtype=np.float64)[0], np.asarray(A, dtype=np.float64)[0]
    rows = _rows(H0.shape, j0, j1)
    ice = holds_ice(H0, A0, min_conc, min_thick)
    out = []
    for q, kind, t in zip(Q, kinds, T):
        if kind not in (PASSIVE, AGE):
            raise ValueError("unknown tracer kind %r" % (kind,))
        new = np.array(t, dtype=np.float64, copy=True)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r = np.asarray(q, dtype=np.float64)[0][ice & rows] / H0[ice & rows]
            new[ice & rows] = r + dt if kind == AGE else r
        new[~ice & rows] = 0.0
        out.append(new)
    return out


def dilute(h_before, h_after, T, j0=0, j1=None):
    """on the rows [j0, j1), with hb = h_before > 0 ? h_before : 0 and ha = h_after: !(ha > 0): T = 0; else ha > hb: T = (T hb) / ha; else
    T unchanged.  Returns a list of new arrays"""
    b, ha = np.asarray(h_before, dtype=np.float64), np.asarray(h_after, dtype=np.float64)
    rows = _rows(ha.shape, j0, j1)
    with np.errstate(invalid="ignore"):
        hb = np.where(b > 0.0, b, 0.0)
        none = ~(ha > 0.0) & rows
        grown = (ha > 0.0) & (ha > hb) & rows
    out = []
    for t in T:
        new = np.array(t, dtype=np.float64, copy=True)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            new[grown] = (new[grown] * hb[grown]) / ha[grown]
        new[none] = 0.0
        out.append(new)
    return out


def tracer_content(H, T, A=None, min_conc=MIN_CONC, min_thick=MIN_THICK):
    """sum over the elements that hold ice of mean(H) T -- what the transport of Q = H T conserves (all elements when A is None)"""
    H0 = np.asarray(H)[0]
    ice = np.ones(H0.shape, dtype=bool) if A is None else holds_ice(H0, np.asarray(A)[0], min_conc, min_thick)
    return float(np.sum(H0[ice] * np.asarray(T)[ice]))

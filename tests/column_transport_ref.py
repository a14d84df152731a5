"""numpy restatement of the column state transport (include/nsdg.h "column state transport"): the surface temperature T rides on the
ice as Q = H T, weighted by the ice volume H, and is divided back after the transport where the element holds ice.  The GPU tests hold
nsdg_tracer_weight / nsdg_tracer_recover to these, bit for bit."""
import numpy as np

MIN_CONC, MIN_THICK = 1e-12, 0.01  # the ice-free-node rule's defaults (nsdg_mevp_default_params, dynamics.min_conc / min_thick)
# closure of the four advected fields of a coupled step with the mode on: H >= 0, A in [0, 1] capped, snow S >= 0, Q unbounded
BOUNDS = ((0.0, np.inf, False), (0.0, 1.0, True), (0.0, np.inf, False), (-np.inf, np.inf, False))


def weight(H, T, j0=0, j1=None, Q=None):
    """Q[c, j, i] = T[j, i] * H[c, j, i] on the rows [j0, j1) (other rows of Q: as given, zero if Q is None)"""
    H = np.asarray(H, dtype=np.float64)
    out = np.zeros_like(H) if Q is None else np.array(Q, dtype=np.float64, copy=True)
    j1 = H.shape[1] if j1 is None else j1
    out[:, j0:j1] = np.asarray(T, dtype=np.float64)[None, j0:j1] * H[:, j0:j1]
    return out


def holds_ice(h, a, min_conc=MIN_CONC, min_thick=MIN_THICK):
    """the ice test of nsdg_tracer_recover on cell means: h > 0, a >= min_conc, h >= min_thick a (False where any of them is NaN)"""
    with np.errstate(invalid="ignore"):
        return (h > 0.0) & (a >= min_conc) & (h >= min_thick * a)


def recover(H, A, Q, T, min_conc=MIN_CONC, min_thick=MIN_THICK, j0=0, j1=None):
    """T = Q[0] / H[0] on the rows [j0, j1) where the element holds ice; T unchanged elsewhere (returns a new array)"""
    H0, A0, Q0 = (np.asarray(x, dtype=np.float64)[0] for x in (H, A, Q))
    out = np.array(T, dtype=np.float64, copy=True)
    j1 = H0.shape[0] if j1 is None else j1
    rows = np.zeros(H0.shape, dtype=bool)
    rows[j0:j1] = True
    ice = holds_ice(H0, A0, min_conc, min_thick) & rows
    with np.errstate(divide="ignore", invalid="ignore"):
        out[ice] = Q0[ice] / H0[ice]
    return out


def heat_content(H, T, A=None, min_conc=MIN_CONC, min_thick=MIN_THICK):
    """sum over the elements that hold ice of mean(H) T -- what the transport of Q conserves (all elements when A is None)"""
    H0 = np.asarray(H)[0]
    ice = np.ones(H0.shape, dtype=bool) if A is None else holds_ice(H0, np.asarray(A)[0], min_conc, min_thick)
    return float(np.sum(H0[ice] * np.asarray(T)[ice]))

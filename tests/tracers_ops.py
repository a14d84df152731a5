"""CPU stand-ins for the ice-tracer calls of abi.Context (include/nsdg.h "ice tracers") on top of the oracle stand-in (tests/oracle_ops.py
with the land calls of tests/land_ref.py), backed by the numpy restatement tests/tracers_ref.py; and the single-tracer calls of the column
state transport from tests/column_transport_ref.py, so that a CoupledCore with advect_column_state runs on them too."""
import column_transport_ref as C
import tracers_ref as R
from land_ref import LandOracleOps


def _fill(dst, arrays):
    for d, a in zip(dst, arrays):
        d.numpy()[...] = a


class TracersOps(LandOracleOps):
    def copy_f64(self, dst, src):
        dst.copy_(src)

    def tracers_weight(self, order, j0, j1, H, T, Q):
        assert 1 <= len(T) == len(Q) <= R.TRACERS_MAX
        _fill(Q, R.weight(H.numpy(), [t.numpy() for t in T], j0, j1, Q=[q.numpy() for q in Q]))

    def tracers_recover(self, order, j0, j1, H, A, Q, kinds, dt, min_conc, min_thick, T):
        assert 1 <= len(T) == len(Q) == len(kinds) <= R.TRACERS_MAX
        _fill(T, R.recover(H.numpy(), A.numpy(), [q.numpy() for q in Q], kinds, dt, [t.numpy() for t in T], min_conc, min_thick, j0, j1))

    def tracers_dilute(self, j0, j1, h_before, h_after, T):
        assert 1 <= len(T) <= R.TRACERS_MAX
        _fill(T, R.dilute(h_before.numpy(), h_after.numpy(), [t.numpy() for t in T], j0, j1))

    def tracer_weight(self, order, j0, j1, H, T, Q):
        q = Q.numpy()
        q[:] = C.weight(H.numpy(), T.numpy(), j0, j1, Q=q)

    def tracer_recover(self, order, j0, j1, H, A, Q, min_conc, min_thick, T):
        t = T.numpy()
        t[:] = C.recover(H.numpy(), A.numpy(), Q.numpy(), t, min_conc, min_thick, j0, j1)


def tracers_ops(**mevp):
    """the stand-in with uniform alpha = beta = 200 unless told otherwise (the single-iteration sub-cycle: ghost depth (1, 1))"""
    mevp.setdefault("alpha", 200.0)
    mevp.setdefault("beta", 200.0)
    return TracersOps(**mevp)

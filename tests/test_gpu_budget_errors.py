"""Error behaviour of nsdg_momentum_budget on a live context, in the manner of tests/test_abi_errors_gpu.py: every error case of
include/nsdg_budget.h returns its status with a message, and launches nothing -- the output planes and the totals still hold their canary."""
import ctypes as C

import pytest
import torch

from nextsimdg_amd import abi

pytestmark = pytest.mark.gpu
NX, NY = 70, 6
CANARY = -3.0
OK, ERR_ARG, ERR_STATE = 0, -1, -3  # NSDG_OK, NSDG_ERR_ARG, NSDG_ERR_STATE


def z(*shape):
    return torch.zeros(*shape, dtype=torch.float64, device="cuda")


class Args:
    """a valid call on a 70 x 6 grid; call(**replacements) makes the raw ABI call and returns (status, message)"""

    def __init__(self, ctx):
        self.ctx = ctx
        n = (2 * NX + 1) * (2 * NY + 1)
        self.t = dict(H=z(6, NY, NX), A=z(6, NY, NX), ua=z(n), va=z(n), s11=ctx.private_zeros(8, NY, NX, "cuda"), s12=ctx.private_zeros(8, NY, NX, "cuda"),
                      s22=ctx.private_zeros(8, NY, NX, "cuda"), u=z(n), v=z(n), packed=z(8 * n))
        self.t["H"][0] = 1.0
        self.t["A"][0] = 0.9
        self.planes = {k: torch.full((n,), CANARY, dtype=torch.float64, device="cuda") for k in ("wind_x", "residual_y")}
        self.power = torch.full((abi.BUDGET_QUANTITIES, NY), CANARY, dtype=torch.float64, device="cuda")

    def out(self, **kw):
        o = abi.BudgetOut()
        for k, t in self.planes.items():
            setattr(o, k, t.data_ptr())
        o.power, o.power_stride, o.row0 = self.power.data_ptr(), NY, 0
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(self, ctx=None, j0=0, j1=NY, out=None, null_out=False, **repl):
        ctx = ctx or self.ctx
        ptr = lambda k: repl[k] if k in repl else self.t[k].data_ptr()
        o = out if out is not None else self.out()
        rc = ctx.lib.nsdg_momentum_budget(ctx.h, j0, j1, *[ptr(k) for k in ("H", "A", "ua", "va", "s11", "s12", "s22", "u", "v", "packed")],
                                          None if null_out else C.byref(o))
        torch.cuda.synchronize()
        return rc, ctx.lib.nsdg_last_error().decode()

    def untouched(self):
        return all(bool((t == CANARY).all()) for t in self.planes.values()) and bool((self.power == CANARY).all())


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def test_every_error_case_returns_its_status_and_launches_nothing(ctx, gpu):
    fresh = abi.Context(gpu)
    a = Args(ctx)
    rc, msg = a.call(ctx=fresh)  # no grid set
    assert rc == ERR_STATE and "nsdg_grid_set was not called" in msg and a.untouched()
    fresh.set_grid(NX, NY, 1000.0, 1000.0)
    rc, msg = a.call(ctx=fresh)  # no packing on the context
    assert rc == ERR_STATE and "no packing" in msg and a.untouched()
    fresh.close()
    ctx.set_grid(NX, NY, 1000.0, 1000.0)
    t = a.t
    ctx.mevp_prepare(120.0, t["H"].view(6, NY, NX), t["A"].view(6, NY, NX), (t["ua"], t["va"]), (t["ua"], t["va"]), (t["u"], t["v"]), t["packed"])
    for j0, j1 in ((-1, NY), (0, NY + 1), (4, 3)):
        rc, msg = a.call(j0=j0, j1=j1)
        assert rc == ERR_ARG and "row range" in msg and a.untouched(), (j0, j1)
    for k in ("H", "A", "ua", "va", "s11", "s12", "s22", "u", "v", "packed"):
        rc, msg = a.call(**{k: None})
        assert rc == ERR_ARG and "null" in msg and a.untouched(), k
    rc, msg = a.call(null_out=True)
    assert rc == ERR_ARG and "null" in msg and a.untouched()
    for k in ("s11", "s12", "s22"):  # untiled: not 16-byte aligned
        rc, msg = a.call(**{k: t[k].data_ptr() + 8})
        assert rc == ERR_ARG and "16-byte aligned" in msg and a.untouched(), k
    rc, msg = a.call(packed=t["packed"].data_ptr() + 8)
    assert rc == ERR_ARG and "16-byte aligned" in msg and a.untouched()
    # an output that aliases an input, packed, or another output
    n = t["u"].numel()
    for k in ("A", "ua", "va", "s11", "s12", "s22", "u", "v", "packed"):  # (H is not read: an output may lie on it)
        rc, msg = a.call(out=a.out(wind_x=t[k].data_ptr()))
        assert rc == ERR_ARG and "overlaps" in msg and a.untouched(), k
    rc, msg = a.call(out=a.out(residual_y=t["packed"].data_ptr() + 8 * (8 * n - 1)))  # the last double of packed
    assert rc == ERR_ARG and "overlaps" in msg and a.untouched()
    rc, msg = a.call(out=a.out(power=t["u"].data_ptr()))
    assert rc == ERR_ARG and "overlaps" in msg and a.untouched()
    rc, msg = a.call(out=a.out(wind_x=a.planes["residual_y"].data_ptr() + 8 * (n - 1)))
    assert rc == ERR_ARG and "overlap" in msg and a.untouched()
    ssh = z(n)
    ctx.set_tilt(ssh)
    rc, msg = a.call(out=a.out(wind_x=ssh.data_ptr()))
    ctx.set_tilt(None)
    assert rc == ERR_ARG and "overlaps" in msg and a.untouched()
    # totals that do not hold the rows
    rc, msg = a.call(out=a.out(power_stride=NY - 1))
    assert rc == ERR_ARG and "power_stride" in msg and a.untouched()
    rc, msg = a.call(j0=1, j1=NY, out=a.out(row0=2))
    assert rc == ERR_ARG and "row0" in msg and a.untouched()
    rc, msg = a.call(j0=1, j1=NY, out=a.out(row0=-1))
    assert rc == ERR_ARG and "row0" in msg and a.untouched()
    # nothing to do is no error, and launches nothing either
    assert a.call(j0=3, j1=3)[0] == OK and a.untouched()
    assert a.call(out=abi.BudgetOut())[0] == OK and a.untouched()
    # and the valid call writes
    assert a.call()[0] == OK and not a.untouched()
    assert not any(bool((x == CANARY).any()) for x in a.planes.values()) and not bool((a.power == CANARY).any())


def test_term_ids_by_name(ctx):
    for i, name in enumerate(abi.BUDGET_TERMS):
        assert ctx.lib.nsdg_budget_term_id(name.encode()) == i
    assert abi.BUDGET_TERMS[0] == "wind" and abi.BUDGET_TERMS[7] == "residual"
    assert ctx.lib.nsdg_budget_term_id(b"ke") == -1 and ctx.lib.nsdg_budget_term_id(b"") == -1 and ctx.lib.nsdg_budget_term_id(None) == -1

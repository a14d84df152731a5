"""The column state transport (include/nsdg.h "column state transport") without a GPU: known answers of the numpy restatement of
nsdg_tracer_weight / nsdg_tracer_recover (tests/column_transport_ref.py) on every branch of the ice test, conservation of sum H T by that
restatement around the oracle's pure transport, and the C++ host's check of dynamics.advect_column_state."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import column_transport_ref as R  # noqa: E402


def test_weight_known_answers():
    H = np.arange(1.0, 1.0 + 6 * 2 * 3).reshape(6, 2, 3) * np.array([1.0, -0.5, 0.25, 0.0, 2.0, -1.0])[:, None, None]
    T = np.array([[-8.0, 0.5, 0.0], [-1.5, np.nan, 2.0]])
    Q = R.weight(H, T)
    for c in range(6):
        for j in range(2):
            for i in range(3):
                want = T[j, i] * H[c, j, i]
                assert (np.isnan(want) and np.isnan(Q[c, j, i])) or Q[c, j, i] == want
    assert Q[0, 0, 0] == -8.0 and Q[0, 0, 1] == 1.0 and Q[4, 1, 2] == 2.0 * H[4, 1, 2]
    # the row range: rows outside it keep what Q held
    Q2 = R.weight(H, T, 1, 2, Q=np.full_like(H, 7.0))
    assert np.all(Q2[:, 0] == 7.0) and Q2[0, 1, 0] == -1.5 * H[0, 1, 0]


def edge_case_inputs():
    """one element per branch of the ice test (min_conc = 1e-12, min_thick = 0.01): (H0, A0, Q0, T_before, T_after)"""
    mc, mt = R.MIN_CONC, R.MIN_THICK
    below = np.nextafter(mc, 0.0)
    a = 0.6
    thin = mt * a
    return [
        (0.5, 0.8, -4.0, 3.0, -8.0),  # ice: T = Q / H
        (0.5, mc, -1.0, 3.0, -2.0),  # A exactly at min_conc: ice
        (0.5, below, -1.0, 3.0, 3.0),  # A just below min_conc: unchanged
        (thin, a, thin * -5.0, 3.0, (thin * -5.0) / thin),  # H exactly at min_thick A: ice
        (np.nextafter(thin, 0.0), a, -1e-3, 3.0, 3.0),  # H just below min_thick A: unchanged
        (0.0, 0.7, 0.0, 3.0, 3.0),  # H = 0: unchanged (no 0 / 0)
        (-0.0, 0.0, 0.0, 3.0, 3.0),  # -0 and no ice at all
        (-1e-3, 0.5, 1e-3, 3.0, 3.0),  # a negative mean thickness: unchanged
        (np.nan, 0.5, 1.0, 3.0, 3.0),  # NaN H: unchanged
        (0.5, np.nan, 1.0, 3.0, 3.0),  # NaN A: unchanged
        (0.5, 0.5, np.nan, 3.0, np.nan),  # NaN Q where there is ice: NaN (an IEEE division)
        (0.5, 0.5, 1.0, np.nan, 2.0),  # a stale NaN temperature is replaced where there is ice
        (np.inf, 0.5, 1.0, 3.0, 0.0),  # H = inf passes the test: 1 / inf = 0
        (1e-13, 1e-12, 1e-13, 3.0, 1.0),  # tiny, but ice by the test
        (1e-300, 1e-300, 1e-300, 3.0, 3.0),  # tinier: A below min_conc
    ]


def test_recover_known_answers_on_every_branch_of_the_ice_test():
    cases = edge_case_inputs()
    n = len(cases)
    H, A, Q = np.zeros((6, 1, n)), np.zeros((6, 1, n)), np.zeros((6, 1, n))
    H[1:] = 123.0  # higher coefficients play no part
    A[1:] = -5.0
    Q[1:] = 9.0
    T = np.zeros((1, n))
    for k, (h, a, q, t, _) in enumerate(cases):
        H[0, 0, k], A[0, 0, k], Q[0, 0, k], T[0, k] = h, a, q, t
    got = R.recover(H, A, Q, T)
    for k, (h, a, q, t, want) in enumerate(cases):
        assert (np.isnan(want) and np.isnan(got[0, k])) or got[0, k] == want, (k, cases[k], got[0, k])
    assert got[0, 0] == -8.0 and got[0, 1] == -2.0 and got[0, 2] == 3.0
    # the input is not modified, and rows outside [j0, j1) keep their value
    assert T[0, 0] == 3.0
    two = R.recover(np.concatenate([H, H], 1), np.concatenate([A, A], 1), np.concatenate([Q, Q], 1), np.concatenate([T, T], 0), j0=1, j1=2)
    assert np.array_equal(two[0], T[0], equal_nan=True) and two[1, 0] == -8.0
    # min_conc = min_thick = 0 (closure off): only H > 0 and A >= 0 count
    loose = R.recover(H, A, Q, T, 0.0, 0.0)
    assert loose[0, 2] == -2.0 and loose[0, 4] == -1e-3 / np.nextafter(cases[3][0], 0.0) and loose[0, 5] == 3.0


def box_flow(n):
    """a CG2 velocity on the (2n+1)^2 lattice of the unit box that vanishes on the walls: a swirl that converges in one place and diverges
    in another"""
    g = np.linspace(0.0, 1.0, 2 * n + 1)
    x, y = np.meshgrid(g, g)
    bump = np.sin(np.pi * x) * np.sin(np.pi * y)
    u = 0.3 * bump * (np.cos(2 * np.pi * y) + 0.5 * np.sin(np.pi * x))
    v = 0.3 * bump * (np.sin(2 * np.pi * x) - 0.4 * np.cos(np.pi * y))
    return np.ascontiguousarray(u), np.ascontiguousarray(v)


def test_heat_content_is_conserved_by_a_pure_transport():
    """weight, the oracle's DG2 transport of H and Q (no closure), recover: sum mean(H) T over the ice is conserved to rounding, and a
    uniform T stays what it was"""
    import oracle_lib as O

    n = 24
    hx = hy = 1.0 / n
    rng = np.random.default_rng(5)
    H = np.zeros((6, n, n))
    H[0] = 0.5 + 0.4 * rng.random((n, n))  # ice everywhere: no element crosses the ice test
    H[1:] = 0.02 * rng.standard_normal((5, n, n))
    A = np.zeros((6, n, n))
    A[0] = 1.0
    T = -10.0 + 6.0 * rng.random((n, n))
    u, v = box_flow(n)
    adv = O.prepare_advection(n, n, 2, u, v)
    dt = 0.2 * hx / 0.3
    before = R.heat_content(H, T, A)
    Tu = np.full((n, n), -8.0)
    Hu = H.copy()
    for _ in range(20):
        Q = R.weight(H, T)
        Qu = R.weight(Hu, Tu)
        for f in (H, Q):
            O.transport_step(n, n, hx, hy, 2, dt, f, adv)
        for f in (Hu, Qu):
            O.transport_step(n, n, hx, hy, 2, dt, f, adv)
        assert np.all(R.holds_ice(H[0], A[0]))
        T = R.recover(H, A, Q, T)
        Tu = R.recover(Hu, A, Qu, Tu)
    after = R.heat_content(H, T, A)
    assert abs(after - before) <= 1e-12 * abs(before), (before, after)
    assert not np.allclose(T, -10.0 + 6.0 * np.random.default_rng(5).random((n, n)))  # the field has moved
    assert np.max(np.abs(Tu + 8.0)) <= 1e-13 * 8.0


def test_host_rejects_advect_column_state_without_thermodynamics(tmp_path):
    """dynamics.advect_column_state is checked when the step is configured, before any device is touched"""
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    host_dir = os.path.join(ROOT, "nextsimdg_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host_dir])
    cfg = os.path.join(str(tmp_path), "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n" % os.path.join(str(tmp_path), "x.nsdg"))
    host = os.path.join(host_dir, "build", "nextsim_amd")
    for args in (["--dynamics.advect_column_state=true"], ["--dynamics.advect_column_state=true", "--dynamics.thermodynamics=false"]):
        p = subprocess.run([host, "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
        out = p.stdout.decode()
        assert p.returncode != 0 and "dynamics.advect_column_state needs dynamics.thermodynamics = true" in out, (args, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(str(tmp_path), "x.nsdg")), out


# ---- the Python driver over gloo, with the oracle and the numpy restatement in place of the kernels -----------------------------------
NX, NY, NSUB = 20, 29, 5


def tracer_ops(variant):
    from oracle_ops import OracleOps

    class TracerOps(OracleOps):
        """the oracle plus the numpy restatement of nsdg_tracer_weight / nsdg_tracer_recover"""

        def tracer_weight(self, order, j0, j1, H, T, Q):
            q = Q.numpy()
            q[:] = R.weight(H.numpy(), T.numpy(), j0, j1, Q=q)

        def tracer_recover(self, order, j0, j1, H, A, Q, min_conc, min_thick, T):
            t = T.numpy()
            t[:] = R.recover(H.numpy(), A.numpy(), Q.numpy(), t, min_conc, min_thick, j0, j1)

    return TracerOps(mevp_variant=variant, alpha=200.0, beta=200.0)


def run_coupled(rank, world, variant, steps, resume=None):
    import torch
    from nextsimdg_amd import rowblock, synthetic

    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    depth = (variant, variant - 1) if variant >= 2 else (1, 1)
    core = rowblock.CoupledCore(tracer_ops(variant), rowblock.RowBlock(NX, NY, rank, world, *depth), bt.hx, bt.hy, 120.0, NSUB,
                                torch.device("cpu"), advect_column_state=True)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    state, forcing, _ = synthetic.column_fields(NX * NY, 5)
    col = {k: v.reshape(NY, NX) for k, v in {**state, **forcing}.items()}
    col["wind"] = 0.2 * col["wind"]
    col["hsnow"] = 0.1 * rng.random((NY, NX))
    col["tice0"] = rng.uniform(-15.0, -2.0, (NY, NX))
    core.load_column(col)
    if resume is not None:
        core.load_state_dict(resume)
        core.col["tice0"].copy_(torch.from_numpy(np.ascontiguousarray(resume["tice0"][core.blk.elem_slice()])))
    for _ in range(steps):
        core.step()
    return core


def owned_state(core):
    b = core.blk
    out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "S", "u")}
    out["tice0"] = core.col["tice0"][b.j0:b.j1].clone()
    return out


def gloo_worker(rank, world, port, outdir, variant, checkpoint):
    import torch
    import torch.distributed as dist
    from nextsimdg_amd import rowblock

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        if checkpoint:  # one step, the merged state of all ranks, a fresh core resumed from it, one more step
            first = run_coupled(rank, world, variant, 1)
            st = first.state_dict()
            b = first.blk
            st["tice0"] = first.col["tice0"][b.j0:b.j1].numpy().copy()
            states = [None] * world
            dist.all_gather_object(states, st)
            merged = rowblock.DynamicsCore.merge_states(states)
            merged["tice0"] = np.concatenate([s["tice0"] for s in sorted(states, key=lambda s: s["rows"][0])], axis=0)
            assert merged["S"].shape == (6, NY, NX)
            core = run_coupled(rank, world, variant, 1, resume=merged)
        else:
            core = run_coupled(rank, world, variant, 2)
        torch.save(owned_state(core), os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,variant", [(2, 4), (3, 2)])
def test_gloo_world_equals_world_one_bitwise_and_the_checkpoint_carries_the_snow(world, variant, tmp_path):
    import socket

    import torch
    import torch.multiprocessing as mp

    ref = run_coupled(0, 1, variant, 2)
    assert float(ref.S[1:].abs().max()) > 0.0  # the snow has grown a sub-cell shape: it was advected
    assert ref.col["hsnow"].data_ptr() == ref.S[0].data_ptr()
    want = owned_state(ref)
    for checkpoint in (False, True):
        out = tmp_path / ("ck" if checkpoint else "plain")
        out.mkdir()
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        mp.spawn(gloo_worker, args=(world, port, str(out), variant, checkpoint), nprocs=world, join=True)
        parts = [torch.load(os.path.join(str(out), "rank%d.pt" % r)) for r in range(world)]
        for key in ("H", "A", "S", "u", "tice0"):
            got = torch.cat([p[key] for p in parts], dim=1 if key in ("H", "A", "S") else 0)
            assert torch.equal(got, want[key]), (checkpoint, key)


def test_state_dict_needs_the_snow_in_the_mode():
    core = run_coupled(0, 1, 2, 0)
    st = core.state_dict()
    assert st["S"].shape == (6, NY, NX) and np.array_equal(st["S"][0], core.col["hsnow"].numpy())
    del st["S"]
    with pytest.raises(ValueError, match="snow S"):
        core.load_state_dict(st)

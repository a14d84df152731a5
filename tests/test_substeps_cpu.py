"""Sub-stepping of the model time step by the strength wave speed (include/nsdg.h "sub-stepping") without a GPU: the step-count rule of
the library (nsdg_substep_count, host only) against its numpy restatement and the documented points, and the Python driver's
DynamicsCore.advance over gloo with the oracle in place of the kernels."""
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import substep_ref as R  # noqa: E402
from nextsimdg_amd import abi, build, rowblock, synthetic  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    build.build_lib(verbose=False)
    return abi.load_library()


def default_params(lib):
    p = abi.MevpParams()
    lib.nsdg_mevp_default_params(C.byref(p))
    return p


def count(lib, p, amax, h, dt, courant=1.5, max_substeps=16):
    n, c = abi.I32(-7), abi.D(0.0)
    rc = lib.nsdg_substep_count(C.byref(p), float(amax), float(h), float(dt), float(courant), int(max_substeps), C.byref(n), C.byref(c))
    return rc, n.value, c.value, lib.nsdg_last_error().decode()


def test_substep_count_matches_the_numpy_restatement(lib):
    p = default_params(lib)
    assert (p.pstar, p.compaction, p.rho_ice) == (27.5e3, 20.0, 900.0)
    checked = 0
    for amax in (0.0, 0.1, 0.5, 0.8, 0.9, 0.95, 0.999, 1.0):
        for h in (62.5, 125.0, 250.0, 500.0, 1000.0, 2000.0, 7812.5):
            for dt in (10.0, 30.0, 60.0, 120.0, 600.0):
                for courant in (0.5, 1.0, 1.5, 3.0):
                    want_n, want_c, ratio = R.substep_count(amax, h, dt, courant)
                    rc, n, c, msg = count(lib, p, amax, h, dt, courant, max_substeps=100000)
                    assert rc == 0, msg
                    assert abs(c - want_c) <= 4e-16 * want_c + 1e-300, (amax, c, want_c)
                    if abs(ratio - round(ratio)) > 1e-9:  # one ulp of c decides the ceiling only at a whole ratio
                        assert n == want_n, (amax, h, dt, courant, n, want_n)
                        checked += 1
    assert checked > 1000


def test_documented_points(lib):
    p = default_params(lib)
    _, _, c09, _ = count(lib, p, 0.9, 250.0, 120.0)
    assert abs(c09 * c09 - 39.28) < 0.005 and abs(c09 - 6.268) < 5e-4
    # at a = 0.9 the ratio c dt / h lands just above whole numbers (2.006 at 250 m, 1.003 at 500 m): the points are taken at a = 1
    assert abs(c09 * 120.0 / (1.5 * 250.0) - 2.006) < 1e-3 and abs(c09 * 120.0 / (1.5 * 500.0) - 1.003) < 1e-3
    for h, want in ((2000.0, 1), (500.0, 3), (250.0, 6), (125.0, 12)):
        rc, n, c, msg = count(lib, p, 1.0, h, 120.0)
        assert rc == 0, msg
        assert abs(c - 17.91) < 5e-3 and n == want, (h, n)
    assert abi.substep_count(p, 1.0, 250.0, 120.0) == (6, pytest.approx(17.9118, abs=1e-4))


def test_edge_cases_and_errors(lib):
    p = default_params(lib)
    rc, n, c, _ = count(lib, p, 0.0, 125.0, 600.0)
    assert rc == 0 and n == 1 and c > 0  # no ice: one step (c(0) is small but not 0)
    # a state that would need more than max_substeps: an error naming the needed n, never a silently capped n
    rc, n, c, msg = count(lib, p, 1.0, 125.0, 120.0, max_substeps=11)
    assert rc == -1 and n == -7 and "n = 12" in msg and "max_substeps = 11" in msg, msg
    assert count(lib, p, 1.0, 125.0, 120.0, max_substeps=12)[:2] == (0, 12)
    with pytest.raises(abi.NsdgError, match="n = 12"):
        abi.substep_count(p, 1.0, 125.0, 120.0, max_substeps=8)
    bad = [(math.nan, 250.0, 120.0, 1.5, 16), (math.inf, 250.0, 120.0, 1.5, 16), (-0.1, 250.0, 120.0, 1.5, 16), (1.5, 250.0, 120.0, 1.5, 16),
           (0.9, 0.0, 120.0, 1.5, 16), (0.9, -250.0, 120.0, 1.5, 16), (0.9, math.nan, 120.0, 1.5, 16), (0.9, 250.0, 0.0, 1.5, 16),
           (0.9, 250.0, math.inf, 1.5, 16), (0.9, 250.0, 120.0, 0.0, 16), (0.9, 250.0, 120.0, math.nan, 16), (0.9, 250.0, 120.0, 1.5, 0)]
    for args in bad:
        rc, n, _, msg = count(lib, p, *args)
        assert rc == -1 and n == -7 and msg.startswith("nsdg_substep_count:"), (args, msg)
    assert lib.nsdg_substep_count(None, 0.5, 250.0, 120.0, 1.5, 16, None, None) == -1
    q = default_params(lib)
    q.pstar = math.nan
    assert count(lib, q, 0.5, 250.0, 120.0)[0] == -1
    # the collective without a communicator leaves the value alone; the reduction needs a context
    assert lib.nsdg_comm_max_f64(None, None) == -1


def test_substeps_argument_is_checked():
    core = rowblock.DynamicsCore.__new__(rowblock.DynamicsCore)
    for bad in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            core.advance(120.0, substeps=bad)


# ---- the Python driver over gloo --------------------------------------------------------------------------------------------------------
NX, NY, NSUB = 20, 29, 6


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def ops_with_max():
    from oracle_ops import OracleOps

    class MaxOps(OracleOps):
        """the oracle plus the numpy restatement of nsdg_concentration_max"""

        def concentration_max(self, H, A, j0=0, j1=None):
            return R.concentration_max(H.numpy(), A.numpy(), j0, j1)

    return MaxOps(mevp_variant=4, alpha=200.0, beta=200.0)


def initial_state():
    """a cover with more ice in the upper rows: the rows of rank 0 of 2 alone would ask for fewer sub-steps than the whole domain"""
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(7)
    H, A = bt.dg_fields()
    A[:] = 0.0
    A[0] = np.where(np.arange(NY)[:, None] < NY // 2, 0.8, 0.97) - 0.02 * rng.random((NY, NX))
    A[1] = 0.01 * rng.standard_normal((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    return bt, H, A


def courant_for_two(model_dt):
    """a courant number for which the whole initial state asks for n = 2 and the rows of rank 0 of 2 for n = 1"""
    bt, H, A = initial_state()
    h = min(bt.hx, bt.hy)
    r0, r1 = rowblock.split_rows(NY, 2, 0)
    full = R.wave_speed(R.concentration_max(H, A)) * model_dt / h
    low = R.wave_speed(R.concentration_max(H, A, r0, r1)) * model_dt / h
    courant = full / 1.6
    assert low / courant < 1.0
    return courant


def run(rank, world, how, model_dt=240.0, steps=2, courant=None):
    bt, H, A = initial_state()
    blk = rowblock.RowBlock(NX, NY, rank, world, 4, 3)
    core = rowblock.DynamicsCore(ops_with_max(), blk, bt.hx, bt.hy, model_dt, NSUB, torch.device("cpu"))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    ns = []
    for _ in range(steps):
        if how == "steps":  # the reference: step() at half the model step, twice
            core.dt = model_dt / 2
            core.step()
            core.step()
            core.dt = model_dt
            ns.append(2)
        else:
            ns.append(core.advance(model_dt, substeps=how, courant=courant))
    assert core.dt == model_dt
    return core, ns


def worker(rank, world, port, outdir, how, courant):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core, ns = run(rank, world, how, courant=courant)
        out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
        out["ns"] = ns
        torch.save(out, os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_advance_world_two_equals_world_one_and_half_steps_bitwise(tmp_path):
    """advance(substeps=2) == two step() calls at dt / 2, bit for bit, on one rank and on two (gloo); auto chooses the same n on every rank
    -- the maximum goes through torch.distributed -- although rank 0's own rows would ask for fewer"""
    ref, _ = run(0, 1, "steps")
    assert float(ref.u.abs().max()) > 1e-5
    two, ns = run(0, 1, 2)
    assert ns == [2, 2]
    for k in ("H", "A", "u", "v"):
        assert torch.equal(getattr(two, k), getattr(ref, k)), k
    one, _ = run(0, 1, 1)
    assert not torch.equal(one.u, ref.u)  # sub-stepping changed the run
    courant = courant_for_two(240.0)
    auto, ns = run(0, 1, "auto", courant=courant)
    assert ns == [2, 2]
    for k in ("H", "A", "u", "v"):
        assert torch.equal(getattr(auto, k), getattr(ref, k)), k
    for how in (2, "auto"):
        out = tmp_path / str(how)
        out.mkdir()
        mp.spawn(worker, args=(2, free_port(), str(out), how, courant), nprocs=2, join=True)
        parts = [torch.load(os.path.join(str(out), "rank%d.pt" % r)) for r in range(2)]
        assert [p["ns"] for p in parts] == [[2, 2], [2, 2]]
        for key in ("H", "A"):
            assert torch.equal(torch.cat([p[key] for p in parts], dim=1), getattr(ref, key)), (how, key)
        for key in ("u", "v"):
            assert torch.equal(torch.cat([p[key] for p in parts], dim=0), getattr(ref, key)), (how, key)


def test_host_rejects_bad_substep_keys(tmp_path):
    """dynamics.substeps / substep_courant / max_substeps are checked when the step is configured, before any device is touched"""
    import subprocess

    build.build_lib(verbose=False)
    host_dir = os.path.join(ROOT, "nextsimdg_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host_dir])
    cfg = os.path.join(str(tmp_path), "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 8\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n" % os.path.join(str(tmp_path), "x.nsdg"))
    for arg, msg in (("--dynamics.substeps=0", "dynamics.substeps must be an integer >= 1 or auto"),
                     ("--dynamics.substeps=2x", "dynamics.substeps must be an integer >= 1 or auto"),
                     ("--dynamics.substeps=Auto", "dynamics.substeps must be an integer >= 1 or auto"),
                     ("--dynamics.substep_courant=0", "dynamics.substep_courant must be positive"),
                     ("--dynamics.max_substeps=0", "dynamics.max_substeps must be >= 1")):
        p = subprocess.run([os.path.join(host_dir, "build", "nextsim_amd"), "--config-file", cfg, arg], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
        out = p.stdout.decode()
        assert p.returncode != 0 and msg in out, (arg, out)

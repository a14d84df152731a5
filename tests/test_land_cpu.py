"""Land mask without a GPU: the entry points' argument checks, the reference construction itself
(tests/land_ref.py: the unchanged oracle with land nodes zeroed after every sub-iteration), the row-block driver on that reference
(rowblock.DynamicsCore(..., land=mask) over LandOracleOps, one rank and gloo worlds of 2 and 3) and the host binary's refusal of bad
mask files."""
import ctypes as C
import math
import os
import subprocess
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

import land_ref  # noqa: E402
import oracle_lib as O  # noqa: E402
from nextsimdg_amd import rowblock, synthetic  # noqa: E402

NX, NY, DT, NSUB = 24, 20, 120.0, 40
UNIFORM = dict(alpha=200.0, beta=200.0)
ADAPTIVE = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=3.0, delta_min=2e-7)


def case(nx=NX, ny=NY, seed=41):
    bt = synthetic.BoxTest(nx, ny)
    rng = np.random.default_rng(seed)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((ny, nx))
    H[1:3] += 0.02 * rng.standard_normal((2, ny, nx))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    return bt, H, A, np.ascontiguousarray(uo), np.ascontiguousarray(vo), np.ascontiguousarray(3.0 * ua), np.ascontiguousarray(3.0 * va)


def test_entry_points_with_a_null_context_return_err_arg():
    from nextsimdg_amd import abi, build

    build.build_lib(verbose=False)
    lib = abi.load_library()
    for name in ("nsdg_land_mask_set", "nsdg_land_clear", "nsdg_land_clear_nodes"):
        assert name in abi.SYMBOLS
    assert lib.nsdg_land_mask_set(None, None) == -1
    assert b"null context" in lib.nsdg_last_error()
    assert lib.nsdg_land_clear(None, 0, 1, 1, None) == -1
    assert lib.nsdg_land_clear_nodes(None, None, None) == -1
    assert lib.nsdg_abi_version() == 6


def test_land_nodes_are_the_nodes_of_land_elements():
    m = np.zeros((3, 4), dtype=bool)
    m[1, 2] = True
    ln = land_ref.land_nodes(m)
    want = np.zeros((7, 9), dtype=bool)
    want[2:5, 4:7] = True
    assert np.array_equal(ln, want)
    m[:] = False
    m[0, 0] = m[2, 3] = True  # corners of the array
    ln = land_ref.land_nodes(m)
    assert ln[:3, :3].all() and ln[4:, 6:].all() and ln.sum() == 18


@pytest.mark.parametrize("pk,nsteps", [(UNIFORM, 5), (ADAPTIVE, 4)])
def test_reference_wall_reproduces_the_smaller_domain_bitwise(pk, nsteps):
    """land columns ix >= 16 of the 24 x 20 case: the ocean part IS the 16 x 20 domain -- H, A, u, v bit for bit"""
    bt, H, A, uo, vo, ua, va = case()
    p = O.mevp_params(**pk)
    m = 16
    land = np.zeros((NY, NX), dtype=bool)
    land[:, m:] = True
    full = land_ref.coupled_steps(NX, NY, bt.hx, bt.hy, DT, NSUB, nsteps, p, land, H, A, uo, vo, ua, va)
    cut = lambda a: np.ascontiguousarray(a[:, :2 * m + 1])
    small = land_ref.coupled_steps(m, NY, bt.hx, bt.hy, DT, NSUB, nsteps, p, None, np.ascontiguousarray(H[:, :, :m]), np.ascontiguousarray(A[:, :, :m]),
                                   cut(uo), cut(vo), cut(ua), cut(va))
    assert np.max(np.abs(small["u"])) > 1e-4
    for k in ("H", "A"):
        assert np.array_equal(full[k][:, :, :m], small[k]), k
        assert np.all(full[k][:, :, m:] == 0.0), k
    for k in ("u", "v"):
        assert np.array_equal(full[k][:, :2 * m + 1], small[k]), k
        assert np.all(full[k][:, 2 * m:] == 0.0), k


@pytest.mark.parametrize("pk,nsteps", [(UNIFORM, 6), (ADAPTIVE, 4)])
def test_reference_shapes_keep_land_at_zero_and_conserve_the_ice(pk, nsteps):
    """island + bay + one-element rock: land H, A, stress and land-node velocities stay EXACTLY 0 after every step, the total of the cell
    means drifts by round-off only, and the mask changes the ocean solution.  Bound of the drift: the flux form conserves the total up to
    the rounding of each cell's update; 64 ulp of the total (1.4e-14 relative) is the allowance the device test gives as well; the
    reference's measured drift on this case is <= 4.9e-16 relative after 6 steps"""
    bt, H, A, uo, vo, ua, va = case()
    p = O.mevp_params(**pk)
    land = land_ref.shapes_mask(NX, NY)
    assert 0 < land.sum() < land.size // 2
    ln = land_ref.land_nodes(land)
    H0 = H.copy()
    H0[:, land] = 0.0
    total0 = math.fsum(H0[0].ravel())
    drift = []

    def each(step, st):
        for k in ("H", "A"):
            assert np.all(st[k][:, land] == 0.0), (step, k)
        for x in st["s"]:
            assert np.all(x[:, land] == 0.0), step
        assert np.all(st["u"][ln] == 0.0) and np.all(st["v"][ln] == 0.0), step
        assert all(np.all(np.isfinite(st[k])) for k in ("H", "A", "u", "v"))
        drift.append(abs(math.fsum(st["H"][0].ravel()) - total0) / total0)

    masked = land_ref.coupled_steps(NX, NY, bt.hx, bt.hy, DT, NSUB, nsteps, p, land, H, A, uo, vo, ua, va, each=each)
    print("relative drift of the total of the cell means of H per step:", drift)
    assert max(drift) <= 64 * np.finfo(float).eps
    plain = land_ref.coupled_steps(NX, NY, bt.hx, bt.hy, DT, NSUB, nsteps, p, None, H, A, uo, vo, ua, va)
    diff = np.max(np.abs(masked["H"][0][~land] - plain["H"][0][~land]))
    assert 1e-5 < diff < 1e-1, diff


def run_core(rank, world, pk, land, nsteps=2, nsub=9, coupled=False):
    bt, H, A, uo, vo, ua, va = case(20, 29)
    blk = rowblock.RowBlock(20, 29, rank, world, 1, 1)
    core = rowblock.DynamicsCore(land_ref.LandOracleOps(**pk), blk, bt.hx, bt.hy, DT, nsub, torch.device("cpu"), land=land)
    core.load_global(H, A, uo, vo, ua, va)
    for _ in range(nsteps):
        core.step()
    return core


def straddling_mask():
    """20 x 29: an island across the block boundaries of worlds 2 (row 14) and 3 (rows 9, 19), and a rock on the boundary row itself"""
    m = np.zeros((29, 20), dtype=bool)
    m[7:21, 5:9] = True
    m[14, 15] = True
    return m


@pytest.mark.parametrize("pk", [UNIFORM, ADAPTIVE])
def test_driver_on_the_reference_equals_the_construction_bitwise(pk):
    bt, H, A, uo, vo, ua, va = case(20, 29)
    land = straddling_mask()
    core = run_core(0, 1, pk, land)
    ref = land_ref.coupled_steps(20, 29, bt.hx, bt.hy, DT, 9, 2, O.mevp_params(**pk), land, H, A, uo, vo, ua, va)
    assert np.max(np.abs(ref["u"])) > 1e-5
    for k in ("H", "A", "u", "v"):
        assert np.array_equal(getattr(core, k).numpy(), ref[k]), k
    for a, b in zip(core.s, ref["s"]):
        assert np.array_equal(a.numpy(), b)
    assert np.all(core.H.numpy()[:, land] == 0.0) and np.all(core.u.numpy()[land_ref.land_nodes(land)] == 0.0)
    core.close()
    assert core.ops.land is None  # close() leaves the ops object without a mask


def worker(rank, world, port, outdir, adaptive):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = run_core(rank, world, ADAPTIVE if adaptive else UNIFORM, straddling_mask())
        out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
        out["s11"] = core.owned(core.s[0]).clone()
        torch.save(out, os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,adaptive", [(2, False), (3, False), (3, True)])
def test_row_blocks_with_a_mask_equal_the_single_domain_bitwise(world, adaptive, tmp_path):
    from test_rowblock_gloo import free_port

    ref = run_core(0, 1, ADAPTIVE if adaptive else UNIFORM, straddling_mask())
    assert float(ref.u.abs().max()) > 1e-5
    mp.spawn(worker, args=(world, free_port(), str(tmp_path), adaptive), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(world)]
    for key, full in (("H", ref.H), ("A", ref.A), ("s11", ref.s[0])):
        assert torch.equal(torch.cat([p[key] for p in parts], dim=1), full), key
    for key, full in (("u", ref.u), ("v", ref.v)):
        assert torch.equal(torch.cat([p[key] for p in parts], dim=0), full), key


def test_land_needs_an_ops_object_with_the_land_calls():
    from oracle_ops import OracleOps

    bt = synthetic.BoxTest(8, 8)
    with pytest.raises(ValueError, match="set_land_mask"):
        rowblock.DynamicsCore(OracleOps(), rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu"), land=np.zeros((8, 8), dtype=bool))
    with pytest.raises(ValueError, match=r"\[8, 8\]"):
        rowblock.DynamicsCore(land_ref.LandOracleOps(), rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu"), land=np.zeros((8, 7), dtype=bool))
    # no land argument: nothing is asked of the ops object
    rowblock.DynamicsCore(OracleOps(), rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu")).close()


# ---- the C++ host: dynamics.land_mask_file is read and checked before a device is touched ------------------------------------------
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_refuses_bad_mask_files_before_any_device(host_build, tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(host_build, "nextsim_amd")
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 6\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\nnsub = 4\n" % os.path.join(tmp, "x.nsdg"))
    good = np.zeros((6, 8), dtype=np.uint8)
    good[2:4, 3:5] = 1
    files = {
        "missing.npy": (None, "cannot open"),
        "shape.npy": (np.zeros((8, 6), dtype=np.uint8), "the mask has the shape (8, 6)"),
        "flat.npy": (np.zeros(48, dtype=np.uint8), "two-dimensional"),
        "dtype.npy": (good.astype(np.float64), "uint8"),
        "value.npy": (np.where(good == 1, 2, 0).astype(np.uint8), "value 2 at (2, 3)"),
    }
    for name, (a, needle) in files.items():
        path = os.path.join(tmp, name)
        if a is not None:
            np.save(path, a)
        p = subprocess.run([exe, "--config-file", cfg, "--dynamics.land_mask_file=" + path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=120, cwd=tmp)
        out = p.stdout.decode()
        assert p.returncode != 0 and "dynamics.land_mask_file" in out and path in out and needle in out, (name, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(tmp, "x.nsdg")), (name, out)
    if not torch.cuda.is_available():  # a good file (uint8 and bool) passes every check: the run gets as far as asking for a device
        for a in (good, good.astype(bool)):
            path = os.path.join(tmp, "good.npy")
            np.save(path, a)
            p = subprocess.run([exe, "--config-file", cfg, "--dynamics.land_mask_file=" + path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               timeout=120, cwd=tmp)
            assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()

"""The sea-surface tilt (include/nsdg_tilt.h) without a GPU: the header and its bindings, the numpy restatement of
the gradient and of the box test's height (tests/tilt_ref.py), and the Python driver (DynamicsCore(tilt="ssh")) on the unchanged oracle with
the tilt injected through the start velocity: one block against gloo worlds of 2 and 3, and every refusal."""
import os
import re
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

import tilt_ref as TR  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402
from oracle_ops import OracleOps  # noqa: E402

UNIFORM = dict(alpha=200.0, beta=200.0)
ADAPTIVE = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=3.0, delta_min=2e-7)
HEADER = os.path.join(ROOT, "include", "nsdg_tilt.h")
FUNCTIONS = {"nsdg_tilt_set", "nsdg_tilt_nodal", "nsdg_boxtest_ssh"}


# ---- header and bindings -----------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_three_functions_and_the_table_binds_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsdg_\w+)\s*\(", text))
    assert declared == FUNCTIONS
    assert set(abi.TILT_SYMBOLS) == FUNCTIONS
    for other in (abi.SYMBOLS, abi.TRACER_SYMBOLS, abi.BASAL_SYMBOLS, abi.OCEAN_SYMBOLS, abi.SNOW_SYMBOLS):
        assert not set(other) & FUNCTIONS
    assert re.search(r"#define\s+NSDG_GRAVITY\s+9\.81", text) and abi.GRAVITY == 9.81
    assert '#include "nsdg_tilt.h"' in open(os.path.join(ROOT, "include", "nsdg.h")).read()


def test_header_compiles_alone_as_c99(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "nsdg_tilt.h"\nint main(void) { return nsdg_tilt_set(0, 0, NSDG_GRAVITY) == 0 && nsdg_tilt_nodal(0, 0, 0) == 0 '
                   '&& nsdg_boxtest_ssh(0, 1.0, 1e-4, NSDG_GRAVITY, 0) == 0; }\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "only.o")])


def test_null_context_is_an_argument_error_not_a_crash():
    lib = abi.load_library()
    assert lib.nsdg_tilt_set(None, None, 9.81) == -1
    assert lib.nsdg_tilt_nodal(None, None, None) == -1
    assert lib.nsdg_boxtest_ssh(None, 1.0, 1e-4, 9.81, None) == -1
    assert lib.nsdg_abi_version() == 6


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_gradient_is_exact_for_a_quadratic_at_interior_nodes():
    """integers on a lattice whose nodes are 1 apart (hx = hy = 2): every operation of the rule is exact, so the centred difference of
    eta = 3 x^2 - 2 x y + 5 y^2 + 7 x - 11 y + 4 IS its gradient at the interior nodes; the outermost row and column take the one-sided
    difference, which is the gradient half a node inwards"""
    nx, ny = 7, 5
    x, y = np.meshgrid(np.arange(2 * nx + 1, dtype=np.float64), np.arange(2 * ny + 1, dtype=np.float64))
    eta = 3 * x * x - 2 * x * y + 5 * y * y + 7 * x - 11 * y + 4
    sx, sy = TR.gradient(eta, 2.0, 2.0)
    gx, gy = 6 * x - 2 * y + 7, -2 * x + 10 * y - 11
    assert np.array_equal(sx[:, 1:-1], gx[:, 1:-1]) and np.array_equal(sy[1:-1], gy[1:-1])
    assert np.array_equal(sx[:, 0], (6 * 0.5 - 2 * y + 7)[:, 0]) and np.array_equal(sx[:, -1], (6 * (2 * nx - 0.5) - 2 * y + 7)[:, -1])
    assert np.array_equal(sy[0], (-2 * x + 10 * 0.5 - 11)[0]) and np.array_equal(sy[-1], (-2 * x + 10 * (2 * ny - 0.5) - 11)[-1])
    # and on an anisotropic mesh to rounding
    sx, sy = TR.gradient(eta, 2.0 * 37.5, 2.0 * 12.25)
    assert np.allclose(sx[:, 1:-1], gx[:, 1:-1] / 37.5, rtol=4e-16, atol=0) and np.allclose(sy[1:-1], gy[1:-1] / 12.25, rtol=4e-16, atol=0)


@pytest.mark.parametrize("nx,ny,row0,nyg", [(1, 1, 0, 1), (32, 2, 0, 2), (33, 3, 0, 3), (70, 9, 0, 9), (70, 4, 3, 9), (512, 512, 0, 512)])
def test_box_height_is_the_geostrophic_height_of_the_box_gyre(nx, ny, row0, nyg):
    """g grad(eta) = fc k x u_o for the box test: |g sx - fc vo| and |g sy + fc uo| at the interior nodes stay within
    16 * 2^-53 * (g max|eta| / hx + 0.01 fc).  The bound is rounding alone -- the centred difference of a quadratic is exact: eta carries
    a few roundings of relative size 2^-53, the difference of two of them is divided by hx (hy) and multiplied by g, and uo, vo carry a
    few roundings of their own size 0.01; measured here on the restatement, the largest ratio to the bound is printed"""
    L, fc, g = 512e3, 1.46e-4, 9.81
    hx, hy = L / nx, L / nyg
    eta = TR.box_ssh(nx, ny, L, fc, g, row0, nyg)
    uo, vo = TR.box_ocean(nx, ny, L, row0, nyg)
    sx, sy = TR.gradient(eta, hx, hy)
    # the height's maximum is that of the whole domain, whichever rows this block holds
    emax = np.abs(TR.box_ssh(nx, nyg, L, fc, g)).max()
    bx = 16 * 2.0 ** -53 * (g * emax / hx + 0.01 * fc)
    by = 16 * 2.0 ** -53 * (g * emax / hy + 0.01 * fc)
    ex = np.abs(g * sx - fc * vo)[:, 1:-1]
    ey = np.abs(g * sy + fc * uo)[1:-1]
    print("box height %dx%d rows %d of %d: max|eta| %.3e m, error / bound x %.3f y %.3f" % (nx, ny, row0, nyg, emax, ex.max() / bx, ey.max() / by))
    assert ex.max() <= bx and ey.max() <= by
    if ny == nyg:  # a row block holds the rows of the single domain, bit for bit
        lo = nyg // 3
        part = TR.box_ssh(nx, nyg - lo, L, fc, g, lo, nyg)
        assert np.array_equal(part, eta[2 * lo:])


def test_start_velocity_identity_by_hand():
    """one node of the oracle's velocity update: the update from (u0', v0') with the geostrophic term equals the update with the tilt
    term written out, to rounding"""
    dt, fc, g, m = 120.0, 1.46e-4, 9.81, 900.0 * 0.7
    u0, v0, uo, vo, sx, sy = 0.03, -0.02, 0.05, 0.02, 3e-6, -2e-6
    u0p, v0p = TR.start_velocity(dt, fc, g, u0, v0, uo, vo, sx, sy)
    c2 = m / dt * u0p - m * fc * vo  # the oracle's c2 without wind, from u0'
    c3 = m / dt * v0p + m * fc * uo
    assert abs(c2 - (m / dt * u0 - m * g * sx)) < 1e-15 * m / dt and abs(c3 - (m / dt * v0 - m * g * sy)) < 1e-15 * m / dt


# ---- the Python driver on the reference -----------------------------------------------------------------------------------------------
NX, NY, NSUB, DT = 20, 29, 5, 120.0
CONFIGS = {"uniform": (UNIFORM, False), "adaptive": (ADAPTIVE, False), "island": (UNIFORM, True)}


def island():
    """five rows across the block boundaries of worlds 2 (row 14) and 3 (rows 9, 19)"""
    land = np.zeros((NY, NX), dtype=bool)
    land[8:21, 7:12] = True
    return land


def slope_height(land=None):
    """a height that no geostrophic current of the run explains: a slope along x, a bump, and NaN strictly inside land"""
    x, y = np.meshgrid(np.linspace(0.0, 1.0, 2 * NX + 1), np.linspace(0.0, 1.0, 2 * NY + 1))
    eta = 4.0 * x + 1.0 * np.sin(3.0 * x + 5.0 * y)
    if land is not None:
        import land_ref

        inside = ~land_ref.land_nodes(~land)  # no ocean element touches the node
        assert inside.any()
        eta[inside] = np.nan
    return eta


def run_core(name, rank, world, steps=2, tilt="ssh", eta=None, **kw):
    pk, masked = CONFIGS[name]
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    land = island() if masked else None
    ops = TR.TiltLandOracleOps(**pk) if masked else TR.TiltOracleOps(**pk)
    core = rowblock.DynamicsCore(ops, rowblock.RowBlock(NX, NY, rank, world, 1, 1), bt.hx, bt.hy, DT, NSUB, torch.device("cpu"), land=land, tilt=tilt, **kw)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    if tilt == "ssh":
        if isinstance(eta, str):
            core.device_ssh(bt.L, ops.p.fc)
        else:
            core.set_ssh(slope_height(land) if eta is None else eta)
    for _ in range(steps):
        core.step()
    return core


def owned_state(core):
    out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
    out["s11"] = core.owned(core.s[0]).clone()
    if core.tilt == "ssh":
        out["sx"], out["sy"] = (t.clone() for t in core.tilt_read())
    return out


def worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for name in CONFIGS:
            torch.save(owned_state(run_core(name, rank, world)), os.path.join(outdir, "%s.rank%d.pt" % (name, rank)))
        torch.save(owned_state(run_core("uniform", rank, world, eta="box")), os.path.join(outdir, "box.rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single_domain():
    out = {name: run_core(name, 0, 1) for name in CONFIGS}
    out["box"] = run_core("uniform", 0, 1, eta="box")
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_driver_feels_the_height_and_leaves_the_ops_object_without_a_field(name, single_domain):
    core = single_domain[name]
    geo = run_core(name, 0, 1, tilt="geostrophic")
    assert torch.isfinite(core.u).all() and torch.isfinite(core.H).all()
    assert float(core.u.abs().max()) > 1e-5 and float((core.u - geo.u).abs().max()) > 1e-4  # 4 m over 512 km: g s dt is 9e-3 m/s per step before the drag answers
    assert core.ops.ssh is None  # set for the packing alone
    assert not hasattr(geo, "ssh") and geo.ops.ssh is None
    sx, sy = core.tilt_read()
    want = TR.gradient(core.ssh.numpy(), core.hx, core.hy)
    assert np.array_equal(sx.numpy(), want[0], equal_nan=True) and np.array_equal(sy.numpy(), want[1], equal_nan=True)
    if CONFIGS[name][1]:
        import land_ref

        ln = land_ref.land_nodes(island())
        assert np.all(core.u.numpy()[ln] == 0.0) and np.all(core.v.numpy()[ln] == 0.0)


def test_box_height_on_the_driver_is_the_geostrophic_run_to_rounding(single_domain):
    """the box test's height is the geostrophic height of its gyre: the run with tilt="ssh" differs from the geostrophic run by the
    rounding of the two statements of the same force"""
    core = single_domain["box"]
    geo = run_core("uniform", 0, 1, tilt="geostrophic")
    du = float((core.u - geo.u).abs().max())
    print("box height against the geostrophic tilt after 2 steps: max |du| = %.3e m/s of %.3e" % (du, float(geo.u.abs().max())))
    assert du < 1e-9


@pytest.mark.parametrize("world", [2, 3])
def test_row_blocks_under_a_height_equal_the_single_domain_bitwise(world, tmp_path, single_domain):
    from test_rowblock_gloo import free_port

    mp.spawn(worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    for name, ref in single_domain.items():
        want = owned_state(ref)
        parts = [torch.load(os.path.join(str(tmp_path), "%s.rank%d.pt" % (name, r))) for r in range(world)]
        for key in want:
            got = torch.cat([p[key] for p in parts], dim=1 if key in ("H", "A", "s11") else 0)
            a, b = got.numpy(), want[key].numpy()
            assert np.array_equal(a, b, equal_nan=key in ("sx", "sy")), (name, key)


def test_driver_refusals_come_before_anything_on_the_ops_object_changes():
    bt = synthetic.BoxTest(8, 8)
    args = (rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu"))

    def sealed(cls):
        class Untouched(cls):
            def __setattr__(self, k, v):
                if getattr(self, "_sealed", False):
                    raise AssertionError("the ops object was changed: " + k)
                super().__setattr__(k, v)

        ops = Untouched()
        ops._sealed = True
        return ops

    with pytest.raises(ValueError, match="'geostrophic' or 'ssh'"):
        rowblock.DynamicsCore(sealed(TR.TiltOracleOps), *args, tilt="barotropic")
    with pytest.raises(ValueError, match="gravity= needs tilt='ssh'"):
        rowblock.DynamicsCore(sealed(TR.TiltOracleOps), *args, gravity=9.8)
    for bad in (np.nan, np.inf, 0.0, -9.81):
        with pytest.raises(ValueError, match="finite and > 0"):
            rowblock.DynamicsCore(sealed(TR.TiltOracleOps), *args, tilt="ssh", gravity=bad)
    with pytest.raises(ValueError, match="set_tilt"):
        rowblock.DynamicsCore(sealed(OracleOps), *args, tilt="ssh")
    plain = rowblock.DynamicsCore(OracleOps(), *args)  # without the feature nothing is asked of the ops object
    for call in (lambda: plain.set_ssh(np.zeros((17, 17))), lambda: plain.device_ssh(bt.L, 1e-4), plain.tilt_read):
        with pytest.raises(ValueError, match="tilt='ssh'"):
            call()
    plain.close()

    # the height itself: its shape, and finite at every node of every ocean element
    land = np.zeros((8, 8), dtype=bool)
    land[2:6, 2:6] = True
    core = rowblock.DynamicsCore(TR.TiltLandOracleOps(), *args, tilt="ssh", land=land)
    with pytest.raises(ValueError, match=r"\[17, 17\]"):
        core.set_ssh(np.zeros((16, 17)))
    eta = np.zeros((17, 17))
    eta[5:12, 5:12] = np.nan  # strictly inside the island: nobody reads it
    core.set_ssh(eta)
    eta[4, 7] = np.inf  # a coast node: a node of the ocean element (1, 3)
    eta[12, 9] = np.nan
    with pytest.raises(ValueError, match=r"inf at node \(row 4, column 7\)"):
        core.set_ssh(eta)
    core.close()

    # the forcing series and the tilt agree on who states it
    col = {k: np.zeros((2, 4, 4)) for k in rowblock.ForcingSeries.COLUMN}
    pair = {"ocean_u": np.zeros((2, 4, 4)), "ocean_v": np.zeros((2, 4, 4))}
    with pytest.raises(ValueError, match="unknown forcing field"):
        rowblock.ForcingSeries([0.0, 1.0], {**col, "eta": np.zeros((2, 4, 4))})
    with_ssh = rowblock.ForcingSeries([0.0, 1e6], {**col, **pair, "ssh": np.zeros((2, 4, 4))})
    without = rowblock.ForcingSeries([0.0, 1e6], {**col, **pair})
    with pytest.raises(ValueError, match="needs tilt='ssh'"):
        rowblock.CoupledCore(sealed(TR.TiltOracleOps), *args, forcing=with_ssh)
    with pytest.raises(ValueError, match="needs the series to hold ssh"):
        rowblock.CoupledCore(sealed(TR.TiltOracleOps), *args, forcing=without, tilt="ssh")
    rowblock.CoupledCore(TR.TiltOracleOps(), *args, forcing=rowblock.ForcingSeries([0.0, 1e6], col), tilt="ssh").close()  # no ocean pair: the height is set_ssh's
    core = rowblock.CoupledCore(TR.TiltOracleOps(), *args, forcing=with_ssh, tilt="ssh")
    assert any("ssh" in names and outs[-1] is core.ssh for _, names, outs in core._series_groups)
    core.close()

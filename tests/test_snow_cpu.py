"""The snow load (include/nsdg_snow.h) without a GPU: the header and its bindings, the reference's substitution
(tests/snow_ref.py) against the unchanged oracle, the steady free drift of the loaded mass against scipy, and the Python driver
(CoupledCore(snow_load=True)) on the reference: one block against gloo worlds of 2 and 3, and every refusal."""
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

import column_transport_ref as CT  # noqa: E402
import oracle_lib as O  # noqa: E402
import snow_ref as SR  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402
from oracle_ops import OracleOps  # noqa: E402

UNIFORM = dict(alpha=200.0, beta=200.0)
ADAPTIVE = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=3.0, delta_min=2e-7)
HEADER = os.path.join(ROOT, "include", "nsdg_snow.h")
FUNCTIONS = {"nsdg_snow_load_set", "nsdg_snow_load_nodal"}


# ---- header and bindings -----------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_two_functions_and_the_table_binds_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(nsdg_\w+)\s*\(", text))
    assert declared == FUNCTIONS
    assert set(abi.SNOW_SYMBOLS) == FUNCTIONS
    for other in (abi.SYMBOLS, abi.TRACER_SYMBOLS, abi.BASAL_SYMBOLS, abi.OCEAN_SYMBOLS):
        assert not set(other) & FUNCTIONS
    assert re.search(r"#define\s+NSDG_SNOW_DENSITY\s+330\.0", text) and abi.SNOW_DENSITY == 330.0
    assert '#include "nsdg_snow.h"' in open(os.path.join(ROOT, "include", "nsdg.h")).read()


def test_header_compiles_alone_as_c99(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "nsdg_snow.h"\nint main(void) { return nsdg_snow_load_set(0, 0, 1, NSDG_SNOW_DENSITY) == 0 && nsdg_snow_load_nodal(0, 0, 0, 0) == 0; }\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "only.o")])


def test_null_context_is_an_argument_error_not_a_crash():
    lib = abi.load_library()
    assert lib.nsdg_snow_load_set(None, None, 1, 330.0) == -1
    assert lib.nsdg_snow_load_nodal(None, None, None, None) == -1
    assert lib.nsdg_abi_version() == 6


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_loaded_thickness_by_hand():
    p = O.mevp_params()
    r = 330.0 / p.rho_ice
    cgh = np.array([1.0, 1.0, 1.0, 5e-5, 0.004, 1.0])
    cga = np.array([0.9, 0.9, 0.9, 0.9, 0.9, 0.0])
    cgs = np.array([0.3, -0.2, 0.0, 2.0, 2.0, 0.5])
    got = SR.loaded_thickness(p, 330.0, cgh, cga, cgs)
    # snow, negative snow (clamped), none, thickness at the mass floor, true thickness below min_thick, no concentration: the last three
    # are ice-free and keep cgH whatever lies on them
    assert np.array_equal(got, np.array([1.0 + r * 0.3, 1.0, 1.0, 5e-5, 0.004, 1.0]))
    assert np.array_equal(SR.loaded_thickness(p, 0.0, cgh, cga, cgs), cgh)
    off = O.mevp_params(min_conc=0.0, min_thick=0.0)  # the rule off: every node carries its snow
    assert np.array_equal(SR.loaded_thickness(off, 330.0, cgh, cga, cgs), cgh + r * np.maximum(cgs, 0.0))
    land = np.zeros((1, 2), dtype=bool)
    land[0, 1] = True
    h = SR.load_nodal(p, 330.0, np.full((3, 5), 1.0), np.full((3, 5), 0.9), np.full((3, 5), 0.3), land)
    assert np.all(h[:, :2] == 1.0 + r * 0.3) and np.all(h[:, 2:] == p.h_min)


def small_case(nx=12, ny=9, seed=3):
    bt = synthetic.BoxTest(nx, ny)
    rng = np.random.default_rng(seed)
    H, A = bt.dg_fields()
    H[1:3] += 0.02 * rng.standard_normal((2, ny, nx))
    uo, vo = (np.ascontiguousarray(a) for a in bt.ocean())
    ua, va = (np.ascontiguousarray(3.0 * a) for a in bt.wind(0.0))
    return bt, H, A, uo, vo, ua, va


def sub_iterations(ops, bt, H, A, uo, vo, ua, va, n=6, dt=120.0):
    nx, ny = H.shape[2], H.shape[1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ops.set_grid(nx, ny, bt.hx, bt.hy)
    u, v = t(np.zeros_like(uo)), t(np.zeros_like(uo))
    s = [t(np.zeros((8, ny, nx))) for _ in range(3)]
    pg = t(O.ice_strength(nx, ny, ops.p, H, A))
    ops.mevp_prepare(dt, t(H), t(A), (t(ua), t(va)), (t(uo), t(vo)), (u, v), None)
    for _ in range(n):
        sn, un, vn = [x.clone() for x in s], u.clone(), v.clone()
        ops.mevp_iterate(0, 0, ny, s, sn, (u, v), (un, vn), None, pg)
        s, u, v = sn, un, vn
    return u.numpy(), v.numpy(), s[0].numpy()


@pytest.mark.parametrize("pk", [UNIFORM, ADAPTIVE], ids=["uniform", "adaptive"])
def test_zero_snow_and_zero_density_give_the_oracle_bit_for_bit(pk):
    case = small_case()
    nx, ny = case[1].shape[2], case[1].shape[1]
    want = sub_iterations(OracleOps(**pk), *case)
    snow = torch.from_numpy(0.3 * np.random.default_rng(8).random((ny, nx)))
    runs = {"zero snow": (torch.zeros(ny, nx, dtype=torch.float64), 330.0), "negative snow": (-snow, 330.0), "rho_snow = 0": (snow, 0.0)}
    for name, (field, rho) in runs.items():
        ops = SR.SnowOracleOps(**pk)
        ops.set_grid(nx, ny, case[0].hx, case[0].hy)
        ops.set_snow_load(field, rho)
        got = sub_iterations(ops, *case)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), name
    ops = SR.SnowOracleOps(**pk)
    ops.set_grid(nx, ny, case[0].hx, case[0].hy)
    ops.set_snow_load(snow)
    loaded = sub_iterations(ops, *case)
    assert not np.array_equal(loaded[0], want[0])  # and the load itself is felt
    ops.set_snow_load(None)
    assert all(np.array_equal(a, b) for a, b in zip(sub_iterations(ops, *case), want))


def test_masked_twin_and_the_composition_with_the_seabed_stress():
    """SnowLandOracleOps: zero snow is LandOracleOps bit for bit, snow is felt, land nodes stay at rest.  snow_ref.basal_subcycle: without
    snow it is basal_ref.subcycle bit for bit, with snow T_b is still that of the ice alone while the velocity changes"""
    import basal_ref as BR
    import land_ref

    case = small_case()
    bt, H, A, uo, vo, ua, va = case
    nx, ny = H.shape[2], H.shape[1]
    land = np.zeros((ny, nx), dtype=bool)
    land[3:6, 4:7] = True
    H[:, land] = 0.0
    A[:, land] = 0.0
    snow = torch.from_numpy(0.3 * np.random.default_rng(8).random((ny, nx)))
    res = {}
    for name, cls, field in (("land", land_ref.LandOracleOps, None), ("zero", SR.SnowLandOracleOps, torch.zeros_like(snow)), ("snow", SR.SnowLandOracleOps, snow)):
        ops = cls(**UNIFORM)
        ops.set_grid(nx, ny, bt.hx, bt.hy)
        ops.set_land_mask(torch.from_numpy(land.astype(np.uint8)))
        if field is not None:
            ops.set_snow_load(field)
        res[name] = sub_iterations(ops, *case)
    assert all(np.array_equal(a, b) for a, b in zip(res["zero"], res["land"])) and not np.array_equal(res["snow"][0], res["land"][0])
    ln = land_ref.land_nodes(land)
    assert np.all(res["snow"][0][ln] == 0.0) and np.all(res["snow"][1][ln] == 0.0)
    # the composition with a depth array
    p, bp = O.mevp_params(**UNIFORM), BR.basal_par()
    depth = np.full((ny, nx), 1.0)
    pg, cgh, cga = O.ice_strength(nx, ny, p, H, A), O.dg_to_cg(nx, ny, H), O.dg_to_cg(nx, ny, A)
    tax, tay = O.wind_stress(p, ua, va)
    runs = {}
    for name, cgs in (("basal_ref", None), ("no snow", np.zeros_like(cgh)), ("snow", SR.nodal_snow(nx, ny, snow.numpy()))):
        u, v = np.zeros_like(uo), np.zeros_like(uo)
        s = [np.zeros((8, ny, nx)) for _ in range(3)]
        if cgs is None:
            tb = BR.subcycle(nx, ny, bt.hx, bt.hy, 120.0, 6, p, bp, depth, land, s, u, v, u, v, tax, tay, uo, vo, cgh, cga, pg)
        else:
            tb = SR.basal_subcycle(nx, ny, bt.hx, bt.hy, 120.0, 6, p, bp, depth, land, SR.RHO_SNOW, cgs, s, u, v, u, v, tax, tay, uo, vo, cgh, cga, pg)
        runs[name] = (u, v, s[0], tb)
    assert all(np.array_equal(a, b) for a, b in zip(runs["no snow"], runs["basal_ref"]))
    assert float(runs["snow"][3].max()) > 0.0 and np.array_equal(runs["snow"][3], runs["basal_ref"][3])  # T_b reads the ice alone
    assert not np.array_equal(runs["snow"][0], runs["basal_ref"][0])


def test_strengthless_cover_under_snow_reaches_the_free_drift_of_the_loaded_mass():
    """the strengthless cover of tests/test_oracle_dynamics.py (6 x 5, P* = 0, 70 steps of 600 s) with 0.3 m of snow on its 0.7 m of ice:
    the steady state is scipy's free drift for m = rho_i h + rho_s s, within that test's 1e-10, and farther than 1e-3 m/s in each
    component from the ice-only solution"""
    from test_oracle_dynamics import free_drift_case, free_drift_solution

    nx, ny = 6, 5
    hx, hy, ua, va, uo, vo, cgh, cga = free_drift_case(nx, ny)
    p = O.mevp_params(pstar=0.0, alpha=5.0, beta=5.0)
    href = SR.loaded_thickness(p, SR.RHO_SNOW, cgh, cga, SR.nodal_snow(nx, ny, np.full((ny, nx), 0.3)))
    tax, tay = O.wind_stress(p, ua, va)
    pg = np.zeros((9, ny, nx))
    u, v = np.zeros_like(ua), np.zeros_like(ua)
    s = [np.zeros((8, ny, nx)) for _ in range(3)]
    for _ in range(70):
        O.mevp_subcycle(nx, ny, hx, hy, 600.0, 30, p, s, u, v, u.copy(), v.copy(), tax, tay, uo, vo, href, cga, pg)
    want = free_drift_solution(p, 9.0, -4.0, 0.05, 0.02, (p.rho_ice * 0.7 + SR.RHO_SNOW * 0.3) / p.rho_ice, 0.85)
    bare = free_drift_solution(p, 9.0, -4.0, 0.05, 0.02, 0.7, 0.85)
    ui, vi = u[1:-1, 1:-1], v[1:-1, 1:-1]
    print("free drift with the load (%.6f, %.6f), without (%.6f, %.6f)" % (want[0], want[1], bare[0], bare[1]))
    assert np.max(np.abs(ui - want[0])) < 1e-10 and np.max(np.abs(vi - want[1])) < 1e-10
    assert abs(want[0] - bare[0]) > 1e-3 and abs(want[1] - bare[1]) > 1e-3
    assert np.min(np.abs(ui - bare[0])) > 1e-3 and np.min(np.abs(vi - bare[1])) > 1e-3


# ---- the Python driver on the reference -----------------------------------------------------------------------------------------------
NX, NY, NSUB, DT = 20, 29, 5, 120.0
# (snow source under advect_column_state?, parameters, rheology)
CONFIGS = {"plane-uniform": (False, UNIFORM, "mevp"), "plane-adaptive": (False, ADAPTIVE, "mevp"), "S-uniform": (True, UNIFORM, "mevp"),
           "S-adaptive": (True, ADAPTIVE, "mevp"), "plane-bbm": (False, {}, "bbm")}


class TracerCalls:
    """the numpy restatement of nsdg_tracer_weight / nsdg_tracer_recover (tests/column_transport_ref.py)"""

    def tracer_weight(self, order, j0, j1, H, T, Q):
        q = Q.numpy()
        q[:] = CT.weight(H.numpy(), T.numpy(), j0, j1, Q=q)

    def tracer_recover(self, order, j0, j1, H, A, Q, min_conc, min_thick, T):
        t = T.numpy()
        t[:] = CT.recover(H.numpy(), A.numpy(), Q.numpy(), t, min_conc, min_thick, j0, j1)


class SnowTracerOps(TracerCalls, SR.SnowOracleOps):
    pass


def make_ops(name):
    advect, pk, rheology = CONFIGS[name]
    return SR.make_bbm_ops() if rheology == "bbm" else SnowTracerOps(**pk)


def run_coupled(name, rank, world, steps=2, snow_load=True, **kw):
    advect, pk, rheology = CONFIGS[name]
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    nsub, dt = (NSUB, DT) if rheology == "mevp" else (4, 8.0)
    core = rowblock.CoupledCore(make_ops(name), rowblock.RowBlock(NX, NY, rank, world, 1, 1), bt.hx, bt.hy, dt, nsub, torch.device("cpu"),
                                advect_column_state=advect, rheology=rheology, snow_load=snow_load, **kw)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    state, forcing, _ = synthetic.column_fields(NX * NY, 5)
    col = {k: v.reshape(NY, NX) for k, v in {**state, **forcing}.items()}
    col["wind"] = 0.2 * col["wind"]
    # a snow field that varies across the block boundaries of worlds 2 (row 14) and 3 (rows 9, 19)
    col["hsnow"] = 0.4 * rng.random((NY, NX)) * (1.0 + np.sin(np.arange(NY) * 0.9))[:, None]
    col["tice0"] = rng.uniform(-15.0, -2.0, (NY, NX))
    core.load_column(col)
    for _ in range(steps):
        core.step()
    return core


def owned_state(core):
    out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
    out["s11"] = core.owned(core.s[0]).clone()
    out["hsnow"] = core.col["hsnow"][core.blk.j0:core.blk.j1].clone()
    return out


def worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for name in CONFIGS:
            torch.save(owned_state(run_coupled(name, rank, world)), os.path.join(outdir, "%s.rank%d.pt" % (name, rank)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single_domain():
    return {name: run_coupled(name, 0, 1) for name in CONFIGS}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_driver_feels_the_load_and_leaves_the_ops_object_without_a_field(name, single_domain):
    core = single_domain[name]
    bare = run_coupled(name, 0, 1, snow_load=False)
    assert float(core.u.abs().max()) > 1e-5 and not torch.equal(core.u, bare.u)
    assert core.ops.snow is not None
    nc = 6 if CONFIGS[name][0] else 1
    assert core.ops.snow.numel() == nc * NX * NY  # (the field of the last packing: the transport has moved S to its other buffer since)
    if nc == 1:
        assert core.ops.snow.data_ptr() == core.col["hsnow"].data_ptr()
    light = run_coupled(name, 0, 1, rho_snow=0.0)  # no density: the run without the load, bit for bit
    assert torch.equal(light.u, bare.u) and torch.equal(light.v, bare.v) and torch.equal(light.H, bare.H)
    light.close()
    assert light.ops.snow is None


@pytest.mark.parametrize("world", [2, 3])
def test_row_blocks_under_a_snow_load_equal_the_single_domain_bitwise(world, tmp_path, single_domain):
    from test_rowblock_gloo import free_port

    mp.spawn(worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    for name, ref in single_domain.items():
        want = owned_state(ref)
        parts = [torch.load(os.path.join(str(tmp_path), "%s.rank%d.pt" % (name, r))) for r in range(world)]
        for key in want:
            got = torch.cat([p[key] for p in parts], dim=1 if key in ("H", "A", "s11") else 0)
            assert torch.equal(got, want[key]), (name, key)


def test_driver_refusals_come_before_anything_on_the_ops_object_changes():
    bt = synthetic.BoxTest(8, 8)
    args = (rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu"))

    class Untouched(SnowTracerOps):
        def __setattr__(self, k, v):
            if getattr(self, "_sealed", False):
                raise AssertionError("the ops object was changed: " + k)
            super().__setattr__(k, v)

    def sealed(cls=Untouched):
        ops = cls()
        ops._sealed = True
        return ops

    with pytest.raises(ValueError, match="CoupledCore"):
        rowblock.DynamicsCore(sealed(), *args, snow_load=True)
    with pytest.raises(ValueError, match="snow_load=True"):
        rowblock.CoupledCore(sealed(), *args, rho_snow=330.0)
    for bad in (np.nan, np.inf, -1.0):
        with pytest.raises(ValueError, match="finite and >= 0"):
            rowblock.CoupledCore(sealed(), *args, snow_load=True, rho_snow=bad)

    class NoSnow(TracerCalls, OracleOps):
        def __setattr__(self, k, v):
            if getattr(self, "_sealed", False):
                raise AssertionError("the ops object was changed: " + k)
            super().__setattr__(k, v)

    with pytest.raises(ValueError, match="set_snow_load"):
        rowblock.CoupledCore(sealed(NoSnow), *args, snow_load=True)
    rowblock.CoupledCore(NoSnow(), *args).close()  # without the feature nothing is asked of the ops object

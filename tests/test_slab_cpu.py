"""The slab ocean (include/nsdg_ocean.h) without a GPU: the numpy restatement tests/slab_ref.py on the oracle's
column step, and the Python driver (CoupledCore(slab_ocean=True)) on the stand-in SlabOps.  Hand values for the four regimes, the salt
identity, relaxation, the skip mask, the refusals, the behaviour the feature exists for (a warm mixed layer is a finite heat source), 1 gloo
rank == 2 == 3 bit for bit, checkpoint and resume, and the default that changes nothing."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as O  # noqa: E402
import slab_ref as R  # noqa: E402
from nextsimdg_amd import rowblock, synthetic  # noqa: E402

DT = 120.0
ULP = np.finfo(np.float64).eps


def ocean_step(dt, state, forcing, newice, params=None, ext=None, skip=None):
    """slab_ref.column_step_ocean on copies: (state, forcing, newice, diag) after the step"""
    st, fo, ni = {k: v.copy() for k, v in state.items()}, {k: v.copy() for k, v in forcing.items()}, newice.copy()
    diag = R.column_step_ocean(O.column_params(), dt, st, fo, ni, params, ext, skip)
    return st, fo, ni, diag


def element(**kw):
    """one element: a cold, dark sky over 10 m of mixed layer at S = 32"""
    v = dict(hice=0.0, cice=0.0, hsnow=0.0, tice0=-5.0, sst=-1.0, sss=32.0, tair=-20.0, tdew=-22.0, slp=1e5, qsw=0.0, qlw=200.0, mld=10.0,
             snowfall=0.0, wind=5.0)
    v.update(kw)
    one = lambda x: np.array([float(x)])
    return {k: one(v[k]) for k in O.STATE}, {k: one(v[k]) for k in O.FORCING}, np.zeros(1)


# ---- hand values ------------------------------------------------------------------------------------------------------------------------
def by_hand(dt, c, H0, S0, T, S, mld, snowfall, wind, H1, S1n, d, s_ice=R.ICE_S):
    """section 3.11 on Python scalars, written out from the issue's formulae (not from slab_ref.update)"""
    mlbhc = mld * 1025.0 * 4186.84
    qnet = c * d["qio"] + (1.0 - c) * d["qow"]
    T1 = T - (qnet * dt) / mlbhc
    evap = 1.5e-3 * d["rho"] * wind * (d["qw"] - d["qa"])
    dMi, dMs = 917.0 * (H1 - H0), 330.0 * (S1n - S0)
    W = (snowfall - (c * d["subl"] + (1.0 - c) * evap)) * dt - dMi - dMs
    M = 1025.0 * mld
    return T1, (M * S - s_ice * dMi) / (M + W)


def hand_case(**kw):
    st0, fo0, ni0 = element(**kw)
    st, fo, ni, diag = ocean_step(600.0, st0, fo0, ni0)
    d = {k: float(v[0]) for k, v in diag.items()}
    f = lambda a, k: float(a[k][0])
    T1, S1 = by_hand(600.0, f(st0, "cice"), f(st0, "hice"), f(st0, "hsnow"), f(fo0, "sst"), f(fo0, "sss"), f(fo0, "mld"), f(fo0, "snowfall"),
                     f(fo0, "wind"), f(st, "hice"), f(st, "hsnow"), d)
    # the scalar statement fuses nothing either: equal to a few ulp (it groups the sums as the formulae are written)
    assert abs(f(fo, "sst") - T1) <= 4 * ULP * max(abs(T1), 1.0) and abs(f(fo, "sss") - S1) <= 4 * ULP * S1
    return st0, fo0, st, fo, ni, d


def test_hand_value_full_cover_over_warm_water_reaches_the_freezing_point_in_one_step():
    st0, fo0, st, fo, ni, d = hand_case(hice=2.0, cice=1.0, hsnow=0.1, sst=-0.76, sss=32.0)
    tf = -0.055 * 32.0
    # Qio = (sst - T_f) mlbhc / dt: the whole excess, one step (BasicIceOceanHeatFlux)
    assert abs(d["qio"] - 1.0 * 10.0 * 1025.0 * 4186.84 / 600.0) <= 1e-9 * d["qio"]
    assert abs(fo["sst"][0] - tf) <= 1e-13
    # the excess melted rho_w c_p mld 1 K / (rho_i L_f) = 0.1403 m from below, less what conduction grew: the layer freshens
    melt = 1025.0 * 4186.84 * 10.0 / (917.0 * 333.55e3)
    assert 0.9 * melt < 2.0 - st["hice"][0] < melt and fo["sss"][0] < 32.0
    assert abs((32.0 - fo["sss"][0]) - (32.0 - 5.0) * 917.0 * (2.0 - st["hice"][0]) / 10250.0) < 0.01


def test_hand_value_open_water_that_cools_and_stays_above_freezing():
    st0, fo0, st, fo, ni, d = hand_case(sst=1.0)
    assert d["qow"] > 0 and st["hice"][0] == 0.0 and ni[0] == 0.0
    want = 1.0 - d["qow"] * 600.0 / (10.0 * 1025.0 * 4186.84)
    assert abs(fo["sst"][0] - want) <= 1e-15 and -0.055 * 32.0 < fo["sst"][0] < 1.0
    assert fo["sss"][0] > 32.0  # evaporation alone concentrates the layer
    assert abs(fo["sss"][0] / 32.0 - 1.0 - 1.5e-3 * d["rho"] * 5.0 * (d["qw"] - d["qa"]) * 600.0 / 10250.0) < 1e-9


def test_hand_value_open_water_that_reaches_the_freezing_point_forms_ice():
    st0, fo0, st, fo, ni, d = hand_case(sst=-1.759, mld=5.0)
    tf = -0.055 * 32.0
    assert ni[0] > 0.0 and st["hice"][0] == ni[0] > 0.0  # Qow is the sensible part only; the rest became new ice
    assert abs(fo["sst"][0] - tf) <= 1e-13
    assert fo["sss"][0] > 32.0  # brine rejection: the ice forms at S_i = 5
    evap = 1.5e-3 * d["rho"] * 5.0 * (d["qw"] - d["qa"])  # and the evaporation concentrates it: dS = ((S - S_i) dMi + S evap dt) / M
    assert abs((fo["sss"][0] - 32.0) - ((32.0 - 5.0) * 917.0 * ni[0] + 32.0 * evap * 600.0) / 5125.0) < 1e-3 * (fo["sss"][0] - 32.0)


def test_hand_value_thin_ice_over_warm_water_melts_out():
    st0, fo0, st, fo, ni, d = hand_case(hice=0.01, cice=0.5, hsnow=0.005, sst=1.0, tice0=-1.0, tair=-2.0, tdew=-3.0)
    assert st["hice"][0] == 0.0 and st["cice"][0] == 0.0 and st["hsnow"][0] == 0.0
    assert -0.055 * 32.0 < fo["sst"][0] < 1.0  # the water paid for the melt and stays above freezing
    assert fo["sss"][0] < 32.0  # 1 cm of ice at 5 and the snow at 0 into 10 m at 32
    want = (10250.0 * 32.0 + 5.0 * 917.0 * 0.01) / (10250.0 + 917.0 * 0.01 + 330.0 * 0.005)
    assert abs(fo["sss"][0] - want) < 2e-5  # (evaporation over the open half: ~1e-5)


# ---- salt identity ----------------------------------------------------------------------------------------------------------------------
def test_salt_is_conserved_and_growth_raises_sss_and_melt_lowers_it():
    n = 4096
    state, forcing, newice = synthetic.column_fields(n)
    st, fo, ni, diag = ocean_step(600.0, state, forcing, newice)
    before = {k: (state[k] if k in state else forcing[k]) for k in R.BEFORE}
    M, W, dMi = R.water(600.0, before, st, diag)
    S, S1 = forcing["sss"], fo["sss"]
    lhs = (M + W) * S1 + R.ICE_S * R.RHO_I * st["hice"]
    rhs = M * S + R.ICE_S * R.RHO_I * state["hice"]
    assert np.all(np.isfinite(S1)) and np.all(np.abs(lhs - rhs) <= 4 * ULP * M * S)
    # without a water flux the sign of dS is the sign of dH: check it where the ice change dominates the fresh-water flux
    dom = np.abs((S - R.ICE_S) * dMi) > 10.0 * np.abs(S * (W + dMi))
    grew, melted = dom & (dMi > 0), dom & (dMi < 0)
    assert grew.sum() > 50 and melted.sum() > 50
    assert np.all(S1[grew] > S[grew]) and np.all(S1[melted] < S[melted])


# ---- relaxation, skip ---------------------------------------------------------------------------------------------------------------------
def test_relaxation_off_never_reads_the_targets_and_on_adds_exactly_g_times_the_difference():
    n = 513
    state, forcing, newice = synthetic.column_fields(n, 7)
    nan = {"sst": np.full(n, np.nan), "sss": np.full(n, np.nan)}
    _, plain, _, _ = ocean_step(600.0, state, forcing, newice)
    _, off, _, _ = ocean_step(600.0, state, forcing, newice, R.SlabParams(), nan)
    assert np.array_equal(off["sst"], plain["sst"]) and np.array_equal(off["sss"], plain["sss"])
    rng = np.random.default_rng(3)
    ext = {"sst": rng.uniform(-1.8, 3.0, n), "sss": rng.uniform(30.0, 35.0, n)}
    p = R.SlabParams(relax_t=5 * 86400.0, relax_s=30 * 86400.0)
    st_on, on, ni_on, _ = ocean_step(600.0, state, forcing, newice, p, ext)
    # twin runs, no skip: the fluxes are the same, so the increment is exactly g (ext - old)
    for k, tau in (("sst", p.relax_t), ("sss", p.relax_s)):
        assert np.array_equal(on[k], plain[k] + (600.0 / tau) * (ext[k] - forcing[k])), k
        assert not np.array_equal(on[k], plain[k])
    # one relaxation alone reads only its own target
    _, only_t, _, _ = ocean_step(600.0, state, forcing, newice, R.SlabParams(relax_t=p.relax_t), {"sst": ext["sst"], "sss": nan["sss"]})
    assert np.array_equal(only_t["sst"], on["sst"]) and np.array_equal(only_t["sss"], plain["sss"])


def test_skip_leaves_the_bits_of_sst_and_sss_and_nothing_else_sees_it():
    n = 513
    state, forcing, newice = synthetic.column_fields(n, 8)
    skip = (np.random.default_rng(5).random(n) < 0.3).astype(np.uint8)
    skip[-1] = 1
    st_a, a, ni_a, _ = ocean_step(600.0, state, forcing, newice)
    st_b, b, ni_b, _ = ocean_step(600.0, state, forcing, newice, skip=skip)
    keep = skip != 0
    for k in ("sst", "sss"):
        assert np.array_equal(b[k][keep].view(np.int64), forcing[k][keep].view(np.int64)), k
        assert np.array_equal(b[k][~keep], a[k][~keep]) and np.any(a[k][keep] != forcing[k][keep]), k
    for k in O.STATE:
        assert np.array_equal(st_a[k], st_b[k]), k
    assert np.array_equal(ni_a, ni_b)
    # and the ice is the plain column step's
    st, fo, ni = {k: v.copy() for k, v in state.items()}, {k: v.copy() for k, v in forcing.items()}, newice.copy()
    O.column_step(O.column_params(), 600.0, st, fo, ni)
    assert all(np.array_equal(st[k], st_a[k]) for k in O.STATE) and np.array_equal(ni, ni_a)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def cpu_core(nx, ny, rank=0, world=1, nsub=3, **kw):
    bt = synthetic.BoxTest(nx, ny)
    ops = kw.pop("ops", None) or R.slab_ops()
    return bt, rowblock.CoupledCore(ops, rowblock.RowBlock(nx, ny, rank, world, 1, 1), bt.hx, bt.hy, DT, nsub, torch.device("cpu"), **kw)


def test_parameter_errors():
    ops = R.slab_ops()
    for bad in (dict(relax_t=-1.0), dict(relax_s=-1e-300), dict(ice_salinity=-0.1), dict(relax_t=np.inf), dict(relax_s=np.nan),
                dict(ice_salinity=np.nan)):
        with pytest.raises(ValueError, match="finite and >= 0"):
            ops.set_slab_params(R.SlabParams(**bad))
        with pytest.raises(ValueError, match="finite and >= 0"):
            cpu_core(8, 8, slab_ocean=True, slab=R.SlabParams(**bad))
    assert (ops.slab.relax_t, ops.slab.relax_s, ops.slab.ice_salinity) == (0.0, 0.0, 5.0)  # a refused set changes nothing
    with pytest.raises(ValueError, match="slab= needs slab_ocean=True"):
        cpu_core(8, 8, slab=R.SlabParams())
    from tracers_ops import tracers_ops

    with pytest.raises(ValueError, match="column_step_ocean, slab_default_params, set_slab_params"):
        cpu_core(8, 8, slab_ocean=True, ops=tracers_ops())
    cpu_core(8, 8, ops=tracers_ops())  # without the flag no new op is required of ops
    with pytest.raises(ValueError, match="collides"):
        cpu_core(8, 8, slab_ocean=True, tracers=("sst",))
    times, rec = [0.0, 1e4], np.zeros((2, 4, 4))
    with pytest.raises(ValueError, match="come as a pair"):
        rowblock.ForcingSeries(times, {"sst": rec})
    # a relaxation without its target
    state, forcing, newice = synthetic.column_fields(4)
    with pytest.raises(KeyError):
        ocean_step(600.0, state, forcing, newice, R.SlabParams(relax_t=1e5), {})
    _, core = cpu_core(8, 8, slab_ocean=True)
    st = core.state_dict()
    assert st["sst"].shape == (8, 8) and st["sss"].shape == (8, 8)
    del st["sss"]
    with pytest.raises(ValueError, match="sst and sss"):
        core.load_state_dict(st)
    _, plain = cpu_core(8, 8)
    assert "sst" not in plain.state_dict() and "sst_ext" not in core.col
    with pytest.raises(ValueError, match="slab_ocean=True"):
        plain.ocean_read()
    _, relaxed = cpu_core(8, 8, slab_ocean=True, slab=R.SlabParams(relax_s=1e6))
    assert "sss_ext" in relaxed.col and "sst_ext" not in relaxed.col


# ---- the behaviour the feature exists for -------------------------------------------------------------------------------------------------
TWIN_NX, TWIN_NY, TWIN_STEPS, TWIN_DT, TWIN_MLD = 16, 8, 20, 600.0, 10.0
TWIN_BOUND = 1.1 * R.RHO_W * R.C_P * TWIN_MLD * 1.0 / (R.RHO_I * R.L_F)  # [m]: the heat of 1 K of the layer as ice, and 10 %


def twin_fields(excess):
    """column_fields_smooth(16, 8) under a full cover of 2 m, mld = 10 m, the mixed layer `excess` K above its freezing point"""
    cs, cf = synthetic.column_fields_smooth(TWIN_NX, TWIN_NY)
    n = TWIN_NX * TWIN_NY
    state = {"hice": np.full(n, 2.0), "cice": np.ones(n), "hsnow": cs["hsnow"].reshape(-1).copy(), "tice0": cs["tice0"].reshape(-1).copy()}
    forcing = {k: cf[k].reshape(-1).copy() for k in O.FORCING}
    forcing["mld"][:] = TWIN_MLD
    forcing["sst"] = -R.MU * forcing["sss"] + excess
    return state, forcing, np.zeros(n)


def twin_differences(step):
    """|sum(hice_A - hice_B)| / n after each of the 20 steps; step(state, forcing, newice) advances one run in place"""
    runs = [twin_fields(1.0), twin_fields(0.0)]
    out = []
    for _ in range(TWIN_STEPS):
        for r in runs:
            step(*r)
        out.append(abs(float(np.sum(runs[0][0]["hice"] - runs[1][0]["hice"]))) / runs[0][0]["hice"].size)
    return out


def test_a_warm_mixed_layer_is_a_finite_heat_source_with_the_slab_and_an_inexhaustible_one_without():
    cp = O.column_params()
    slab = twin_differences(lambda st, fo, ni: R.column_step_ocean(cp, TWIN_DT, st, fo, ni))
    plain = twin_differences(lambda st, fo, ni: O.column_step(cp, TWIN_DT, st, fo, ni))
    print("twin runs: bound %.4f m; slab max %.4f m (step 1 %.4f, step 20 %.4f); plain step 1 %.4f, step 2 %.4f, step 20 %.4f"
          % (TWIN_BOUND, max(slab), slab[0], slab[-1], plain[0], plain[1], plain[-1]))
    assert slab[0] > 0.5 * TWIN_BOUND  # the excess did melt
    assert all(d <= TWIN_BOUND for d in slab), slab
    assert plain[0] <= TWIN_BOUND < plain[1] and plain[-1] > 10 * TWIN_BOUND, plain


# ---- the driver: row blocks over gloo, checkpoint, default -----------------------------------------------------------------------------------
NX, NY, NSUB = 20, 29, 5  # the grid and the step count of tests/test_tracers_cpu.py's gloo case
SLAB = dict(relax_t=40 * DT, relax_s=0.0)


def run_coupled(rank, world, steps, resume=None, slab_ocean=True, keyword=True):
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    A[0, 10:14, 3:9] = 0.0  # a lead
    H[0, 10:14, 3:9] = 0.0
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    kw = dict(slab_ocean=True, slab=R.SlabParams(**SLAB)) if slab_ocean else (dict(slab_ocean=False) if keyword else {})
    core = rowblock.CoupledCore(R.slab_ops(), rowblock.RowBlock(NX, NY, rank, world, 1, 1), bt.hx, bt.hy, DT, NSUB, torch.device("cpu"), **kw)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    state, forcing, _ = synthetic.column_fields(NX * NY, 5)
    col = {k: v.reshape(NY, NX) for k, v in {**state, **forcing}.items()}
    col["wind"] = 0.2 * col["wind"]
    if slab_ocean:
        col["sst_ext"] = col["sst"] + 0.5
    core.load_column(col)
    if resume is not None:
        core.load_state_dict(resume)
        es = core.blk.elem_slice()
        for k in ("hsnow", "tice0"):
            core.col[k].copy_(torch.from_numpy(np.ascontiguousarray(resume[k][es])))
        core.newice.copy_(torch.from_numpy(np.ascontiguousarray(resume["newice"][es])))
    for _ in range(steps):
        core.step()
    return core


def owned_state(core):
    b = core.blk
    out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
    for k in ("sst", "sss", "tice0", "hsnow"):
        out[k] = core.col[k][b.j0:b.j1].clone()
    return out


def gloo_worker(rank, world, port, outdir):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = run_coupled(rank, world, 2)
        states = [None] * world
        dist.all_gather_object(states, core.state_dict())
        merged = rowblock.DynamicsCore.merge_states(states)
        for k in ("sst", "sss"):  # the ghost rows equal their owners without a message
            assert np.array_equal(core.col[k].numpy(), merged[k][core.blk.elem_slice()]), k
        assert core.ocean_read()["rows"] == (core.blk.r0, core.blk.r1)
        torch.save(owned_state(core), os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_world_equals_world_one_bitwise(world, tmp_path):
    import torch.multiprocessing as mp

    ref = run_coupled(0, 1, 2)
    want = owned_state(ref)
    start = synthetic.column_fields(NX * NY, 5)[1]
    assert not np.array_equal(want["sst"].numpy().reshape(-1), start["sst"]) and not np.array_equal(want["sss"].numpy().reshape(-1), start["sss"])
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(gloo_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(world)]
    for key in want:
        got = torch.cat([p[key] for p in parts], dim=1 if key in ("H", "A") else 0)
        assert torch.equal(got, want[key]), key


def test_n_steps_equal_half_plus_state_dict_plus_half():
    full, half = run_coupled(0, 1, 4), run_coupled(0, 1, 2)
    state = rowblock.DynamicsCore.merge_states([half.state_dict()])
    assert state["sst"].shape == (NY, NX) and np.array_equal(state["sss"], half.ocean_read()["sss"])
    for k in ("hsnow", "tice0"):  # the column state a coupled run carries besides (as tests/test_column_transport_cpu.py does)
        state[k] = half.col[k].numpy().copy()
    state["newice"] = half.newice.numpy().copy()
    rest = run_coupled(0, 1, 2, resume=state)
    a, b = owned_state(full), owned_state(rest)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_the_default_is_the_core_without_the_keyword():
    a, b = run_coupled(0, 1, 2, slab_ocean=False, keyword=True), run_coupled(0, 1, 2, slab_ocean=False, keyword=False)
    x, y = owned_state(a), owned_state(b)
    for k in x:
        assert torch.equal(x[k], y[k]), k
    start = synthetic.column_fields(NX * NY, 5)[1]
    assert np.array_equal(x["sst"].numpy().reshape(-1), start["sst"])  # and its ocean is the forcing it was given
    assert sorted(a.state_dict()) == sorted(b.state_dict())


# ---- the header of the calls ----------------------------------------------------------------------------------------------------------------
def test_ocean_header_is_plain_c_and_every_call_is_exported_and_bound():
    import ctypes as C
    import re
    import subprocess

    from nextsimdg_amd import abi, build

    inc = os.path.join(ROOT, "include")
    for header in ("nsdg_ocean.h", "nsdg.h"):
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, header)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()
    assert '#include "nsdg_ocean.h"' in open(os.path.join(inc, "nsdg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nsdg_ocean.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(abi.OCEAN_SYMBOLS) == ["nsdg_column_step_ocean", "nsdg_slab_default_params", "nsdg_slab_params_set"]
    assert not set(abi.OCEAN_SYMBOLS) & (set(abi.SYMBOLS) | set(abi.TRACER_SYMBOLS) | set(abi.BASAL_SYMBOLS))
    build.build_lib(verbose=False)
    lib = abi.load_library()
    for n in names:
        assert hasattr(lib, n), "libnsdg.so does not export " + n
    assert lib.nsdg_abi_version() == 6
    p = abi.slab_default_params()
    assert (p.relax_t, p.relax_s, p.ice_salinity) == (0.0, 0.0, R.ICE_S) and C.sizeof(p) == 32
    # without a context: argument errors, never a crash
    assert lib.nsdg_slab_params_set(None, C.byref(p)) == -1
    assert lib.nsdg_column_step_ocean(None, 1, 600.0, *([None] * 18)) == -1

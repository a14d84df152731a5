"""Ice tracers (include/nsdg.h "ice tracers") without a GPU: the Python driver on the oracle stand-in with the numpy
restatement of the three tracer calls (tests/tracers_ops.py, tests/tracers_ref.py).  The refusals of tracers=, 1 gloo rank == 2 == 3 bit
for bit, checkpoint and resume, the rest of the model untouched by the tracers, the calls a tracer group adds to a step, and the analytic
properties the GPU tests assert (tests/test_gpu_tracers.py) -- here they confirm that the chosen inputs keep the reference itself inside
the bounds, the closed-pack condition included."""
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

import tracers_ref as R  # noqa: E402
from nextsimdg_amd import rowblock, synthetic  # noqa: E402
from tracers_ops import tracers_ops  # noqa: E402

DT = 120.0


# ---- the runs the CPU and the GPU tests share -----------------------------------------------------------------------------------------
def pack(n, L, closed=False, seed=4):
    """the box of tests/test_gpu_column_transport.py's core runs: the cyclone on a uniform wind over the box test's ice -- or, closed, over
    a pack with H in 1-2 m and A in 0.8-0.95 per element, where no element comes near the ice test.  (bt, H, A, uo, vo, ua, va)"""
    bt = synthetic.BoxTest(n, n, L)
    H, A = bt.dg_fields()
    if closed:
        rng = np.random.default_rng(seed)
        H[0] = 1.0 + rng.random((n, n))
        A[0] = 0.8 + 0.15 * rng.random((n, n))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    return bt, H, A, uo, vo, 4.0 * ua + 10.0, 4.0 * va + 6.0


def freezing_column(core, n, tice0=-8.0):
    """column planes under which the ice grows: a cold, dry, dark sky over an ocean at its freezing point"""
    col = {k: np.zeros((n, n)) for k in core.col}
    col["tice0"][:] = tice0
    col["sst"][:], col["sss"][:], col["tair"][:], col["tdew"][:] = -1.76, 32.0, -30.0, -32.0
    col["slp"][:], col["qlw"][:], col["mld"][:], col["wind"][:] = 1e5, 150.0, 10.0, 5.0
    return col


def origin_field(n, seed=9):
    return np.random.default_rng(seed).uniform(1.0, 5.0, (n, n))


def assert_uniform(core, name, value, steps):
    """the tracer equals `value` in every element that holds ice, to steps x 1e-13 relative"""
    H, A, T = core.H.cpu().numpy(), core.A.cpu().numpy(), core._tr[core.tracers.index(name)].cpu().numpy()
    ice = R.holds_ice(H[0], A[0], core.min_conc, core.min_thick)
    assert ice.any()
    err = float(np.max(np.abs(T[ice] - value)))
    assert err <= steps * 1e-13 * abs(value), (name, value, err)
    assert np.all(T[~ice] == 0.0)


def dynamics_step(core):
    """one step without the column model: DynamicsCore.step(); on a CoupledCore the momentum and the transport alone, as the column
    state transport's own core tests run it (no thermodynamics: the age is the clock, nothing dilutes)"""
    if isinstance(core, rowblock.CoupledCore):
        core._set_grid()
        core.momentum()
        core.transport()
        core.time += core.dt
    else:
        core.step()


def run_properties(make_core, n, L, steps):
    """the table of the driver runs for a DynamicsCore or a CoupledCore made by make_core(bt, tracers): returns nothing, asserts everything"""
    # a uniform passive tracer stays uniform, and the age of a pack that holds ice throughout is the elapsed time
    bt, H, A, uo, vo, ua, va = pack(n, L)
    core = make_core(bt, ("age", "origin"))
    core.load_global(H, A, uo, vo, ua, va)
    core.load_tracers({"origin": np.full((n, n), 7.0)})
    for k in range(1, steps + 1):
        dynamics_step(core)
        assert_uniform(core, "origin", 7.0, k)
        assert_uniform(core, "age", k * DT, k)
    assert float(core.u.abs().max()) > 1e-4
    assert not np.array_equal(core.H.cpu().numpy(), H)
    core.close()
    # the content sum mean(H) T of a non-uniform passive tracer is conserved by each transport of a closed pack, and the tracer moves
    bt, H, A, uo, vo, ua, va = pack(n, L, closed=True)
    core = make_core(bt, ("origin",))
    core.load_global(H, A, uo, vo, ua, va)
    T0 = origin_field(n)
    core.load_tracers({"origin": T0})
    before = R.tracer_content(H, T0, A)
    for k in range(steps):
        dynamics_step(core)
        Hn, An, T = core.H.cpu().numpy(), core.A.cpu().numpy(), core.tracers_read()["origin"]
        assert R.holds_ice(Hn[0], An[0]).all(), "an element of the closed pack crossed the ice test"
        after = R.tracer_content(Hn, T, An)
        assert abs(after - before) <= 1e-12 * abs(before), (k, before, after)
        before = after
    assert float(core.u.abs().max()) > 1e-4
    assert float(np.max(np.abs(T - T0))) > 1e-6
    core.close()


def cpu_core(bt, tracers, cls=rowblock.DynamicsCore, blk=None, nsub=5, **kw):
    blk = blk if blk is not None else rowblock.RowBlock(bt.nx, bt.ny)
    return cls(tracers_ops(), blk, bt.hx, bt.hy, DT, nsub, torch.device("cpu"), tracers=tracers, **kw)


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    H = np.zeros((6, 1, 6))
    H[0, 0] = [2.0, 0.5, 0.0, -1.0, np.nan, 1e-3]
    H[1:] = 3.0
    A = np.zeros((6, 1, 6))
    A[0, 0] = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    T = [np.array([[4.0, -2.0, 1.0, 1.0, 1.0, 1.0]]), np.array([[10.0] * 6])]
    Q = R.weight(H, T)
    assert Q[0][0, 0, 0] == 8.0 and Q[0][3, 0, 1] == -6.0 and Q[1][0, 0, 1] == 5.0
    got = R.recover(H, A, Q, (R.PASSIVE, R.AGE), 120.0, [np.full((1, 6), 99.0)] * 2)
    assert list(got[0][0]) == [4.0, -2.0, 0.0, 0.0, 0.0, 0.0]  # 1e-3 < min_thick * 0.5: no ice
    assert list(got[1][0]) == [130.0, 130.0, 0.0, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="kind"):
        R.recover(H, A, Q, (0, 2), 1.0, T)
    hb = np.array([[1.0, 1.0, 1.0, -1.0, np.nan, 0.0, 2.0]])
    ha = np.array([[2.0, 1.0, 0.5, 1.0, 1.0, 0.0, np.nan]])
    (t,) = R.dilute(hb, ha, [np.full((1, 7), 6.0)])
    assert list(t[0]) == [3.0, 6.0, 6.0, 0.0, 0.0, 0.0, 0.0]
    (t,) = R.dilute(hb, ha, [np.full((1, 7), 6.0)], 0, 0)
    assert np.all(t == 6.0)
    assert R.tracer_content(H, T[0], A) == 2.0 * 4.0 + 0.5 * -2.0


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
def test_driver_refuses_bad_tracer_names():
    bt = synthetic.BoxTest(8, 8)

    class Watch(type(tracers_ops())):
        touched = False

        def set_transport_bounds(self, bounds):
            Watch.touched = True
            super().set_transport_bounds(bounds)

    make = lambda tracers, ops=None, cls=rowblock.DynamicsCore: cls(ops if ops is not None else Watch(alpha=200.0, beta=200.0), rowblock.RowBlock(8, 8),
                                                                     bt.hx, bt.hy, DT, 3, torch.device("cpu"), tracers=tracers)
    for bad, match in ((("a", "b", "c", "d", "e"), "at most 4"), (("age", "age"), "more than once"), (("2nd",), "identifier"),
                       (("my tracer",), "identifier"), ((3,), "identifier"), (("H",), "collides"), (("tracers",), "collides"),
                       (("u",), "collides"), (("tice0",), "collides")):
        with pytest.raises(ValueError, match=match):
            make(bad)
    from oracle_ops import OracleOps

    with pytest.raises(ValueError, match="tracers_weight, tracers_recover, tracers_dilute"):
        make(("age",), ops=OracleOps())
    assert not Watch.touched  # a refusing constructor has changed nothing on ops
    for none in (None, ()):
        core = make(none)
        assert core.tracers == () and core.tracers_read() == {} and "tracers" not in core.state_dict()
        with pytest.raises(ValueError, match="not among"):
            core.load_tracers({"age": np.zeros((8, 8))})
    core = make(("age", "origin"))
    assert core.tracers == ("age", "origin") and core._tracer_kinds == (R.AGE, R.PASSIVE)
    with pytest.raises(ValueError, match="shape"):
        core.load_tracers({"origin": np.zeros((4, 8))})


@pytest.mark.parametrize("cls", [rowblock.DynamicsCore, rowblock.CoupledCore])
def test_properties_hold_on_the_reference(cls):
    run_properties(lambda bt, tracers: cpu_core(bt, tracers, cls=cls), 24, 96e3, 4)


def run_one(cls, tracers, steps, n=16, resume=None, advance=None, land=None, load=None, **kw):
    bt, H, A, uo, vo, ua, va = pack(n, 64e3, closed=True, seed=11)
    A[0, :3, :5] = 0.0  # open water in a corner: both branches of the ice test
    H[0, :3, :5] = 0.0
    core = cpu_core(bt, tracers, cls=cls, land=land, **kw)
    core.load_global(H, A, uo, vo, ua, va)
    if cls is rowblock.CoupledCore:
        core.load_column(freezing_column(core, n))
    if tracers:
        core.load_tracers({name: origin_field(n, seed=3 + k) for k, name in enumerate(tracers) if load is None or name in load})
    if resume is not None:
        core.load_state_dict(resume)
    for _ in range(steps):
        if advance:
            core.advance(DT, substeps=advance)
        else:
            core.step()
    return core


def test_n_steps_equal_half_plus_state_dict_plus_half():
    full = run_one(rowblock.DynamicsCore, ("age", "origin"), 4)
    half = run_one(rowblock.DynamicsCore, ("age", "origin"), 2)
    state = rowblock.DynamicsCore.merge_states([half.state_dict()])
    assert sorted(state["tracers"]) == ["age", "origin"] and state["tracers"]["age"].shape == (16, 16)
    rest = run_one(rowblock.DynamicsCore, ("age", "origin"), 2, resume=state)
    a, b = full.state_dict(), rest.state_dict()
    for k in ("H", "A", "u", "v", "s11", "s12", "s22"):
        assert np.array_equal(a[k], b[k]), k
    for name in ("age", "origin"):
        assert np.array_equal(a["tracers"][name], b["tracers"][name]), name
    assert float(np.abs(a["tracers"]["age"]).max()) > 0 and np.any(a["tracers"]["origin"] == 0.0)  # the open corner
    # a state without the key loads zeros; one without one of the names loads zeros for that name
    del state["tracers"]["age"]
    rest.load_state_dict(state)
    assert float(rest._tr[0].abs().max()) == 0.0 and np.array_equal(rest.tracers_read()["origin"], state["tracers"]["origin"])
    del state["tracers"]
    rest.load_state_dict(state)
    assert all(float(t.abs().max()) == 0.0 for t in rest._tr)


@pytest.mark.parametrize("cls", [rowblock.DynamicsCore, rowblock.CoupledCore])
def test_the_rest_of_the_model_does_not_see_the_tracers(cls):
    a, b = run_one(cls, ("age", "origin", "x", "y"), 3), run_one(cls, None, 3)
    for k in ("H", "A", "u", "v"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for x, y in zip(a.s, b.s):
        assert torch.equal(x, y)
    assert float(a.u.abs().max()) > 1e-4


def test_advance_with_two_substeps_equals_two_steps_at_half_dt():
    a = run_one(rowblock.DynamicsCore, ("age", "origin"), 2, advance=2)
    b = run_one(rowblock.DynamicsCore, ("age", "origin"), 0)
    b.dt = DT / 2
    for _ in range(4):
        b.step()
    for name in a.tracers:
        assert np.array_equal(a.tracers_read()[name], b.tracers_read()[name]), name
    assert torch.equal(a.H, b.H)


def test_coupled_growth_dilutes_and_the_mean_age_lags_the_clock():
    """the column step under a freezing sky: where it raises the mean thickness the tracers fall by the ratio of the restatement, and
    the domain-mean age grows by less than dt per step"""
    n, steps = 16, 3
    core = run_one(rowblock.CoupledCore, ("age", "origin"), 0, load=("origin",))  # the age starts at 0
    grew = 0
    for k in range(1, steps + 1):
        core._set_grid()
        core.external_forcing()
        hb, tb = core.H[0].numpy().copy(), [t.numpy().copy() for t in core._tr]
        core.thermodynamics()
        ha = core.H[0].numpy().copy()
        want = R.dilute(hb, ha, tb)
        for t, w in zip(core._tr, want):
            assert np.array_equal(t.numpy(), w)
        up = ha > np.maximum(hb, 0.0)
        grew += int(up.sum())
        had = up & (tb[1] > 0.0)  # (a lead that froze over held 0 and holds 0)
        assert had.any() and np.all(core._tr[1].numpy()[had] < tb[1][had])  # origin > 0 falls where the ice grew
        core.momentum()
        core.transport()
        core.time += core.dt
    assert grew > n * n // 2
    ice = R.holds_ice(core.H[0].numpy(), core.A[0].numpy())
    assert 0.0 < float(core._tr[0].numpy()[ice].mean()) < steps * DT  # without growth every element's age is the clock's steps x dt


def test_land_and_open_water_hold_exactly_zero():
    n = 16
    land = np.zeros((n, n), dtype=bool)
    land[6:9, 4:8] = True
    core = run_one(rowblock.DynamicsCore, ("age", "origin"), 3, land=land)
    H, A = core.H.numpy(), core.A.numpy()
    ice = R.holds_ice(H[0], A[0])
    assert (~ice).sum() > land.sum() and ice.sum() > 0
    for t in core._tr:
        assert np.all(t.numpy()[land] == 0.0) and np.all(t.numpy()[~ice] == 0.0) and np.all(t.numpy()[ice] != 0.0)


def test_column_state_run_stays_finite_and_uniform():
    """advect_column_state and tracers together (the brittle rheology has no CPU stand-in with the tracer calls: on the GPU only); the
    column step off, as in the uniform-temperature test of the column state transport"""
    n, steps = 16, 2
    bt, H, A, uo, vo, ua, va = pack(n, 64e3)
    core = cpu_core(bt, ("age", "origin"), cls=rowblock.CoupledCore, advect_column_state=True)
    core.load_global(H, A, uo, vo, ua, va)
    core.load_column(freezing_column(core, n))
    core.load_tracers({"origin": np.full((n, n), 7.0)})
    for k in range(1, steps + 1):
        core._set_grid()
        core.momentum()
        core.transport()
        assert all(bool(torch.isfinite(f).all()) for f in (core.H, core.A, core.S, core.Q, core.u, *core._tr))
        assert_uniform(core, "origin", 7.0, k)
        assert_uniform(core, "age", k * DT, k)
        assert_uniform_tice = core.col["tice0"].numpy()
        assert float(np.max(np.abs(assert_uniform_tice + 8.0))) <= 8.0 * k * 1e-13


# ---- the calls a tracer group adds ---------------------------------------------------------------------------------------------------
def test_call_trace_without_tracers_is_unchanged_and_a_group_adds_only_its_own_calls():
    import test_driver_trace_cpu as TR

    def names(tracers, cls):
        rec = TR.Recorder()
        bt, H, A, uo, vo, ua, va = pack(12, 48e3)

        class Ops(TR.StubOps):
            pass

        for name in ("tracers_weight", "tracers_recover", "tracers_dilute", "copy_f64"):
            setattr(Ops, name, lambda self, *a, **kw: None)
        ops = TR.RecordingOps(Ops(alpha=200.0, beta=200.0), rec)
        core = cls(ops, rowblock.RowBlock(12, 12), bt.hx, bt.hy, DT, 3, torch.device("cpu"), **({} if tracers == "absent" else {"tracers": tracers}))
        core.load_global(H, A, uo, vo, ua, va)
        if cls is rowblock.CoupledCore:
            core.load_column(freezing_column(core, 12))
        for _ in range(2):
            core.step()
        core.close()
        return rec.trace

    for cls in (rowblock.DynamicsCore, rowblock.CoupledCore):
        base = names("absent", cls)
        assert names(None, cls) == base and names((), cls) == base
        assert not [c for c in base if c[0].startswith("tracers_") or c[0] == "copy_f64"]
        with_group = names(("age", "origin"), cls)
        count = lambda trace, name: sum(1 for c in trace if c[0] == name)
        added = {"tracers_weight": 2, "tracers_recover": 2, "transport_stage": 6}
        if cls is rowblock.CoupledCore:
            added.update(tracers_dilute=2, copy_f64=2)
        for name in sorted({c[0] for c in with_group} | {c[0] for c in base}):
            assert count(with_group, name) == count(base, name) + added.get(name, 0), name
        # the calls of the first group are the same calls, in the same order
        own = [c[0] for c in with_group if not (c[0].startswith("tracers_") or c[0] == "copy_f64")]
        stages = [i for i, nm in enumerate(own) if nm == "transport_stage"]
        drop = set(stages[3:6] + stages[9:12])  # the tracer group's three stages of each step follow the first group's
        assert [nm for i, nm in enumerate(own) if i not in drop] == [c[0] for c in base]


# ---- row blocks over gloo ---------------------------------------------------------------------------------------------------------------
NX, NY, NSUB = 20, 29, 5


def run_coupled(rank, world, steps):
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    A[0, 10:14, 3:9] = 0.0  # a lead: the ice test fails there
    H[0, 10:14, 3:9] = 0.0
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    core = rowblock.CoupledCore(tracers_ops(), rowblock.RowBlock(NX, NY, rank, world, 1, 1), bt.hx, bt.hy, DT, NSUB, torch.device("cpu"),
                                tracers=("age", "origin"))
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    state, forcing, _ = synthetic.column_fields(NX * NY, 5)
    col = {k: v.reshape(NY, NX) for k, v in {**state, **forcing}.items()}
    col["wind"] = 0.2 * col["wind"]
    core.load_column(col)
    core.load_tracers({"age": rng.uniform(0.0, 1e6, (NY, NX)), "origin": rng.uniform(-3.0, 3.0, (NY, NX))})
    for _ in range(steps):
        core.step()
    return core


def owned_state(core):
    b = core.blk
    out = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
    out["s11"] = core.owned(core.s[0]).clone()
    out["tice0"] = core.col["tice0"][b.j0:b.j1].clone()
    for name, t in core.tracers_read().items():
        out[name] = torch.from_numpy(t)
    return out


def gloo_worker(rank, world, port, outdir):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        core = run_coupled(rank, world, 2)
        # the ghost rows of the tracers equal their owners without a message of their own
        states = [None] * world
        dist.all_gather_object(states, core.state_dict())
        merged = rowblock.DynamicsCore.merge_states(states)
        for name, t in zip(core.tracers, core._tr):
            assert np.array_equal(t.numpy(), merged["tracers"][name][core.blk.elem_slice()]), name
        torch.save(owned_state(core), os.path.join(outdir, "rank%d.pt" % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_world_equals_world_one_bitwise(world, tmp_path):
    import torch.multiprocessing as mp

    ref = run_coupled(0, 1, 2)
    want = owned_state(ref)
    assert float(want["age"].abs().max()) > 0 and bool((want["origin"] == 0).any())
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(gloo_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    parts = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r)) for r in range(world)]
    for key in want:
        got = torch.cat([p[key] for p in parts], dim=1 if key in ("H", "A", "s11") else 0)
        assert torch.equal(got, want[key]), key


# ---- the header of the calls --------------------------------------------------------------------------------------------------------------
def test_tracer_header_is_plain_c_and_every_call_is_exported_and_bound():
    """include/nsdg_tracers.h compiles as C99 on its own and through include/nsdg.h; the library exports what it declares and
    abi.TRACER_SYMBOLS binds exactly that"""
    import re
    import subprocess

    from nextsimdg_amd import abi, build

    inc = os.path.join(ROOT, "include")
    for header in ("nsdg_tracers.h", "nsdg.h"):
        p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, header)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert p.returncode == 0, p.stdout.decode()
    assert '#include "nsdg_tracers.h"' in open(os.path.join(inc, "nsdg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nsdg_tracers.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(nsdg_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(abi.TRACER_SYMBOLS) and len(names) == 3
    assert "#define NSDG_TRACERS_MAX %d" % abi.TRACERS_MAX in src and "NSDG_TRACER_AGE = %d" % abi.TRACER_AGE in src
    build.build_lib(verbose=False)
    lib = abi.load_library()
    for n in names:
        assert hasattr(lib, n), "libnsdg.so does not export " + n
    # without a context: an argument error, never a crash
    assert lib.nsdg_tracers_weight(None, 2, 0, 1, None, 1, None, None) == -1 and lib.nsdg_tracers_dilute(None, 0, 1, None, None, 1, None) == -1
    assert lib.nsdg_tracers_recover(None, 2, 0, 1, None, None, 1, None, None, 1.0, 0.0, 0.0, None) == -1

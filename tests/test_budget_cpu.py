"""The momentum budget (include/nsdg_budget.h) without a GPU: the header and its bindings, the numpy restatement
(tests/budget_ref.py) held to its own identities, and the Python driver (DynamicsCore(budget=...)) on the CPU twin: one block against gloo
worlds of 2 and 3 bit for bit, the refusals, and the call trace of a driver without budget=."""
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

import budget_ref as BU  # noqa: E402
import mevp_ref as MR  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402
from oracle_ops import OracleOps  # noqa: E402

UNIFORM = dict(alpha=200.0, beta=200.0)
ADAPTIVE = dict(aevp_c=(2.4 * np.pi) ** 2, aevp_alpha_min=3.0, delta_min=2e-7)
HEADER = os.path.join(ROOT, "include", "nsdg_budget.h")
FUNCTIONS = {"nsdg_momentum_budget", "nsdg_budget_term_id"}
EPS = 2.0 ** -53


# ---- header and bindings -----------------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_two_functions_and_the_table_binds_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert set(re.findall(r"\b(nsdg_\w+)\s*\(", text)) == FUNCTIONS
    assert set(abi.BUDGET_SYMBOLS) == FUNCTIONS
    for other in (abi.SYMBOLS, abi.TRACER_SYMBOLS, abi.BASAL_SYMBOLS, abi.OCEAN_SYMBOLS, abi.SNOW_SYMBOLS, abi.TILT_SYMBOLS):
        assert not set(other) & FUNCTIONS
    assert '#include "nsdg_budget.h"' in open(os.path.join(ROOT, "include", "nsdg.h")).read()
    assert re.search(r"#define\s+NSDG_BUDGET_QUANTITIES\s+9", text) and abi.BUDGET_QUANTITIES == 9 and abi.BUDGET_KE == 8
    # the struct's members in the header's order
    members = re.search(r"struct nsdg_budget_out \{(.*?)\};", text, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)\s*[,;]", members) == [f[0] for f in abi.BudgetOut._fields_[:17]]
    assert [f[0] for f in abi.BudgetOut._fields_[17:]] == ["power_stride", "row0"]
    assert abi.BUDGET_TERMS == BU.TERMS


def test_header_compiles_alone_as_c99(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "nsdg_budget.h"\nint main(void) { struct nsdg_budget_out o = { 0 }; return nsdg_momentum_budget(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &o) '
                   '== 0 && nsdg_budget_term_id("wind") == 0 && NSDG_BUDGET_TERMS == 8; }\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "only.o")])


def test_term_ids_and_a_null_context_without_a_device():
    lib = abi.load_library()
    for i, name in enumerate(abi.BUDGET_TERMS):
        assert lib.nsdg_budget_term_id(name.encode()) == i
    assert lib.nsdg_budget_term_id(b"friction") == -1 and lib.nsdg_budget_term_id(None) == -1
    assert lib.nsdg_momentum_budget(None, 0, 0, *([None] * 11)) == -1
    assert lib.nsdg_abi_version() == 6


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def random_case(nx=9, ny=7, seed=5, free_columns=True):
    rng = np.random.default_rng(seed)
    p = MR.par()
    hx, hy, dt = 4000.0, 3000.0, 120.0
    shape = (2 * ny + 1, 2 * nx + 1)
    H, A = np.zeros((6, ny, nx)), np.zeros((6, ny, nx))
    H[0], A[0] = 1.0 + rng.random((ny, nx)), 0.7 + 0.3 * rng.random((ny, nx))
    if free_columns:
        H[:, :, 2] = A[:, :, 2] = 0.0
    f = lambda s: s * rng.standard_normal(shape)
    u, v, u0, v0, ua, va, uo, vo = f(0.05), f(0.05), f(0.05), f(0.05), f(8.0), f(8.0), f(0.03), f(0.03)
    for x in (u, v):
        x[0] = x[-1] = 0.0
        x[:, 0] = x[:, -1] = 0.0
    S = [2e3 * rng.standard_normal((8, ny, nx)) for _ in range(3)]
    prep = MR.prepare(p, H, A, ua, va, uo, vo)
    c = MR.packed_coefficients(p, dt, u0, v0, prep)
    return dict(p=p, hx=hx, hy=hy, dt=dt, H=H, A=A, u=u, v=v, u0=u0, v0=v0, ua=ua, va=va, uo=uo, vo=vo, S=S, prep=prep, c=c, shape=shape)


def test_restated_residual_is_the_defect_of_one_more_update_of_the_independent_sub_iteration():
    """the identity that holds the device's residual to nsdg_mevp_velocity, on the restatements: with u' the velocity of
    mevp_ref.velocity from (S, u), R = (K2 h' + drag) (u' - u) to rounding -- two statements of the balance that share no line"""
    k = random_case()
    p, dt = dict(k["p"], alpha=1.0, beta=1.0), k["dt"]
    F = BU.forces(p, dt, k["hx"], k["hy"], k["c"], k["A"], k["ua"], k["va"], k["S"], k["u"], k["v"])
    ny = k["H"].shape[1]
    un, vn, g0, g1 = MR.velocity(p, k["hx"], k["hy"], dt, k["S"], None, 0, k["u"], k["v"], k["u0"], k["v0"], k["prep"], 0, ny)
    free = k["c"][0] > 2.0 ** 50
    assert free.any() and not free.all()
    hp = np.where(free, 2.0 ** -100, 1.0) * k["c"][0]
    cd = np.where(free, 2.0 ** -100, 1.0) * k["c"][1]
    den = p["rho_ice"] * (1.0 + p["beta"]) / dt * hp + cd * np.sqrt((k["uo"] - k["u"]) ** 2 + (k["vo"] - k["v"]) ** 2)
    scale = BU.scale(F)
    live = ~F["fixed"]
    for key, new, old in (("residual_x", un, k["u"]), ("residual_y", vn, k["v"])):
        err = np.abs(F[key] - den * (new - old))[live]
        print("%s: worst %.3g eps sum|terms|" % (key, float(np.max(err / (EPS * scale[live])))))
        assert np.all(err <= 64 * EPS * scale[live])
    for c in "xy":  # and the seven terms add up to it
        assert np.all(np.abs(sum(F[t + "_" + c] for t in BU.TERMS[:-1]) - F["residual_" + c]) <= 16 * EPS * scale)
    # inertia is -m (u - u^n) / dt
    m = F["m"]
    lim = 16 * EPS * (scale + np.abs((m / dt) * k["u0"]) + np.abs((m / dt) * k["u"]))  # c2 is a rounded sum that holds mdt u0
    assert np.all(np.abs(F["inertia_x"] - (-(m / dt) * (k["u"] - k["u0"])))[live] <= lim[live])
    assert np.all(F["internal_x"][free] == 0.0) and np.abs(F["internal_x"][live & ~free]).min() > 0.0


def test_row_totals_fold_in_the_stated_order():
    """the fold by halves of 64 lanes, by hand on integers whose sums are exact in any order, and on values whose order shows"""
    acc = np.arange(64.0)[None, :]
    assert BU.fold(acc)[0] == 63 * 64 / 2
    x = np.zeros((1, 64))
    x[0, 0], x[0, 32], x[0, 16] = 1.0, 2.0 ** -53, 2.0 ** -53  # s = 32: 1 + 2^-53 rounds to 1; s = 16: the other 2^-53 meets 1 and is lost too
    assert BU.fold(x)[0] == 1.0 and (x[0, 16] + x[0, 32]) + x[0, 0] == 1.0 + 2.0 ** -52  # another order keeps them
    k = random_case(nx=70, ny=3, free_columns=False)
    F = BU.forces(k["p"], k["dt"], k["hx"], k["hy"], k["c"], k["A"], k["ua"], k["va"], k["S"], k["u"], k["v"])
    whole = BU.row_totals(F, k["u"], k["v"], k["hx"], k["hy"], 0, 3)
    part = BU.row_totals(F, k["u"], k["v"], k["hx"], k["hy"], 1, 3)
    assert np.array_equal(whole[:, 1:], part) and whole[BU.KE].min() > 0.0
    # a row's total is the plain sum to rounding
    area = k["hx"] * k["hy"]
    ml = np.zeros(k["shape"])
    ml[0::2, 0::2], ml[0::2, 1::2], ml[1::2, 0::2], ml[1::2, 1::2] = area / 9.0, area / 4.5, area / 4.5, area / 2.25
    p = ml * (k["u"] * F["wind_x"] + k["v"] * F["wind_y"])
    assert abs(whole[0, 1] - p[2:4, :-1].sum()) <= 1e-12 * np.abs(p[2:4]).sum()


# ---- the Python driver on the twin ------------------------------------------------------------------------------------------------------
NX, NY, NSUB, DT = 20, 29, 5, 120.0
CONFIGS = {"uniform": (UNIFORM, {}), "adaptive": (ADAPTIVE, {}), "all": (UNIFORM, dict(land=True, basal=True, tilt=True))}
TERMS = ("wind", "water", "tilt", "internal", "basal", "inertia", "residual")


def island():
    """five rows across the block boundaries of worlds 2 (row 14) and 3 (rows 9, 19)"""
    land = np.zeros((NY, NX), dtype=bool)
    land[8:21, 7:12] = True
    return land


def run_core(name, rank, world, steps=2, budget=TERMS, power=True, cls=rowblock.DynamicsCore, **kw):
    pk, setting = CONFIGS[name]
    bt = synthetic.BoxTest(NX, NY)
    rng = np.random.default_rng(43)
    H, A = bt.dg_fields()
    A[0] -= 0.3 * rng.random((NY, NX))
    H[1:3] += 0.02 * rng.standard_normal((2, NY, NX))
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    ops = BU.BudgetOracleOps(**pk) if name == "all" else BU.make_ops(**setting, **pk)  # "all": the twin with every call
    extra = {}
    if setting.get("land"):
        extra["land"] = island()
    if setting.get("basal"):
        extra["bathymetry"] = rng.uniform(0.5, 4.0, (NY, NX))
    if setting.get("tilt"):
        extra["tilt"] = "ssh"
    core = cls(ops, rowblock.RowBlock(NX, NY, rank, world, 1, 1), bt.hx, bt.hy, DT, NSUB, torch.device("cpu"), budget=budget, budget_power=power,
               **extra, **kw)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    if setting.get("tilt"):
        x, y = np.meshgrid(np.linspace(0.0, 1.0, 2 * NX + 1), np.linspace(0.0, 1.0, 2 * NY + 1))
        core.set_ssh(4.0 * x + np.sin(3.0 * x + 5.0 * y))
    for _ in range(steps):
        core.step()
    return core


def worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for name in CONFIGS:
            torch.save(run_core(name, rank, world).budget_read(), os.path.join(outdir, "%s.rank%d.pt" % (name, rank)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def single_domain():
    return {name: run_core(name, 0, 1) for name in CONFIGS}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_driver_reads_the_balance_of_the_state_it_left(name, single_domain):
    core = single_domain[name]
    got = core.budget_read()
    assert got["rows"] == (0, NY) and set(got) == {"rows", "power", "ke"} | {t + "_" + c for t in TERMS for c in "xy"}
    assert got["wind_x"].shape == (2 * NY + 1, 2 * NX + 1) and got["ke"].shape == (NY,) and set(got["power"]) == set(abi.BUDGET_TERMS)
    assert all(np.isfinite(got[k]).all() for k in got if k not in ("rows", "power"))
    assert np.abs(got["residual_x"]).max() > 1e-6 and np.abs(got["internal_y"]).max() > 1e-6 and got["ke"].max() > 0.0
    assert (np.abs(got["basal_x"]).max() > 0.0) == (name == "all")
    # the seven terms add up to the residual at the state the step left (coriolis was not asked for: it is the difference)
    rest = got["residual_x"] - sum(got[t + "_x"] for t in TERMS[:-1])
    v = core.v.numpy()
    F = BU.scale({k: got.get(k, np.zeros_like(v)) for k in BU.PLANES})
    cor = abi_k3(core) * hp_of(core) * v
    live = F > 0
    assert np.all(np.abs(rest - cor)[live] <= 64 * EPS * (F + np.abs(cor))[live])
    merged = rowblock.DynamicsCore.merge_budget([got])
    assert merged["rows"] == (0, NY) and np.array_equal(merged["ke"], got["ke"])
    assert merged["ke_total"] == float(np.add.accumulate(got["ke"])[-1]) and set(merged["power_total"]) == set(abi.BUDGET_TERMS)
    if name == "all":
        assert core.ops.ssh is None  # on the ops object for the launch alone
        import land_ref

        ln = land_ref.land_nodes(island())
        assert all(np.all(got[t + "_" + c][ln] == 0.0) for t in TERMS for c in "xy")


def abi_k3(core):
    return core.ops.p.rho_ice * core.ops.p.fc


def hp_of(core):
    _, _, _, _, cgh, _ = core.ops.nodal
    return np.maximum(cgh, core.ops.p.h_min)


@pytest.mark.parametrize("world", [2, 3])
def test_row_blocks_equal_the_single_domain_bitwise(world, tmp_path, single_domain):
    """planes and merged totals, in any order of the parts"""
    from test_rowblock_gloo import free_port

    mp.spawn(worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    for name, ref in single_domain.items():
        want = rowblock.DynamicsCore.merge_budget([ref.budget_read()])
        parts = [torch.load(os.path.join(str(tmp_path), "%s.rank%d.pt" % (name, r)), weights_only=False) for r in range(world)]
        got = rowblock.DynamicsCore.merge_budget(parts[::-1])
        assert got["rows"] == want["rows"]
        for k in want:
            if k in ("rows",):
                continue
            if isinstance(want[k], dict):
                for t in want[k]:
                    assert np.array_equal(got[k][t], want[k][t]), (name, k, t)
            else:
                assert np.array_equal(got[k], want[k]), (name, k)
    with pytest.raises(ValueError, match="do not join"):
        rowblock.DynamicsCore.merge_budget([parts[0], parts[0]])


def test_substeps_read_the_last_sub_steps_balance_and_the_state_is_untouched():
    with_budget = run_core("uniform", 0, 1, steps=0)
    without = run_core("uniform", 0, 1, steps=0, budget=None, power=False)
    for core in (with_budget, without):
        core.advance(2 * DT, substeps=2)
    for k in ("H", "A", "u", "v"):
        assert torch.equal(getattr(with_budget, k), getattr(without, k)), k
    assert all(torch.equal(a, b) for a, b in zip(with_budget.s, without.s))
    assert set(with_budget.state_dict()) == set(without.state_dict())
    # one more plain step of DT from the state after the first sub-step is the second sub-step
    single = run_core("uniform", 0, 1, steps=2)
    a, b = with_budget.budget_read(), single.budget_read()
    assert all(np.array_equal(a[k], b[k]) for k in a if k not in ("rows", "power")) and all(np.array_equal(a["power"][t], b["power"][t]) for t in a["power"])
    assert not hasattr(without, "_budget_planes")


def test_refusals_come_before_anything_on_the_ops_object_changes():
    bt = synthetic.BoxTest(8, 8)
    args = (rowblock.RowBlock(8, 8), bt.hx, bt.hy, DT, 4, torch.device("cpu"))

    def sealed(ops):
        class Untouched(type(ops)):
            def __setattr__(self, k, v):
                if getattr(self, "_sealed", False):
                    raise AssertionError("the ops object was changed: " + k)
                super().__setattr__(k, v)

        ops.__class__ = Untouched
        ops._sealed = True
        return ops

    import bbm_ref

    class BbmWithBudget(BU.BudgetCalls, type(bbm_ref.make_ops())):
        pass

    with pytest.raises(ValueError, match="budget= needs rheology='mevp'"):
        rowblock.DynamicsCore(sealed(BbmWithBudget()), *args, rheology="bbm", budget=("wind",))
    with pytest.raises(ValueError, match="budget= needs rheology='mevp'"):
        rowblock.DynamicsCore(sealed(BbmWithBudget()), *args, rheology="bbm", budget_power=True)
    with pytest.raises(ValueError, match="unknown budget term 'friction'"):
        rowblock.DynamicsCore(sealed(BU.make_ops()), *args, budget=("wind", "friction"))
    with pytest.raises(ValueError, match="more than once"):
        rowblock.DynamicsCore(sealed(BU.make_ops()), *args, budget=("wind", "wind"))
    with pytest.raises(ValueError, match="at least one term"):
        rowblock.DynamicsCore(sealed(BU.make_ops()), *args, budget=())
    with pytest.raises(ValueError, match="momentum_budget"):
        rowblock.DynamicsCore(sealed(OracleOps()), *args, budget=("wind",))
    plain = rowblock.DynamicsCore(OracleOps(), *args)
    with pytest.raises(ValueError, match="budget="):
        plain.budget_read()
    plain.close()
    only_totals = rowblock.DynamicsCore(BU.make_ops(), *args, budget_power=True)
    assert only_totals.budget == () and only_totals._budget_planes == {}
    only_totals.close()


def test_a_driver_without_budget_asks_for_the_same_work():
    """the trace of tests/test_driver_trace_cpu.py's kind: without budget= an ops object that HAS the call sees the calls of one that has
    not; with budget= the trace is that trace plus one momentum_budget per step, after the step's last sub-iteration and before the
    transport's first call"""
    import test_driver_trace_cpu as T

    class WithBudget(T.StubOps):
        def momentum_budget(self, *a, **kw):
            return None

    def trace(stub, **kw):
        rec = T.Recorder()
        bt = synthetic.BoxTest(T.NX, 12)
        ops = T.RecordingOps(stub(mevp_variant=1, alpha=200.0, beta=200.0), rec)
        core = rowblock.DynamicsCore(ops, rowblock.RowBlock(T.NX, 12), bt.hx, bt.hy, 120.0, 3, torch.device("cpu"), **kw)
        H, A = bt.dg_fields()
        ua, va = bt.wind(0.0)
        core.load_global(H, A, *bt.ocean(), ua, va)
        for _ in range(2):
            core.step()
        core.close()
        return rec.trace

    base = trace(T.StubOps)
    assert trace(WithBudget) == base and not any(c[0] == "momentum_budget" for c in base)
    on = trace(WithBudget, budget=("wind", "residual"), budget_power=True)
    names = [c[0] for c in on]
    assert names.count("momentum_budget") == 2
    assert [c[0] for c in on if c[0] != "momentum_budget"] == [c[0] for c in base]
    for i, n in enumerate(names):
        if n == "momentum_budget":
            assert names[i - 1] == "mevp_iterate" and names[i + 1] == "prepare_advection"

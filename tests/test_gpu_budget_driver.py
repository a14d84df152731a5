"""The momentum budget in the Python driver on the device: DynamicsCore(budget=..., budget_power=True) leaves
the state of a run without it, bit for bit; one block equals four blocks, graphs equal no graphs, the native plan equals the Python
sequence, in the planes, the row totals and the merged domain totals; sub-steps read the last sub-step's balance; the coupled core
inherits it; and what budget_read() returns is the restatement's balance (tests/budget_ref.py) of the state the step left."""
import threading

import numpy as np
import pytest
import torch

import budget_ref as BU
import land_ref
from nextsimdg_amd import abi, rowblock
from test_gpu_budget import check_planes
from test_gpu_land import AD, UNIFORM
from test_gpu_parity import host
from test_gpu_tilt import driver_height, driver_island, thick_fields
from thread_ranks import Mailbox, ThreadExchanger, _local_group, fields, gather

pytestmark = pytest.mark.gpu
NX, NY, DT = 70, 96, 120.0
STATE = ("H", "A", "u", "v", "s11")


def shoal(nx=NX, ny=NY):
    """deep water with a shoal across the boundary of blocks 2 and 3 of 4 (row 48)"""
    depth = np.full((ny, nx), 500.0)
    depth[40:56, 45:60] = 1.0
    return depth


def _rank(rank, world, mailbox, out, local_group, pk, nsub, nsteps, native, use_graph, setting, budget, power, variant=4):
    try:
        ctx = abi.Context(torch.device("cuda:0"))
        ctx.set_mevp_variant(variant)
        ctx.set_mevp_params(ctx.mevp_default_params(**pk))
        bt, H, A, uo, vo, ua, va = thick_fields(NX, NY)
        # variant 4: two passes of four sub-iterations between two exchanges; variant 1: one sub-iteration per pass, ghost depth (1, 1)
        blk = rowblock.RowBlock(NX, NY, rank, world, 8, 7) if variant == 4 else rowblock.RowBlock(NX, NY, rank, world, 1, 1)
        if native:
            exchanger = rowblock.NativeHaloExchanger(ctx, blk, local_group=local_group) if world > 1 else None
        else:
            exchanger = ThreadExchanger(blk, mailbox)
        land = driver_island() if setting == "all" else None
        kw = dict(land=land, tilt="ssh", bathymetry=shoal()) if setting == "all" else {}
        core = rowblock.DynamicsCore(ctx, blk, bt.hx, bt.hy, DT, nsub, torch.device("cuda"), exchanger=exchanger, native=native, use_graph=use_graph,
                                     budget=budget, budget_power=power, **kw)
        core.load_global(H, A, uo, vo, ua, va)
        if setting == "all":
            core.set_ssh(driver_height(NX, NY, land))
        for _ in range(nsteps):
            core.step()
        torch.cuda.synchronize()
        res = {k: core.owned(getattr(core, k)).clone() for k in STATE if k != "s11"}
        res["s11"] = core.owned(core.s[0]).clone()
        if core.budget is not None:
            res["budget"] = core.budget_read()
            if rank == 0 and world == 1:
                # the transport has moved H and A on since the launch: one more momentum phase (packing, sub-cycle, budget) without a
                # transport, and the restatement from the state it leaves
                core._set_grid()
                core.momentum()
                torch.cuda.synchronize()
                res["again"] = core.budget_read()
                S = [host(ctx.private_to_planes(x, NX)) for x in core.s]
                c, tb = BU.unpack(host(core.packed), (2 * NY + 1, 2 * NX + 1))
                res["restated"] = BU.forces(BU.MR.par(**pk), DT, bt.hx, bt.hy, c, host(core.A),
                                            host(core.ua), host(core.va), S, host(core.u), host(core.v), tb=tb if setting == "all" else None,
                                            u0=abi.basal_default_params().u0, eta=host(core.ssh) if setting == "all" else None, g=abi.GRAVITY)
            assert ctx.ssh is None
        core.close()
        ctx.close()
        out[rank] = res
    except BaseException as e:  # noqa: BLE001 -- wake the peers up, then re-raise in the main thread
        with mailbox.cv:
            mailbox.error = e
            mailbox.cv.notify_all()
        out[rank] = e


def run_world(world, pk, setting, nsub=21, nsteps=2, native=True, use_graph=False, budget=abi.BUDGET_TERMS, power=True, variant=4):
    mailbox, out = Mailbox(), {}
    _local_group[0] += 1
    threads = [threading.Thread(target=_rank, args=(r, world, mailbox, out, _local_group[0], pk, nsub, nsteps, native, use_graph, setting, budget, power, variant))
               for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return out


def same_budget(got, want, what):
    assert got["rows"] == want["rows"], what
    for k in want:
        if k == "rows":
            continue
        if isinstance(want[k], dict):
            for t in want[k]:
                assert np.array_equal(got[k][t], want[k][t]), (what, k, t)
        else:
            assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("pk,setting", [pytest.param(UNIFORM, "plain", id="uniform-plain"), pytest.param(AD, "all", id="adaptive-island-shoal-ssh")])
def test_blocks_graphs_and_the_native_plan_give_the_same_budget_and_leave_the_state_alone(gpu, pk, setting):
    ref = run_world(1, pk, setting)[0]
    bare = run_world(1, pk, setting, budget=None, power=False)[0]
    assert "budget" not in bare and float(ref["u"].abs().max()) > 1e-5
    for k in STATE:  # u, v, S, H, A after the steps with budget= are those of the steps without
        assert torch.equal(ref[k], bare[k]), k
    want = rowblock.DynamicsCore.merge_budget([ref["budget"]])
    assert set(want["power_total"]) == set(abi.BUDGET_TERMS) and want["ke_total"] > 0.0
    assert abs(want["power_total"]["residual"] - sum(want["power_total"][t] for t in abi.BUDGET_TERMS[:-1])) <= 1e-9 * sum(abs(want["power_total"][t]) for t in abi.BUDGET_TERMS)
    print("%s: domain totals [W] %s, kinetic energy %.6e J" % (setting, {t: "%.4e" % p for t, p in want["power_total"].items()}, want["ke_total"]))
    # what the driver hands the launch is the state the step left: the restatement from that state, at the planes' own tolerance
    check_planes("driver %s" % setting, {k: v for k, v in ref["again"].items() if k in BU.PLANES}, ref["restated"])
    got = {k: v for k, v in want.items() if k in BU.PLANES}
    if setting == "all":
        ln = land_ref.land_nodes(driver_island())
        assert all(np.all(got[k][ln] == 0.0) for k in BU.PLANES) and np.abs(got["basal_x"]).max() > 0.0
    for world, native, graph in ((4, True, False), (1, True, True), (4, True, True), (1, False, False), (4, False, False)):
        parts = run_world(world, pk, setting, native=native, use_graph=graph)
        for k in STATE:
            assert torch.equal(gather(parts, world, k), ref[k]), (k, world, native, graph)
        same_budget(rowblock.DynamicsCore.merge_budget([parts[r]["budget"] for r in reversed(range(world))]), want, (world, native, graph))


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_single_iteration_passes_one_block_equals_four(gpu, native):
    """per_pass = 1 (variant 1, ghost depth (1, 1)): after the last sub-iteration only the velocity's ghost rows are exchanged, and the stress of
    the ghost row j0 - 1 that the launch gathers is this rank's own redundant update of it (mevp_iterate's k0 = j0 - 1) from the velocity
    its owner used -- the owner's bits.  One block against four, state and budget"""
    ref = run_world(1, AD, "all", variant=1, native=native)[0]
    assert float(ref["u"].abs().max()) > 1e-5
    want = rowblock.DynamicsCore.merge_budget([ref["budget"]])
    parts = run_world(4, AD, "all", variant=1, native=native)
    for k in STATE:
        assert torch.equal(gather(parts, 4, k), ref[k]), k
    same_budget(rowblock.DynamicsCore.merge_budget([parts[r]["budget"] for r in range(4)]), want, "per_pass = 1")


def dynamics_core(c, dt, nsub, ny=64, cls=rowblock.DynamicsCore, **kw):
    bt, H, A, uo, vo, ua, va = thick_fields(NX, ny)
    c.set_mevp_params(c.mevp_default_params(**AD))
    core = cls(c, rowblock.RowBlock(NX, ny), bt.hx, bt.hy, dt, nsub, torch.device("cuda"), native=True, budget=("wind", "internal", "inertia", "residual"),
               budget_power=True, **kw)
    core.load_global(H, A, uo, vo, ua, va)
    return core


def test_substeps_read_the_last_sub_steps_balance(gpu):
    """advance(substeps=2) reads what the second of two steps of half the length reads; substeps="auto" is the same run for the n it chose"""
    c = abi.Context(gpu)
    try:
        a = dynamics_core(c, 240.0, 16)
        assert a.advance(240.0, substeps=2) == 2
        got = a.budget_read()
        a.close()
        b = dynamics_core(c, 120.0, 16)
        b.step()
        first = b.budget_read()
        b.step()
        want = b.budget_read()
        b.close()
        same_budget(got, want, "substeps=2")
        assert not np.array_equal(first["residual_x"], want["residual_x"]) and np.abs(want["inertia_x"]).max() > 1e-6
        auto = dynamics_core(c, 240.0, 16)
        n = auto.advance(240.0, substeps="auto", courant=0.1, max_substeps=64)
        got = auto.budget_read()
        auto.close()
        fixed = dynamics_core(c, 240.0, 16)
        fixed.advance(240.0, substeps=n)
        same_budget(got, fixed.budget_read(), "substeps=auto (%d)" % n)
        fixed.close()
        print("substeps='auto' chose %d" % n)
    finally:
        c.close()


def test_coupled_core_inherits_the_budget_and_the_brittle_rheology_refuses_it(gpu):
    from test_gpu_snow import driver_column

    res = {}
    for name, native in (("native", True), ("python", False)):
        c = abi.Context(gpu)
        try:
            bt, H, A, uo, vo, ua, va = thick_fields(NX, 24)
            c.set_mevp_params(c.mevp_default_params(**AD))
            core = rowblock.CoupledCore(c, rowblock.RowBlock(NX, 24), bt.hx, bt.hy, DT, 16, torch.device("cuda"), native=native, snow_load=True,
                                        budget=("water", "inertia", "residual"), budget_power=True)
            core.load_global(H, A, uo, vo, ua, va)
            core.load_column(driver_column(NX, 24))
            core.step()
            core.step()
            torch.cuda.synchronize()
            res[name] = core.budget_read()
            assert "budget" not in core.state_dict() and set(core.state_dict()) <= set(rowblock.DynamicsCore.STATE_KEYS)
            core.close()
        finally:
            c.close()
    same_budget(res["native"], res["python"], "coupled")
    assert np.abs(res["native"]["inertia_x"]).max() > 1e-6 and res["native"]["ke"].max() > 0.0
    c = abi.Context(gpu)
    try:
        bt = fields(NX, 24)[0]
        with pytest.raises(ValueError, match="budget= needs rheology='mevp'"):
            rowblock.DynamicsCore(c, rowblock.RowBlock(NX, 24), bt.hx, bt.hy, 8.0, 8, torch.device("cuda"), rheology="bbm", budget=("wind",))
    finally:
        c.close()

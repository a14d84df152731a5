"""The brittle sub-cycle in the native row-block plan (nsdg_rb_bbm_*, csrc/rowblock.hip) against the Python-driven sequence of
DynamicsCore.subcycle(), which tests/test_gpu_bbm.py section 6 holds to the numpy restatement at 1e-9: the fields, shapes and margins are
that section's (24 x 18 cells, dt = 2.5 s, 3 steps).  Everything here is bit for bit: the plan issues the same launches in the same order.
Shapes: 18 rows as three blocks of 6 owned rows run the split launches (>= 4 rows), 9 rows as three blocks of 3 the unsplit branch; nsub = 7
is the odd count whose damage ends in the work buffer and is copied back."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bbm_ref as R  # noqa: E402
import test_gpu_bbm as G  # noqa: E402 -- section 6: driver_fields, start_state, the margins
import thread_ranks  # noqa: E402
from nextsimdg_amd import abi, rowblock  # noqa: E402

pytestmark = pytest.mark.gpu
HX, HY, DDT, DNX, DNY, DNSTEPS = G.HX, G.HY, G.DDT, G.DNX, G.DNY, G.DNSTEPS
KEYS = ("H", "A", "D", "u", "v", "s11", "s12", "s22")
ODD_NSUB = 7  # sub-iterations of 2.5 / 7 s; the margins of the reference run with it: tests/test_bbm_native_cpu.py


def island(ny):
    """an island across both block boundaries of three row blocks, two rows on each side of them at least"""
    land = np.zeros((ny, DNX), dtype=bool)
    land[ny // 3 - 2:2 * ny // 3 + 2, 10:13] = True
    return land


def fields_rows(ny):
    """section 6's fields (18 rows), or their lowest `ny` element rows"""
    f = G.driver_fields()
    if ny == DNY:
        return f
    cut = lambda a: np.ascontiguousarray(a[:, :ny])
    nodes = lambda a: np.ascontiguousarray(a[:2 * ny + 1])
    return dict(H=cut(f["H"]), A=cut(f["A"]), D=cut(f["D"]), S=[cut(s) for s in f["S"]], ua=nodes(f["ua"]), va=nodes(f["va"]), uo=nodes(f["uo"]),
                vo=nodes(f["vo"]))


def start_state(f, ny, land=None):
    z = np.zeros((2 * ny + 1, 2 * DNX + 1))
    S = [s.copy() for s in f["S"]]
    if land is not None:  # the driver clears H, A, D and the velocity on land; the stress a state brings is the caller's
        for s in S:
            s[:, land] = 0.0
    return dict(rows=(0, ny), ny_global=ny, nx=DNX, H=f["H"], A=f["A"], D=f["D"], u=z, v=z, s11=S[0], s12=S[1], s22=S[2])


def run_core(ops, device, nsub, native, rank=0, world=1, exchanger=None, nsteps=DNSTEPS, resume=None, ny=DNY, overlap=True, land=None,
             substeps=None, **kw):
    f = fields_rows(ny)
    blk = rowblock.RowBlock(DNX, ny, rank, world, 1, 1)
    core = rowblock.DynamicsCore(ops, blk, HX, HY, DDT, nsub, device, exchanger=exchanger, rheology="bbm", native=native, overlap=overlap,
                                 land=land, **kw)
    core.load_global(f["H"], f["A"], f["uo"], f["vo"], f["ua"], f["va"])
    if resume is None:
        resume = start_state(f, ny, land)
        if core._drifters is not None:  # a state brings its list: the constructor's
            resume["drifters"] = core._drifters.state()
    core.load_state_dict(resume)
    for _ in range(nsteps):
        if substeps is None:
            core.step()
        else:
            core.advance(DDT, substeps=substeps)
    return core


def result(core):
    torch.cuda.synchronize()
    res = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "D", "u", "v")}
    for k, s in zip(("s11", "s12", "s22"), core.s):
        res[k] = core.ops.private_to_planes(s, DNX)[:, core.blk.j0:core.blk.j1].clone()
    return res


def one_block(nsub, native, **kw):
    c = abi.Context(torch.device("cuda:0"))
    core = run_core(c, torch.device("cuda"), nsub, native, **kw)
    res = result(core)
    res["history"] = core.history_read() if core.history is not None else None
    res["drifters"] = core.drifters_read() if core._drifters is not None else None
    res["state"] = core.state_dict()
    core.close()
    c.close()
    return res


def native_world(world, nsub, **kw):
    """`world` thread ranks, each with a context of its own and the native exchange's in-process transport"""
    out = {}
    thread_ranks._local_group[0] += 1
    gid = thread_ranks._local_group[0]

    def rank_main(rank):
        try:
            c = abi.Context(torch.device("cuda:0"))
            c.comm_deadline(60.0)
            blk = rowblock.RowBlock(DNX, kw.get("ny", DNY), rank, world, 1, 1)
            core = run_core(c, torch.device("cuda"), nsub, True, rank, world, rowblock.NativeHaloExchanger(c, blk, local_group=gid), **kw)
            res = result(core)
            res["history"] = core.history_read() if core.history is not None else None
            res["drifters"] = core.drifters_read() if core._drifters is not None else None
            res["stats"] = core._run_mevp.stats()
            core.close()
            c.close()
            out[rank] = res
        except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread; the peers' waits end at their deadline
            out[rank] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return out


def joined(parts, k):
    return torch.cat([parts[r][k] for r in range(len(parts))], dim=0 if k in ("u", "v") else 1)


def assert_same(got, want, what):
    for k in KEYS:
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def built(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)


@pytest.fixture(scope="module")
def python_run(built):
    """the Python-driven sequence on one block, once per sub-iteration count"""
    cache = {}

    def get(nsub):
        if nsub not in cache:
            cache[nsub] = one_block(nsub, False)
        return cache[nsub]

    return get


# ---- 1. native equals the Python sequence -----------------------------------------------------------------------------------------------
# (that the reference run keeps the branch margins of section 6 with the odd count is asserted without a device:
# tests/test_bbm_native_cpu.py::test_the_odd_count_keeps_the_margins_of_the_reference_run)
@pytest.mark.parametrize("nsub", [G.DNSUB, ODD_NSUB])
def test_native_equals_the_python_sequence(python_run, nsub):
    want = python_run(nsub)
    got = one_block(nsub, True)
    assert float(want["u"].abs().max()) > 1e-4 and float((want["D"][0] - torch.from_numpy(G.driver_fields()["D"][0]).cuda()).abs().max()) > 1e-6
    assert_same(got, want, "native, nsub %d" % nsub)


# ---- 2. three row blocks equal one --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsub,overlap,ny", [(G.DNSUB, True, DNY), (ODD_NSUB, True, DNY), (ODD_NSUB, False, DNY), (ODD_NSUB, True, 9)])
def test_three_native_blocks_equal_one(python_run, nsub, overlap, ny):
    """6 owned rows with overlap: the split launches; without overlap, and with 3 owned rows whatever overlap says: the unsplit branch"""
    want = python_run(nsub) if ny == DNY else one_block(nsub, False, ny=ny)
    parts = native_world(3, nsub, overlap=overlap, ny=ny)
    assert_same({k: joined(parts, k) for k in KEYS}, want, (nsub, overlap, ny))
    # per step and block: nsub exchanges of the velocity and one of the damage
    assert all(parts[r]["stats"]["exchanges"] == DNSTEPS * (nsub + 1) for r in range(3)), [parts[r]["stats"] for r in range(3)]


def test_three_native_blocks_with_an_island_across_the_boundaries(built):
    land = island(DNY)
    want = one_block(ODD_NSUB, False, land=land)
    parts = native_world(3, ODD_NSUB, land=land)
    got = {k: joined(parts, k) for k in KEYS}
    assert_same(got, want, "land")
    tl = torch.from_numpy(land).cuda()
    for k in ("H", "D", "s11", "s12", "s22"):
        assert bool((got[k][:, tl] == 0).all()), k
    assert float(got["D"][0][~tl].max()) > 0.1 and bool(torch.isfinite(got["u"]).all())


def test_sub_steps_on_three_native_blocks(built):
    """advance(dt, substeps=2): every sub-step runs nsub sub-iterations of dt / (2 nsub)"""
    want = one_block(ODD_NSUB, False, nsteps=2, substeps=2)
    parts = native_world(3, ODD_NSUB, nsteps=2, substeps=2)
    assert_same({k: joined(parts, k) for k in KEYS}, want, "substeps")


# ---- 3. checkpoint ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_and_resume_agree_bit_for_bit(python_run):
    first = one_block(ODD_NSUB, True, nsteps=2)
    state = rowblock.DynamicsCore.merge_states([first["state"]])
    assert state["D"].shape == (6, DNY, DNX)
    again = one_block(ODD_NSUB, True, nsteps=1, resume=state)
    assert_same(again, python_run(ODD_NSUB), "resume")


# ---- 4. outputs ---------------------------------------------------------------------------------------------------------------------------
def drifter_points():
    """the wind converges on the centre, so below y = 9 km the ice moves up: drifters a micrometre below the block boundary at 6 km have their
    predictor in the ghost row above it; the others sit inside the blocks"""
    xs = np.linspace(1500.0, 22500.0, 8)
    near = np.stack([xs, np.full_like(xs, 6000.0 - 1e-6)], axis=1)
    inside = np.stack([xs, np.linspace(1000.0, 17000.0, 8)], axis=1)
    return np.concatenate([near, inside])


def test_history_and_drifters_on_three_native_blocks(built):
    kw = dict(history=("damage", "damage:max"), drifters=drifter_points(), drifter_min_conc=0.15)
    want = one_block(ODD_NSUB, False, **kw)
    parts = native_world(3, ODD_NSUB, **kw)
    assert_same({k: joined(parts, k) for k in KEYS}, want, "outputs")
    hist = rowblock.DynamicsCore.merge_history([parts[r]["history"] for r in range(3)])
    assert hist["count"] == want["history"]["count"] == DNSTEPS
    for k in ("damage", "damage:max"):
        assert np.array_equal(hist[k], want["history"][k]), k
    assert 0.0 <= hist["damage:max"].min() and hist["damage:max"].max() <= 1.0 and hist["damage:max"].max() > 0.1
    start = drifter_points()
    end = want["drifters"]
    assert np.all(end["status"] == abi.DRIFTER_ACTIVE)
    assert np.any(end["y"][:8] > 6000.0), "no drifter crossed the boundary at 6 km: the predictor in the ghost row above is not tested"
    assert np.abs(end["y"] - start[:, 1]).max() > 1e-6
    for r in range(3):
        for k in ("x", "y", "status"):
            assert np.array_equal(parts[r]["drifters"][k], end[k]), (r, k)
    # a native block with drifters ends its sub-cycle with one more exchange, of every ghost node row
    assert all(parts[r]["stats"]["exchanges"] == DNSTEPS * (ODD_NSUB + 2) for r in range(3))


def test_drifters_with_a_land_mask_on_three_native_blocks(built):
    """complete_nodes together with a land mask: the plan's last exchange carries velocities whose land nodes are held at 0, and the
    drifter that starts on the island is marked so on every block"""
    land = island(DNY)
    kw = dict(land=land, drifters=drifter_points(), drifter_min_conc=0.15)
    want = one_block(ODD_NSUB, False, **kw)
    parts = native_world(3, ODD_NSUB, **kw)
    assert_same({k: joined(parts, k) for k in KEYS}, want, "land and drifters")
    end = want["drifters"]
    assert (end["status"] == abi.DRIFTER_LAND).sum() >= 1 and (end["status"] == abi.DRIFTER_ACTIVE).sum() >= 8
    assert np.any(end["y"][:8] > 6000.0)
    for r in range(3):
        for k in ("x", "y", "status"):
            assert np.array_equal(parts[r]["drifters"][k], end[k]), (r, k)


# ---- 5. ABI errors ------------------------------------------------------------------------------------------------------------------------
class Plan:
    """the buffers of a plan on an 8 x 6 local array and nsdg_rb_bbm_create on a descriptor with members replaced"""

    def __init__(self, c, nx=8, ny=6):
        self.c, self.nx, self.ny = c, nx, ny
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
        self.S = [c.private_zeros(8, ny, nx, "cuda") for _ in range(6)]
        self.G = [c.private_zeros(9, ny, nx, "cuda") for _ in range(3)]
        self.D = [z(6, ny, nx) for _ in range(3)]
        self.uv = [z(2 * ny + 1, 2 * nx + 1) for _ in range(4)]
        self.packed = z(8 * self.uv[0].numel())

    def desc(self, **kw):
        d = abi.RbBbmDesc()
        d.nx, d.ny, d.j0, d.j1, d.depth_below, d.depth_above, d.rank_below, d.rank_above = self.nx, self.ny, 0, self.ny, 1, 1, -1, -1
        d.nsub, d.overlap = 3, 1
        for k in range(2):
            d.s11[k], d.s12[k], d.s22[k] = (self.S[3 * k + i].data_ptr() for i in range(3))
            d.u[k], d.v[k] = self.uv[2 * k].data_ptr(), self.uv[2 * k + 1].data_ptr()
            d.D[k] = self.D[k].data_ptr()
        d.D_work, d.packed = self.D[2].data_ptr(), self.packed.data_ptr()
        d.hg, d.eg, d.pm = (g.data_ptr() for g in self.G)
        for name, value in kw.items():
            if isinstance(value, tuple):
                getattr(d, name)[value[0]] = value[1]
            else:
                setattr(d, name, value)
        return d

    def create(self, **kw):
        h = abi.VP()
        rc = self.c.lib.nsdg_rb_bbm_create(self.c.h, abi.C.byref(self.desc(**kw)), abi.C.byref(h))
        assert (rc == 0) == bool(h.value)
        return rc, h


def test_abi_errors_are_statuses(built):
    c, other = abi.Context(torch.device("cuda:0")), abi.Context(torch.device("cuda:0"))
    lib = c.lib
    P = Plan(c)
    c.set_grid(P.nx, P.ny, HX, HY)
    err = lambda: lib.nsdg_last_error().decode()
    # the ghost depth: (2, 1) with a neighbour above (owned rows [0, 5) of 6)
    rc, _ = P.create(depth_below=2, rank_above=1, j1=P.ny - 1)
    assert rc == -1 and "(1, 1)" in err()
    # a null buffer, aliased halves, aliased damage buffers
    for kw in (dict(s12=(1, None)), dict(u=(0, None)), dict(D=(1, None)), dict(D_work=None), dict(packed=None), dict(pm=None)):
        assert P.create(**kw)[0] == -1, kw
    for kw in (dict(s11=(1, P.S[0].data_ptr())), dict(v=(1, P.uv[1].data_ptr())), dict(D=(1, P.D[0].data_ptr())), dict(D_work=P.D[1].data_ptr())):
        rc, _ = P.create(**kw)
        assert rc == -1 and "alias" in err(), kw
    assert P.create(nsub=-1)[0] == -1
    # neighbours without a communicator
    rc, _ = P.create(rank_above=1, j1=P.ny - 1)
    assert rc == -3 and "nsdg_comm_init" in err()
    # a good plan: run and stats refuse another context, a bad parity, a grid that does not match; nothing was launched before a packing
    rc, h = P.create()
    assert rc == 0
    out, st = abi.I32(-7), abi.HaloStats()
    assert lib.nsdg_rb_bbm_run(other.h, h, 0, 0, abi.C.byref(out)) == -1 and lib.nsdg_rb_bbm_stats(other.h, h, abi.C.byref(st), 0) == -1
    assert lib.nsdg_rb_bbm_run(c.h, h, 2, 0, abi.C.byref(out)) == -1 and lib.nsdg_rb_bbm_run(c.h, h, 0, -1, abi.C.byref(out)) == -1
    assert lib.nsdg_rb_bbm_run(c.h, h, 0, 0, None) == -1
    assert lib.nsdg_rb_bbm_run(c.h, h, 0, 0, abi.C.byref(out)) == -3  # NSDG_ERR_STATE: before any packing
    c.set_grid(P.nx, P.ny + 1, HX, HY)
    assert lib.nsdg_rb_bbm_run(c.h, h, 0, 0, abi.C.byref(out)) == -1 and "does not match" in err()
    c.set_grid(P.nx, P.ny, HX, HY)
    assert out.value == -7
    assert lib.nsdg_rb_bbm_stats(c.h, h, abi.C.byref(st), 0) == 0 and st.exchanges == 0
    assert lib.nsdg_rb_bbm_destroy(h) == 0 and lib.nsdg_rb_bbm_destroy(None) == 0
    # the driver: graphs are refused, and neighbours need the native exchanger
    with pytest.raises(ValueError, match="use_graph"):
        rowblock.DynamicsCore(c, rowblock.RowBlock(8, 6), HX, HY, DDT, 3, torch.device("cuda"), rheology="bbm", native=True, use_graph=True)
    with pytest.raises(ValueError, match="NativeHaloExchanger"):
        rowblock.DynamicsCore(c, rowblock.RowBlock(8, 12, 0, 2, 1, 1), HX, HY, DDT, 3, torch.device("cuda"), rheology="bbm", native=True)
    torch.cuda.synchronize()
    other.close()
    c.close()


# ---- 6. no sub-iterations -----------------------------------------------------------------------------------------------------------------
def test_zero_sub_iterations_write_nothing(built):
    c = abi.Context(torch.device("cuda:0"))
    P = Plan(c)
    c.set_grid(P.nx, P.ny, HX, HY)
    every = P.S + P.D + P.uv
    for k, t in enumerate(every):
        t.fill_(100.0 + k)  # guard values: the partners of either parity included
    rc, h = P.create(nsub=0, complete_nodes=1)
    assert rc == 0
    out = abi.I32(-7)
    for par in (0, 1):
        for dpar in (0, 1):
            assert c.lib.nsdg_rb_bbm_run(c.h, h, par, dpar, abi.C.byref(out)) == 0 and out.value == par
    torch.cuda.synchronize()
    for k, t in enumerate(every):
        assert bool((t == 100.0 + k).all()), k
    assert c.lib.nsdg_rb_bbm_destroy(h) == 0
    c.close()

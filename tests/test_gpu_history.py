"""History output on the device (csrc/history.hip; include/nsdg.h "history output"): nsdg_history_accumulate against
the numpy statement of the samples (tests/history_ref.py), its row ranges, guards and checks, and the Python driver's history=.

Shapes: nx = 63, 64, 65 sit around the seam of the 64-element stress tiles, 130 is three tiles with a remainder of two, 1 is the smallest
row; ny = 1 has no interior node row, 3 has one.  The copy fields and sigma_n must match bit for bit; speed, divergence, shear and sigma_s
within n_samples * 16 * 2^-53 * scale (history_ref.rounding_scale: under ten roundings per sample, FMA contraction either way)."""
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

import history_ref as R  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
HX, HY = 1300.0, 700.0
NSAMPLES = 3
ALL = R.FIELDS
PERMUTED = ("sigma_s", "v", "damage", "divergence", "hice", "tice", "speed")
I32 = abi.I32


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def random_state(nx, ny, rng):
    """one state of random fields, every coefficient and every node filled: an index that strays reads a different number"""
    st = {k: rng.standard_normal((6, ny, nx)) for k in ("H", "A", "D")}
    st.update({k: 0.3 * rng.standard_normal((2 * ny + 1, 2 * nx + 1)) for k in ("u", "v")})
    st.update({k: 1e4 * rng.standard_normal((8, ny, nx)) for k in ("s11", "s12", "s22")})
    st.update({k: rng.standard_normal((ny, nx)) for k in ("hsnow", "tice")})
    return st


def to_device(st):
    return {k: (abi.tile(dev(a)) if k in ("s11", "s12", "s22") else dev(a)) for k, a in st.items()}


_cases = {}


def case(nx, ny):
    """NSAMPLES random states of an nx x ny array, the reference samples of all fields [NSAMPLES, 12, ny, nx] and the scale of every
    rounded field -- computed once per shape and left unchanged"""
    if (nx, ny) not in _cases:
        rng = np.random.default_rng(1000 * nx + ny)
        states = [random_state(nx, ny, rng) for _ in range(NSAMPLES)]
        ref = np.stack([R.samples(ALL, HX, HY, **st) for st in states])
        scale = {n: max(R.rounding_scale(n, HX, HY, **{k: st[k] for k in ("u", "v", "s11", "s12", "s22")}) for st in states)
                 for n in ALL if n not in R.EXACT_FIELDS}
        ref.setflags(write=False)
        _cases[(nx, ny)] = (states, ref, scale)
    return _cases[(nx, ny)]


def reference_sum(ref, fields):
    acc = np.full((len(fields),) + ref.shape[2:], np.nan)
    idx = [ALL.index(n) for n in fields]
    for k in range(ref.shape[0]):
        R.accumulate(acc, ref[k][idx], 0, ref.shape[2], k == 0)
    return acc


def compare(got, want, fields, scale, nsamples, what):
    for k, name in enumerate(fields):
        if name in R.EXACT_FIELDS:
            assert np.array_equal(got[k], want[k]), (what, name, float(np.max(np.abs(got[k] - want[k]))))
        else:
            bound = nsamples * 16 * R.EPS * scale[name]
            err = float(np.max(np.abs(got[k] - want[k])))
            print("%s %-10s largest error %.3e, bound %.3e (%.3f of it)" % (what, name, err, bound, err / bound))
            assert err <= bound, (what, name, err, bound)


def device_sum(ctx, nx, ny, states, fields, ranges=None, acc=None, row0=0):
    ctx.set_grid(nx, ny, HX, HY)
    if acc is None:
        acc = torch.full((len(fields), ny - row0, nx), float("nan"), dtype=torch.float64, device="cuda")  # the first sample stores
    for k, st in enumerate(states):
        d = to_device(st)
        for (j0, j1) in ranges or [(0, ny)]:
            ctx.history_accumulate(j0, j1, fields, d, k == 0, row0, acc)
    torch.cuda.synchronize()
    return acc


# ------------------------------------------------------------------------------------------------ a. the kernel against the reference
@pytest.mark.parametrize("ny", [1, 3])
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130])
def test_three_accumulated_samples_match_the_reference(ctx, nx, ny):
    states, ref, scale = case(nx, ny)
    for fields in (ALL, PERMUTED, ("shear",)):
        got = device_sum(ctx, nx, ny, states, fields).cpu().numpy()
        compare(got, reference_sum(ref, fields), fields, scale, NSAMPLES, "%dx%d %d fields:" % (nx, ny, len(fields)))


def test_every_field_alone_reads_only_its_own_sources(ctx):
    """one field per call with every source it does not read left NULL: the library asks for no more than the header says"""
    nx, ny = 65, 3
    states, ref, scale = case(nx, ny)
    needs = {"hice": "H", "cice": "A", "u": "u", "v": "v", "speed": "u v", "divergence": "u v", "shear": "u v", "sigma_n": "s11 s22",
             "sigma_s": "s11 s12 s22", "hsnow": "hsnow", "tice": "tice", "damage": "D"}
    for name in ALL:
        only = [{k: a for k, a in st.items() if k in needs[name].split()} for st in states]
        got = device_sum(ctx, nx, ny, only, (name,)).cpu().numpy()
        compare(got, reference_sum(ref, (name,)), (name,), scale, NSAMPLES, "alone:")


# ------------------------------------------------------------------------------------------------ b. row ranges and guards
def test_a_row_range_between_nan_neighbours_writes_nothing_else(ctx):
    nx, ny = 65, 3
    states, ref, scale = case(nx, ny)
    fields = ALL
    idx = list(range(len(ALL)))
    d = to_device(states[0])
    ctx.set_grid(nx, ny, HX, HY)
    # planes of all three rows: the rows beside [1, 2) stay NaN
    acc = torch.full((len(fields), ny, nx), float("nan"), dtype=torch.float64, device="cuda")
    ctx.history_accumulate(1, 2, fields, d, True, 0, acc)
    got = acc.cpu().numpy()
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isnan(got[:, 2]))
    compare(got[:, 1:2], ref[0][idx][:, 1:2], fields, scale, 1, "row 1 stored:")  # store = 1 cleared the NaN
    ctx.history_accumulate(0, 1, fields, d, False, 0, acc)  # store = 0 keeps a NaN
    assert bool(torch.isnan(acc[:, 0]).all())
    # planes of ONE row (row0 = 1) between guards of NaN
    guard = 4 * nx
    buf = torch.full((2 * guard + len(fields) * nx,), float("nan"), dtype=torch.float64, device="cuda")
    own = buf[guard:guard + len(fields) * nx].view(len(fields), 1, nx)
    ctx.history_accumulate(1, 2, fields, d, True, 1, own)
    ctx.history_accumulate(1, 2, fields, d, False, 1, own)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[-guard:]).all())
    twice = ref[0][idx][:, 1:2] + ref[0][idx][:, 1:2]
    compare(own.cpu().numpy(), twice, fields, scale, 2, "row 1 of its own plane, twice:")
    assert bool(torch.equal(own[ALL.index("hice"), 0], 2 * d["H"][0, 1]))


def test_two_row_ranges_equal_one_call_bitwise(ctx):
    nx, ny = 130, 3
    states, _, _ = case(nx, ny)
    one = device_sum(ctx, nx, ny, states, ALL)
    two = device_sum(ctx, nx, ny, states, ALL, ranges=[(0, 1), (1, 3)])
    assert not bool(torch.isnan(one).any()) and torch.equal(one, two)


def test_the_call_checks_its_arguments(gpu):
    c = abi.Context(gpu)
    lib, nx, ny = c.lib, 8, 4
    st = to_device(random_state(nx, ny, np.random.default_rng(1)))
    acc = torch.full((2, ny, nx), 7.0, dtype=torch.float64, device="cuda")
    ids = lambda *a: (I32 * len(a))(*a)
    src = lambda **drop: abi.HistorySources(*[None if n in drop else st[n].data_ptr() for n in abi.HISTORY_SOURCES])
    call = lambda j0, j1, n, f, s, store, row0, stride: lib.nsdg_history_accumulate(c.h, j0, j1, n, f, abi.C.byref(s), store, row0, stride,
                                                                                     acc.data_ptr())
    assert call(0, ny, 1, ids(0), src(), 1, 0, nx * ny) == -3 and b"nsdg_grid_set" in lib.nsdg_last_error()  # NSDG_ERR_STATE
    c.set_grid(nx, ny, HX, HY)
    for j0, j1 in ((-1, 2), (3, 2), (0, ny + 1)):
        assert call(j0, j1, 1, ids(0), src(), 1, 0, nx * ny) == -1, (j0, j1)
    assert call(0, ny, 0, ids(0), src(), 1, 0, nx * ny) == -1 and call(0, ny, 17, ids(*range(12), 0, 0, 0, 0, 0), src(), 1, 0, nx * ny) == -1
    assert call(0, ny, 1, ids(12), src(), 1, 0, nx * ny) == -1 and b"unknown field id 12" in lib.nsdg_last_error()
    assert call(0, ny, 1, ids(-1), src(), 1, 0, nx * ny) == -1
    assert call(0, ny, 2, ids(3, 3), src(), 1, 0, nx * ny) == -1 and b"'v' is listed twice" in lib.nsdg_last_error()
    assert call(0, ny, 2, ids(0, 11), src(D=1), 1, 0, nx * ny) == -1 and b"'damage'" in lib.nsdg_last_error()
    assert call(0, ny, 1, ids(8), src(s12=1), 1, 0, nx * ny) == -1 and b"'sigma_s'" in lib.nsdg_last_error() and b"s12" in lib.nsdg_last_error()
    assert call(0, ny, 1, ids(7), src(s12=1, D=1, hsnow=1, tice=1, H=1, A=1, u=1, v=1), 1, 0, nx * ny) == 0  # sigma_n reads s11 and s22 only
    assert call(1, ny, 1, ids(0), src(), 1, 2, nx * ny) == -1 and b"row0" in lib.nsdg_last_error()
    assert call(1, ny, 1, ids(0), src(), 1, -1, nx * ny) == -1
    assert call(0, ny, 1, ids(0), src(), 1, 0, nx * ny - 1) == -1 and b"plane_stride" in lib.nsdg_last_error()
    assert call(1, ny, 1, ids(0), src(), 1, 1, nx * (ny - 1)) == 0
    assert lib.nsdg_history_accumulate(c.h, 0, ny, 1, None, abi.C.byref(src()), 1, 0, nx * ny, acc.data_ptr()) == -1
    assert lib.nsdg_history_accumulate(c.h, 0, ny, 1, ids(0), None, 1, 0, nx * ny, acc.data_ptr()) == -1
    assert lib.nsdg_history_accumulate(c.h, 0, ny, 1, ids(0), abi.C.byref(src()), 1, 0, nx * ny, None) == -1
    acc.fill_(7.0)
    assert call(2, 2, 1, ids(0), src(), 1, 0, nx * ny) == 0  # an empty range is no error and does nothing
    torch.cuda.synchronize()
    assert bool((acc == 7.0).all())
    with pytest.raises(abi.NsdgError, match="unknown history field"):
        c.history_accumulate(0, ny, ("thickness",), st, True, 0, acc[:1])
    with pytest.raises(abi.NsdgError, match="acc has shape"):
        c.history_accumulate(0, ny, ("hice",), st, True, 0, acc)
    with pytest.raises(abi.NsdgError, match="source u has"):
        c.history_accumulate(0, ny, ("u",), dict(st, u=st["u"][:-1]), True, 0, acc[:1])
    c.close()


# ------------------------------------------------------------------------------------------------ c. the driver
DNX, DNY, DNSUB, DSTEPS = 70, 9, 12, 3
DYN = ("hice", "cice", "u", "v", "speed", "divergence", "shear", "sigma_n", "sigma_s")


def rock():
    land = np.zeros((DNY, DNX), dtype=bool)
    land[4, 30] = True  # one land element, on the row where three blocks of three rows have their middle
    land[2:4, 64] = True  # and two across the boundary of the first two blocks, on the tile seam
    return land


def driver_data():
    from thread_ranks import fields

    return fields(DNX, DNY)


def make_core(c, history, rank=0, world=1, exchanger=None, variant=1, cls=rowblock.DynamicsCore, **kw):
    c.set_mevp_variant(variant)
    c.set_mevp_params(c.mevp_default_params(alpha=300.0, beta=300.0))
    bt, H, A, uo, vo, ua, va = driver_data()
    blk = rowblock.RowBlock(DNX, DNY, rank, world, 1, 1)
    core = cls(c, blk, bt.hx, bt.hy, 120.0, DNSUB, torch.device("cuda"), exchanger=exchanger, land=rock(), history=history, **kw)
    core.load_global(H, A, uo, vo, ua, va)
    return core, bt


def reference_of_states(states, fields, hx, hy):
    acc = np.full((len(fields), DNY, DNX), np.nan)
    scale = {}
    for k, st in enumerate(states):
        R.accumulate(acc, R.samples(fields, hx, hy, **st), 0, DNY, k == 0)
        for n in fields:
            if n not in R.EXACT_FIELDS:
                scale[n] = max(scale.get(n, 0.0), R.rounding_scale(n, hx, hy, **{q: st.get(q) for q in ("u", "v", "s11", "s12", "s22")}))
    return acc / len(states), scale


@pytest.fixture(scope="module")
def one_block(ctx):
    """the one-block run the driver tests share: the record of DSTEPS steps and the device's own per-step state_dict() downloads"""
    core, bt = make_core(ctx, DYN)
    states = []
    for _ in range(DSTEPS):
        core.step()
        st = core.state_dict()
        states.append({k: st[k] for k in ("H", "A", "u", "v", "s11", "s12", "s22")})
    rec = core.history_read()
    core.close()
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())
    return rec, states, bt


def test_driver_means_equal_the_reference_of_its_own_states(one_block):
    rec, states, bt = one_block
    assert rec["count"] == DSTEPS and rec["rows"] == (0, DNY)
    want, scale = reference_of_states(states, DYN, bt.hx, bt.hy)
    assert np.max(np.abs(rec["speed"])) > 1e-4 and np.max(np.abs(rec["sigma_s"])) > 0 and np.max(np.abs(rec["shear"])) > 0
    land = rock()
    assert np.all(rec["hice"][land] == 0) and np.all(rec["speed"][land] == 0)
    # the mean is acc / n: the bound of the sum, divided by n
    compare(np.stack([rec[n] for n in DYN]), want, DYN, {n: s / DSTEPS for n, s in scale.items()}, DSTEPS, "driver:")


def thread_world(world, history):
    from thread_ranks import Mailbox, ThreadExchanger

    mailbox, out = Mailbox(), {}

    def rank_main(rank):
        try:
            c = abi.Context(torch.device("cuda:0"))
            blk = rowblock.RowBlock(DNX, DNY, rank, world, 1, 1)
            core, _ = make_core(c, history, rank, world, ThreadExchanger(blk, mailbox))
            for _ in range(DSTEPS):
                core.step()
            out[rank] = core.history_read()
            core.close()
            c.close()
        except BaseException as e:  # noqa: BLE001 -- wake the peers up, then re-raise in the main thread
            with mailbox.cv:
                mailbox.error = e
                mailbox.cv.notify_all()
            out[rank] = e

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return [out[r] for r in range(world)]


def test_one_block_equals_three_blocks_bitwise(one_block):
    rec = one_block[0]
    parts = thread_world(3, DYN)
    assert [p["rows"] for p in parts] == [(0, 3), (3, 6), (6, 9)]
    got = rowblock.DynamicsCore.merge_history(parts)
    assert got["count"] == DSTEPS and got["rows"] == (0, DNY)
    for n in DYN:
        assert np.array_equal(got[n], rec[n]), n


def test_graphs_equal_no_graphs_and_passes_of_four_equal_single_sub_iterations(gpu, one_block):
    """the native plan (one C call per sub-cycle, passes of four sub-iterations) with and without hipGraph replay: the sample is taken
    outside every captured graph, from the ping-pong side the plan left the result on"""
    rec = one_block[0]
    for use_graph in (False, True):
        c = abi.Context(gpu)
        core, _ = make_core(c, DYN, variant=4, native=True, use_graph=use_graph)
        assert core.per_pass == 4
        for _ in range(DSTEPS):
            core.step()
        got = core.history_read()
        core.close()
        c.close()
        for n in DYN:
            assert np.array_equal(got[n], rec[n]), (n, use_graph)


def test_advance_samples_once_and_windows_reset(ctx):
    core, _ = make_core(ctx, ("hice", "speed", "sigma_n"))
    core._history.acc.fill_(float("nan"))
    assert core.advance(120.0, substeps=2) == 2
    rec = core.history_read()
    assert rec["count"] == 1 and np.array_equal(rec["hice"], core.H[0].cpu().numpy())
    assert np.array_equal(rec["sigma_n"], 0.5 * (abi.untile(core.s[0], DNX)[0] + abi.untile(core.s[2], DNX)[0]).cpu().numpy())
    core.step()
    core.step()
    assert core.history_read(reset=False)["count"] == 2 and core.history_read()["count"] == 2
    with pytest.raises(ValueError, match="no sample"):
        core.history_read()
    core.close()
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


def test_coupled_core_samples_the_snow_plane_it_uses(ctx):
    """advect_column_state: the column's hsnow IS plane 0 of the advected snow field S, whose buffer changes with every transport step"""
    ctx.set_column_params(ctx.column_default_params())
    fields = ("hsnow", "tice", "hice")
    core, _ = make_core(ctx, fields, cls=rowblock.CoupledCore, advect_column_state=True)
    st, fo, _ = synthetic.column_fields(DNX * DNY, 5)
    column = {k: v.reshape(DNY, DNX) for k, v in {**st, **fo}.items()}
    column["wind"] = 0.2 * column["wind"]
    core.load_column(column)
    acc = np.full((3, DNY, DNX), np.nan)
    for k in range(2):
        core.step()
        x = np.stack([core.col["hsnow"].cpu().numpy(), core.col["tice0"].cpu().numpy(), core.H[0].cpu().numpy()])
        assert core.col["hsnow"].data_ptr() == core.S.data_ptr()
        R.accumulate(acc, x, 0, DNY, k == 0)
    rec = core.history_read()
    assert rec["count"] == 2 and np.max(np.abs(rec["hsnow"])) > 0
    for k, n in enumerate(fields):
        assert np.array_equal(rec[n], acc[k] / 2), n
    core.close()
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_params(ctx.mevp_default_params())


def test_brittle_rheology_with_damage(ctx):
    import test_gpu_bbm as B

    ctx.set_mevp_params(ctx.mevp_default_params())
    ctx.set_bbm_params(ctx.bbm_default_params())
    fields = ("damage", "sigma_n", "sigma_s", "hice", "speed")
    f = B.driver_fields()
    core = rowblock.DynamicsCore(ctx, rowblock.RowBlock(B.DNX, B.DNY), B.HX, B.HY, B.DDT, B.DNSUB, torch.device("cuda"), rheology="bbm",
                                 history=fields)
    core.load_global(f["H"], f["A"], f["uo"], f["vo"], f["ua"], f["va"])
    core.load_state_dict(B.start_state(f))
    acc, scale = np.full((len(fields), B.DNY, B.DNX), np.nan), {}
    for k in range(2):
        core.step()
        st = core.state_dict()
        R.accumulate(acc, R.samples(fields, B.HX, B.HY, **{q: st[q] for q in ("H", "D", "u", "v", "s11", "s12", "s22")}), 0, B.DNY, k == 0)
        for n in ("sigma_s", "speed"):
            scale[n] = max(scale.get(n, 0.0), R.rounding_scale(n, B.HX, B.HY, **{q: st[q] for q in ("u", "v", "s11", "s12", "s22")}) / 2)
    rec = core.history_read()
    core.close()
    assert rec["count"] == 2 and 0.0 < rec["damage"].min() and rec["damage"].max() < 1.0 and np.max(np.abs(rec["sigma_s"])) > 1e3  # Pa
    compare(np.stack([rec[n] for n in fields]), acc / 2, fields, scale, 2, "bbm:")
    with pytest.raises(ValueError, match="'damage' needs rheology='bbm'"):
        rowblock.DynamicsCore(ctx, rowblock.RowBlock(B.DNX, B.DNY), B.HX, B.HY, B.DDT, B.DNSUB, torch.device("cuda"), history=("damage",))

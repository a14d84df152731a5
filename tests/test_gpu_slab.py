"""The slab ocean on the device (include/nsdg_ocean.h): nsdg_column_step_ocean against nsdg_column_step (the ice,
bit for bit) and against the numpy restatement tests/slab_ref.py fed with the device's own diagnostic planes (sst and sss, bit for bit)
on both launch routes; its refusals; CoupledCore(slab_ocean=True) on a 64 x 48 box with a land strip and a shoal -- 1 block = 4 blocks,
graphs = no graphs, native = the Python sequence, restart = uninterrupted --; and the warm-water twin runs of tests/test_slab_cpu.py."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import basal_ref as BR
import slab_ref as R
import test_slab_cpu as TC
from nextsimdg_amd import abi, rowblock, synthetic
from thread_ranks import fields

pytestmark = pytest.mark.gpu
SENTINEL, GUARD = -7.0, 16
PLANES = abi.STATE + abi.FORCING + ["newice"]
READ_ONLY = [k for k in abi.FORCING if k not in ("sst", "sss")]


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults_after_each_test(ctx):
    yield
    ctx.set_slab_params(ctx.slab_default_params())
    ctx.set_column_params(ctx.column_default_params())
    ctx.set_mevp_params(ctx.mevp_default_params())


def placed(a, off):
    """the plane in a sentinel-filled buffer of its own, `off` doubles (bytes for a mask) from a 16-byte boundary: (buffer, view)"""
    buf = torch.full((a.size + 2 * GUARD + off,), SENTINEL if a.dtype == np.float64 else 7, dtype=torch.from_numpy(a).dtype, device="cuda")
    view = buf[GUARD + off:GUARD + off + a.size]
    assert view.data_ptr() % 16 == (off * a.itemsize) % 16
    view.copy_(torch.from_numpy(a))
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    fill = SENTINEL if buf.dtype == torch.float64 else 7
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + view.numel():] == fill).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- 1. bit equality
CASES = [(n, off, relax, skip) for n in (1, 2, 513, 50001) for off, relax, skip in ((0, False, False), (0, True, True), (1, True, True), (1, False, False))]


@pytest.mark.parametrize("n,off,relax,skip", CASES)
def test_ice_equals_the_plain_column_step_and_the_ocean_equals_the_restatement(ctx, n, off, relax, skip):
    """10 steps of 600 s on synthetic.column_fields(n); off = 1 breaks the 16-byte alignment of every plane (the scalar twin runs), n odd
    leaves a tail element, 50 001 is more than one workgroup of either kernel"""
    state, forcing, newice = synthetic.column_fields(n)
    rng = np.random.default_rng(n + off)
    ext = {"sst": rng.uniform(-1.8, 3.0, n), "sss": rng.uniform(30.0, 35.0, n)}
    mask = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    par = R.SlabParams(relax_t=5 * 86400.0, relax_s=30 * 86400.0, ice_salinity=4.0) if relax else R.SlabParams()
    ctx.set_slab_params(ctx.slab_default_params(relax_t=par.relax_t, relax_s=par.relax_s, ice_salinity=par.ice_salinity))
    dq = ctx.column_default_params().drag_ocean_q
    host = {**state, **forcing, "newice": newice}
    bufs = {k: placed(host[k], off) for k in PLANES}
    w = {k: v for k, (_, v) in bufs.items()}
    ebufs = {k: placed(ext[k], off) for k in ext} if relax else {}
    mbuf = placed(mask, off) if skip else None
    diag = torch.empty(abi.NDIAG * n, dtype=torch.float64, device="cuda")
    worst = 0
    for step in range(10):
        before = {k: w[k].cpu().numpy() for k in PLANES}
        p = {k: w[k].clone() for k in PLANES}  # the plain call on copies of the same inputs
        ctx.column_step(600.0, {k: p[k] for k in abi.STATE}, {k: p[k] for k in abi.FORCING}, p["newice"], diag)
        ctx.column_step_ocean(600.0, {k: w[k] for k in abi.STATE}, {k: w[k] for k in abi.FORCING}, w["newice"],
                              {k: v for k, (_, v) in ebufs.items()}, mbuf[1] if skip else None)
        torch.cuda.synchronize()
        for k in abi.STATE + ["newice"]:
            assert torch.equal(w[k].view(torch.int64), p[k].view(torch.int64)), (step, k)
        d = dict(zip(abi.DIAG, diag.view(abi.NDIAG, n).cpu().numpy()))
        after = {k: p[k].cpu().numpy() for k in ("hice", "hsnow")}
        T1, S1 = R.update(600.0, before, after, d, par, dq, ext, mask if skip else None)
        got_t, got_s = w["sst"].cpu().numpy(), w["sss"].cpu().numpy()
        with np.errstate(all="ignore"):
            worst = max(worst, int(np.nanmax(np.abs(got_s - S1) / np.spacing(np.abs(before["sss"])))))
        assert np.array_equal(bits(got_t), bits(T1)), (step, "sst", int((bits(got_t) != bits(T1)).sum()))
        assert np.array_equal(bits(got_s), bits(S1)), (step, "sss", int((bits(got_s) != bits(S1)).sum()), worst)
        if skip:
            keep = mask != 0
            assert np.array_equal(bits(got_t[keep]), bits(before["sst"][keep])) and np.array_equal(bits(got_s[keep]), bits(before["sss"][keep]))
        for k in READ_ONLY:
            assert np.array_equal(bits(w[k].cpu().numpy()), bits(host[k])), (step, k)
    free = mask == 0 if skip else np.ones(n, dtype=bool)
    assert free.any() or n == 1  # (the one element of n = 1 may be a skipped one)
    assert not free.any() or (np.any(got_t[free] != forcing["sst"][free]) and np.any(got_s[free] != forcing["sss"][free]))
    for k, (buf, view) in list(bufs.items()) + list(ebufs.items()) + ([("skip", mbuf)] if skip else []):
        assert guards_intact(buf, view), k
    for k, (_, view) in ebufs.items():
        assert np.array_equal(bits(view.cpu().numpy()), bits(ext[k])), k
    if skip:
        assert np.array_equal(mbuf[1].cpu().numpy(), mask)


# ---------------------------------------------------------------------------------------------------------------- 2. argument errors
def test_argument_errors_launch_nothing(ctx):
    n = 64
    lib, h = ctx.lib, ctx.h
    pool = torch.full((24 * n,), SENTINEL, dtype=torch.float64, device="cuda")
    base = pool.data_ptr()
    at = lambda k, shift=0: base + 8 * (k * n + shift)  # plane k of the pool, `shift` doubles on
    good = [at(k) for k in range(15)]
    ext_t, ext_s, mask = at(16), at(17), at(18)

    def call(planes, et=None, es=None, sk=None, count=n):
        return lib.nsdg_column_step_ocean(h, count, 600.0, *[C.c_void_p(p) if p else None for p in planes], C.c_void_p(et) if et else None,
                                          C.c_void_p(es) if es else None, C.c_void_p(sk) if sk else None)

    ERR_ARG = -1
    assert call(good, count=-1) == ERR_ARG
    assert call(good, count=0) == 0  # nothing to do, and nothing looked at
    assert call([None] * 15, count=0) == 0
    for k in range(15):  # a null state or forcing pointer
        assert call(good[:k] + [None] + good[k + 1:]) == ERR_ARG, PLANES[k]
    assert lib.nsdg_column_step_ocean(None, n, 600.0, *[C.c_void_p(p) for p in good], None, None, None) == ERR_ARG
    # sst (plane 4) or sss (5) overlapping each other or any other plane: the same pointer, and one double shared at either end
    for k in (4, 5):
        for j in range(15):
            if j == k:
                continue
            for shift in (0, n - 1, 1 - n):
                planes = list(good)
                planes[j] = at(k, shift)
                assert call(planes) == ERR_ARG, (PLANES[k], PLANES[j], shift)
        planes = list(good)
        assert call(planes, sk=at(k) + 8 * n - 1) == ERR_ARG  # the mask's first byte is the plane's last
        assert call(planes, sk=at(k) - n + 1) == ERR_ARG  # the mask's last byte is the plane's first
    # a mask, and targets without their relaxation, may be NULL or anywhere; a target that is not read may even overlap
    ctx.set_slab_params(ctx.slab_default_params(relax_t=1e5))
    assert call(good, None, ext_s, mask) == ERR_ARG  # a null target while its relaxation is on
    assert call(good, at(4, 3), None, mask) == ERR_ARG and call(good, at(5, n - 1), None, mask) == ERR_ARG
    ctx.set_slab_params(ctx.slab_default_params(relax_s=1e5))
    assert call(good, ext_t, None, mask) == ERR_ARG
    assert call(good, None, at(5, 1 - n), mask) == ERR_ARG
    assert b"nsdg_column_step_ocean" in lib.nsdg_last_error()
    # the parameters: a negative or non-finite member, a null argument
    good_p = ctx.slab_default_params(relax_t=3.0, relax_s=4.0, ice_salinity=6.0)
    ctx.set_slab_params(good_p)
    for bad in (dict(relax_t=-1.0), dict(relax_s=-1.0), dict(ice_salinity=-1.0), dict(relax_t=float("inf")), dict(relax_s=float("nan")),
                dict(ice_salinity=float("inf"))):
        assert lib.nsdg_slab_params_set(h, C.byref(abi.slab_default_params(**bad))) == ERR_ARG, bad
    assert lib.nsdg_slab_params_set(h, None) == ERR_ARG and lib.nsdg_slab_params_set(None, C.byref(good_p)) == ERR_ARG
    with pytest.raises(abi.NsdgError, match="unknown slab-ocean parameter"):
        ctx.slab_default_params(relax=1.0)
    # nothing changed: a call that needs BOTH targets still refuses a null one of either, and nothing was launched
    assert call(good, None, ext_s, mask) == ERR_ARG and call(good, ext_t, None, mask) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((pool == SENTINEL).all())
    # the binding refuses what the ABI cannot see: a short plane, a mask of the wrong type
    st, fo, ni = synthetic.column_fields(8)
    dv = lambda a: torch.from_numpy(a).cuda()
    s, f, m = {k: dv(v) for k, v in st.items()}, {k: dv(v) for k, v in fo.items()}, dv(ni)
    with pytest.raises(abi.NsdgError, match="skip must be"):
        ctx.column_step_ocean(600.0, s, f, m, None, torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(abi.NsdgError, match="sst_ext has 4 elements"):
        ctx.column_step_ocean(600.0, s, f, m, {"sst": torch.zeros(4, dtype=torch.float64, device="cuda")}, None)


# ---------------------------------------------------------------------------------------------------------------- 3. the driver
NX, NY, DT, NSUB, STEPS = 64, 48, 120.0, 16, 6
_groups = [61000]


def box():
    """the 64 x 48 box: thread_ranks.fields under the thick cover of the shoal case, a land strip across the block boundaries (rows 12, 24,
    36) with a rock on a boundary row, a shoal beside it, a lead, and a mixed layer half a kelvin above freezing that relaxes to sst + 1"""
    bt, H, A, uo, vo, ua, va = fields(NX, NY)
    BR.thick_cover(H, A)
    A[0, 30:34, 40:50] = 0.0
    H[0, 30:34, 40:50] = 0.0
    land = np.zeros((NY, NX), dtype=bool)
    land[8:40, 20:23] = True
    land[24, 5] = True
    depth, _ = BR.shoal_depth(NX, NY, box=(10, 38, 28, 40))
    cs, cf = synthetic.column_fields_smooth(NX, NY)
    col = {**cs, **cf}
    col["sst"] = col["sst"] + 0.5
    col["sst_ext"] = col["sst"] + 1.0
    return (bt, H, A, uo, vo, ua, va), land, depth, col


def slab_rank(rank, world, native, graph, steps, resume, out, group, slab_ocean=True):
    try:
        (bt, H, A, uo, vo, ua, va), land, depth, col = box()
        c = abi.Context(torch.device("cuda:0"))
        c.set_mevp_variant(4)
        c.set_mevp_params(c.mevp_default_params(**bt.subcycle_parameters(DT)))
        blk = rowblock.RowBlock(NX, NY, rank, world, 4, 3)
        ex = rowblock.NativeHaloExchanger(c, blk, local_group=group) if world > 1 else None
        kw = dict(slab_ocean=True, slab=c.slab_default_params(relax_t=50 * DT)) if slab_ocean else {}
        core = rowblock.CoupledCore(c, blk, bt.hx, bt.hy, DT, NSUB, torch.device("cuda"), exchanger=ex, native=native, use_graph=graph, land=land,
                                    bathymetry=depth, **kw)
        core.load_global(H, A, uo, vo, ua, va)
        if not slab_ocean:
            col.pop("sst_ext")
        core.load_column(col)
        if resume is not None:
            core.load_state_dict(resume)
            es = blk.elem_slice()
            for k in ("hsnow", "tice0"):
                core.col[k].copy_(torch.from_numpy(np.ascontiguousarray(resume[k][es])))
            core.newice.copy_(torch.from_numpy(np.ascontiguousarray(resume["newice"][es])))
        for _ in range(steps):
            core.step()
        torch.cuda.synchronize()
        res = {k: core.owned(getattr(core, k)).clone() for k in ("H", "A", "u", "v")}
        for k in ("sst", "sss", "hsnow", "tice0"):
            res[k] = core.col[k][blk.j0:blk.j1].clone()
        res["newice"] = core.newice[blk.j0:blk.j1].clone()
        res["state"] = core.state_dict()
        res["ghosts"] = {k: core.col[k].clone() for k in ("sst", "sss")}
        res["rows"] = blk.elem_slice()
        out[rank] = res
    except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread
        out[rank] = e


def slab_world(world, native=True, graph=False, steps=STEPS, resume=None, **kw):
    out = {}
    _groups[0] += 1
    threads = [threading.Thread(target=slab_rank, args=(r, world, native, graph, steps, resume, out, _groups[0]), kwargs=kw) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return out


KEYS = ("H", "A", "sst", "sss", "u", "v", "hsnow", "tice0")


def gathered(parts, world, key):
    return torch.cat([parts[r][key] for r in range(world)], dim=1 if key in ("H", "A") else 0)


@pytest.fixture(scope="module")
def one_block(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    return slab_world(1)[0]


def test_the_ocean_evolves_and_keeps_its_bits_on_land(one_block):
    _, land, _, col = box()
    sst, sss = one_block["sst"].cpu().numpy(), one_block["sss"].cpu().numpy()
    assert np.array_equal(bits(sst[land]), bits(col["sst"][land])) and np.array_equal(bits(sss[land]), bits(col["sss"][land]))
    assert np.all(sst[~land] != col["sst"][~land]) and np.any(sss[~land] != col["sss"][~land])
    assert np.all(np.isfinite(sst)) and np.all(np.isfinite(sss)) and float(one_block["u"].abs().max()) > 1e-5
    # under the cover the half kelvin is gone after the first step; what is left is the relaxation towards sst + 1.5 K
    ice = (one_block["A"][0].cpu().numpy() > 0.5) & ~land
    assert float(np.max(np.abs(sst[ice] + R.MU * sss[ice]))) < 0.25
    # and the run is another run than the one without the mode
    plain = slab_world(1, slab_ocean=False)[0]
    assert np.array_equal(bits(plain["sst"].cpu().numpy()), bits(col["sst"])) and not torch.equal(plain["H"], one_block["H"])


@pytest.mark.parametrize("world,graph", [(4, False), (1, True), (4, True)])
def test_one_block_equals_four_blocks_and_graphs_equal_no_graphs(one_block, world, graph):
    parts = slab_world(world, graph=graph)
    for key in KEYS:
        assert torch.equal(gathered(parts, world, key), one_block[key]), (key, world, graph)
    merged = rowblock.DynamicsCore.merge_states([parts[r]["state"] for r in range(world)])
    for r in range(world):  # the ghost rows equal their owners without a message
        for k in ("sst", "sss"):
            assert np.array_equal(bits(parts[r]["ghosts"][k].cpu().numpy()), bits(merged[k][parts[r]["rows"]])), (r, k)


def test_native_equals_the_python_sequence(one_block):
    python = slab_world(1, native=False)[0]
    for key in KEYS:
        assert torch.equal(python[key], one_block[key]), key


def test_restart_in_the_middle_equals_the_uninterrupted_run(one_block):
    half = slab_world(1, steps=STEPS // 2)[0]
    state = rowblock.DynamicsCore.merge_states([half["state"]])
    assert np.array_equal(bits(state["sst"]), bits(half["sst"].cpu().numpy()))
    for k in ("hsnow", "tice0", "newice"):
        state[k] = half[k].cpu().numpy()
    rest = slab_world(1, steps=STEPS - STEPS // 2, resume=state)[0]
    for key in KEYS:
        assert torch.equal(rest[key], one_block[key]), key


# ---------------------------------------------------------------------------------------------------------------- 4. warm-water twins
def test_a_warm_mixed_layer_is_a_finite_heat_source_on_the_device(ctx):
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def differences(fused):
        runs = []
        for excess in (1.0, 0.0):
            st, fo, ni = TC.twin_fields(excess)
            runs.append(({k: dv(v) for k, v in st.items()}, {k: dv(v) for k, v in fo.items()}, dv(ni)))
        out = []
        for _ in range(TC.TWIN_STEPS):
            for st, fo, ni in runs:
                (ctx.column_step_ocean if fused else ctx.column_step)(TC.TWIN_DT, st, fo, ni)
            out.append(abs(float((runs[0][0]["hice"] - runs[1][0]["hice"]).sum())) / runs[0][0]["hice"].numel())
        return out

    slab, plain = differences(True), differences(False)
    print("twin runs on the device: bound %.4f m; slab max %.4f m; plain step 1 %.4f, step 2 %.4f, step 20 %.4f"
          % (TC.TWIN_BOUND, max(slab), plain[0], plain[1], plain[-1]))
    assert slab[0] > 0.5 * TC.TWIN_BOUND
    assert all(d <= TC.TWIN_BOUND for d in slab), slab
    assert plain[0] <= TC.TWIN_BOUND < plain[1] and plain[-1] > 10 * TC.TWIN_BOUND, plain

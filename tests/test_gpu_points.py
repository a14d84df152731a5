"""Point samples on the device (csrc/points.hip; include/nsdg.h "point samples"): nsdg_points_sample against the float64
reference (tests/points_ref.py) on the inputs of tests/points_cases.py, against the history's samples at element centres, its row ranges,
guard words and checks, and the Python driver on 1 row block against 3.

The bound, |device - reference| <= K 2^-53 M per sample, is derived, not measured.  M (tests/points_ref.py) is the sample's expression with
every source value, coefficient and monomial of a weight or basis function replaced by its absolute value.  For an expression of +, -, * and
division by an exact h in which every operation rounds once (relative 2^-53), the computed value is within k 2^-53 M of the exact one to
first order, with k counted along the tree: an input 0, a sum 1 + the larger count of its operands, a product 1 + the SUM of the counts of
its factors (both factors' errors scale the product), a constant that is itself rounded (1/12) as one rounding.  FMA contraction only
removes roundings; terms of second order (K^2 2^-53 of the bound) are not counted.  The local coordinates are not counted: x / hx - ix - 1/2
is the same float64 on the device and in the reference (one IEEE division, two exact subtractions), and the sample is defined at that
(xi, eta).  A square root r = sqrt(a^2 + b^2) takes M_a + M_b and
max(k_a, k_b) + 2: |dr| <= |da| + |db|, the two squares and their sum (positive terms: relative 2 * 2^-53, halved by the root) and the root's
own rounding are relative to r <= M_a + M_b.

The device's paths (csrc/points.hip), K = the count at the sample:
  weights       s = 2 t t: 1; L = s -+ t, 1 - 2 s: 2; L' = 4 t -+ 1: 1
  u, v          a row: L_c w: 3, three of them summed: 5; L_r (row): 2 + 5 + 1 = 8; three summed: 10
  speed         10 + 2 = 12
  e11, e22      a row with L': 4, L_r (row): 7, summed: 9, / h: 10 (the row with L, then L': 5, 7, 9, 10); divergence = e11 + e22: 11
  shear         g: two such quotients added: 11; e11 - e22: 11; the root: 13
  hice, ...     xi xi - 1/12: 1 + 1 + the constant = 3; c3 times it: 4, entering the third of five additions: 4 + 3 = 7
  stress        eta (xi xi - 1/12): 4; c3 (xi xi - 1/12): 4, entering the third of seven additions: 4 + 5 = 9
  sigma_n       s11 + s22: 10, halved exactly
  sigma_s       s11 - s22: 10; the root: 12
-- points_ref.K: hice, cice, damage 7; u, v 10; speed 12; divergence 11; shear 13; sigma_n 10; sigma_s 12.  hsnow and tice are copies: bit for
bit.  The bound is the device's alone, so the reference must not spend it: its float64 route computes every sum and product compensated
(double-double from float64 operations) and rounds once, and tests/test_points_cpu.py holds it to a quarter of the bound against extended
precision on every case used here."""
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

import points_cases as cases  # noqa: E402
import points_ref as R  # noqa: E402
import test_gpu_bbm_native as BN  # noqa: E402 -- its fields and run_core: the brittle rheology in the native row-block plan
import thread_ranks  # noqa: E402
from nextsimdg_amd import abi, rowblock, synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -7777.25


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_refs = {}


def case(*key):
    """the inputs and the float64 reference of one case, computed once and left unchanged"""
    if key not in _refs:
        c = cases.make(*key)
        want, M = cases.reference(c)
        want.setflags(write=False)
        M.setflags(write=False)
        _refs[key] = (c, want, M)
    return _refs[key]


def sources(c, lo=0, hi=None):
    """the device arrays of the element rows [lo, hi) of case c (the planes of the stress stay on the host)"""
    src = c["src"] if (lo, hi) in ((0, None), (0, c["ny"])) else cases.local_sources(c, lo, hi)
    return {k: dev(a) for k, a in src.items() if not k.endswith("p")}


def sample(ctx, c, fields=None, j0=0, j1=None, lo=0, hi=None, ny_global=0, src=None, pad=5):
    """one launch on the rows [lo, hi) of case c as the local array, into planes `pad` doubles apart with guard words around and between
    them; asserts the guards and returns the samples [nfields, n]"""
    fields = fields or c["fields"]
    hi = c["ny"] if hi is None else hi
    n = len(c["x"])
    ctx.set_grid(c["nx"], hi - lo, c["hx"], c["hy"])
    ctx.set_block(lo, ny_global)
    src = src or sources(c, lo, hi)
    stride = n + pad
    buf = torch.full((GUARD + len(fields) * stride + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    out = buf[GUARD:GUARD + len(fields) * stride].view(len(fields), stride)[:, :n]
    x, y = dev(c["x"]), dev(c["y"])
    ctx.points_sample(j0, hi - lo if j1 is None else j1, c["order"], x, y, fields, src, out)
    torch.cuda.synchronize()
    ctx.set_block(0, 0)
    assert torch.equal(x, dev(c["x"])) and torch.equal(y, dev(c["y"]))
    host = buf.cpu().numpy()
    body = host[GUARD:GUARD + len(fields) * stride].reshape(len(fields), stride)
    assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL) and np.all(body[:, n:] == SENTINEL), "a guard word was written"
    return body[:, :n].copy()


def compare(got, want, M, fields, what, record=None):
    bound = R.bound(fields, M)
    for k, f in enumerate(fields):
        if R.K[f] == 0:
            assert np.array_equal(got[k], want[k]), (what, f)
            continue
        err = np.abs(got[k] - want[k])
        ratio = float(np.max(np.where(bound[k] > 0, err / np.where(bound[k] > 0, bound[k], 1.0), np.where(err > 0, np.inf, 0.0))))
        print("%s %s: largest difference %.3g of the bound" % (what, f, ratio))
        if record is not None:
            record[f] = max(record.get(f, 0.0), ratio)
        assert ratio <= 1.0, (what, f, ratio)


# ------------------------------------------------------------------------------------------------ the kernel against the reference
@pytest.mark.parametrize("nx,ny,n,order,rheology", cases.CASES)
def test_every_field_matches_the_reference(ctx, nx, ny, n, order, rheology):
    assert abi.POINTS_BLOCK == cases.BLOCK
    c, want, M = case(nx, ny, n, order, rheology)
    got = sample(ctx, c)
    assert np.all(np.isfinite(got))  # a single domain owns every point, and no padding lane of a tile (NaN) was read
    compare(got, want, M, c["fields"], "%dx%d n=%d order %d %s:" % (nx, ny, n, order, rheology))


def test_at_element_centres_the_samples_are_the_historys(ctx):
    """u, v, speed bit for bit nsdg_history_accumulate(store=1) of the same state; divergence and shear, which the history forms from
    differences of two nodes, within the bound"""
    c, _, _ = case(70, 9, 1000, 2, "bbm")
    nx, ny = c["nx"], c["ny"]
    X, Y = np.meshgrid((np.arange(nx) + 0.5) * c["hx"], (np.arange(ny) + 0.5) * c["hy"])
    at = dict(c, x=X.ravel(), y=Y.ravel())
    fields = ("u", "v", "speed", "divergence", "shear", "hsnow", "tice")
    src = sources(c)
    got = sample(ctx, at, fields, src=src)
    acc = torch.full((len(fields), ny, nx), float("nan"), dtype=torch.float64, device="cuda")
    ctx.history_accumulate(0, ny, fields, src, True, 0, acc)
    hist = acc.cpu().numpy().reshape(len(fields), -1)
    for k in (0, 1, 2, 5, 6):
        assert np.array_equal(got[k], hist[k]), fields[k]
    _, M = cases.reference(at, fields)
    bound = R.bound(fields, M)
    assert np.all(np.abs(got[3:5] - hist[3:5]) <= bound[3:5])
    cell = sample(ctx, dict(at, order=0), ("hice", "cice", "damage"), src=src)  # order 0: the cell means, as the history's
    for k, name in enumerate(("H", "A", "D")):
        assert np.array_equal(cell[k], c["src"][name][0].ravel())


def test_two_row_ranges_and_their_maximum_equal_one_launch(ctx):
    c, want, _ = case(70, 9, 1000, 2, "bbm")
    whole = sample(ctx, c)
    a, b = sample(ctx, c, j0=0, j1=4), sample(ctx, c, j0=4, j1=9)
    rows = R.locate(c["y"], c["hy"], 9)
    for part, (j0, j1) in ((a, (0, 4)), (b, (4, 9))):
        outside = (rows < j0) | (rows >= j1)
        assert outside.any() and np.all(np.isneginf(part[:, outside])) and np.all(np.isfinite(part[:, ~outside]))
    assert np.array_equal(np.maximum(a, b), whole)
    assert np.all(np.isneginf(sample(ctx, c, j0=3, j1=3)))  # an empty range owns nothing, and says so


def test_a_placed_row_block_computes_what_the_domain_computes(ctx):
    """rows [3, 6) of the 9 as a local array [2, 7) placed by nsdg_block_set, and the blocks at the two ends: bit for bit the single domain,
    -inf exactly where not owned"""
    c, _, _ = case(70, 9, 1000, 2, "bbm")
    whole = sample(ctx, c)
    rows = R.locate(c["y"], c["hy"], 9)
    merged = np.full_like(whole, -np.inf)
    for lo, hi, j0, j1 in ((0, 4, 0, 3), (2, 7, 1, 4), (5, 9, 1, 4)):
        part = sample(ctx, c, j0=j0, j1=j1, lo=lo, hi=hi, ny_global=9)
        owned = (rows >= lo + j0) & (rows < lo + j1)
        assert np.all(np.isneginf(part[:, ~owned])) and np.all(np.isfinite(part[:, owned]))
        merged = np.maximum(merged, part)
    assert np.array_equal(merged, whole)


def test_a_subset_in_another_order_gives_the_same_values(ctx):
    c, _, _ = case(65, 3, cases.BLOCK, 1, "bbm")
    src = sources(c)
    whole = sample(ctx, c, src=src)
    for subset in (("shear", "hice"), ("sigma_s", "damage", "u"), ("tice", "speed", "sigma_n", "cice", "divergence", "v", "hsnow"), ("cice",)):
        only = {k: t for k, t in src.items() if any(k in abi.POINTS_SOURCES[f] for f in subset)}  # what it does not read may be NULL
        part = sample(ctx, c, subset, src=only, pad=0 if len(subset) == 1 else 3)
        for k, f in enumerate(subset):
            assert np.array_equal(part[k], whole[c["fields"].index(f)]), (subset, f)


def test_a_nan_source_reaches_the_points_of_its_element_only(ctx):
    c, _, _ = case(70, 9, 1000, 2, "bbm")
    ex, ey = 64, 4  # the first element of the second stress tile
    ix, iy = R.locate(c["x"], c["hx"], 70), R.locate(c["y"], c["hy"], 9)
    inside = (ix == ex) & (iy == ey)
    pts = dict(c, x=np.concatenate([c["x"], [(ex + 0.3) * c["hx"], (ex + 1.0) * c["hx"]]]), y=np.concatenate([c["y"], [(ey + 0.6) * c["hy"]] * 2]))
    inside = np.concatenate([inside, [True, False]])  # the second one sits on the element's east edge: it belongs to the neighbour
    clean = sample(ctx, pts)
    for name, fields in (("H", ("hice",)), ("s12", ("sigma_s",)), ("hsnow", ("hsnow",)), ("D", ("damage",))):
        bad = {k: a.copy() for k, a in c["src"].items()}
        if name == "s12":
            planes = bad["s12p"].copy()
            planes[7, ey, ex] = np.nan
            bad["s12"] = cases.tile(planes)
        elif bad[name].ndim == 3:
            bad[name][-1, ey, ex] = np.nan
        else:
            bad[name][ey, ex] = np.nan
        got = sample(ctx, pts, src={k: dev(a) for k, a in bad.items() if not k.endswith("p")})
        for k, f in enumerate(c["fields"]):
            hit = inside & (f in fields)
            assert np.all(np.isnan(got[k][hit])) and np.array_equal(got[k][~hit], clean[k][~hit]), (name, f)
    bad = {k: a.copy() for k, a in c["src"].items()}
    bad["u"][2 * ey + 1, 2 * ex + 1] = np.nan  # the centre node belongs to this element alone
    got = sample(ctx, pts, src={k: dev(a) for k, a in bad.items() if not k.endswith("p")})
    for k, f in enumerate(c["fields"]):
        hit = inside & (f in ("u", "speed", "divergence", "shear"))
        assert np.all(np.isnan(got[k][hit])) and np.array_equal(got[k][~hit], clean[k][~hit]), ("u", f)


def test_checks(ctx, gpu):
    c, _, _ = case(70, 9, cases.BLOCK - 1, 2, "bbm")
    n, nf = len(c["x"]), 3
    ctx.set_grid(70, 9, c["hx"], c["hy"])
    ctx.set_block(0, 0)
    src_t = sources(c)
    src = ctx._history_sources("test", src_t)
    x, y = dev(c["x"]), dev(c["y"])
    out = torch.empty(nf, n, dtype=torch.float64, device="cuda")
    ids = (abi.I32 * 16)(*[abi.HISTORY_FIELDS.index(f) for f in ("hice", "shear", "sigma_s")])
    call = lambda *a: ctx.lib.nsdg_points_sample(ctx.h, *a)
    good = [0, 9, 2, n, x.data_ptr(), y.data_ptr(), nf, ids, abi.C.byref(src), n, out.data_ptr()]
    assert call(*good) == 0

    def refused(changes, text, status=-1):
        args = list(good)
        for k, value in changes.items():
            args[k] = value
        assert call(*args) == status, changes
        assert text in ctx.lib.nsdg_last_error().decode(), ctx.lib.nsdg_last_error()

    refused({0: -1}, "row range")
    refused({1: 10}, "row range")
    refused({0: 5, 1: 4}, "row range")
    refused({2: 3}, "order must be 0, 1 or 2")
    refused({2: -1}, "order must be 0, 1 or 2")
    refused({3: -1}, "n must be >= 0")
    refused({6: 0}, "nfields must be in [1, NSDG_HISTORY_MAX_FIELDS]")
    refused({6: 17}, "nfields must be in [1, NSDG_HISTORY_MAX_FIELDS]")
    refused({9: n - 1}, "out_stride is smaller")
    for k in (4, 5, 7, 8, 10):
        refused({k: None}, "null pointer")
    refused({7: (abi.I32 * 3)(0, 12, 1)}, "unknown field id 12 at position 1")
    refused({7: (abi.I32 * 3)(0, -1, 1)}, "unknown field id -1 at position 1")
    refused({7: (abi.I32 * 3)(6, 0, 6)}, "field 'shear' is listed twice")
    for name, field in (("H", "hice"), ("A", "cice"), ("u", "speed"), ("v", "divergence"), ("s11", "sigma_n"), ("s12", "sigma_s"), ("s22", "sigma_n"),
                        ("hsnow", "hsnow"), ("tice", "tice"), ("D", "damage")):
        less = ctx._history_sources("test", {k: t for k, t in src_t.items() if k != name})
        refused({6: 1, 7: (abi.I32 * 1)(abi.HISTORY_FIELDS.index(field)), 8: abi.C.byref(less)},
                "field '%s' needs the source %s, which is a null pointer" % (field, name))
    # the tiled stress is loaded 16 bytes at a time: a view 8 bytes into a buffer is refused for whichever component the list reads, out
    # stays as it was, and a component no listed field reads is not looked at
    torch.cuda.synchronize()
    out.fill_(SENTINEL)
    shifted = {}
    for name in ("s11", "s12", "s22"):
        buf = torch.zeros(src_t[name].numel() + 1, dtype=torch.float64, device="cuda")
        buf[1:].copy_(src_t[name].reshape(-1))
        shifted[name] = buf[1:]
        assert shifted[name].data_ptr() % 16 == 8
    for name, field in (("s11", "sigma_n"), ("s12", "sigma_s"), ("s22", "sigma_n"), ("s22", "sigma_s")):
        off = ctx._history_sources("test", dict(src_t, **{name: shifted[name]}))
        refused({6: 1, 7: (abi.I32 * 1)(abi.HISTORY_FIELDS.index(field)), 8: abi.C.byref(off)},
                "nsdg_points_sample: tiled arrays (stress, ice strength) must be 16-byte aligned")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    off = ctx._history_sources("test", dict(src_t, s12=shifted["s12"]))
    assert call(*good[:6], 2, (abi.I32 * 2)(abi.HISTORY_FIELDS.index("hice"), abi.HISTORY_FIELDS.index("sigma_n")), abi.C.byref(off), n,
                out.data_ptr()) == 0  # sigma_n reads s11 and s22 alone
    torch.cuda.synchronize()
    assert bool((out[:2] != SENTINEL).all()) and bool((out[2] == SENTINEL).all())
    args = list(good)
    args[3], args[4], args[5], args[10], args[9] = 0, None, None, None, 0
    assert call(*args) == 0  # n == 0 launches nothing
    torch.cuda.synchronize()
    with pytest.raises(abi.NsdgError, match="order 2 needs"):
        ctx.points_sample(0, 9, 2, x, y, ("hice",), {"H": src_t["H"][:3].contiguous()}, out[:1])
    with pytest.raises(abi.NsdgError, match="unit stride"):
        ctx.points_sample(0, 9, 2, x, y[:-1], ("hice",), src_t, out[:1])
    with pytest.raises(abi.NsdgError, match="unknown history field"):
        ctx.points_sample(0, 9, 2, x, y, ("thickness",), src_t, out[:1])
    fresh = abi.Context(gpu)
    try:
        assert fresh.lib.nsdg_points_sample(fresh.h, *good) == -3  # NSDG_ERR_STATE: no grid
    finally:
        fresh.close()


# ------------------------------------------------------------------------------------------------ the driver: 1 row block against 3
NX, NY, NSUB, NSTEPS, WIND = 64, 48, 24, 4, 3.0
DRIFTER_FIELDS = ("hice", "cice", "shear")
STATION_FIELDS = ("divergence", "sigma_s", "speed", "hice", "sigma_n")


def seeds(L, hy, boundaries):
    rng = np.random.default_rng(5)
    xy = []
    for row in boundaries:  # the boundaries of three row blocks: on them, next to them
        for off in (0.0, 0.01, -0.01, 1.0, -1.0):
            for fx in np.linspace(0.08, 0.92, 7):
                xy.append((fx * L[0], row * hy + off))
    xy += [(x, y) for x, y in zip(rng.uniform(0, L[0], 40), rng.uniform(0, L[1], 40))]
    xy += [(0.0, 0.0), (L[0], L[1]), (0.0, 0.5 * L[1]), (0.5 * L[0], L[1])]
    return np.array(xy)


class CountingExchanger(rowblock.NativeHaloExchanger):
    """counts what crosses the ranks: every ghost exchange started and every reduction"""
    exchanges = 0

    def _start(self, plan):
        self.exchanges += 1
        return super()._start(plan)

    def max_array(self, tensor):
        self.exchanges += 1
        super().max_array(tensor)


def mevp_rank(rank, world, gid, out, variant=4, native=False, use_graph=False, steps=NSTEPS, resume=None, substeps=None, **kw):
    try:
        c = abi.Context(torch.device("cuda:0"))
        c.set_mevp_variant(variant)
        c.set_mevp_params(c.mevp_default_params(alpha=300.0, beta=300.0))
        bt, H, A, uo, vo, ua, va = thread_ranks.fields(NX, NY, WIND)
        depth = (variant, variant - 1) if variant >= 2 else (1, 1)
        blk = rowblock.RowBlock(NX, NY, rank, world, *depth)
        exchanger = None
        if world > 1:
            c.comm_deadline(60.0)
            exchanger = CountingExchanger(c, blk, local_group=gid)
        core = rowblock.DynamicsCore(c, blk, bt.hx, bt.hy, 120.0, NSUB, torch.device("cuda"), exchanger=exchanger, native=native, use_graph=use_graph, **kw)
        core.load_global(H, A, uo, vo, ua, va)
        if resume is not None:
            core.load_state_dict(resume)
        for _ in range(steps):
            if substeps is None:
                core.step()
            else:
                core.advance(240.0, substeps=substeps)
        out[rank] = collect(core, exchanger)
        core.close()
        c.close()
    except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread; the peers' waits end at their deadline
        out[rank] = e


def bbm_rank(rank, world, gid, out, **kw):
    try:
        c = abi.Context(torch.device("cuda:0"))
        exchanger = None
        if world > 1:
            c.comm_deadline(60.0)
            exchanger = CountingExchanger(c, rowblock.RowBlock(BN.DNX, BN.DNY, rank, world, 1, 1), local_group=gid)
        core = BN.run_core(c, torch.device("cuda"), BN.ODD_NSUB, True, rank, world, exchanger, **kw)
        out[rank] = collect(core, exchanger)
        core.close()
        c.close()
    except BaseException as e:  # noqa: BLE001
        out[rank] = e


def collect(core, exchanger):
    torch.cuda.synchronize()
    res = {k: core.owned(getattr(core, k)).cpu().numpy() for k in ("H", "A", "u", "v")}
    res["drifters"] = core.drifters_read() if core._drifters is not None else None
    res["stations"] = core.stations_read() if core._stations is not None else None
    res["state"] = core.state_dict()
    res["rows"] = (core.blk.r0, core.blk.r1)
    res["exchanges"] = exchanger.exchanges if exchanger is not None else 0
    return res


def run_world(target, world, **kw):
    out = {}
    thread_ranks._local_group[0] += 1
    threads = [threading.Thread(target=target, args=(r, world, thread_ranks._local_group[0], out), kwargs=kw) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for r in range(world):
        if isinstance(out[r], BaseException):
            raise out[r]
    return out


def mevp_points():
    bt = synthetic.BoxTest(NX, NY)
    p = seeds((bt.L, bt.L), bt.hy, (16, 32))
    return dict(drifters=p, drifter_fields=DRIFTER_FIELDS, stations=p, station_fields=STATION_FIELDS, station_capacity=NSTEPS), bt.hy, NY


def bbm_points():
    p = seeds((BN.DNX * BN.HX, BN.DNY * BN.HY), BN.HY, (6, 12))
    fields = DRIFTER_FIELDS + ("damage",)
    return dict(drifters=p, drifter_fields=fields, stations=p, station_fields=STATION_FIELDS + ("damage",), station_capacity=8), BN.HY, BN.DNY


def assert_points_equal(parts, one, kw, hy, ny):
    merged = rowblock.DynamicsCore.merge_stations([parts[r]["stations"] for r in (2, 0, 1)])
    want = rowblock.DynamicsCore.merge_stations([one["stations"]])
    assert want["count"] == merged["count"] > 0
    rows = R.locate(kw["stations"][:, 1], hy, ny)
    for f in kw["station_fields"]:
        assert np.all(np.isfinite(want[f])) and np.array_equal(merged[f], want[f]), f
    for r in range(3):
        r0, r1 = parts[r]["rows"]
        mine = (rows >= r0) & (rows < r1)
        assert mine.any() and np.all(np.isneginf(parts[r]["stations"]["hice"][:, ~mine])) and np.all(np.isfinite(parts[r]["stations"]["hice"][:, mine]))
        for k in ("x", "y", "status"):
            assert np.array_equal(parts[r]["drifters"][k], one["drifters"][k]), (r, k)
        for f in kw["drifter_fields"]:
            assert np.all(np.isfinite(one["drifters"]["fields"][f]))
            assert np.array_equal(parts[r]["drifters"]["fields"][f], one["drifters"]["fields"][f]), (r, f)


@pytest.fixture(scope="module")
def one_block(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    kw, _, _ = mevp_points()
    return run_world(mevp_rank, 1, **kw)[0]


@pytest.mark.parametrize("variant,native,use_graph", [(4, False, False), (1, False, False), (4, True, True)], ids=["v4", "v1", "v4_native_graph"])
def test_three_blocks_sample_what_one_block_samples(one_block, variant, native, use_graph):
    """thread ranks on the native exchange's local transport: the drifters' fields on every rank and the merged stations agree bit for bit
    with the 1-block run; variant 1 runs the ghost depth (1, 1), whose upper ghost node rows a sample never reads; and a step with
    drifter_fields makes at most one exchange more than a step without"""
    kw, hy, ny = mevp_points()
    parts = run_world(mevp_rank, 3, variant=variant, native=native, use_graph=use_graph, **kw)
    assert_points_equal(parts, one_block, kw, hy, ny)
    for k in ("H", "A"):
        assert np.array_equal(np.concatenate([parts[r][k] for r in range(3)], axis=1), one_block[k]), k
    if not native:  # (the native plans exchange inside their C calls: the Python exchanger sees the drifters' own only)
        plain = run_world(mevp_rank, 3, variant=variant, drifters=kw["drifters"])
        for r in range(3):
            assert 0 < parts[r]["exchanges"] - plain[r]["exchanges"] <= NSTEPS, (parts[r]["exchanges"], plain[r]["exchanges"])


def test_three_native_brittle_blocks_sample_what_one_block_samples(gpu):
    kw, hy, ny = bbm_points()
    one = run_world(bbm_rank, 1, **kw)[0]
    parts = run_world(bbm_rank, 3, **kw)
    assert_points_equal(parts, one, kw, hy, ny)
    assert np.abs(one["drifters"]["fields"]["damage"]).max() > 0


def test_the_fields_do_not_know_about_the_points(one_block):
    plain = run_world(mevp_rank, 1)[0]
    assert plain["drifters"] is None and plain["stations"] is None
    for k in ("H", "A", "u", "v"):
        assert plain[k].tobytes() == one_block[k].tobytes(), k
    for k in ("s11", "s12", "s22"):
        assert plain["state"][k].tobytes() == one_block["state"][k].tobytes(), k
    assert one_block["state"]["drifters"].shape == (3, len(mevp_points()[0]["drifters"]))


def test_checkpoint_and_resume_agree_bit_for_bit(one_block):
    kw, _, _ = mevp_points()
    first = run_world(mevp_rank, 1, steps=NSTEPS // 2, **kw)[0]
    state = rowblock.DynamicsCore.merge_states([first["state"]])
    second = run_world(mevp_rank, 1, steps=NSTEPS - NSTEPS // 2, resume=state, **kw)[0]
    for f in DRIFTER_FIELDS:
        assert np.array_equal(second["drifters"]["fields"][f], one_block["drifters"]["fields"][f]), f
    for f in STATION_FIELDS:
        assert np.array_equal(np.concatenate([first["stations"][f], second["stations"][f]]), one_block["stations"][f]), f


def test_advance_samples_the_stations_once_per_model_step(one_block):
    kw, _, _ = mevp_points()
    a = run_world(mevp_rank, 1, steps=1, substeps=2, **kw)[0]
    assert a["stations"]["count"] == 1
    for f in STATION_FIELDS:
        assert np.array_equal(a["stations"][f][0], one_block["stations"][f][1]), f  # two sub-steps of 120 s are two steps
    for f in DRIFTER_FIELDS:
        assert np.all(np.isfinite(a["drifters"]["fields"][f]))

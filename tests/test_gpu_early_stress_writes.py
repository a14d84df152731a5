"""When the stress of a row leaves its stage of the stage-per-wave mEVP pass (csrc/mevp_fused4.hip, NSDG_P2P_EARLY in csrc/mevp_p2p.h:
the hand-over slot may be waited for and written, and the last stage's stress stored, right after the relaxation instead of at the end
of the row).  Whatever the switch is built with, the pass must equal single sub-iterations bit for bit and no pipeline wait may give
up.  The cases are the smallest that reach what moves: one, two and three column groups, strips shorter than the two-row links and
longer than the seven-row rings (both slot parities wrap), passes of 4, 3 and 2 stages (nsub = 27, 26 -- 25 ends on the
single-iteration kernel -- so the last stage is wave 3, 2 or 1), both forms of alpha / beta, each with and without a land mask, and
the split launches of the row-block plan.  The library under test is the one the package loads (NSDG_LIB selects another build of the
same ABI, as for every A/B run)."""
import numpy as np
import pytest
import torch

import land_ref
from nextsimdg_amd import abi
from test_gpu_land import AD, UNIFORM, box_inputs, device_subcycle, mask_dev
from test_gpu_parity import Box, dev, mevp_state, pack, tdev

pytestmark = pytest.mark.gpu
FORMS = [pytest.param(UNIFORM, id="uniform"), pytest.param(AD, id="adaptive")]
MASKS = [pytest.param(False, id="ocean"), pytest.param(True, id="land")]
GRIDS = [(2, 2), (57, 1), (58, 3), (70, 9), (150, 37)]
STRIPS = (0, 1, 2, 3, 8)
NSUB = (25, 26, 27)


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults_after_each_test(ctx):
    yield
    if ctx.nx:
        ctx.set_land_mask(None)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    ctx.set_mevp_strip_rows(0)
    ctx.set_mevp_params(ctx.mevp_default_params())


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_fused_pass_equals_single_sub_iterations_bitwise(ctx, grid, pk, masked):
    """nsdg_mevp_subcycle from rest: variant 4 (passes of four, then a pass of 3 or 2 stages or the single-iteration kernel) against
    variant 1 (single sub-iterations), u, v and the three stress arrays bit for bit, for every strip height; no wait gave up"""
    nx, ny = grid
    b = Box(ctx, nx, ny, **pk)
    land = land_ref.shapes_mask(nx, ny) if masked else None
    inputs = box_inputs(b, land if masked else np.zeros((ny, nx), dtype=bool))
    for nsub in NSUB:
        ctx.set_mevp_variant(1)
        ctx.set_mevp_strip_rows(0)
        ref = device_subcycle(ctx, b, nsub, inputs, land=land)  # computed once per case, compared against and left unchanged
        assert bool(torch.isfinite(ref[0]).all()) and (masked or float(ref[0].abs().max()) > 0)
        ctx.set_mevp_variant(4)
        for rows in STRIPS:
            ctx.set_mevp_strip_rows(rows)
            got = device_subcycle(ctx, b, nsub, inputs, land=land)
            assert same(ref, got), (nx, ny, nsub, rows, float((ref[0] - got[0]).abs().max()))
    given_up = ctx.pipeline_waits_given_up()
    print("%d x %d: pipeline waits given up: %d" % (nx, ny, given_up))
    assert given_up == 0


def pass_state(ctx, nx, ny, pk, masked):
    """a random state, packed coefficients and the ice strength for direct calls of the pass (the mask, if any, stays set)"""
    b = Box(ctx, nx, ny, **pk)
    land = land_ref.shapes_mask(nx, ny) if masked else np.zeros((ny, nx), dtype=bool)
    pg, cgh, cga, tax, tay = box_inputs(b, land)
    u, v, s = mevp_state(b, np.random.default_rng(83))
    u, v = 0.01 * u, 0.01 * v  # strain rates for which the adaptive alphas spread over the elements
    if masked:
        ln = land_ref.land_nodes(land)
        u[ln] = v[ln] = 0.0
        for x in s:
            x[:, land] = 0.0
        ctx.set_land_mask(mask_dev(land))
    packed = pack(ctx, 120.0, 0.5 * u, 0.5 * v, tax, tay, b.uo, b.vo, cgh, cga)
    return [tdev(x) for x in s], (dev(u), dev(v)), packed, tdev(pg)


def fresh(s_in, uv, fill):
    return [torch.full_like(x, fill) for x in s_in] + [torch.full_like(uv[0], fill), torch.full_like(uv[1], fill)]


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("pk", FORMS)
def test_split_launches_equal_the_single_launch_bitwise(ctx, pk, masked):
    """nsdg_mevp_iterate4 over a row sub-range of 150 x 37, and the launches of the row-block plan on 70 x 9 -- the two boundary bands
    [(0, 4), (5, 9)] in one launch plus the interior row -- against the single launch over all rows"""
    ctx.set_mevp_variant(4)
    nx, ny = 150, 37
    s_in, uv, packed, pg = pass_state(ctx, nx, ny, pk, masked)
    for rows in (0, 3):
        ctx.set_mevp_strip_rows(rows)
        ref, out = fresh(s_in, uv, 0.0), fresh(s_in, uv, 0.0)
        ctx.mevp_iterate4(0, ny, s_in, ref[:3], uv, (ref[3], ref[4]), packed, pg)
        ctx.mevp_iterate4(4, ny - 3, s_in, out[:3], uv, (out[3], out[4]), packed, pg)
        for k in range(3):
            assert torch.equal(abi.untile(out[k], nx)[:, 4:ny - 3], abi.untile(ref[k], nx)[:, 4:ny - 3]), (rows, k)
        for k in (3, 4):
            assert torch.equal(out[k][8:2 * (ny - 3)], ref[k][8:2 * (ny - 3)]), (rows, k)
        assert masked or float(ref[3].abs().max()) > 0
    nx, ny = 70, 9
    s_in, uv, packed, pg = pass_state(ctx, nx, ny, pk, masked)
    for rows in (0, 1, 2):
        ctx.set_mevp_strip_rows(rows)
        ref, out = fresh(s_in, uv, -7.0), fresh(s_in, uv, -7.0)
        ctx.mevp_iterate4(0, ny, s_in, ref[:3], uv, (ref[3], ref[4]), packed, pg)
        ctx.mevp_iterate4_pair((0, 4), (5, 9), s_in, out[:3], uv, (out[3], out[4]), packed, pg)
        ctx.mevp_iterate4(4, 5, s_in, out[:3], uv, (out[3], out[4]), packed, pg)
        for k, (a, c) in enumerate(zip(ref, out)):
            assert torch.equal(a, c), (rows, k, float((a - c).abs().max()))
    assert ctx.pipeline_waits_given_up() == 0

"""Where the loads of the loader wave of the stage-per-wave mEVP pass land (csrc/mevp_fused4.hip, NSDG_P2P_LAND in csrc/mevp_p2p.h: the
coefficients behind the projected stress, the stress request at the end of the row).  The switch moves requests
and waits of one wave and no formula: whatever it is built with, the pass must equal single sub-iterations bit for bit and no pipeline
wait may give up.  Grids: one column group (5, 57 columns), two (58, 64) and three (115) -- 64 and 115 straddle the 57-column seam --,
with 1, 2, 3, 9 and 20 rows: strips shorter than the two-row links and longer than the seven-row rings; passes of 4, 3 and 2 stages
(nsub = 27, 26; 25 ends on the single-iteration kernel); both forms of alpha / beta, each with and without a land mask; the split
launches of the row-block plan.  The library under test is the one the package loads (NSDG_LIB selects another build of the same ABI,
as for every A/B run: that is how every non-zero value of the switch is taken through this file)."""
import numpy as np
import pytest
import torch

import land_ref
from nextsimdg_amd import abi
from test_gpu_early_stress_writes import fresh, pass_state, same
from test_gpu_land import AD, UNIFORM, box_inputs, device_subcycle
from test_gpu_parity import Box

pytestmark = pytest.mark.gpu
FORMS = [pytest.param(UNIFORM, id="uniform"), pytest.param(AD, id="adaptive")]
MASKS = [pytest.param(False, id="ocean"), pytest.param(True, id="land")]
GRIDS = [(5, 1), (57, 2), (58, 3), (64, 9), (115, 20)]
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


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("pk", FORMS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_fused_pass_equals_single_sub_iterations_bitwise(ctx, grid, pk, masked):
    """nsdg_mevp_subcycle from rest: variant 4 against variant 1 (single sub-iterations), u, v and the three stress arrays bit for bit,
    for every strip height and every length of the last pass; no wait gave up"""
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


@pytest.mark.parametrize("masked", MASKS)
@pytest.mark.parametrize("pk", FORMS)
def test_split_launches_equal_the_single_launch_bitwise(ctx, pk, masked):
    """nsdg_mevp_iterate4 over a row sub-range of 115 x 20, and the launches of the row-block plan on 64 x 9 -- the two boundary bands
    [(0, 4), (5, 9)] in ONE launch of two ranges plus the interior row -- against the single launch over all rows"""
    ctx.set_mevp_variant(4)
    nx, ny = 115, 20
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
    nx, ny = 64, 9
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

"""Error behaviour of the C ABI on a live context: bad arguments and call-sequence errors are reported
through the status code + nsdg_last_error() (-> NsdgError in the Python binding), never ignored."""
import pytest
import torch

from nextsimdg_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()


def z(*shape):
    return torch.zeros(*shape, dtype=torch.float64, device="cuda")


def test_grid_must_be_set_first(gpu):
    c = abi.Context(gpu)
    with pytest.raises(abi.NsdgError, match="nsdg_grid_set was not called"):
        c.dg_to_cg(z(6, 4, 4), z(9, 9))
    c.close()


def test_bad_grid_and_params(ctx):
    for bad in ((0, 4, 1.0, 1.0), (4, -1, 1.0, 1.0), (4, 4, 0.0, 1.0)):
        with pytest.raises(abi.NsdgError):
            ctx.set_grid(*bad)
    with pytest.raises(abi.NsdgError, match="alpha and beta"):
        ctx.set_mevp_params(ctx.mevp_default_params(alpha=0.0))
    with pytest.raises(abi.NsdgError):
        ctx.set_mevp_variant(5)
    with pytest.raises(abi.NsdgError):
        ctx.set_mevp_occupancy(4)


def test_row_ranges_aliasing_and_sequence(ctx):
    nx, ny = 70, 12
    ctx.set_grid(nx, ny, 1.0, 1.0)
    s = [ctx.private_zeros(8, ny, nx, "cuda") for _ in range(3)]
    so = [torch.zeros_like(x) for x in s]
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    u, v, un, vn = (z(2 * ny + 1, 2 * nx + 1) for _ in range(4))
    packed = z(8 * u.numel())
    fresh = abi.Context(ctx.device)
    fresh.set_grid(nx, ny, 1.0, 1.0)
    with pytest.raises(abi.NsdgError, match="nsdg_mevp_pack_nodal was not called"):
        fresh.mevp_iterate(0, 0, ny, s, so, (u, v), (un, vn), packed, pg)
    fresh.close()
    nodal = [(u, v), (u, v), (u, v), u, v]
    ctx.mevp_pack_nodal(120.0, *nodal, packed)
    with pytest.raises(abi.NsdgError, match="row range|need 0 <= k0"):
        ctx.mevp_iterate(0, 0, ny + 1, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="k0 == j0 - 1"):
        ctx.mevp_iterate(0, 3, ny, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="must not alias"):
        ctx.mevp_iterate(0, 0, ny, s, s, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="must not alias"):
        ctx.mevp_iterate(0, 0, ny, s, so, (u, v), (u, vn), packed, pg)
    ctx.set_mevp_variant(2)
    with pytest.raises(abi.NsdgError, match="two ghost rows"):
        ctx.mevp_iterate2(1, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_mevp_variant(1)
    with pytest.raises(abi.NsdgError, match="variant 2"):
        ctx.mevp_iterate2(0, ny, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="variant 3"):
        ctx.mevp_iterate3(0, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_mevp_variant(3)
    with pytest.raises(abi.NsdgError, match="three ghost rows"):
        ctx.mevp_iterate3(2, ny, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="two ghost rows above"):
        ctx.mevp_iterate3(0, ny - 1, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="variant 4"):
        ctx.mevp_iterate4(0, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_mevp_variant(4)
    with pytest.raises(abi.NsdgError, match="four ghost rows"):
        ctx.mevp_iterate4(3, ny, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="three ghost rows above"):
        ctx.mevp_iterate4(0, ny - 2, s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="disjoint"):
        ctx.mevp_iterate4_pair((0, ny), (4, ny), s, so, (u, v), (un, vn), packed, pg)
    with pytest.raises(abi.NsdgError, match="must not alias"):
        ctx.mevp_iterate4(0, ny, s, s, (u, v), (un, vn), packed, pg)
    ctx.mevp_iterate3(0, ny, s, so, (u, v), (un, vn), packed, pg)  # a variant-4 context still serves the three-iteration pass (remainders)
    ctx.set_mevp_variant(abi.DEFAULT_MEVP_VARIANT)
    with pytest.raises(abi.NsdgError, match="order must be"):
        ctx.prepare_advection(3, u, v, z(6, ny, nx), z(6, ny, nx), z(3, ny, nx + 1), z(3, ny + 1, nx))
    with pytest.raises(abi.NsdgError, match="ncoef"):
        ctx.dg_to_cg(z(4, ny, nx), u)
    # wrong dtype / device never reaches the library
    with pytest.raises(abi.NsdgError, match="float64 CUDA"):
        ctx.wind_stress(u.float(), v, un, vn)
    with pytest.raises(abi.NsdgError, match="float64 CUDA"):
        ctx.wind_stress(u.cpu(), v, un, vn)
    # empty row ranges are no-ops
    ctx.mevp_iterate2(4, 4, s, so, (u, v), (un, vn), packed, pg)
    ctx.transport_stage(2, 5, 5, 1.0, 0.0, 1.0, [z(6, ny, nx)], [z(6, ny, nx)], [z(6, ny, nx)],
                        (z(6, ny, nx), z(6, ny, nx), z(3, ny, nx + 1), z(3, ny + 1, nx)))
    torch.cuda.synchronize()


def test_parameter_or_grid_change_invalidates_the_packed_coefficients(ctx):
    """the launch constants of the velocity update (K1, K2 from beta, rho_ice and dt) belong to the packing: changing the
    mEVP parameters or the grid between nsdg_mevp_pack_nodal and an iterate must be an error, not a silent mix of two
    parameter sets; repacking makes the call valid again"""
    nx, ny = 70, 12
    ctx.set_grid(nx, ny, 1.0, 1.0)
    s = [ctx.private_zeros(8, ny, nx, "cuda") for _ in range(3)]
    so = [torch.zeros_like(x) for x in s]
    pg = ctx.private_zeros(9, ny, nx, "cuda")
    u, v, un, vn = (z(2 * ny + 1, 2 * nx + 1) for _ in range(4))
    packed = z(8 * u.numel())
    nodal = [(u, v), (u, v), (u, v), u, v]
    ctx.mevp_pack_nodal(120.0, *nodal, packed)
    ctx.mevp_iterate(0, 0, ny, s, so, (u, v), (un, vn), packed, pg)  # fine
    ctx.set_mevp_params(ctx.mevp_default_params(beta=777.0))
    for call in (lambda: ctx.mevp_iterate(0, 0, ny, s, so, (u, v), (un, vn), packed, pg),
                 lambda: ctx.mevp_iterate3(0, ny, s, so, (u, v), (un, vn), packed, pg),
                 lambda: ctx.mevp_velocity(0, ny, s, (u, v), (un, vn), packed)):
        with pytest.raises(abi.NsdgError, match="pack_nodal was not called"):
            call()
    ctx.mevp_pack_nodal(120.0, *nodal, packed)
    ctx.mevp_iterate3(0, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_grid(nx, ny, 2.0, 1.0)  # another cell size: the coefficients belong to the old grid
    with pytest.raises(abi.NsdgError, match="pack_nodal was not called"):
        ctx.mevp_iterate(0, 0, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_grid(nx, ny, 2.0, 1.0)  # setting the same grid again changes nothing ...
    ctx.mevp_pack_nodal(120.0, *nodal, packed)
    ctx.set_grid(nx, ny, 2.0, 1.0)  # ... and does not invalidate a packing
    ctx.mevp_iterate(0, 0, ny, s, so, (u, v), (un, vn), packed, pg)
    # another SHAPE with the same cell size: the packed coefficients (and the arrays) belong to the old local array
    ctx.set_grid(nx, ny - 2, 2.0, 1.0)
    with pytest.raises(abi.NsdgError, match="pack_nodal was not called"):
        ctx.mevp_iterate(0, 0, ny - 2, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_grid(nx - 6, ny, 2.0, 1.0)
    with pytest.raises(abi.NsdgError, match="pack_nodal was not called"):
        ctx.mevp_iterate3(0, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_grid(nx, ny, 2.0, 1.0)  # back to the first shape: still invalid until repacked
    with pytest.raises(abi.NsdgError, match="pack_nodal was not called"):
        ctx.mevp_iterate(0, 0, ny, s, so, (u, v), (un, vn), packed, pg)
    ctx.set_mevp_params(ctx.mevp_default_params())
    torch.cuda.synchronize()


def test_mevp_pass_contract(gpu):
    """Every check of the six nsdg_mevp_iterate* entry points, with the status code and the full nsdg_last_error() text
    (the entry point's name at its front), in the order each makes them: the empty range of nsdg_mevp_iterate (k0 == j1)
    is checked before the packing, that of iterate2 / 3 / 4 after it and before the variant gate; the pair forms have
    no empty range and gate the variant after the packing"""
    nx, ny = 70, 12
    ARG, STATE = -1, -3
    not_packed = (STATE, "nsdg_mevp_pack_nodal was not called on this context")
    below = "need %s ghost rows below the %s (or j0 == 0 at the physical boundary)"
    above = "need %s ghost rows above the %s (or j1 == ny at the physical boundary)"
    empty = (ARG, "row range outside the local array (or empty)")
    variant2 = (STATE, "select variant 2, 3 or 4 (nsdg_mevp_variant_set) or call nsdg_mevp_iterate twice")
    variant3 = (STATE, "select variant 3 or 4 (nsdg_mevp_variant_set)")
    variant4 = (STATE, "select variant 4 (nsdg_mevp_variant_set)")
    fresh, packed_ctx = abi.Context(gpu), abi.Context(gpu)
    for c in (fresh, packed_ctx):
        c.set_grid(nx, ny, 1.0, 1.0)
    s = [fresh.private_zeros(8, ny, nx, "cuda") for _ in range(3)]
    so = [torch.zeros_like(x) for x in s]
    pg = fresh.private_zeros(9, ny, nx, "cuda")
    u, v, un, vn = (z(2 * ny + 1, 2 * nx + 1) for _ in range(4))
    packed = z(8 * u.numel())
    packed_ctx.mevp_pack_nodal(120.0, (u, v), (u, v), (u, v), u, v, packed)
    bufs = dict(s_in=s, s_out=so, uv_old=(u, v), uv_new=(un, vn), packed=packed, pg=pg)
    cases = [  # (context, variant, entry point, row arguments, buffers replaced, expected status and message; None = NSDG_OK)
        (fresh, 1, "mevp_iterate", (0, 0, 0), {}, None),
        (fresh, 1, "mevp_iterate", (0, 0, ny), {}, not_packed),
        (fresh, 1, "mevp_iterate2", (4, 4), {}, not_packed),
        (fresh, 1, "mevp_iterate3", (4, 4), {}, not_packed),
        (fresh, 1, "mevp_iterate4", (4, 4), {}, not_packed),
        (fresh, 1, "mevp_iterate2", (0, ny), {}, not_packed),
        (fresh, 1, "mevp_iterate3_pair", ((0, 4), (6, 10)), {}, not_packed),
        (fresh, 1, "mevp_iterate4_pair", ((0, 4), (6, 8)), {}, not_packed),
        (packed_ctx, 1, "mevp_iterate2", (4, 4), {}, None),
        (packed_ctx, 1, "mevp_iterate3", (4, 4), {}, None),
        (packed_ctx, 1, "mevp_iterate4", (4, 4), {}, None),
        (packed_ctx, 1, "mevp_iterate2", (0, ny), {}, variant2),
        (packed_ctx, 2, "mevp_iterate3", (0, ny), {}, variant3),
        (packed_ctx, 3, "mevp_iterate4", (0, ny), {}, variant4),
        (packed_ctx, 2, "mevp_iterate3_pair", ((0, 4), (6, 10)), {}, variant3),
        (packed_ctx, 3, "mevp_iterate4_pair", ((0, 4), (6, 8)), {}, variant4),
        (packed_ctx, 2, "mevp_iterate3_pair", ((4, 4), (8, 10)), {}, empty),
        (packed_ctx, 4, "mevp_iterate3_pair", ((4, 4), (8, 10)), {}, empty),
        (packed_ctx, 4, "mevp_iterate4_pair", ((4, 8), (10, 10)), {}, empty),
        (packed_ctx, 4, "mevp_iterate3_pair", ((2, 6), (8, 10)), {}, (ARG, below % ("three", "rows of a range"))),
        (packed_ctx, 4, "mevp_iterate3_pair", ((0, 4), (6, 11)), {}, (ARG, above % ("two", "rows of a range"))),
        (packed_ctx, 4, "mevp_iterate4_pair", ((4, 8), (2, 3)), {}, (ARG, below % ("four", "rows of a range"))),
        (packed_ctx, 4, "mevp_iterate4_pair", ((0, 10), (11, 12)), {}, (ARG, above % ("three", "rows of a range"))),
        (packed_ctx, 4, "mevp_iterate3_pair", ((0, 6), (4, 12)), {}, (ARG, "the two row ranges must be disjoint")),
        (packed_ctx, 4, "mevp_iterate", (0, 0, ny + 1), {}, (ARG, "need 0 <= k0 <= j0 <= j1 <= ny")),
        (packed_ctx, 4, "mevp_iterate", (0, 3, ny), {}, (ARG, "need k0 == j0 - 1 (one ghost row below) or k0 == j0 == 0")),
        (packed_ctx, 4, "mevp_iterate2", (0, ny + 1), {}, (ARG, "row range outside the local array")),
        (packed_ctx, 4, "mevp_iterate2", (1, 1), {}, (ARG, below % ("two", "owned rows"))),
        (packed_ctx, 4, "mevp_iterate3", (2, 2), {}, (ARG, below % ("three", "owned rows"))),
        (packed_ctx, 4, "mevp_iterate3", (0, ny - 1), {}, (ARG, above % ("two", "owned rows"))),
        (packed_ctx, 4, "mevp_iterate4", (3, ny), {}, (ARG, below % ("four", "owned rows"))),
        (packed_ctx, 4, "mevp_iterate4", (0, ny - 2), {}, (ARG, above % ("three", "owned rows"))),
        (packed_ctx, 2, "mevp_iterate2", (0, ny - 1), {}, None),  # a pass of two needs no ghost row above
        (packed_ctx, 4, "mevp_iterate", (0, 0, ny), {"pg": None}, (ARG, "null field pointer")),
        (packed_ctx, 4, "mevp_iterate4_pair", ((0, 4), (6, 8)), {"pg": pg.view(-1)[1:]},
         (ARG, "tiled arrays (stress, ice strength) must be 16-byte aligned")),
        (packed_ctx, 4, "mevp_iterate3", (0, ny), {"s_out": s}, (ARG, "the output stress must not alias the input stress")),
        (packed_ctx, 4, "mevp_iterate2", (0, ny), {"uv_new": (u, vn)}, (ARG, "u_new/v_new must not alias u_old/v_old")),
    ]
    for c, variant, name, rows, replaced, expected in cases:
        c.set_mevp_variant(variant)
        call = lambda: getattr(c, name)(*rows, **dict(bufs, **replaced))
        if expected is None:
            call()
            continue
        with pytest.raises(abi.NsdgError) as e:
            call()
        assert str(e.value) == "nsdg error %d: nsdg_%s: %s" % (expected[0], name, expected[1]), (variant, name, rows)
    torch.cuda.synchronize()
    fresh.close()
    packed_ctx.close()


def test_iterate_without_velocity_rows_updates_stress_row_k0(gpu):
    """nsdg_mevp_iterate(k0 = j0 - 1, j0 = j1) computes the stress rows [k0, j1) (include/nsdg.h): row k0 equals that row of a call
    on the whole array bit for bit, and neither another stress row nor any velocity is written -- in the two-kernel form and in the
    fused kernel"""
    nx, ny, k0 = 70, 12, 4
    gen = torch.Generator().manual_seed(11)
    rnd = lambda lo, hi, *shape: (lo + (hi - lo) * torch.rand(*shape, generator=gen, dtype=torch.float64)).cuda()
    c = abi.Context(gpu)
    c.set_grid(nx, ny, 1000.0, 1000.0)
    nodes = (2 * ny + 1, 2 * nx + 1)
    u, v = rnd(-0.1, 0.1, *nodes), rnd(-0.1, 0.1, *nodes)
    packed = z(8 * u.numel())
    c.mevp_pack_nodal(120.0, (u, v), (rnd(-0.1, 0.1, *nodes), rnd(-0.1, 0.1, *nodes)), (rnd(-0.1, 0.1, *nodes), rnd(-0.1, 0.1, *nodes)),
                      rnd(0.5, 1.5, *nodes), rnd(0.5, 1.0, *nodes), packed)
    s = [abi.tile(rnd(-1e3, 1e3, 8, ny, nx)) for _ in range(3)]
    pg = abi.tile(rnd(1e4, 3e4, 9, ny, nx))
    for variant in (0, 1):
        c.set_mevp_variant(variant)
        out = []
        for rows in ((0, 0, ny), (k0, k0 + 1, k0 + 1)):
            so, uvn = [torch.full_like(x, 7.0) for x in s], (torch.full_like(u, 7.0), torch.full_like(v, 7.0))
            c.mevp_iterate(*rows, s, so, (u, v), uvn, packed, pg)
            out.append((so, uvn))
        (full, _), (one, one_uv) = out
        for a, b in zip(full, one):
            assert not torch.all(a[k0] == 7.0) and torch.equal(b[k0], a[k0]), variant
            assert torch.all(b[:k0] == 7.0) and torch.all(b[k0 + 1:] == 7.0), variant
        assert all(torch.all(t == 7.0) for t in one_uv), variant
    c.close()

"""Sub-stepping of the model time step by the strength wave speed (include/nsdg.h "sub-stepping") on the device: the concentration
maximum against numpy, the cross-rank maximum of the local transport, the C++ host's dynamics.substeps byte for byte against runs that
take the short steps themselves, and the graph cache of the row-block plan across a change of the adaptive constants."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import torch

import substep_ref as R
from nextsimdg_amd import abi, build, rowblock, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fields(nx, ny, seed, dg0=False, spread=False):
    rng = np.random.default_rng(seed)
    H, A = np.zeros((6, ny, nx)), np.zeros((6, ny, nx))
    if spread:  # out of range on purpose: negative thickness, concentration above 1 and below 0
        H[0] = rng.uniform(-0.5, 1.0, (ny, nx))
        A[0] = rng.uniform(-0.3, 1.3, (ny, nx))
    else:
        H[0] = rng.uniform(0.05, 1.0, (ny, nx))
        A[0] = rng.uniform(0.3, 0.95, (ny, nx))
    if not dg0:
        H[1:] = 0.1 * rng.standard_normal((5, ny, nx))
        A[1:] = 0.05 * rng.standard_normal((5, ny, nx))
    return H, A


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,j0,j1,dg0,spread", [
    (37, 23, 3, 18, False, False),  # odd nx, a row range that is no multiple of 4
    (37, 23, 0, 23, True, True),
    (1, 1, 0, 1, False, False),
    (1, 1, 0, 1, True, True),
    (129, 67, 5, 62, False, True),
    (2048, 2048, 0, 2048, True, False),
    (2048, 2048, 0, 2048, False, True),
])
def test_concentration_max_matches_numpy(ctx, nx, ny, j0, j1, dg0, spread):
    H, A = fields(nx, ny, nx * 7 + ny, dg0, spread)
    ctx.set_grid(nx, ny, 250.0, 250.0)
    got = ctx.concentration_max(dev(H), dev(A), j0, j1)
    want = R.concentration_max(H, A, j0, j1)
    assert 0.0 <= want <= 1.0 and (want > 0.0 or nx == 1)
    if dg0:
        assert got == want
    else:
        assert abs(got - want) <= 1e-15 * want, (got, want)


@pytest.mark.gpu
def test_ghost_rows_do_not_count_and_blocks_agree_with_the_whole_grid(ctx):
    nx, ny = 203, 61
    H, A = fields(nx, ny, 3)
    A[1:] *= 0.1  # Gauss-point values below the clamp at 1: the blocks' maxima differ
    ctx.set_grid(nx, ny, 250.0, 250.0)
    dH, dA = dev(H), dev(A)
    whole = ctx.concentration_max(dH, dA)
    assert abs(whole - R.concentration_max(H, A)) <= 1e-15 * whole
    bounds = [rowblock.split_rows(ny, 4, r) for r in range(4)]
    parts = [ctx.concentration_max(dH, dA, r0, r1) for r0, r1 in bounds]
    assert max(parts) == whole and len(set(parts)) > 1
    # a full cover in the rows around [j0, j1): ghost rows of a block must not count, nor a NaN there
    j0, j1 = 9, 47
    G, B = H.copy(), A.copy()
    B[0, :j0] = B[0, j1:] = 1.0
    B[3, j1 + 1] = np.nan
    got = ctx.concentration_max(dev(G), dev(B), j0, j1)
    assert got < 0.99 and abs(got - R.concentration_max(H, A, j0, j1)) <= 1e-15 * got
    # no ice at all: 0; an empty row range: 0
    assert ctx.concentration_max(dev(np.zeros_like(H)), dA) == 0.0
    assert ctx.concentration_max(dH, dA, 5, 5) == 0.0


@pytest.mark.gpu
def test_non_finite_input_is_an_error_status(ctx):
    nx, ny = 37, 23
    ctx.set_grid(nx, ny, 250.0, 250.0)
    H, A = fields(nx, ny, 11)
    for name, plane, iy, ix, bad in (("A", 3, 7, 12, np.nan), ("H", 0, 20, 36, np.inf), ("A", 0, 0, 0, -np.inf),
                                     ("H", 5, 11, 2, np.nan)):
        G, B = H.copy(), A.copy()
        (G if name == "H" else B)[plane, iy, ix] = bad
        if name == "H" and plane == 5:
            G[:, iy, ix] = [-1.0, 0, 0, 0, 0, np.nan]  # a NaN where the clamped thickness is 0: the clamp must not hide it
        with pytest.raises(abi.NsdgError, match="non-finite H or A in element %d " % (iy * nx + ix)):
            ctx.concentration_max(dev(G), dev(B))
    # a NaN outside the rows asked for does not count
    B = A.copy()
    B[2, 20, 5] = np.nan
    assert ctx.concentration_max(dev(H), dev(B), 0, 20) == pytest.approx(R.concentration_max(H, A, 0, 20), rel=1e-15)
    # the context is usable after the error
    assert ctx.concentration_max(dev(H), dev(A)) > 0.0


@pytest.mark.gpu
def test_comm_max_on_the_local_transport(gpu):
    world, group = 4, 70_001
    ctxs = [abi.Context(gpu) for _ in range(world)]
    values = [0.25, 0.875, 0.5, 0.125]
    out = [None] * world
    errors = []

    def rank(r):
        try:
            ctxs[r].comm_deadline(60.0)
            ctxs[r].comm_init_local(group, r, world)
            out[r] = [ctxs[r].comm_max_f64(values[r]), ctxs[r].comm_max_f64(-values[r])]  # two reductions in a row
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    try:
        assert not errors, errors
        assert out == [[0.875, -0.125]] * world
    finally:
        for c in ctxs:
            c.comm_finalize()
            c.close()
    # without a communicator the value stays
    c = abi.Context(gpu)
    assert c.comm_max_f64(0.3) == 0.3
    c.close()


@pytest.mark.gpu
def test_graph_cache_follows_a_change_of_the_adaptive_constants(gpu):
    """a plan with use_graph = 1 run under uniform alpha, beta and then under adaptive_converged -- alpha, beta, Delta_min and dt
    unchanged, only aevp_c and aevp_alpha_min differ -- must not replay graphs recorded with the old constants: equal to a plan without
    graphs, bit for bit"""
    nx, ny, nsub, dt = 150, 64, 12, 120.0
    bt = synthetic.BoxTest(nx, ny, 16e3)
    H, A = (dev(x) for x in bt.dg_fields())
    uo, vo = (dev(x) for x in bt.ocean())
    ua, va = (dev(3.0 * x) for x in bt.wind(0.0))
    results = []
    for use_graph in (False, True):
        c = abi.Context(gpu)
        c.set_grid(nx, ny, bt.hx, bt.hy)
        z = lambda: torch.zeros(2 * ny + 1, 2 * nx + 1, dtype=torch.float64, device="cuda")
        s2 = ([c.private_zeros(8, ny, nx, "cuda") for _ in range(3)], [c.private_zeros(8, ny, nx, "cuda") for _ in range(3)])
        uv2 = ((z(), z()), (z(), z()))
        pg = c.private_zeros(9, ny, nx, "cuda")
        packed = torch.zeros(8 * uv2[0][0].numel(), dtype=torch.float64, device="cuda")
        c.ice_strength(H, A, pg)
        run, _, _ = c.rb_mevp(rowblock.RowBlock(nx, ny, 0, 1), (None, None), nsub, True, use_graph, s2, uv2, packed, pg)
        uniform = c.mevp_default_params()
        converged = abi.stable_mevp_params(c.mevp_default_params(), abi.SUBCYCLE_ADAPTIVE_CONVERGED, min(bt.hx, bt.hy), dt)
        assert converged.aevp_c > 0 and (converged.alpha, converged.beta, converged.delta_min) == (uniform.alpha, uniform.beta, uniform.delta_min)
        par = 0
        for p in (uniform, uniform, converged, converged):
            c.set_mevp_params(p)
            c.mevp_prepare(dt, H, A, (ua, va), (uo, vo), uv2[par], packed)
            par = run(par)
        torch.cuda.synchronize()
        results.append([x.clone() for x in list(s2[par]) + list(uv2[par])])
        del run
        c.close()
    assert float(results[0][3].abs().max()) > 1e-6
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ---- the C++ host -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(gpu):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build", "nextsim_amd")


def run_host(host, tmp, name, n, L, time_step, model="start = 0\nstop = 360\n", dynamics="", init="hice = 0.3\ncice = 0.9\n"):
    """runs nextsim_amd on an n x n box of side L; returns (restart file bytes, output)"""
    final = os.path.join(tmp, name + ".nsdg")
    cfg = os.path.join(tmp, name + ".cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %s\n%sfinal_file = %s\ntiming = true\n"
                "[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\nnsub = 16\n%s"
                % (time_step, model, final, n, n, init, L, dynamics))
    p = subprocess.run([host, "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    with open(final, "rb") as f:
        return f.read(), out


def chosen(out):
    return [int(n) for n in re.findall(r"dynamics substeps: t=\S+ s n=(\d+)", out)]


@pytest.mark.gpu
def test_host_two_substeps_equal_half_the_time_step(host, tmp_path):
    """substeps = 2 at time_step = 120 == substeps = 1 at time_step = 60 with twice the steps, byte for byte (thermodynamics on, winter
    forcing at the sub-step's model time)"""
    tmp = str(tmp_path)
    init = "hice = 0.3\ncice = 0.9\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"
    thermo = "thermodynamics = true\nforcing = winter\n"
    two, out = run_host(host, tmp, "two", 64, 128e3, 120, dynamics=thermo + "substeps = 2\n", init=init)
    assert "launches=3" in out  # three model steps
    half, _ = run_host(host, tmp, "half", 64, 128e3, 60, dynamics=thermo, init=init)
    assert two == half
    one, _ = run_host(host, tmp, "one", 64, 128e3, 120, dynamics=thermo, init=init)
    assert one != two


@pytest.mark.gpu
def test_host_auto_on_the_2km_box_is_the_unsplit_step(host, tmp_path):
    tmp = str(tmp_path)
    auto, out = run_host(host, tmp, "auto", 256, 512e3, 120, dynamics="substeps = auto\n")
    assert chosen(out) == [1], out
    plain, _ = run_host(host, tmp, "plain", 256, 512e3, 120)
    assert auto == plain


@pytest.mark.gpu
def test_host_auto_at_250m_blocks_graphs_and_restart(host, tmp_path):
    """250 m cells, A0 = 0.9, the converging sub-cycle: auto chooses n > 1; 1 block == 4 row blocks, graph = true == graph = false, and
    N steps == N / 2 + restart + N / 2, byte for byte"""
    tmp = str(tmp_path)
    dyn = "substeps = auto\nsubcycle = adaptive_converged\n"
    one, out = run_host(host, tmp, "one", 128, 32e3, 120, model="start = 0\nstop = 480\n", dynamics=dyn)
    ns = chosen(out)
    assert ns and ns[0] == 3 and min(ns) > 1, out  # c(0.9) dt / (1.5 h) = 2.006
    four, _ = run_host(host, tmp, "four", 128, 32e3, 120, model="start = 0\nstop = 480\n", dynamics=dyn + "row_blocks = 4\n")
    assert four == one
    graph, _ = run_host(host, tmp, "graph", 128, 32e3, 120, model="start = 0\nstop = 480\n", dynamics=dyn + "graph = true\n")
    assert graph == one
    half, _ = run_host(host, tmp, "half", 128, 32e3, 120, model="start = 0\nstop = 240\n", dynamics=dyn)
    resumed, _ = run_host(host, tmp, "resumed", 128, 32e3, 120, model="init_file = %s\nstart = 240\nstop = 480\n" % os.path.join(tmp, "half.nsdg"),
                          dynamics=dyn)
    assert resumed == one
    fixed, _ = run_host(host, tmp, "fixed", 128, 32e3, 120, model="start = 0\nstop = 480\n", dynamics="subcycle = adaptive_converged\n")
    assert fixed != one


@pytest.mark.gpu
def test_host_rejects_a_state_that_needs_more_than_max_substeps(host, tmp_path):
    p_cfg = os.path.join(str(tmp_path), "x.cfg")
    with open(p_cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 64\nny = 64\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\ndomain_size = 8e3\nnsub = 8\n"
                "substeps = auto\nmax_substeps = 4\n" % os.path.join(str(tmp_path), "x.nsdg"))
    p = subprocess.run([host, "--config-file", p_cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode != 0 and "n = 5" in out and "max_substeps = 4" in out, out

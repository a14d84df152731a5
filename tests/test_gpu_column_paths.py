"""The launch routes of nsdg_column_step (csrc/column_step.hip) that production takes -- diag == nullptr: the two-elements-per-lane
kernel with 16-byte accesses (X2), the scalar kernel from 2 * (n / 2) for an odd last element (TAIL), the scalar kernel over everything
when a plane is not 16-byte aligned (SCALAR, which is what the C++ host's block of an odd size gets) -- held to the reference's own
recording (tests/golden/ref_column_v1.npz) for all four module sets, at the sizes around the 512-element workgroup seam, between guard
words, and to each other.  Inputs and expectations: tests/column_path_cases.py (their conditions: tests/test_column_paths_cpu.py).

Against the recording the tolerance is that of test_gpu_parity.py::test_column_step_matches_reference_build (1e-11 relative + 1e-13,
newice + 1e-16, NaN / +Inf / -Inf class for class).  Between routes: == on finite values and the same non-finite classes, not bit
patterns (the build has -fno-signed-zeros, the sign of a zero may differ between instantiations).  -s prints the worst err / limit."""
import ctypes as C

import numpy as np
import pytest
import torch

import column_path_cases as P
import oracle_lib as O
from nextsimdg_amd import abi
from test_gpu_parity import RC, RC_META, RC_SETS, assert_close_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    from nextsimdg_amd import build

    build.build_lib(verbose=False)
    c = abi.Context(gpu)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _default_params_after_each_test(ctx):
    yield
    ctx.set_column_params(ctx.column_default_params())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def use_set(ctx, name):
    ctx.set_column_params(ctx.column_default_params(**O.ref_column_set_params(P.META, name)))


class Worst(dict):
    """worst err / limit per field over the finite entries of a test, printed when the test ends (also when it fails)"""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        print("worst err / limit: " + ", ".join("%s %.3f" % kv for kv in self.items()))

    def close_ref(self, got, want, rtol, atol, k, what):
        fin = np.isfinite(want) & np.isfinite(got)
        if fin.any():
            r = float(np.max(np.abs(got[fin] - want[fin]) / (atol + rtol * np.abs(want[fin]))))
            self[k] = max(self.get(k, 0.0), r)
        assert_close_ref(got, want, rtol, atol, "%s %s" % (what, k))

    def state(self, got, want, what):
        for k in P.OUT:
            self.close_ref(got[k], want[k], P.RTOL, P.ATOL[k], k, what)


def same(a, b):
    """== on finite values, the same NaN / +Inf / -Inf elsewhere"""
    fa, fb = np.isfinite(a), np.isfinite(b)
    return (np.array_equal(fa, fb) and np.array_equal(a[fa], b[fb]) and np.array_equal(np.isnan(a), np.isnan(b))
            and np.array_equal(np.isposinf(a), np.isposinf(b)))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


class Placed:
    """the planes of column_path_cases.placed() on the device: one allocation per plane, the plane a view into it"""

    def __init__(self, inputs, n, offset=2):
        self.n, self.inputs = n, inputs
        self.host = P.placed(inputs, n, P.GUARD, offset)
        self.buf = {k: dev(b) for k, (b, _) in self.host.items()}
        self.off = {k: off for k, (_, off) in self.host.items()}
        self.view = {k: self.buf[k][self.off[k]:self.off[k] + n] for k in P.PLANES}
        for k in P.PLANES:  # offset 2 keeps the allocation's alignment, offset 1 breaks it
            assert self.view[k].data_ptr() % 16 == (8 if self.off[k] % 2 else 0), k

    def step(self, ctx, diag=None):
        ctx.column_step(P.DT, {k: self.view[k] for k in P.STATE}, {k: self.view[k] for k in P.FORCING}, self.view["newice"], diag)
        torch.cuda.synchronize()
        return {k: host(self.view[k]) for k in P.OUT}

    def assert_untouched_outside(self):
        """guards on both sides of all 15 planes; the ten read-only planes bit for bit"""
        for k in P.PLANES:
            assert P.guards_intact(host(self.buf[k]), self.off[k], self.n), "guard of " + k
        for k in P.READ_ONLY:
            assert np.array_equal(bits(host(self.view[k])), bits(self.inputs[k])), "read-only plane " + k


_ALIGNED = {}


def aligned_run(ctx, name, n):
    """tiled(name, n) with every plane aligned (offset 2, guard 4), through the production entry: X2 (+ TAIL for odd n).  Computed once
    per (set, n) and left unchanged; ctx holds the set's parameters afterwards"""
    use_set(ctx, name)
    if (name, n) not in _ALIGNED:
        inputs, want, _ = P.tiled(name, n)
        d = Placed(inputs, n, 2)
        got = d.step(ctx)
        d.assert_untouched_outside()
        for v in got.values():
            v.setflags(write=False)
        _ALIGNED[name, n] = (got, want)
    return _ALIGNED[name, n]


# ---- 1. every recording through the production entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC_SETS)
def test_production_entry_matches_reference_build(ctx, name):
    """the loop of test_gpu_parity.py::test_column_step_matches_reference_build with diag = None: the random draw (n = 256), the edge
    grids (650) and the chains (32, re-synchronised from the recording before every step) through X2; after each call state and newice
    equal what the diagnostic kernel gives on the same inputs"""
    use_set(ctx, name)
    with Worst() as worst:
        for g in (x for x in RC_META["groups"] if x["set"] == name):
            key, ikey = "%s/%s/" % (name, g["group"]), g["inputs"] + "in/"
            nsteps = g["nsteps"]
            rec = RC.get(key + "out/record")
            for step in range(nsteps):
                if step == 0:
                    state = {k: RC[ikey + k] for k in abi.STATE}
                    newice = np.zeros(state["hice"].size)
                else:
                    state = {k: rec[step - 1][i] for i, k in enumerate(abi.STATE)}
                    newice = rec[step - 1][4]
                n = newice.size
                forcing = {k: RC[ikey + k][step] if nsteps > 1 else RC[ikey + k] for k in abi.FORCING}
                ds, df, dn = {k: dev(v) for k, v in state.items()}, {k: dev(v) for k, v in forcing.items()}, dev(newice)
                assert n % 2 == 0 and all(t.data_ptr() % 16 == 0 for t in list(ds.values()) + list(df.values()) + [dn])  # route X2
                ctx.column_step(g["dt"], ds, df, dn, None)
                if rec is not None:
                    want = {k: rec[step][i] for i, k in enumerate(abi.STATE + ["newice"])}
                else:
                    want = {k: RC[key + "out/" + k] for k in abi.STATE + ["newice"]}
                what = "%s step %d" % (key, step)
                got = dict({k: host(ds[k]) for k in abi.STATE}, newice=host(dn))
                worst.state(got, want, what)
                es, en = {k: dev(v) for k, v in state.items()}, dev(newice)
                ctx.column_step(g["dt"], es, df, en, torch.zeros(abi.NDIAG, n, dtype=torch.float64, device="cuda"))
                for k in abi.STATE:
                    assert same(got[k], host(es[k])), "%s %s: production and diagnostic kernel differ" % (what, k)
                assert same(got["newice"], host(en)), what + " newice: production and diagnostic kernel differ"
                for k in abi.FORCING:
                    assert np.array_equal(bits(host(df[k])), bits(forcing[k])), what + " read-only " + k


# ---- 2. the seams of X2 and TAIL ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.SEAM_SIZES)
@pytest.mark.parametrize("name", P.SETS)
def test_seams_match_the_recording_between_untouched_guards(ctx, name, n):
    """aligned planes between guards of 4: n = 1 is TAIL alone, even n X2 alone, odd n X2 + TAIL; one X2 workgroup covers 512 elements.
    The seam elements are live, change again under a second step and differ within their pairs (tests/test_column_paths_cpu.py)"""
    got, want = aligned_run(ctx, name, n)
    with Worst() as worst:
        worst.state(got, want, "%s n = %d" % (name, n))


# ---- 3. alignment: SCALAR ----------------------------------------------------------------------------------------------------------------
BROKEN = [("hice",), ("tice0",), ("sst",), ("wind",), ("newice",), tuple(P.PLANES)]


@pytest.mark.parametrize("broken", BROKEN, ids=lambda b: b[0] if len(b) == 1 else "all15")
@pytest.mark.parametrize("n", [2, 513, 1024])
@pytest.mark.parametrize("name", ["all_params", "default"])
def test_one_misaligned_plane_takes_the_scalar_route_to_the_same_result(ctx, name, n, broken):
    """one plane 8 bytes off (the first, tice0, the first and the last read-only one, the last), then all 15: the scalar kernel over all
    n gives what the aligned run gives, and the recording.  Guards of 4 around a plane at offset 1: a 16-byte access issued on the
    broken plane, or past the end of an aligned one, would reach them"""
    aligned, want = aligned_run(ctx, name, n)
    inputs, _, _ = P.tiled(name, n)
    d = Placed(inputs, n, {k: 1 for k in broken})
    assert all(d.off[k] == (1 if k in broken else 2) for k in P.PLANES)
    got = d.step(ctx)
    d.assert_untouched_outside()
    for k in P.OUT:
        assert same(got[k], aligned[k]), "%s n = %d, %s misaligned: %s differs from the aligned run" % (name, n, broken, k)
    with Worst() as worst:
        worst.state(got, want, "%s n = %d scalar" % (name, n))


# ---- 4. the C++ host's block ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.HOST_SIZES)
@pytest.mark.parametrize("name", P.SETS)
def test_host_block_layout_matches_the_recording(ctx, name, n):
    """HipStep.cpp's call: one allocation, plane k at k n, the 15 pointers straight into nsdg_column_step, diag = nullptr.  n = 99: every
    odd plane is 8 bytes off, so SCALAR; n = 100 (host_tests.cpp's size): X2"""
    use_set(ctx, name)
    inputs, want, _ = P.tiled(name, n)
    hbuf, starts = P.host_block(inputs, n)
    buf = dev(hbuf)
    base = buf.data_ptr()
    assert base % 16 == 0
    ptrs = [base + 8 * s for s in starts]
    assert [p % 16 for p in ptrs] == [8 if (n % 2 and k % 2) else 0 for k in range(15)]
    ctx._call(ctx.lib.nsdg_column_step(ctx.h, n, P.DT, *[C.c_void_p(p) for p in ptrs], None))
    torch.cuda.synchronize()
    after = host(buf)
    plane = {k: after[s:s + n] for k, s in zip(P.PLANES, starts)}
    assert np.all(after[:P.GUARD] == P.SENTINEL) and np.all(after[-P.GUARD:] == P.SENTINEL), "guards of the block"
    for k in P.READ_ONLY:
        assert np.array_equal(bits(plane[k]), bits(inputs[k])), "read-only plane " + k
    with Worst() as worst:
        worst.state(plane, want, "%s host block n = %d" % (name, n))


# ---- 5. the diagnostic kernel at its own seams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.DIAG_SIZES)
@pytest.mark.parametrize("name", P.SETS)
def test_diagnostic_kernel_at_its_seams_and_against_production(ctx, name, n):
    """column_step_kernel<true> with 256 elements per workgroup: state, newice and the 15 diagnostics against the recording (diagnostics
    at the tolerance of test_column_step_matches_reference_build: 1e-11 relative + 1e-13 of the plane's largest expected value), diag a
    view between guards -- plane k is written at k n + e --, and the production routes on the same inputs (X2, + TAIL for odd n) give
    the same state"""
    use_set(ctx, name)
    inputs, want, want_diag = P.tiled(name, n)
    d = Placed(inputs, n, 2)
    dbuf = torch.full((abi.NDIAG * n + 2 * P.GUARD,), P.SENTINEL, dtype=torch.float64, device="cuda")
    got = d.step(ctx, dbuf[P.GUARD:P.GUARD + abi.NDIAG * n])
    d.assert_untouched_outside()
    hd = host(dbuf)
    assert P.guards_intact(hd, P.GUARD, abi.NDIAG * n), "guards of diag"
    gd = hd[P.GUARD:P.GUARD + abi.NDIAG * n].reshape(abi.NDIAG, n)
    with Worst() as worst:
        worst.state(got, want, "%s n = %d diag kernel" % (name, n))
        for i, k in enumerate(abi.DIAG):
            assert np.all(np.isfinite(want_diag[i]))
            worst.close_ref(gd[i], want_diag[i], 1e-11, 1e-13 * np.max(np.abs(want_diag[i])) + 1e-300, "diag " + k, "%s n = %d" % (name, n))
    prod = Placed(inputs, n, 2)
    pgot = prod.step(ctx)
    prod.assert_untouched_outside()
    for k in P.OUT:
        assert same(pgot[k], got[k]), "%s n = %d %s: production and diagnostic kernel differ" % (name, n, k)


# ---- 6. the wrapper ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["hice", "cice", "tice0", "sst", "wind", "newice", "diag", "diag_for_n_minus_1"])
def test_wrapper_refuses_planes_of_another_length_before_the_launch(ctx, short):
    """abi.Context.column_step takes n from hice; the C ABI sees pointers only.  A plane one element short, or a diag that is not
    NDIAG * n, raises NsdgError and nothing is launched: the live inputs (every seam element changes under a step) are unchanged"""
    n = 3
    inputs, _, _ = P.tiled("default", n)
    t = {k: dev(v) for k, v in inputs.items()}
    diag = None
    if short == "diag":
        diag = torch.zeros(abi.NDIAG * n - 1, dtype=torch.float64, device="cuda")
    elif short == "diag_for_n_minus_1":
        diag = torch.zeros(abi.NDIAG, n - 1, dtype=torch.float64, device="cuda")
    else:
        t[short] = t[short][:n - 1].clone()
    with pytest.raises(abi.NsdgError, match="column_step"):
        ctx.column_step(P.DT, {k: t[k] for k in P.STATE}, {k: t[k] for k in P.FORCING}, t["newice"], diag)
    torch.cuda.synchronize()
    for k in P.PLANES:
        assert np.array_equal(bits(host(t[k])), bits(inputs[k][:t[k].numel()])), k
    # the same tensors at full length go through
    t[short if short in t else "hice"] = dev(inputs[short if short in inputs else "hice"])
    ctx.column_step(P.DT, {k: t[k] for k in P.STATE}, {k: t[k] for k in P.FORCING}, t["newice"],
                    None if diag is None else torch.zeros(abi.NDIAG, n, dtype=torch.float64, device="cuda"))
    assert not np.array_equal(host(t["hice"]), inputs["hice"])

"""Inputs for the launch routes of nsdg_column_step (csrc/column_step.hip): two elements per lane with 16-byte accesses for the even
part of aligned planes (X2), the scalar kernel from 2 * (n / 2) for an odd last element (TAIL), the scalar kernel over everything when
one plane is not 16-byte aligned (SCALAR), and the scalar kernel with diagnostics.  The column step is element-local, so every expected
value is the reference's own recording (tests/golden/ref_column_v1.npz, group `random`: 256 elements per module set, dt = 600 s, newice
0 on entry) taken by index: no oracle run stands between the recording and the device.  numpy only; the conditions the cases must hold
are asserted in tests/test_column_paths_cpu.py, the device runs them in tests/test_gpu_column_paths.py."""
import numpy as np

import oracle_lib as O

META, RC = O.ref_column_fixture()
SETS = list(META["sets"])
STATE, FORCING = list(O.STATE), list(O.FORCING)
OUT = STATE + ["newice"]  # what a step writes
PLANES = STATE + FORCING + ["newice"]  # the argument order of nsdg_column_step and the plane order of the C++ host (HipStep.cpp)
READ_ONLY = FORCING  # sst, sss and the forcing proper
NRANDOM = RC["random/in/hice"].size
DT = next(g["dt"] for g in META["groups"] if g["group"] == "random")
SENTINEL = -7.0  # finite: a guard that is read by mistake does not hide behind a NaN
GUARD = 4

# the tolerance of test_gpu_parity.py::test_column_step_matches_reference_build
RTOL = 1e-11
ATOL = {"hice": 1e-13, "cice": 1e-13, "hsnow": 1e-13, "tice0": 1e-13, "newice": 1e-16}
MARGIN = 100.0  # conditions (a) and (b): a skipped or twice-stepped element misses the limit by this factor at least

# one X2 workgroup covers 512 elements: a partial workgroup, a full one, one pair into the next, and a tail after each; 650 is the size
# of the recording's own edge groups
SEAM_SIZES = (1, 2, 3, 511, 512, 513, 514, 650, 1023, 1024, 1025)
HOST_SIZES = (99, 100)  # the C++ host's block: odd (every odd plane misaligned) and even (what host_tests.cpp runs)
DIAG_SIZES = (1, 255, 256, 257)  # the diagnostic kernel's workgroup is 256 elements

# Start of the cyclic repetition of the 256 recorded elements.  Chosen (tests/test_column_paths_cpu.py holds it to that) so that the
# conditions (a), (b), (c) of seam_conditions() hold for every module set at every n of SEAM_SIZES, HOST_SIZES and DIAG_SIZES (29 of the
# 256 offsets do at SEAM_SIZES; 83 is one that does at the other sizes too, with every margin above 1e7).
OFFSET = 83  # one offset serves every size: no size has one of its own, no seam element is exempt


def index(n, offset=None):
    return (np.arange(n) + (OFFSET if offset is None else offset)) % NRANDOM


def tiled(name, n, offset=None):
    """(inputs, expected, expected diagnostics) for n elements of module set `name`: inputs has the 15 PLANES, expected the five OUT
    planes, the diagnostics are [15, n]; element e is recorded element (offset + e) mod 256"""
    i = index(n, offset)
    inputs = {k: np.ascontiguousarray(RC["random/in/" + k][i]) for k in STATE + FORCING}
    inputs["newice"] = np.zeros(n)
    key = "%s/random/out/" % name
    want = {k: np.ascontiguousarray(RC[key + k][i]) for k in OUT}
    return inputs, want, np.ascontiguousarray(RC[key + "diag"][:, i])


def limit(k, want):
    return ATOL[k] + RTOL * np.abs(want)


def seam_elements(n):
    """first element, last element of the X2 part, the TAIL element, last element"""
    even = 2 * (n // 2)
    return sorted({0, n - 1} | ({even - 1} if even else set()) | ({even} if n % 2 else set()))


def seam_pairs(n):
    """the first and the last lane of X2, and the last X2 element with the TAIL element"""
    even = 2 * (n // 2)
    pairs = {(0, 1), (even - 2, even - 1)} if even else set()
    if even and n % 2:
        pairs.add((even - 1, even))
    return sorted(pairs)


def twice(name, inputs, want):
    """the oracle applied to the expected state once more, under the same forcing: what an element stepped twice would hold"""
    state = {k: want[k].copy() for k in STATE}
    newice = want["newice"].copy()
    O.column_step(O.column_params(**O.ref_column_set_params(META, name)), DT, state, {k: inputs[k] for k in FORCING}, newice)
    return dict(state, newice=newice)


def seam_conditions(name, n, offset=None):
    """margins of the conditions at the seam elements of n, each to be > 1 (0 where an element is not finite):
    (a) max over the OUT planes of |expected - input| / (MARGIN * limit), min over the seam elements: a skipped element fails;
    (b) the same for |second application - expected|: an element stepped twice fails;
    (c) min over the seam pairs and the STATE planes of |expected[x] - expected[y]| / (MARGIN * limit), and 0 unless input[x] != input[y]
        in all 14 drawn planes: a swap of the halves of a lane fails in whichever plane it happens"""
    inputs, want, _ = tiled(name, n, offset)
    again = twice(name, inputs, want)
    es = seam_elements(n)
    finite = all(np.all(np.isfinite(v[es])) for v in list(want.values()) + list(again.values()))
    a = min(max(abs(want[k][e] - inputs[k][e]) / (MARGIN * limit(k, want[k][e])) for k in OUT) for e in es)
    b = min(max(abs(again[k][e] - want[k][e]) / (MARGIN * limit(k, want[k][e])) for k in OUT) for e in es)
    c = np.inf
    for x, y in seam_pairs(n):
        for k in STATE:
            c = min(c, abs(want[k][x] - want[k][y]) / (MARGIN * max(limit(k, want[k][x]), limit(k, want[k][y]))))
        for k in STATE + FORCING:
            c = min(c, 1e300 if inputs[k][x] != inputs[k][y] else 0.0)
    return (float(a), float(b), float(c)) if finite else (0.0, 0.0, 0.0)


# ---- where the planes lie ---------------------------------------------------------------------------------------------------------------
def placed(arrays, n, guard=GUARD, offset=2):
    """every plane of `arrays` in a buffer of its own of n + 2 * guard doubles filled with SENTINEL, at `offset` elements from its start
    (one int, or a dict per plane with 2 for those it does not name).  Device allocations are 16-byte aligned, so offset 2 keeps a plane
    aligned and offset 1 breaks it.  Returns {plane: (buffer, offset)}; the plane is buffer[offset:offset + n]"""
    out = {}
    for k, v in arrays.items():
        off = offset.get(k, 2) if isinstance(offset, dict) else offset
        assert v.shape == (n,) and 0 <= off <= 2 * guard
        buf = np.full(n + 2 * guard, SENTINEL)
        buf[off:off + n] = v
        out[k] = (buf, off)
    return out


def guards_intact(buf, off, n):
    """everything outside buffer[off:off + n] still holds SENTINEL"""
    return bool(np.all(buf[:off] == SENTINEL) and np.all(buf[off + n:] == SENTINEL))


def host_block(arrays, n, guard=GUARD):
    """the C++ host's layout (HipStep.cpp): ONE allocation of 15 n doubles, plane k of PLANES at k n -- here between two guards of
    SENTINEL (an even guard keeps the block's own alignment).  For an odd n every odd plane starts 8 bytes off a 16-byte boundary.
    Returns (buffer, [start of each plane])"""
    assert guard % 2 == 0
    buf = np.full(len(PLANES) * n + 2 * guard, SENTINEL)
    starts = [guard + k * n for k in range(len(PLANES))]
    for k, s in zip(PLANES, starts):
        assert arrays[k].shape == (n,)
        buf[s:s + n] = arrays[k]
    return buf, starts

"""The inputs of tests/test_gpu_column_paths.py (tests/column_path_cases.py) on the CPU: the seam elements of every size are live, change
again under a second step and differ within their pairs, so that a skipped, a twice-stepped or a swapped element cannot pass; the indexing
of the expected values is what the oracle computes from the indexed inputs; and the C++ host's block puts its planes where the device
tests say it does."""
import numpy as np
import pytest

import column_path_cases as P
import oracle_lib as O

SIZES = sorted(set(P.SEAM_SIZES + P.HOST_SIZES + P.DIAG_SIZES))


def test_sizes_are_the_seams_of_the_launch():
    assert P.SEAM_SIZES == (1, 2, 3, 511, 512, 513, 514, 650, 1023, 1024, 1025) and P.NRANDOM == 256 and P.DT == 600.0
    assert P.seam_elements(1) == [0] and P.seam_pairs(1) == []  # TAIL alone
    assert P.seam_elements(2) == [0, 1] and P.seam_pairs(2) == [(0, 1)]
    assert P.seam_elements(3) == [0, 1, 2] and P.seam_pairs(3) == [(0, 1), (1, 2)]
    assert P.seam_elements(513) == [0, 511, 512] and P.seam_pairs(513) == [(0, 1), (510, 511), (511, 512)]
    assert P.seam_elements(1024) == [0, 1023] and P.seam_pairs(1024) == [(0, 1), (1022, 1023)]


@pytest.mark.parametrize("name", P.SETS)
def test_seam_elements_are_live_change_again_and_differ_within_their_pair(name):
    """conditions (a), (b), (c) of column_path_cases.seam_conditions at every size a device test runs, no seam element left out; (b) by two
    applications of the oracle (the recording is the first)"""
    worst = [np.inf] * 3
    for n in SIZES:
        m = P.seam_conditions(name, n)
        assert min(m) > 1.0, (name, n, m)
        worst = [min(w, x) for w, x in zip(worst, m)]
    print("%s: smallest margin over %d sizes (a) %.3g (b) %.3g (c) %.3g, each in units of %g x the comparison limit"
          % (name, len(SIZES), worst[0], worst[1], worst[2], P.MARGIN))


@pytest.mark.parametrize("name", P.SETS)
def test_oracle_reproduces_the_tiled_expectation(name):
    """the oracle on tiled() inputs gives tiled() expectations, state, newice and diagnostics, at the device tolerance (in fact bit for
    bit: tests/test_oracle_column.py): expected values and inputs are indexed alike"""
    params = O.column_params(**O.ref_column_set_params(P.META, name))
    for n in SIZES:
        inputs, want, want_diag = P.tiled(name, n)
        assert all(inputs[k].shape == (n,) for k in P.PLANES) and want_diag.shape == (len(O.DIAG), n)
        state, newice = {k: inputs[k].copy() for k in P.STATE}, inputs["newice"].copy()
        diag = O.column_step(params, P.DT, state, {k: inputs[k] for k in P.FORCING}, newice, want_diag=True)
        got = dict(state, newice=newice)
        for k in P.OUT:
            assert np.all(np.isfinite(want[k])) and np.all(np.abs(got[k] - want[k]) <= P.limit(k, want[k])), (name, n, k)
        for i, k in enumerate(O.DIAG):
            assert np.array_equal(diag[k], want_diag[i]), (name, n, k)
    # the repetition is cyclic from OFFSET: element e is recorded element (OFFSET + e) mod 256
    inputs, want, _ = P.tiled(name, 600)
    assert inputs["hice"][0] == P.RC["random/in/hice"][P.OFFSET] and want["tice0"][256 + 7] == want["tice0"][7]


def test_placed_planes_sit_between_untouched_guards():
    inputs, _, _ = P.tiled("default", 513)
    pl = P.placed(inputs, 513, P.GUARD, {"hice": 1, "wind": 1})
    assert set(pl) == set(P.PLANES)
    for k, (buf, off) in pl.items():
        assert off == (1 if k in ("hice", "wind") else 2) and buf.size == 513 + 2 * P.GUARD
        assert np.array_equal(buf[off:off + 513], inputs[k]) and P.guards_intact(buf, off, 513)
        assert not np.any(inputs[k] == P.SENTINEL)
        buf[off + 513] = 0.0
        assert not P.guards_intact(buf, off, 513)


@pytest.mark.parametrize("n", P.HOST_SIZES)
def test_host_block_misaligns_every_odd_plane_of_an_odd_size(n):
    """HipStep.cpp's planes at d_block + k n: 8 bytes off a 16-byte boundary for every odd k when n is odd (so the whole call takes the
    scalar route), none when n is even"""
    inputs, _, _ = P.tiled("default", n)
    buf, starts = P.host_block(inputs, n)
    assert buf.size == 15 * n + 2 * P.GUARD and starts == [P.GUARD + k * n for k in range(15)]
    for k, (name, s) in enumerate(zip(P.PLANES, starts)):
        assert np.array_equal(buf[s:s + n], inputs[name])
        assert (8 * s) % 16 == (8 if (n % 2 and k % 2) else 0), (n, k)
    assert np.all(buf[:P.GUARD] == P.SENTINEL) and np.all(buf[-P.GUARD:] == P.SENTINEL)

"""Per-phase device timing (include/nsdg.h "per-phase device timing"), the part that needs no device: the three entry points refuse a null
context by name, the host's timer prints device-time nodes in the tree's line format with shares taken from device times
(host/test/timer_tests.cpp, a program of its own), the phase mode installs no synchronisation hook, and the Python driver asks nothing new
of an `ops` object unless phase_timing is on -- and then refuses one without the phase calls."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from nextsimdg_amd import abi, build, rowblock, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")


@pytest.fixture(scope="module")
def lib():
    build.build_lib(verbose=False)
    return abi.load_library()


@pytest.fixture(scope="module")
def host_build():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_null_context_is_an_argument_error_that_names_the_function(lib):
    table = abi.PhaseTable()
    for name, call in (("nsdg_phase_timing_set", lambda: lib.nsdg_phase_timing_set(None, 1)),
                       ("nsdg_phase_mark", lambda: lib.nsdg_phase_mark(None, 0)),
                       ("nsdg_phase_mark", lambda: lib.nsdg_phase_mark(None, abi.PHASE_END)),
                       ("nsdg_phase_times", lambda: lib.nsdg_phase_times(None, C.byref(table), 0)),
                       ("nsdg_phase_times", lambda: lib.nsdg_phase_times(None, None, 1))):
        assert call() == -1, name  # NSDG_ERR_ARG
        assert name in lib.nsdg_last_error().decode(), (name, lib.nsdg_last_error())


def test_python_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "nsdg.h")).read()
    ids = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"NSDG_PHASE_([A-Z]+) = (-?\d+)", src))
    assert [ids[n.replace("-", "").upper()] for n in abi.PHASES] == list(range(len(abi.PHASES)))
    assert (ids["MAX"], ids["END"]) == (abi.PHASE_MAX, abi.PHASE_END)
    assert int(re.search(r"#define NSDG_PHASE_RING (\d+)", src).group(1)) == abi.PHASE_RING
    assert (rowblock.PHASE_FORCING, rowblock.PHASE_COLUMN, rowblock.PHASE_PREPARE, rowblock.PHASE_SUBCYCLE, rowblock.PHASE_TRANSPORT,
            rowblock.PHASE_REDUCTION, rowblock.PHASE_END) == tuple(ids[n] for n in ("FORCING", "COLUMN", "PREPARE", "SUBCYCLE", "TRANSPORT",
                                                                                   "REDUCTION", "END"))
    assert C.sizeof(abi.PhaseTable) == 8 * (2 * abi.PHASE_MAX + 2)


def test_timer_tests_program(host_build):
    """Timer with device-time nodes on synthetic numbers: line format, share of the parent from device times, children in first-mark
    order, tock() without a hook, PhaseTiming's tree (slowest block per phase) and JSON"""
    p = subprocess.run([os.path.join(host_build, "timer_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert re.search(r"timer tests: \d+ checks, 0 failures", out), out


def test_phase_mode_installs_no_sync_hook():
    """main.cpp hangs the device synchronisation on tock() for model.timing alone; model.phase_timing prints the tree without one"""
    src = open(os.path.join(HOST, "src", "main.cpp")).read()
    hooks = re.findall(r"if \(([^)]*)\)[^\n]*\n\s*Timer::main\.setDeviceSync", src)
    assert hooks == ["timing"], hooks
    assert src.count("setDeviceSync") == 1
    assert re.search(r"if \(timing \|\| phaseTiming\)\s*\n\s*Timer::main\.report", src)
    for f in ("DynamicsStep.cpp", "HipStep.cpp", "PhaseTiming.cpp"):  # ... and no step sets one either
        assert "setDeviceSync" not in open(os.path.join(HOST, "src", f)).read(), f


def oracle_core(cls=rowblock.DynamicsCore, **kw):
    from oracle_ops import OracleOps

    nx, ny = 12, 10
    bt = synthetic.BoxTest(nx, ny)
    return cls(OracleOps(mevp_variant=1, alpha=200.0, beta=200.0), rowblock.RowBlock(nx, ny), bt.hx, bt.hy, 120.0, 4, torch.device("cpu"), **kw), bt


def test_ops_without_the_phase_calls():
    """phase_timing=True needs the C ABI's phase calls: an ops object without them (the oracle's) is refused at construction; with False
    nothing new is asked of it -- the step runs, and no attribute of the phase calls is ever looked up"""
    from oracle_ops import OracleOps

    assert not hasattr(OracleOps, "phase_mark")
    for cls in (rowblock.DynamicsCore, rowblock.CoupledCore):
        with pytest.raises(ValueError, match="phase_timing"):
            oracle_core(cls, phase_timing=True)
    core, bt = oracle_core(phase_timing=False)
    H, A = bt.dg_fields()
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    core.load_global(H, A, uo, vo, 3.0 * ua, 3.0 * va)
    core.step()
    assert float(core.u.abs().max()) > 0
    with pytest.raises(ValueError, match="phase_timing=True"):
        core.phase_times()

"""Per-phase device timing (include/nsdg.h "per-phase device timing") on the device: the ABI on known work, the sum rule, off is off,
nothing is lost when the ring runs full, reset; the C++ hosts -- the run with model.phase_timing is the same run, byte for byte, and its
tree and JSON hold exactly the phases the step ran -- and the Python driver.

THE SUM RULE.  The phases of a span share their boundary events, and the span's total comes from its own pair (first mark, end mark), so
sum(ms of the phases) and total_ms are two sums over the same timestamps.  hipEventElapsedTime returns float milliseconds computed from
the difference of two integer timestamps (a conversion of the difference to float and a division by 1e6f: two roundings of at most
2^-24 each, 2^-23 per call), so the two sums may differ by (intervals + spans) * 2^-23 * total_ms.
IS THE CONVERSION ADDITIVE?  Yes, found on the first run on the MI355X: 200 adjacent intervals of torch events (the same
hipEventElapsedTime) came back as whole nanoseconds -- multiples of 40 ns, now and then + 1 ns from the tick -> ns conversion of the
timestamps themselves -- and their sum met elapsed(first, last) to 3.6e-8 ms of 1.87 ms (float bound: 4.5e-5 ms).  Differences of integer
timestamps add exactly, so the bound carries NO tick term (SUM_RULE_TICK_MS = 0).  Measured |sum - total| here: 3e-8 ms of 1.1 ms (2
intervals), 3e-9 of 8.6 ms (1098 intervals, 183 spans), 1e-6 ... 5e-6 of 102 ms and 3e-5 of 158 ms (hosts, 50 and 310 intervals): all within
a twentieth of the bound.

No measured number goes into an assert except through that bound and through orderings of work that differs by construction."""
import filecmp
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nextsimdg_amd import abi, build, rowblock, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")

# One tick of the event clock per interval would be added if the runtime's tick -> ms conversion were not additive over adjacent
# intervals.  It is additive (module docstring): no tick term.
SUM_RULE_TICK_MS = 0.0


def sum_rule(phases, total_ms, spans):
    """(difference, bound) of the sum rule for {name: (ms, count)}"""
    n = sum(c for _, c in phases.values())
    s = sum(ms for ms, _ in phases.values())
    bound = (n + spans) * 2.0 ** -23 * total_ms + n * SUM_RULE_TICK_MS
    print("sum rule: sum(phases) = %.9f ms, total = %.9f ms, difference = %.3e ms, bound = %.3e ms (%d intervals, %d spans)"
          % (s, total_ms, s - total_ms, bound, n, spans))
    return abs(s - total_ms), bound


@pytest.fixture()
def ctx(gpu):
    c = abi.Context(gpu)
    yield c
    c.close()


def test_known_work(ctx):
    """phase 0 = k copies of 256 MB, phase 1 = 4 k of the same: counts 1 and 1, both times positive, phase 1 longer (an ordering of work
    that differs fourfold by construction), one span -- and the sum rule.  An interval is device time BETWEEN two marks, idle time included:
    the marks are therefore issued behind some 10 ms of queued copies, so that the host has enqueued the whole sequence while the device is
    still busy and neither interval contains a wait for the host (the first launch of a kernel loads its code object: 0.5 ms)"""
    n = 32 * 1024 * 1024
    a, b = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.ones(n, dtype=torch.float64, device="cuda")
    ctx.phase_timing(True)
    k = 4
    for _ in range(60):
        ctx.copy_f64(a, b)
    ctx.phase_mark(0)
    for _ in range(k):
        ctx.copy_f64(a, b)
    ctx.phase_mark(1)
    for _ in range(4 * k):
        ctx.copy_f64(a, b)
    ctx.phase_mark(abi.PHASE_END)
    phases, (total, spans) = ctx.phase_times()
    print(phases, total, spans)
    assert sorted(phases) == [0, 1]
    assert phases[0][1] == 1 and phases[1][1] == 1
    assert phases[0][0] > 0 and phases[1][0] > 0
    assert phases[1][0] > phases[0][0]
    assert spans == 1 and total > 0
    diff, bound = sum_rule(phases, total, spans)
    assert diff <= bound
    # reading again changes nothing; reading with reset, then again, gives zeros
    assert ctx.phase_times() == (phases, (total, spans))
    assert ctx.phase_times(reset=True) == (phases, (total, spans))
    assert ctx.phase_times() == ({}, (0.0, 0))


def test_off_is_off(ctx):
    a, b = torch.zeros(4096, dtype=torch.float64, device="cuda"), torch.ones(4096, dtype=torch.float64, device="cuda")
    for phase in (0, 3, abi.PHASE_MAX - 1, abi.PHASE_END):  # a new context is off: the marks are accepted and do nothing
        ctx.phase_mark(phase)
        ctx.copy_f64(a, b)
    assert ctx.phase_times() == ({}, (0.0, 0))
    # turned on, marked, turned off: what was pending is discarded
    ctx.phase_timing(True)
    ctx.phase_mark(2)
    ctx.copy_f64(a, b)
    ctx.phase_mark(abi.PHASE_END)
    ctx.phase_timing(False)
    assert ctx.phase_times() == ({}, (0.0, 0))
    ctx.phase_mark(1)
    assert ctx.phase_times() == ({}, (0.0, 0))
    # and on again starts from nothing
    ctx.phase_timing(True)
    ctx.phase_mark(4)
    ctx.copy_f64(a, b)
    ctx.phase_mark(abi.PHASE_END)
    phases, (total, spans) = ctx.phase_times()
    assert list(phases) == [4] and phases[4][1] == 1 and spans == 1


def test_arguments_and_capture(ctx):
    lib = ctx.lib
    ctx.phase_timing(True)
    for bad in (abi.PHASE_MAX, abi.PHASE_MAX + 7, -2):
        assert lib.nsdg_phase_mark(ctx.h, bad) == -1 and b"nsdg_phase_mark" in lib.nsdg_last_error()
    assert lib.nsdg_phase_times(ctx.h, None, 0) == -1 and b"nsdg_phase_times" in lib.nsdg_last_error()
    assert ctx.phase_times() == ({}, (0.0, 0))
    ctx.phase_mark(abi.PHASE_END)  # nothing runs: nothing to close, no event
    assert ctx.phase_times() == ({}, (0.0, 0))


def test_mark_on_a_capturing_stream_is_refused(gpu):
    """an event query inside a capture would invalidate it: the mark tests hipStreamIsCapturing first and returns NSDG_ERR_STATE; the
    capture itself stays valid and replays"""
    s = torch.cuda.Stream()
    a, b = torch.zeros(4096, dtype=torch.float64, device="cuda"), torch.ones(4096, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        c = abi.Context(gpu, stream=s)
        c.phase_timing(True)
        c.phase_mark(0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc = c.lib.nsdg_phase_mark(c.h, 1)
            err = c.lib.nsdg_last_error()
            c.copy_f64(a, b)
        assert rc == -3 and b"captured" in err, (rc, err)  # NSDG_ERR_STATE
        g.replay()
        c.phase_mark(abi.PHASE_END)
        phases, (total, spans) = c.phase_times()
        assert list(phases) == [0] and phases[0][1] == 1 and spans == 1
        s.synchronize()
        assert bool((a == 1).all())
        c.close()


def test_nothing_is_lost_when_the_ring_runs_full(ctx):
    """five times the ring's capacity in marks, issued behind ~100 ms of queued copies so that the host is a full ring ahead of the device
    and a mark has to wait for the oldest one: every count and the number of spans are exact, and the sum rule holds"""
    n = 32 * 1024 * 1024
    big_a, big_b = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.ones(n, dtype=torch.float64, device="cuda")
    a, b = torch.zeros(4096, dtype=torch.float64, device="cuda"), torch.ones(4096, dtype=torch.float64, device="cuda")
    ctx.phase_timing(True)
    for _ in range(1000):  # 1000 x 0.5 GB of traffic: far longer than the loop below takes the host
        ctx.copy_f64(big_a, big_b)
    marks = 5 * abi.PHASE_RING
    expect, spans, running = {}, 0, None
    for i in range(marks):
        phase = abi.PHASE_END if i % 7 == 6 else (i * 5) % 6
        if running is not None:
            expect[running] = expect.get(running, 0) + 1
        if phase == abi.PHASE_END:
            spans += running is not None
            running = None
        else:
            running = phase
        ctx.phase_mark(phase)
        ctx.copy_f64(a, b)
    if running is not None:  # close the last span
        expect[running] = expect.get(running, 0) + 1
        spans += 1
        ctx.phase_mark(abi.PHASE_END)
    phases, (total, got_spans) = ctx.phase_times()
    assert {k: c for k, (_, c) in phases.items()} == expect
    assert got_spans == spans
    assert all(ms > 0 for ms, _ in phases.values()) and total > 0
    diff, bound = sum_rule(phases, total, got_spans)
    assert diff <= bound
    assert ctx.phase_times(reset=True)[1] == (total, spans)
    assert ctx.phase_times() == ({}, (0.0, 0))


# ---- the C++ hosts --------------------------------------------------------------------------------------------------------------------
STEPS, DT, N = 10, 120, 512
INIT = "hice = 0.3\ncice = %s\nsst = -1.76\nhsnow = 0.05\ntice = -8\n"
THERMO = "thermodynamics = true\nforcing = winter\n"
# name -> (domain size, initial concentration, extra [dynamics] keys)
CASES = {
    "one": (512e3, "0.9", "row_blocks = 1\n"),
    "four_graph": (512e3, "0.9", "row_blocks = 4\ngraph = true\n"),
    "auto": (N * 250.0, "1.0", "substeps = auto\n"),  # A = 1 on 250 m cells, dt = 120 s: n > 1 (checked below on the CPU)
}


def run_host(exe, tmp, name, phase_timing):
    L, conc, dyn = CASES[name]
    tag = name + ("_on" if phase_timing else "_off")
    final, js, cfg = (os.path.join(tmp, tag + ext) for ext in (".nsdg", ".json", ".cfg"))
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\nstart = 0\nstop = %d\ntime_step = %d\n"
                "final_file = %s\n%s[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\ndomain_size = %r\n%s%s"
                % (STEPS * DT, DT, final, "phase_timing = true\nphase_timing_file = %s\n" % js if phase_timing else "", N, N, INIT % conc, L,
                   THERMO, dyn))
    p = subprocess.run([exe, "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out  # (the first non-zero status ends the test: nothing else is started)
    table = None
    if phase_timing:
        with open(js) as f:
            table = json.load(f)
    return final, out, table


@pytest.fixture(scope="module")
def host_runs(gpu, tmp_path_factory):
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe = os.path.join(HOST, "build", "nextsim_amd")
    tmp = str(tmp_path_factory.mktemp("phase"))
    return {name: (run_host(exe, tmp, name, False), run_host(exe, tmp, name, True)) for name in CASES}


def auto_substeps():
    """n of the sub-stepping rule for the `auto` case's first step, from the wave-speed formula of include/nsdg.h (CPU)"""
    p = abi.MevpParams()
    abi.load_library().nsdg_mevp_default_params(abi.C.byref(p))
    return abi.substep_count(p, 1.0, 250.0, float(DT))[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_run_is_the_same_run(host_runs, name):
    (off_file, off_out, _), (on_file, on_out, _) = host_runs[name]
    assert filecmp.cmp(off_file, on_file, shallow=False)
    assert "device time" not in off_out and "ticks =" not in off_out  # neither timing key: no tree


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_tree(host_runs, name):
    _, (_, out, table) = host_runs[name]
    auto = name == "auto"
    if auto:
        assert auto_substeps() > 1
    names = ["forcing", "column", "prepare", "sub-cycle", "transport"] + (["reduction"] if auto else [])
    assert (table["rank"], table["world"], table["steps"]) == (0, 1, STEPS)
    substeps = table["substeps"]
    assert substeps > STEPS if auto else substeps == STEPS
    blocks = table["blocks"]
    assert [b["block"] for b in blocks] == list(range(4 if name == "four_graph" else 1))
    for b in blocks:
        ph = b["phases"]
        assert sorted(ph) == sorted(names)
        for n in names:
            # the reduction of the sub-stepping rule runs once per MODEL step, every other phase once per sub-step
            assert ph[n]["count"] == (STEPS if n == "reduction" else substeps), (n, ph[n])
            assert ph[n]["ms"] > 0
        assert b["spans"] == STEPS and b["total_ms"] > 0
        diff, bound = sum_rule({n: (ph[n]["ms"], ph[n]["count"]) for n in names}, b["total_ms"], b["spans"])
        assert diff <= bound
        for n in names:
            ex = ph[n].get("exchange")
            if name == "four_graph" and n in ("sub-cycle", "transport"):
                assert ex["exchanges"] > 0 and ex["overlapped"] is True
            else:
                assert not ex or ex["exchanges"] == 0
    # the printed report: iterate keeps its host-clock line, and below it one device-time line per phase
    lines = out.splitlines()
    at = [i for i, l in enumerate(lines) if re.search(r"iterate: ticks = %d wall time .* cpu time " % STEPS, l)]
    assert len(at) == 1, out
    below = lines[at[0] + 1:]
    for n in names:
        count = STEPS if n == "reduction" else substeps
        assert any(re.search(r"[+`]- %s: ticks = %d device time \d+\.\d+ s \(\d+\.\d%% of parent\)" % (re.escape(n), count), l) for l in below), (n, out)
    if name == "four_graph":
        assert sum("exchange: ticks = " in l and "(overlapped, in no sum)" in l for l in below) == 2, out


def test_column_path(gpu, tmp_path):
    """HipStep (run/dev1.cfg): `column` with count 4 under iterate; with model.timing alone the output has no device-time line"""
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe, tmp = os.path.join(HOST, "build", "nextsim_amd"), str(tmp_path)
    js = os.path.join(tmp, "p.json")
    base = [exe, "--config-file", os.path.join(ROOT, "run", "dev1.cfg"), "--model.init_file=", "--model.stop=4",
            "--model.final_file=%s" % os.path.join(tmp, "r.nsdg")]
    p = subprocess.run(base + ["--model.phase_timing=true", "--model.phase_timing_file=%s" % js], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       cwd=tmp, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert re.search(r"iterate: ticks = 4 wall time .*ms/tick", out), out
    assert re.search(r"`- column: ticks = 4 device time \d+\.\d+ s \(\d+\.\d% of parent\) \d+\.\d+ ms/tick", out), out
    with open(js) as f:
        table = json.load(f)
    (b,) = table["blocks"]
    assert list(b["phases"]) == ["column"] and b["phases"]["column"]["count"] == 4 and b["phases"]["column"]["ms"] > 0
    assert b["spans"] == 4 and table["steps"] == 4
    diff, bound = sum_rule({"column": (b["phases"]["column"]["ms"], 4)}, b["total_ms"], 4)
    assert diff <= bound
    p = subprocess.run(base + ["--model.timing=true"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    assert re.search(r"iterate: ticks = 4 .*ms/tick", out) and "device time" not in out, out


# ---- the Python driver ------------------------------------------------------------------------------------------------------------------
def python_run(gpu, phase_timing, steps=3):
    nx = ny = 256
    L, dt, nsub = 512e3, 120.0, 120
    c = abi.Context(gpu)
    bt = synthetic.BoxTest(nx, ny, L)
    c.set_mevp_params(c.mevp_default_params(**bt.subcycle_parameters(dt)))
    core = rowblock.CoupledCore(c, rowblock.RowBlock(nx, ny, 0, 1), L / nx, L / ny, dt, nsub, gpu, native=True, forcing="winter",
                                phase_timing=phase_timing)
    cs, cf = synthetic.column_fields_smooth(nx, ny, L)
    cs = {"hsnow": np.full((ny, nx), 0.05), "tice0": np.full((ny, nx), -8.0)}
    cf["sst"], cf["sss"] = np.full((ny, nx), -1.76), np.full((ny, nx), 32.0)
    core.load_column({**cs, **cf})
    H, A = np.zeros((6, ny, nx)), np.zeros((6, ny, nx))
    H[0], A[0] = 0.3, 0.9
    uo, vo = bt.ocean()
    ua, va = bt.wind(0.0)
    core.load_global(H, A, uo, vo, ua, va)
    for step in range(steps):
        core.device_wind(L, step * dt)
        core.step()
    times = core.phase_times() if phase_timing else None
    c.synchronize()
    fields = {k: getattr(core, k).detach().cpu().numpy().copy() for k in ("H", "A", "u", "v")}
    fields.update({k: core.col[k].detach().cpu().numpy().copy() for k in ("hsnow", "tice0")})
    core.close()
    c.close()
    return fields, times


def test_python_driver(gpu):
    off, _ = python_run(gpu, False)
    on, times = python_run(gpu, True)
    print(times)
    assert sorted(times) == sorted(["forcing", "column", "prepare", "sub-cycle", "transport", "total"])
    for name, (ms, count) in times.items():
        assert count == 3 and ms > 0, (name, ms, count)
    total, spans = times.pop("total")
    diff, bound = sum_rule(times, total, spans)
    assert diff <= bound
    assert float(np.abs(on["u"]).max()) > 0
    for k in off:
        assert np.array_equal(off[k], on[k]), k

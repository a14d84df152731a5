"""The C++ host's momentum budget (host/include/BudgetOutput.hpp "model.budget_*").  Without a device: the
host's own test program (keys, refusals, record clock, series lines) and the binary's refusals before it asks for a device.  On the device:
a 48 x 64 box, 3 steps of the analytic box-test forcing -- records and series with 1 row block against 4 byte for byte, a run with the keys
against a run without them (the restart file byte for byte: the budget changes nothing of the state), periodic records against the record
at the end, and the record against the Python driver's budget_read() for the same configuration."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nextsimdg_amd import abi, build, rowblock, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST = 48, 64  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
DT, STEPS, NSUB = 120, 3, 8
TERMS = ("wind", "water", "internal", "residual")


@pytest.fixture(scope="module")
def host_dir():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_budget_program(host_dir):
    p = subprocess.run([os.path.join(host_dir, "budget_tests")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and re.search(r"host budget tests: \d+ checks, 0 failures", out), out


def write_cfg(tmp, name, step="Nextsim::DynamicsStep", extra=""):
    cfg = os.path.join(tmp, name + ".cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = %s\n[model]\nstructure = rectgrid\ntime_step = %d\nstart = 0\nstop = %d\nfinal_file = %s\n%s"
                "[rectgrid]\nnx = %d\nny = %d\n[init]\nhice = 0.3\ncice = 0.9\n[dynamics]\nnsub = %d\n"
                % (step, DT, DT * STEPS, os.path.join(tmp, name + ".nsdg"), extra, NSLOW, NFAST, NSUB))
    return cfg


def test_host_refuses_before_any_device(host_dir, tmp_path):
    """a multi-process run, the brittle rheology and HipStep, and the bad keys: each ends the binary before it asks for a device"""
    tmp = str(tmp_path)
    exe = os.path.join(host_dir, "nextsim_amd")
    cfg, hip = write_cfg(tmp, "x"), write_cfg(tmp, "hip", step="Nextsim::HipStep")
    two = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    cases = (
        (cfg, ["--model.budget_file=f.nsdg"], two, "model.budget_file is set in a run of 2 processes"),
        (cfg, ["--model.budget_series_file=p.txt"], two, "model.budget_series_file is set in a run of 2 processes"),
        (cfg, ["--model.budget_file=f.nsdg", "--dynamics.rheology=bbm"], None, "model.budget_file is set with dynamics.rheology = bbm"),
        (cfg, ["--model.budget_series_file=p.txt", "--dynamics.rheology=bbm"], None, "model.budget_series_file is set with dynamics.rheology = bbm"),
        (hip, ["--model.budget_file=f.nsdg"], None, "Nextsim::HipStep has no momentum balance"),
        (hip, ["--model.budget_series_file=p.txt"], None, "Nextsim::HipStep has no momentum balance"),
        (hip, ["--model.budget_terms=wind"], None, "Nextsim::HipStep has no momentum balance"),
        (hip, ["--model.budget_period=120"], None, "Nextsim::HipStep has no momentum balance"),
        (cfg, ["--model.budget_file=f.nsdg", "--model.budget_terms=wind,friction"], None, "unknown term \"friction\""),
        (cfg, ["--model.budget_file=f.nsdg", "--model.budget_period=100"], None, "not a whole multiple of model.time_step"),
        (cfg, ["--model.budget_terms=wind"], None, "model.budget_file must name the record files"),
    )
    for config, args, env, needle in cases:
        p = subprocess.run([exe, "--config-file", config] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp, env=env)
        out = p.stdout.decode()
        assert p.returncode != 0 and needle in out, (args, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(tmp, "x.nsdg")) and not os.path.exists(os.path.join(tmp, "p.txt")), (args, out)
    if not torch.cuda.is_available():  # good keys pass every check: the run gets as far as asking for a device
        p = subprocess.run([exe, "--config-file", cfg, "--model.budget_file=f.nsdg", "--model.budget_series_file=q.txt"], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()


def run_host(host, tmp, name, args):
    """the run in a directory of its own: (restart file, {record name: bytes}, series text or None, stdout)"""
    d = os.path.join(tmp, name)
    os.makedirs(d)
    cfg = write_cfg(d, "run")
    p = subprocess.run([os.path.join(host, "nextsim_amd"), "--config-file", cfg] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=d, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    records = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.startswith("forces.")}
    series = open(os.path.join(d, "power.txt")).read() if os.path.exists(os.path.join(d, "power.txt")) else None
    return open(os.path.join(d, "run.nsdg"), "rb").read(), records, series, out


def read_record(raw):
    head, body = raw.split(b"END-HEADER\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "NSDG-HISTORY 1"
    h = dict(line.split("=", 1) for line in lines[1:])
    fields = h["fields"].split(",")
    planes = np.frombuffer(body, dtype=np.float64).reshape(len(fields), int(h["rows"]), int(h["y"]))
    return h, dict(zip(fields, planes))


@pytest.mark.gpu
def test_host_records_series_blocks_restart_and_python_driver(host_dir, gpu, tmp_path):
    tmp = str(tmp_path)
    keys = ["--model.budget_file=forces.nsdg", "--model.budget_terms=" + ",".join(TERMS), "--model.budget_series_file=power.txt"]
    bare, none, no_series, _ = run_host(host_dir, tmp, "bare", [])
    assert none == {} and no_series is None
    one = run_host(host_dir, tmp, "one", keys)
    four = run_host(host_dir, tmp, "four", keys + ["--dynamics.row_blocks=4"])
    # the budget changes nothing of the state: the restart file of the run without the keys, byte for byte; and 1 block = 4 blocks in the
    # restart file, the record and the series
    assert one[0] == bare and four[0] == bare
    assert list(one[1]) == ["forces.%010d.nsdg" % (DT * STEPS)] and four[1] == one[1] and four[2] == one[2]
    # the series: the header and one line per model step, %.17g, the residual's power the sum of the other seven to rounding
    lines = one[2].splitlines()
    assert lines[0] == "# time wind water coriolis tilt internal basal inertia residual ke" and len(lines) == 1 + STEPS
    table = np.array([[float(x) for x in line.split()] for line in lines[1:]])
    assert list(table[:, 0]) == [DT * (k + 1) for k in range(STEPS)] and np.all(table[:, 9] > 0.0) and np.all(table[:, 6] == 0.0)  # (no depth: basal 0)
    assert all(("%.17g" % v) == s for v, s in zip(table[-1, 1:], lines[-1].split()[1:]))
    assert np.all(np.abs(table[:, 8] - table[:, 1:8].sum(axis=1)) <= 1e-9 * np.abs(table[:, 1:8]).sum(axis=1))
    # periodic records: one per step, the last one the record at the end; the .nc form goes through the HDF5 writer
    every = run_host(host_dir, tmp, "every", keys + ["--model.budget_period=%d" % DT, "--dynamics.row_blocks=4"])
    assert list(every[1]) == ["forces.%010d.nsdg" % (DT * (k + 1)) for k in range(STEPS)] and every[0] == bare and every[2] == one[2]
    assert every[1]["forces.%010d.nsdg" % (DT * STEPS)] == one[1]["forces.%010d.nsdg" % (DT * STEPS)]
    assert every[1]["forces.%010d.nsdg" % DT] != every[1]["forces.%010d.nsdg" % (2 * DT)]
    nc = run_host(host_dir, tmp, "nc", ["--model.budget_file=forces.nc"])
    assert list(nc[1]) == ["forces.%010d.nc" % (DT * STEPS)] and nc[1]["forces.%010d.nc" % (DT * STEPS)][:8] == b"\x89HDF\r\n\x1a\n" and nc[0] == bare
    h, rec = read_record(one[1]["forces.%010d.nsdg" % (DT * STEPS)])
    nx, ny = NFAST, NSLOW  # the dynamics ABI calls the fast dimension nx
    assert h["kind"] == "snapshot" and h["fields"] == ",".join(t + "_" + c for t in TERMS for c in "xy")
    assert (int(h["x"]), int(h["y"]), int(h["row0"]), int(h["rows"])) == (2 * ny + 1, 2 * nx + 1, 0, 2 * ny + 1) and int(h["time_end"]) == DT * STEPS

    # the Python driver with the same configuration (tests/test_host_layer.py: the two hosts agree to 1e-10 of their diagnostics, the
    # analytic wind evaluated by the same launch): the record against budget_read() and the last line against the merged totals, within
    # 1e-9 (sum|terms| + max|plane|) per value -- the hosts' own agreement with a margin of 10, not the kernel's bound
    bt = synthetic.BoxTest(nx, ny)
    c = abi.Context(gpu)
    try:
        c.set_mevp_params(c.mevp_default_params(**bt.subcycle_parameters(float(DT))))  # the hosts' policy
        core = rowblock.DynamicsCore(c, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, float(DT), NSUB, torch.device("cuda"), budget=TERMS, budget_power=True)
        H = np.zeros((6, ny, nx)); H[0] = 0.3
        A = np.zeros((6, ny, nx)); A[0] = 0.9
        uo, vo = bt.ocean()
        ua, va = bt.wind(0.0)
        core.load_global(H, A, uo, vo, ua, va)
        for k in range(STEPS):
            core.device_wind(bt.L, float(DT * k))
            core.step()
        torch.cuda.synchronize()
        want = rowblock.DynamicsCore.merge_budget([core.budget_read()])
        core.close()
    finally:
        c.close()
    scale = sum(np.abs(want[t + "_" + c]) for t in TERMS for c in "xy")
    worst = 0.0
    for k, plane in rec.items():
        lim = 1e-9 * (scale + np.abs(want[k]).max())
        worst = max(worst, float(np.max(np.abs(plane - want[k]) / lim)))
        assert np.abs(want[k]).max() > 1e-6 and np.all(np.abs(plane - want[k]) <= lim), k
    print("host record against budget_read(): worst %.3g of 1e-9 (sum|terms| + max|plane|)" % worst)
    totals = [want["power_total"][t] for t in abi.BUDGET_TERMS] + [want["ke_total"]]
    size = sum(abs(x) for x in totals[:8])
    for got, w in zip(table[-1, 1:], totals):
        assert abs(got - w) <= 1e-9 * max(size, abs(w)), (table[-1], totals)

"""The C++ host's sea-surface tilt (host/include/DynamicsStep.hpp "dynamics.tilt", "dynamics.gravity").
Without a device: the host's own test program (keys, refusals, the forcing file's optional ssh) and the binary's refusals before it asks
for a device.  On the device: a 96 x 64 box, 4 steps, a forcing file with a time-varying ssh beside its wind and ocean pairs -- 1 row block
against 4 and N steps against N/2 + restart + N/2, the restart files equal byte for byte; the Python driver with the same series to 1e-12
of the diagnostics (what tests/test_gpu_forcing_file.py settles for); the height moves the ice; and the box test's height without a file."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nextsimdg_amd import abi, build, rowblock, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "nextsimdg_amd", "host")
NSLOW, NFAST = 96, 64  # rectgrid.nx (the slow index, split into row blocks), rectgrid.ny
DT, STEPS, NSUB = 120, 4, 16
INIT = "hice = 0.3\ncice = 0.9\nsst = -1.76\nsss = 32\nhsnow = 0.05\ntice = -8\n"


@pytest.fixture(scope="module")
def host_dir():
    build.build_lib(verbose=False)
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "build")


def test_host_tilt_program(host_dir, tmp_path):
    """the keys, their defaults, their refusals and the forcing file with and without ssh: needs no device"""
    p = subprocess.run([os.path.join(host_dir, "tilt_tests"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0 and re.search(r"host tilt tests: \d+ checks, 0 failures", out), out


def make_file(host, tmp, name, times, fields):
    np.save(os.path.join(tmp, name + "_t.npy"), np.asarray(times, dtype=np.float64))
    args = [os.path.join(host, "make_forcing"), "--out", os.path.join(tmp, name + ".nc"), "--time", os.path.join(tmp, name + "_t.npy")]
    for k, a in fields.items():
        np.save(os.path.join(tmp, "%s_%s.npy" % (name, k)), np.ascontiguousarray(a, dtype=np.float64))
        args.append("%s=%s" % (k, os.path.join(tmp, "%s_%s.npy" % (name, k))))
    out = subprocess.check_output(args).decode()
    return os.path.join(tmp, name + ".nc"), out


def varying_series():
    """irregular records on a coarse 9 x 7 lattice around the run's 0 .. 480 s (the run crosses records within its steps): the column
    planes, both pairs and a height that slopes by metres across the domain and changes from record to record"""
    rng = np.random.default_rng(23)
    t = np.array([-60.0, 100.0, 250.0, 400.0, 600.0])
    nt, nyr, nxr = t.size, 7, 9
    base = {"tair": (-12.0, 4.0), "tdew": (-14.0, 3.0), "slp": (1.0e5, 800.0), "qsw": (60.0, 40.0), "qlw": (250.0, 30.0),
            "mld": (20.0, 5.0), "snowfall": (2e-5, 1e-5), "wind_u": (2.0, 10.0), "wind_v": (-1.0, 10.0), "ocean_u": (0.0, 0.05),
            "ocean_v": (0.0, 0.05)}
    fields = {k: m + s * rng.uniform(-1, 1, (nt, nyr, nxr)) for k, (m, s) in base.items()}
    fields["qsw"], fields["snowfall"] = np.abs(fields["qsw"]), np.abs(fields["snowfall"])
    fields["ssh"] = np.linspace(0.0, 3.0, nxr)[None, None, :] * np.linspace(0.5, 1.5, nt)[:, None, None] + 0.5 * rng.uniform(-1, 1, (nt, nyr, nxr))
    return t, fields


def test_host_refuses_bad_tilt_keys_before_any_device(host_dir, tmp_path):
    tmp = str(tmp_path)
    exe = os.path.join(host_dir, "nextsim_amd")
    t, fields = varying_series()
    full, listing = make_file(host_dir, tmp, "full", t, fields)
    assert re.search(r"variables:.* ssh", listing), listing
    bare, _ = make_file(host_dir, tmp, "bare", t, {k: v for k, v in fields.items() if k != "ssh"})
    cfg = os.path.join(tmp, "x.cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = 120\nstart = 0\nstop = 120\n"
                "final_file = %s\n[rectgrid]\nnx = 6\nny = 8\n[init]\nhice = 0.3\ncice = 0.9\nhsnow = 0.1\n[dynamics]\nnsub = 4\n" % os.path.join(tmp, "x.nsdg"))
    hip = os.path.join(tmp, "hip.cfg")  # the same run under the column step alone
    with open(hip, "w") as f:
        f.write(open(cfg).read().replace("Nextsim::DynamicsStep", "Nextsim::HipStep"))
    thermo = "--dynamics.thermodynamics=true"
    cases = (
        (["--dynamics.tilt=eta"], "dynamics.tilt must be geostrophic or ssh"),
        (["--dynamics.gravity=9.81"], "dynamics.gravity needs dynamics.tilt = ssh"),
        (["--dynamics.tilt=ssh", "--dynamics.gravity=-1"], "dynamics.gravity = -1"),
        ([thermo, "--dynamics.tilt=ssh", "--dynamics.forcing=file", "--dynamics.forcing_file=" + bare], "holds ocean_u / ocean_v but no ssh"),
        ([thermo, "--dynamics.forcing=file", "--dynamics.forcing_file=" + full], "holds ssh: it needs dynamics.tilt = ssh"),
        ([hip, "--dynamics.tilt=ssh"], "Nextsim::HipStep runs the column step alone"),
        ([hip, "--dynamics.gravity=9.81"], "Nextsim::HipStep runs the column step alone"),
    )
    for args, needle in cases:
        config, args = (args[0], args[1:]) if args[0].endswith(".cfg") else (cfg, args)
        p = subprocess.run([exe, "--config-file", config] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        out = p.stdout.decode()
        assert p.returncode != 0 and needle in out, (args, out)
        assert "no HIP device" not in out and not os.path.exists(os.path.join(tmp, "x.nsdg")), (args, out)
    if not torch.cuda.is_available():  # good keys pass every check: the run gets as far as asking for a device
        p = subprocess.run([exe, "--config-file", cfg, thermo, "--dynamics.tilt=ssh", "--dynamics.gravity=9.8", "--dynamics.forcing=file",
                            "--dynamics.forcing_file=" + full], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=tmp)
        assert p.returncode != 0 and "no HIP device" in p.stdout.decode(), p.stdout.decode()


def run_host(host, tmp, name, dynamics, model="start = 0\nstop = %d\n" % (DT * STEPS)):
    final = os.path.join(tmp, name + ".nsdg")
    cfg = os.path.join(tmp, name + ".cfg")
    with open(cfg, "w") as f:
        f.write("[Modules]\nNextsim::IModelStep = Nextsim::DynamicsStep\n[model]\nstructure = rectgrid\ntime_step = %d\n%sfinal_file = %s\n"
                "[rectgrid]\nnx = %d\nny = %d\n[init]\n%s[dynamics]\nnsub = %d\nthermodynamics = true\n%s"
                % (DT, model, final, NSLOW, NFAST, INIT, NSUB, dynamics))
    p = subprocess.run([os.path.join(host, "nextsim_amd"), "--config-file", cfg], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=tmp,
                       timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    with open(final, "rb") as f:
        return f.read(), out


def diagnostics(out):
    m = re.search(r"dynamics umax=(\S+) sumH=(\S+) sumA=(\S+)", out)
    assert m, out
    return [float(m.group(i)) for i in (1, 2, 3)]


@pytest.mark.gpu
def test_host_time_varying_height_blocks_restart_and_python_driver(host_dir, gpu, tmp_path):
    tmp = str(tmp_path)
    t, fields = varying_series()
    path, _ = make_file(host_dir, tmp, "vary", t, fields)
    dyn = "tilt = ssh\nforcing = file\nforcing_file = %s\n" % path
    one, out = run_host(host_dir, tmp, "one", dyn)
    four, _ = run_host(host_dir, tmp, "four", dyn + "row_blocks = 4\n")
    assert four == one
    half, _ = run_host(host_dir, tmp, "half", dyn, model="start = 0\nstop = %d\n" % (DT * STEPS // 2))
    resumed, _ = run_host(host_dir, tmp, "resumed", dyn + "row_blocks = 4\n",
                          model="init_file = %s\nstart = %d\nstop = %d\n" % (os.path.join(tmp, "half.nsdg"), DT * STEPS // 2, DT * STEPS))
    assert resumed == one
    # the height is felt: the same file without ssh under the geostrophic tilt is another run, and so is another gravity
    bare, _ = make_file(host_dir, tmp, "bare", t, {k: v for k, v in fields.items() if k != "ssh"})
    geo, geo_out = run_host(host_dir, tmp, "geo", "forcing = file\nforcing_file = %s\n" % bare)
    moon, _ = run_host(host_dir, tmp, "moon", dyn + "gravity = 1.62\n")
    assert geo != one and moon != one and len(geo) == len(one)  # the restart file holds nothing new
    got = diagnostics(out)
    print("host, 4 steps: umax %.6g m/s with the height, %.6g with the geostrophic tilt" % (got[0], diagnostics(geo_out)[0]))

    # the Python driver with the same series: the same diagnostics
    nx, ny = NFAST, NSLOW
    bt = synthetic.BoxTest(nx, ny)
    c = abi.Context(gpu)
    try:
        c.set_mevp_params(c.mevp_default_params(**bt.subcycle_parameters(float(DT))))  # the hosts' policy
        core = rowblock.CoupledCore(c, rowblock.RowBlock(nx, ny), bt.hx, bt.hy, float(DT), NSUB, torch.device("cuda"),
                                    forcing=rowblock.ForcingSeries(t, fields), tilt="ssh")
        H = np.zeros((6, ny, nx)); H[0] = 0.3
        A = np.zeros((6, ny, nx)); A[0] = 0.9
        z = np.zeros((2 * ny + 1, 2 * nx + 1))
        core.load_global(H, A, z, z, z, z)
        col = {k: np.zeros((ny, nx)) for k in core.col}
        col["hsnow"][:], col["tice0"][:], col["sst"][:], col["sss"][:] = 0.05, -8.0, -1.76, 32.0
        core.load_column(col)
        for _ in range(STEPS):
            core.step()
        want = [float(core.u.abs().max()), float(core.H[0].sum()), float(core.A[0].sum())]
        core.close()
    finally:
        c.close()
    assert want[0] > 1e-6
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-12 * abs(w), (got, want)


@pytest.mark.gpu
def test_host_box_height_without_a_file_runs_in_blocks(host_dir, gpu, tmp_path):
    """forcing = dummy: the height is nsdg_boxtest_ssh's, placed by nsdg_block_set: 1 row block equals 4, and the run is finite"""
    tmp = str(tmp_path)
    dyn = "tilt = ssh\nforcing = dummy\n"
    one, out = run_host(host_dir, tmp, "one", dyn)
    four, _ = run_host(host_dir, tmp, "four", dyn + "row_blocks = 4\n")
    assert four == one
    got = diagnostics(out)
    assert all(np.isfinite(got)) and got[0] > 1e-6

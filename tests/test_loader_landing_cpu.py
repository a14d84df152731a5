"""Compile side of NSDG_P2P_LAND (csrc/mevp_p2p.h; csrc/mevp_fused4.hip, table above p2p_row): where the loader wave of the stage-per-wave
mEVP pass requests its loads and where they land.  For every value of the switch, read from the compiler's listing: no scratch memory
and no spilled vector register in any of the four instantiations of the kernel; no more registers per wave than the parent of the
switch had (364 adaptive / 346 uniform alpha and beta); the fp64 instruction counts of both loops equal to the ones bench.py states
(tools/isa_flops.py, as tests/test_bench_launch.py re-counts them for the default).  For the default build, the loader's loop is walked
with the vmcnt counter in hand: no s_waitcnt may force a stress load to land before the loader has issued this row's requests of P, u
and v, i.e. before the row has reached the stress copy in front of the relaxation.  Needs hipcc, no GPU."""
import concurrent.futures
import os
import re
import subprocess
import sys

import pytest

from nextsimdg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
VALUES = [None, 0, 1, 2, 3]  # None: the flags of the product build (the default of the switch)
PARENT_VGPRS = {True: 364, False: 346}  # adaptive / uniform: vgpr_count of the kernel before the switch existed
N_P, N_UV, N_STRESS = 5, 8, 12  # loads per row: ice strength, u and v, stress (the table above p2p_row)

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and not os.environ.get("HIPCC"), reason="needs hipcc")


def kernel_metadata(text):
    """{kernel symbol: {key: int}} of the amdhsa.kernels entries of a listing"""
    out = {}
    for entry in re.split(r"\n  - \.", text[text.index("amdhsa.kernels:"):])[1:]:
        fields = dict(re.findall(r"^\s*\.?(\w+):\s+(\S+)\s*$", "." + entry, flags=re.M))
        if "name" in fields:
            out[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return out


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{value: listing}: one compilation per value of the switch, side by side"""
    d = tmp_path_factory.mktemp("landing")

    def compile_one(value):
        out = str(d / ("fused4_%s.s" % value))
        flags = build.FLAGS + ([] if value is None else ["-DNSDG_P2P_LAND=%d" % value])
        subprocess.check_call([build.hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(ROOT, "nextsimdg_amd", "csrc", "mevp_fused4.hip"), "-o", out],
                              stderr=subprocess.DEVNULL)
        return open(out).read()

    with concurrent.futures.ThreadPoolExecutor(max_workers=len(VALUES)) as pool:
        return dict(zip(VALUES, pool.map(compile_one, VALUES)))


@pytest.mark.parametrize("value", VALUES)
def test_no_scratch_no_spills_and_no_more_registers_than_the_parent(listings, value):
    meta = {k: v for k, v in kernel_metadata(listings[value]).items() if "mevp_fused4_kernel" in k}
    assert len(meta) == 4, sorted(meta)  # <AD, LAND> = <false, false>, <true, false>, <false, true>, <true, true>
    for name, m in sorted(meta.items()):
        adaptive = "mevp_fused4_kernelILb1E" in name
        print("NSDG_P2P_LAND=%s %s: vgpr_count %d, vgpr_spill_count %d, private_segment_fixed_size %d"
              % (value, name, m["vgpr_count"], m["vgpr_spill_count"], m["private_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= PARENT_VGPRS[adaptive], name


@pytest.mark.parametrize("value", VALUES)
def test_fp64_counts_are_the_pinned_ones(listings, value):
    import bench
    import isa_flops

    for adaptive in (False, True):
        loops = isa_flops.loops(listings[value], adaptive)
        assert len(loops) == 2
        for label, ins in loops:  # the stages 1-3, then the loader
            c = isa_flops.flops(ins)
            print("NSDG_P2P_LAND=%s adaptive=%s %s: fma %d add/mul %d rcp/rsq %d other %d" % (value, adaptive, label, c["fma"], c["addmul"], c["trans"], c["other_f64"]))
            assert c["flops"] == bench.FP64_FLOPS_PER_ELEMENT_SUBITER[adaptive], c
            assert c["fma"] == bench.FP64_FMA_PER_ELEMENT_SUBITER[adaptive], c
            assert c["fma"] + c["addmul"] + 4 * c["trans"] + c["other_f64"] == bench.FP64_ISSUE_SLOTS_PER_ELEMENT_SUBITER[adaptive], c


def stress_landings(ins):
    """Walks the loader's loop twice (the second trip is the steady state) with the queue of its loads in flight: vmcnt(N) lets the
    oldest land until N are left.  The stress loads are the streaming ones (`nt`: NSDG_P2P_NT bit 1; the ice strength is not).
    Returns, for every wait of the second trip that makes a stress load land, (position in the loop, N, loads in flight that are
    younger than the youngest stress load of that group)."""
    queue, out = [], []
    for trip in range(2):
        group = 0
        for pos, t in enumerate(ins):
            op = t.split()[0]
            if op.startswith("global_load"):
                stress = t.rstrip().endswith(" nt")
                queue.append((trip, stress))
            elif op == "s_waitcnt" and "vmcnt(" in t:
                n = int(re.search(r"vmcnt\((\d+)\)", t).group(1))
                landed = queue[:max(len(queue) - n, 0)]
                if trip == 1 and any(s for _, s in landed):
                    g = next(tr for tr, s in landed if s)  # the trip that requested the landing stress
                    last = max(i for i, (tr, s) in enumerate(queue) if s and tr == g)
                    out.append((pos, n, len(queue) - 1 - last))
                queue = queue[len(landed):]
    return out


@pytest.mark.parametrize("adaptive", [False, True], ids=["uniform", "adaptive"])
def test_default_build_lands_the_stress_no_earlier_than_its_copy(listings, adaptive):
    """the copy stands behind the requests of P, u and v of the row (13 loads younger than the stress) and in front of the relaxation; a
    wait that makes a stress load land while fewer than those 13 have been issued stands before the copy (the parent: vmcnt(12) at the
    top of the row, 12 younger loads -- the coefficients -- in flight)"""
    import isa_flops

    loops = isa_flops.loops(listings[None], adaptive)
    assert len(loops) == 2
    ins = loops[1][1]
    assert sum(1 for t in ins if t.startswith("global_load")) == 37 and sum(1 for t in ins if t.startswith("global_load") and t.rstrip().endswith(" nt")) == N_STRESS
    landings = stress_landings(ins)
    print("adaptive=%s: waits that land a stress load (position, N, younger loads in flight): %s" % (adaptive, landings))
    assert landings
    for pos, n, younger in landings:
        assert younger >= N_P + N_UV, (pos, n, younger)

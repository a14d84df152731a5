"""Resources of the stage-per-wave mEVP pass (csrc/mevp_fused4.hip) for every value of NSDG_P2P_EARLY (csrc/mevp_p2p.h): moving the
stress writes of a row forward must not cost scratch memory or spilled vector registers in any of the four instantiations of the kernel
(uniform / adaptive alpha and beta, each with and without the land mask), and each must fit the 512 vector registers of a wave at one
wave per SIMD.  Read from the code object's metadata in the compiler's listing; needs hipcc, no GPU."""
import os
import re
import subprocess

import pytest

from nextsimdg_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_metadata(text):
    """{kernel symbol: {key: int}} of the amdhsa.kernels entries of a listing"""
    out = {}
    for entry in re.split(r"\n  - \.", text[text.index("amdhsa.kernels:"):])[1:]:
        fields = dict(re.findall(r"^\s*\.?(\w+):\s+(\S+)\s*$", "." + entry, flags=re.M))
        if "name" in fields:
            out[fields["name"]] = {k: int(v) for k, v in fields.items() if re.fullmatch(r"\d+", v)}
    return out


@pytest.mark.parametrize("early", [None, 0, 1, 2, 3])
def test_no_scratch_no_spills_and_registers_fit(tmp_path, early):
    """early = None: the flags of the product build (the default of the switch)"""
    out = str(tmp_path / "fused4.s")
    flags = build.FLAGS + ([] if early is None else ["-DNSDG_P2P_EARLY=%d" % early])
    subprocess.check_call([build.hipcc()] + flags + ["-S", "--cuda-device-only", os.path.join(ROOT, "nextsimdg_amd", "csrc", "mevp_fused4.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    meta = {k: v for k, v in kernel_metadata(open(out).read()).items() if "mevp_fused4_kernel" in k}
    assert len(meta) == 4, sorted(meta)  # <AD, LAND> = <false, false>, <true, false>, <false, true>, <true, true>
    for name, m in sorted(meta.items()):
        print("NSDG_P2P_EARLY=%s %s: vgpr_count %d, vgpr_spill_count %d, private_segment_fixed_size %d"
              % (early, name, m["vgpr_count"], m["vgpr_spill_count"], m["private_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0, name
        assert m["vgpr_count"] <= 512, name

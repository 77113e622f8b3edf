"""CPU (no GPU needed): the compensator kernels of art_kernels.hip -- the pilot and the main pass for 2, 4, 6 and 8 columns
and the fold -- compile for gfx950 without scratch memory, without spilled registers and without accumulation registers,
read from the code object's metadata as test_sensitivity_isa.py reads it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")
KERNELS = [f"k_alignment_{kind}ILi{nc}E" for kind in ("pilot", "sums") for nc in (2, 4, 6, 8)] + ["k_alignment_foldE"]


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "art.s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                          stderr=subprocess.DEVNULL)
    s = open(out).read()
    res = {}
    for m in re.finditer(r"- \.agpr_count:\s+(\d+)\n(.*?)(?=\n  - \.|\namdhsa\.target)", s, re.S):
        body = m.group(2)
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, body).group(1))
        res[re.search(r"\.name:\s+(\S+)", body).group(1)] = {
            "agpr": int(m.group(1)), "vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "lds": g("group_segment_fixed_size"),
            "scratch": g("private_segment_fixed_size"), "vgpr_spill": g("vgpr_spill_count"),
            "sgpr_spill": g("sgpr_spill_count")}
    return res


@pytest.mark.parametrize("kernel", KERNELS)
def test_alignment_kernels_have_no_scratch_and_no_spills(meta, kernel):
    found = [k for k in meta if re.search(r"\d%s" % kernel, k) and not k.endswith(".kd")]
    assert len(found) == 1, found
    m = meta[found[0]]
    print(kernel, m)
    assert m["scratch"] == 0, m
    assert m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, m
    assert m["agpr"] == 0, m                     # (no spilling into the accumulation registers either)
    assert m["vgpr"] <= 256, m                   # at least two waves per SIMD at eight columns
    assert m["lds"] <= 65536, m                  # two workgroups per CU and more

"""CPU (no GPU needed): the polarisation kernels of art_kernels.hip compile for gfx950 without scratch memory, within
128 VGPRs (no AGPRs), and with LDS that lets four workgroups share a CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")


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
            "agpr": int(m.group(1)), "vgpr": g("vgpr_count"), "lds": g("group_segment_fixed_size"),
            "scratch": g("private_segment_fixed_size")}
    return res


@pytest.mark.parametrize("kernel", ["k_polarisationE", "k_polarisation_foldE"])
def test_polarisation_kernels_fit(meta, kernel):
    found = [k for k in meta if re.search(r"\d%s" % kernel, k) and not k.endswith(".kd")]
    assert len(found) == 1, found
    m = meta[found[0]]
    assert m["scratch"] == 0, m
    assert m["vgpr"] <= 128 and m["agpr"] == 0, m
    assert m["lds"] <= 40 * 1024, m       # 160 KiB of LDS per CU: four workgroups

"""CPU (no GPU needed): the kernels of art_focal_vector_spectrum in art_kernels.hip compile for gfx950 without scratch
memory; the ray-spectra kernel within k_polarisation's budget (128 VGPRs, no AGPRs, LDS for four workgroups per CU), the
field kernel within k_focal_spectrum_field's (256 VGPRs, LDS for two workgroups per CU)."""
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


def _one(meta, kernel):
    found = [k for k in meta if re.search(r"\d%s[A-Z]" % kernel, k) and not k.endswith(".kd")]
    assert len(found) == 1, found
    return meta[found[0]]


def test_ray_spectra_kernel_fits_four_workgroups_per_cu(meta):
    m = _one(meta, "k_vecspec_rays")
    assert m["scratch"] == 0, m
    assert m["vgpr"] <= 128 and m["agpr"] == 0, m
    assert m["lds"] <= 40 * 1024, m       # 160 KiB of LDS per CU: four workgroups


def test_vector_field_kernel_fits_two_workgroups_per_cu(meta):
    m = _one(meta, "k_vecspec_field")
    assert m["scratch"] == 0, m
    assert m["vgpr"] + m["agpr"] <= 256, m
    assert m["lds"] <= 80 * 1024, m       # 160 KiB of LDS per CU: two workgroups


@pytest.mark.parametrize("kernel", ["k_polarisation", "k_polarisation_fold", "k_focal_spectrum_prep",
                                    "k_focal_spectrum_field", "k_focal_prep", "k_focal_field", "k_focal_fold"])
def test_existing_kernels_are_still_found_once(meta, kernel):
    """The new kernels' names do not match the patterns by which the other ISA tests find theirs."""
    _one(meta, kernel)

"""CPU (no GPU needed): the two kernels of art_focal_vector_chromatic in art_kernels.hip compile for gfx950 without
scratch memory; k_vecchrom_rays within k_vecspec_rays' budget (128 VGPRs, no AGPRs, LDS for four workgroups per CU),
k_vecchrom_field within k_vecspec_field's (256 registers, LDS for two workgroups per CU); and their names match none of
the patterns by which the other ISA tests find their kernels."""
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


def test_table_ray_spectra_kernel_fits_four_workgroups_per_cu(meta):
    m = _one(meta, "k_vecchrom_rays")
    assert m["scratch"] == 0, m
    assert m["vgpr"] <= 128 and m["agpr"] == 0, m
    assert m["lds"] <= 40 * 1024, m       # 160 KiB of LDS per CU: four workgroups


def test_chromatic_vector_field_kernel_fits_two_workgroups_per_cu(meta):
    m = _one(meta, "k_vecchrom_field")
    assert m["scratch"] == 0, m
    assert m["vgpr"] + m["agpr"] <= 256, m
    assert m["lds"] <= 80 * 1024, m       # 160 KiB of LDS per CU: two workgroups


@pytest.mark.parametrize("kernel", ["k_vecspec_rays", "k_vecspec_field", "k_focal_chromatic_prep", "k_focal_chromatic_field",
                                    "k_focal_spectrum_prep", "k_focal_spectrum_field", "k_focal_field", "k_focal_fold",
                                    "k_polarisation"])
def test_existing_kernels_are_still_found_once(meta, kernel):
    """One ray-spectra body serves two kernels: each has a name of its own, and the shared body is no kernel."""
    _one(meta, kernel)

"""CPU (no GPU needed): the focal-image kernels of art_kernels.hip compile for gfx950 without scratch memory, within the
register file, and the image kernel's LDS stage fits two workgroups per CU.  Reads the kernels' metadata only."""
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
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
        g = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, m.group(2)).group(1))
        res[m.group(1)] = {"vgpr": g("next_free_vgpr"), "lds": g("group_segment_fixed_size"),
                           "scratch": g("private_segment_fixed_size")}
    return res


@pytest.mark.parametrize("kernel", ["k_focal_image", "k_focal_image_fold", "k_focal_image_fold_split"])
def test_image_kernels_compile_without_scratch(meta, kernel):
    found = [k for k in meta if re.search(r"\d%s[A-Z]" % kernel, k)]
    assert len(found) == 1, found
    m = meta[found[0]]
    print(kernel, m)
    assert m["scratch"] == 0, m
    assert m["vgpr"] <= 256, m
    assert m["lds"] <= 80 * 1024, m       # 160 KiB of LDS per CU: two workgroups of the image kernel


@pytest.mark.parametrize("kernel", ["k_focal_prep", "k_focal_field", "k_focal_fold"])
def test_image_kernels_do_not_shadow_the_focal_kernels(meta, kernel):
    """tests/test_focal_isa.py finds each focal kernel by name and demands one match: the image kernels' names must not
    match those patterns."""
    assert len([k for k in meta if re.search(r"\d%s[A-Z]" % kernel, k)]) == 1

"""CPU (no GPU needed): the select, rank and staging kernels of csrc/art_quantile.h compile for gfx950 without scratch memory,
without spilled registers and without AGPRs, read from the code object's metadata; and their code adds in integers only:
no floating-point atomic add anywhere in them (the sums must be the same bytes on every run)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")
KERNELS = ["k_select_histILb1EE", "k_select_histILb0EE", "k_select_pickE", "k_rank_binsE", "k_rank_finishE", "k_stage_keysE",
           "k_metric_momentsE", "k_metric_centresE"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "art.s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                          stderr=subprocess.DEVNULL)
    s = open(out).read()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:\s+(\d+)\n(.*?)(?=\n  - \.|\namdhsa\.target)", s, re.S):
        body = m.group(2)
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, body).group(1))
        meta[re.search(r"\.name:\s+(\S+)", body).group(1)] = {
            "agpr": int(m.group(1)), "vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "lds": g("group_segment_fixed_size"),
            "scratch": g("private_segment_fixed_size"), "vgpr_spill": g("vgpr_spill_count"),
            "sgpr_spill": g("sgpr_spill_count")}
    return s, meta


def _name(meta, kernel):
    found = [k for k in meta if re.search(r"artq\d+%s" % kernel, k) and not k.endswith(".kd")]
    assert len(found) == 1, found
    return found[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_quantile_kernels_have_no_scratch_no_spills_no_agprs(asm, kernel):
    _, meta = asm
    m = meta[_name(meta, kernel)]
    print(kernel, m)
    assert m["scratch"] == 0, m
    assert m["vgpr_spill"] == 0 and m["sgpr_spill"] == 0, m
    assert m["agpr"] == 0, m


@pytest.mark.parametrize("kernel", KERNELS)
def test_quantile_kernels_add_in_integers_only(asm, kernel):
    s, meta = asm
    name = _name(meta, kernel)
    body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), s, re.S | re.M).group(1)
    assert "s_endpgm" in body
    atomics = re.findall(r"^\s*((?:ds|global|flat|buffer)_\w*(?:atomic|add|pk_add)\w*)", body, re.M)
    floats = [a for a in atomics if re.search(r"_f(16|32|64)|_bf16", a)]
    assert not floats, floats
    if kernel.startswith(("k_select_hist", "k_rank_bins")):
        assert any(a.startswith("ds_add") and a.endswith("u64") for a in atomics), atomics          # the LDS bins
        assert any(a.startswith("global_atomic_add") and a.endswith("x2") for a in atomics), atomics   # the flush

"""CPU (no GPU needed): the host side of the row summaries (include/art_hip.h: art_bundle_row_summary,
art_scene_set_row_summaries).  They were added WITHOUT touching a layout: the ABI version, every public struct and the
scene image keep their sizes; the summaries' pointer travels in spare words of the image's header; a backend without the
kernel (the CPU twin) attaches nothing; and the key a bundle's summary is cached under moves with every way its arrays or
weights can change."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import load_golden
import parity_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sizeof of every public struct of include/art_hip.h, as they were before the summaries were added
STRUCT_BYTES = {"ArtGridDefect": 48, "ArtElementDesc": 312, "ArtBundleView": 72, "ArtDetectorDesc": 120, "ArtGratingDesc": 64,
                "ArtQuadricDesc": 80, "ArtFigureDesc": 24, "ArtChainReadout": 200, "ArtHistogramDesc": 216, "ArtFocalDesc": 696,
                "ArtFocalSpectrumDesc": 712, "ArtFocalChromaticDesc": 728, "ArtWavefrontJob": 304, "ArtCoatingMaterial": 16,
                "ArtCoatingLayer": 24, "ArtCoating": 6272, "ArtPolarisationJob": 504, "ArtTubeJob": 224,
                "ArtSensitivityJob": 216, "ArtFocalVectorSpectrumDesc": 1064, "ArtFocalVectorChromaticDesc": 1088,
                "ArtFocalImageDesc": 712, "ArtAnalysisJob": 176}
HEADER_BYTES = 64
CHAIN_BYTES = 8 * 312 + 8 * 72 + 72 + 200 + 8        # elements, history views, input view, read-out, count + flags
POINTER_OFFSET = 24                                   # header: magic, 4 counts / flags, one spare word, then the pointer


@pytest.fixture(scope="module")
def fn():
    import torch  # noqa: F401  (before the library: one HIP runtime per process, see __graft_entry__.build)
    import __graft_entry__ as g
    from attosecondraytracing_amd import _abi
    g.ensure_built()
    return _abi.bind(C.CDLL(g.HIP_LIB))


@pytest.fixture()
def twin():
    from twin_backend import TwinBackend
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = TwinBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _scene():
    scene, a = load_golden("c3_twisted_chain00")
    return pc.source_bundle(a, scene), pc.build_elements(scene, a)


def test_layouts_are_what_they_were(fn, tmp_path):
    from attosecondraytracing_amd import _abi
    assert _abi.ART_ABI_VERSION == 14 and fn["art_abi_version"]() == 14
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    assert re.search(r"#define ART_ABI_VERSION 14\b", hdr)
    names = re.findall(r"typedef struct (\w+)", hdr)
    assert set(names) == set(STRUCT_BYTES)
    src = '#include <stdio.h>\n#include "art_hip.h"\nint main(void) {\n'
    src += "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) + "  return 0;\n}\n"
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
    got = dict((k, int(v)) for k, v in (line.split() for line in subprocess.check_output([exe]).decode().splitlines()))
    assert got == STRUCT_BYTES
    for name, size in STRUCT_BYTES.items():
        if hasattr(_abi, name):
            assert C.sizeof(getattr(_abi, name)) == size, name
    for chains, elems in ((1, 1), (1, 8), (3, 9), (11, 3), (2, 17)):
        assert fn["art_scene_bytes"](chains, elems) == HEADER_BYTES + -(-elems // 8) * chains * CHAIN_BYTES
    assert fn["art_scene_bytes"](0, 1) == 0 and fn["art_scene_bytes"](1, 0) == 0
    assert fn["art_row_summary_bytes"]() == 88          # a mask word, a pad word, the slot count, nine 8-byte patterns


def test_pointer_round_trips_through_the_header(fn, twin):
    """art_scene_set_row_summaries writes the pointer into the packed image's header and nowhere else; packing again
    clears it; a buffer that art_scene_pack did not write is refused."""
    from attosecondraytracing_amd import _abi
    from attosecondraytracing_amd.graph import SceneProgram
    src, els = _scene()
    prog = SceneProgram([src] * 2, [els, els])       # (the twin packs with the library's own packer, art_scene.h)
    img = prog.host.numpy()
    assert img.nbytes == fn["art_scene_bytes"](2, len(els))
    before = img.copy()
    assert not before[POINTER_OFFSET:POINTER_OFFSET + 8].any()
    ptr = 0x7F12_3456_7800
    assert fn["art_scene_set_row_summaries"](img.ctypes.data, ptr) == 0
    assert int(img[POINTER_OFFSET:POINTER_OFFSET + 8].view(np.uint64)[0]) == ptr
    changed = np.nonzero(img != before)[0]
    assert len(changed) and changed.min() >= POINTER_OFFSET and changed.max() < POINTER_OFFSET + 8
    assert fn["art_scene_set_row_summaries"](img.ctypes.data, None) == 0      # NULL detaches
    assert np.array_equal(img, before)
    fn["art_scene_set_row_summaries"](img.ctypes.data, ptr)
    prog.update([els, els])                                                    # packing clears the header's spare words
    assert np.array_equal(prog.host.numpy(), before)
    junk = np.zeros(img.nbytes, dtype=np.uint8)
    assert fn["art_scene_set_row_summaries"](junk.ctypes.data, ptr) == _abi.ART_ERR_BAD_ARG
    assert b"art_scene_pack" in fn["art_last_error"]()
    assert not junk.any()
    assert fn["art_scene_set_row_summaries"](None, ptr) == _abi.ART_ERR_BAD_ARG


def test_a_backend_without_the_kernel_attaches_nothing(twin):
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd.graph import SceneProgram
    src, els = _scene()
    assert src.row_summary() is None
    assert mp._scene_row_summaries(twin, [src], None) == (None, None)
    prog = SceneProgram([src], [els])
    for _ in range(2):
        out = prog.run()[0]
        assert prog._summaries is None
        assert not prog.host.numpy()[POINTER_OFFSET:POINTER_OFFSET + 8].any()
        ref = mp.RayTracingCalculation(src, els)
        for x, y in zip(out, ref):
            m = x.alive.numpy().astype(bool)
            assert np.array_equal(x.alive.numpy(), y.alive.numpy())
            assert np.array_equal(x.data.numpy()[:, m].view(np.int64), y.data.numpy()[:, m].view(np.int64))
    # ... nor does the one-shot scene launch, however often the source comes back
    two = [[src, src.copy()], [els, els]]
    a, b = mp.RayTracingCalculationMany(*two), mp.RayTracingCalculationMany(*two)
    assert np.array_equal(a[1][-1].alive.numpy(), b[1][-1].alive.numpy())


def test_the_cache_key_follows_every_change(twin):
    """What a captured program compares at every run(): the key moves when the arrays are written in place (an element, a
    whole copy_, the alive bytes), when the weights are written in place or replaced, and when a writer that went through
    a raw view says so with touch() -- and stays put otherwise."""
    import torch
    src, _ = _scene()
    other = src.copy()
    seen = [src.row_summary_key()]
    assert src.row_summary_key() == seen[0]

    def moved(what):
        k = src.row_summary_key()
        assert k not in seen, what
        assert src.row_summary_key() == k
        seen.append(k)

    src.data[0, 5] = 1.0
    moved("one element written")
    src.data.copy_(other.data)
    moved("data.copy_")
    src.alive[3] = 0
    moved("an alive byte written")
    src.intensity.mul_(2.0)
    moved("weights written in place")
    src.intensity.copy_(torch.rand(src.n_slots, dtype=torch.float64))
    moved("weights copy_")
    src.intensity = src.intensity.clone()
    moved("weights replaced")
    src.intensity = None
    moved("weights removed")
    src.touch()
    moved("touch() after a write through a raw view")
    # the weights a fused read-out was built with, not the bundle's own
    w = torch.ones(src.n_slots, dtype=torch.float64)
    k = src.row_summary_key(w)
    assert k not in seen and src.row_summary_key(w) == k
    w[0] = 2.0
    assert src.row_summary_key(w) != k
    # a range of slots is a bundle of its own; it shares torch's counters with the arrays it was cut from
    part = src.slots(64, 128)
    kp = part.row_summary_key()
    assert kp != src.row_summary_key()
    src.data[1, 100] = 3.0
    assert part.row_summary_key() != kp


def test_library_writers_through_raw_views_touch_their_bundle(twin):
    import ART.ModuleSource as msource
    from attosecondraytracing_amd.bundle import RayBundle
    b = msource.PointSource(np.zeros(3), np.array([1.0, 0, 0]), 0.02, 100)
    assert b.version > 0
    assert msource.ExtendedSource(np.zeros(3), np.array([1.0, 0, 0]), 1.0, 0.02, 9000).version > 0
    assert RayBundle.from_arrays(np.zeros((4, 3)), np.tile([1.0, 0, 0], (4, 1))).version > 0
    assert b.transformed(np.eye(3), np.ones(3)).version > 0

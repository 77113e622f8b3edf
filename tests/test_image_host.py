"""CPU: the Python layer of the partially coherent focal image (attosecondraytracing_amd/image.py,
Detector.get_FocalImage, OpticalChain.get_FocalImage) against a NumPy stand-in for art_focal_image on top of the CPU
twin backend (tests/image_common.py), and ArtFocalImageDesc against include/art_hip.h."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import focal_common as fc
import image_common as ic
from attosecondraytracing_amd import _abi
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)).copy() if n else np.zeros(0)


class NumpyImageBackend(TwinBackend):
    """art_focal_image's contract in NumPy (tests/image_common.py); records the last descriptor, offsets and group
    count it was given."""

    def focal_image(self, fdesc, seg, groups, view, w, n):
        self.last, self.seg, self.groups = fdesc, seg.numpy().copy(), groups
        assert seg.dtype == torch.int64 and seg.shape == (groups + 1,) and groups >= 1
        P = np.stack([_host(p, n) for p in (view.ox, view.oy, view.oz)], axis=1) if n else np.zeros((0, 3))
        D = np.stack([_host(p, n) for p in (view.dx, view.dy, view.dz)], axis=1) if n else np.zeros((0, 3))
        alive = _host(view.alive, n, C.c_uint8).astype(bool) if n else np.zeros(0, dtype=bool)
        x = fdesc.x0 + np.arange(fdesc.nx) * fdesc.dx
        y = fdesc.y0 + np.arange(fdesc.ny) * fdesc.dy
        I = ic.image(P, D, _host(view.path, n), alive, None if w is None else w[:n].numpy(), self.seg, fdesc.k,
                     fdesc.L_ref, fdesc.det.centre[:], fdesc.det.normal[:], fdesc.det.rot[:], x, y,
                     [fdesc.shift[q] for q in range(fdesc.planes)])
        return torch.from_numpy(I)


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyImageBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _detector(z=0.0):
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, z]), np.array([0.0, 0.0, -1.0]))


KW = dict(Size=0.02, Pixels=(5, 3), Centre=(0.0, 0.0))


def test_rays_per_source_gives_the_documented_seg(twin):
    B = fc.converging_bundle(100, 0.05, 2.0, backend=twin)
    D = _detector()
    f = D.get_FocalImage(B, RaysPerSource=30, **KW)
    assert list(twin.seg) == [0, 30, 60, 90, 100] and twin.groups == 4 and f.groups == 4
    assert f.intensity.shape == (1, 3, 5) and f.intensity.dtype == torch.float64
    D.get_FocalImage(B, RaysPerSource=100, **KW)
    assert list(twin.seg) == [0, 100]
    D.get_FocalImage(B, RaysPerSource=1000, **KW)
    assert list(twin.seg) == [0, 100]
    # a view with lo != 0 carries its ray numbers: the groups follow the numbers, not the view's slots
    D.get_FocalImage(B.slots(20, 95), RaysPerSource=30, **KW)
    assert list(twin.seg) == [0, 10, 40, 70, 75]
    # an explicit number
    B.number = torch.from_numpy(np.repeat([3, 4, 9, 64], 25) * 7 + np.tile(np.arange(25) % 7, 4))
    D.get_FocalImage(B, RaysPerSource=7, **KW)
    assert list(twin.seg) == [0, 25, 50, 75, 100] and twin.groups == 4


def test_groups_give_the_documented_seg_and_the_truth(twin):
    w = np.linspace(0.5, 1.5, 100)
    B = fc.converging_bundle(100, 0.05, 2.0, backend=twin, weights=w)
    B.alive[40:45] = 0
    B.touch()
    D = _detector()
    sizes = [1, 31, 5, 63]
    ids = ic.ids_of_sizes(sizes, first=-2, gap_after=1)          # negative ids and a gap are fine
    for g in (ids, list(ids), torch.from_numpy(ids), ids.astype(np.int32)):
        f = D.get_FocalImage(B, Groups=g, Shifts=(0.0, 0.2), **KW)
        assert list(twin.seg) == [0, 1, 32, 37, 100] and f.groups == 4
    assert list(twin.seg) == list(ic.seg_of_ids(ids)) == list(ic.seg_of_sizes(sizes))
    I = ic.image_of(B, D, f, twin.seg)
    assert np.abs(f.intensity.numpy() - I).max() <= 1e-12 * f.ideal_peak
    alive = B.alive.numpy().astype(bool)
    assert f.ideal_peak == pytest.approx(ic.ideal_peak(alive, w, twin.seg), rel=1e-13)
    assert f.power == pytest.approx(w[alive].sum(), rel=1e-14)
    assert np.all(f.strehl <= 1.0 + 1e-12) and f.strehl[0] > f.strehl[1]      # (every group focuses at (0, 0))


@pytest.mark.parametrize("kw, msg", [
    (dict(), "exactly one"), (dict(RaysPerSource=10, Groups=np.zeros(50, dtype=int)), "exactly one"),
    (dict(Groups=np.r_[np.zeros(20, dtype=int), 2 * np.ones(10, dtype=int), np.ones(20, dtype=int)]), "non-decreasing"),
    (dict(Groups=np.zeros(49, dtype=int)), "one integer id per slot"), (dict(Groups=np.zeros(50)), "one integer id per slot"),
    (dict(RaysPerSource=0), "positive integer"), (dict(RaysPerSource=2.5), "positive integer")])
def test_bad_group_arguments_raise(twin, kw, msg):
    B = fc.converging_bundle(50, 0.05, 2.0, backend=twin)
    with pytest.raises(ValueError, match=msg):
        _detector().get_FocalImage(B, **dict(KW, **kw))


def test_extended_source_carries_rays_per_source(twin):
    import ART.ModuleSource as msource
    B = msource.ExtendedSource(np.zeros(3), np.array([0.0, 0.0, 1.0]), 0.1, 0.02, 9000, Wavelength=1e-3)
    assert B.rays_per_source == 300 and B.n_slots == 30 * 300
    B = msource.ExtendedSource(np.zeros(3), np.array([0.0, 0.0, 1.0]), 0.2, 0.02, 40000, Wavelength=1e-3)
    assert B.rays_per_source == 800 and B.n_slots == 50 * 800
    assert B.alias().rays_per_source == 800 and B.copy().rays_per_source == 800
    assert not hasattr(msource.PointSource(np.zeros(3), np.array([0.0, 0.0, 1.0]), 0.02, 100), "rays_per_source")


def _parabola_chain(source_size):
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    SP = {"Divergence": 0.02, "SourceSize": source_size, "Wavelength": 800e-6, "DeltaFT": 1, "NumberRays": 9000}
    par = mmirror.MirrorParabolic(100.0, 30.0, msupp.SupportRound(30.0))
    return mp.OEPlacement(SP, [par], [200.0], [0])


def test_chain_defaults_to_the_sources_rays_per_source(twin):
    import ART.ModuleDetector as mdet
    chain = _parabola_chain(0.05)
    assert chain.source_rays.rays_per_source == 300
    out = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(out, 100.0)
    f = chain.get_FocalImage(D, Pixels=3, Size=0.01)
    assert list(twin.seg) == list(range(0, 9001, 300)) and f.groups == 30
    g = D.get_FocalImage(out, RaysPerSource=300, Pixels=3, Size=0.01)
    assert f.intensity.numpy().tobytes() == g.intensity.numpy().tobytes()
    chain.get_FocalImage(D, RaysPerSource=4500, Pixels=3, Size=0.01)
    assert list(twin.seg) == [0, 4500, 9000]
    chain.get_FocalImage(D, Groups=np.zeros(9000, dtype=int), Pixels=3, Size=0.01)
    assert list(twin.seg) == [0, 9000]
    point = _parabola_chain(0)
    with pytest.raises(ValueError, match="RaysPerSource"):
        point.get_FocalImage(D, Pixels=3, Size=0.01)
    assert point.get_FocalImage(D, RaysPerSource=9000, Pixels=3, Size=0.01).groups == 1


def test_metrics_on_a_hand_made_image():
    from attosecondraytracing_amd.image import FocalImage, image_metrics
    x, y = np.array([-1.0, 0.0, 1.0, 2.0]), np.array([10.0, 20.0, 30.0])
    I = np.zeros((3, 3, 4))
    I[0, 2, 1] = 9.0
    I[0, 0, 3] = 3.0
    I[1, 1, 3] = 2.5
    I[1, 2, 0] = 2.5          # a tie: the first in row-major order
    s, p, r = image_metrics(I, x, y, 18.0)
    assert np.array_equal(s[:2], [0.5, 2.5 / 18.0]) and s[2] == 0.0
    assert np.array_equal(p[:2], [[0.0, 30.0], [2.0, 20.0]])
    # plane 0: x = 0 (weight 3/4) and 2 (1/4): mean 0.5, variance 0.75; y = 30 (3/4) and 10 (1/4): mean 25, variance 75
    assert r[0] == pytest.approx([np.sqrt(0.75), np.sqrt(75.0)], rel=1e-15)
    assert r[1] == pytest.approx([1.5, 5.0], rel=1e-15)
    assert np.isnan(r[2]).all()                                   # no intensity in the plane
    s, p, r = image_metrics(np.zeros((2, 3, 4)), x, y, 0.0)
    assert np.isnan(s).all() and s.shape == (2,) and np.isnan(p).all() and p.shape == (2, 2) and np.isnan(r).all()
    f = FocalImage(torch.from_numpy(I), x, y, (0.0, 0.1, 0.2), 1e-3, 5.0, 7, 12.0, 18.0)
    assert (f.groups, f.power, f.ideal_peak, f.ref_path, f.wavelength) == (7, 12.0, 18.0, 5.0, 1e-3)
    assert np.array_equal(f.strehl, [0.5, 2.5 / 18.0, 0.0]) and list(f.shifts) == [0.0, 0.1, 0.2]


def test_ideal_peak_of_a_perfect_focus_and_of_dead_bundles(twin):
    w = np.linspace(1.0, 2.0, 300)
    B = fc.converging_bundle(300, 0.05, 2.0, backend=twin, weights=w)
    f = _detector().get_FocalImage(B, RaysPerSource=100, Size=0.02, Pixels=5, Centre=(0.0, 0.0))
    a = np.sqrt(w)
    assert f.ideal_peak == pytest.approx(sum(a[i:i + 100].sum() ** 2 for i in (0, 100, 200)), rel=1e-13)
    assert abs(f.strehl[0] - 1.0) <= 1e-12 and np.array_equal(f.peak[0], [0.0, 0.0])   # every group focuses at (0, 0)
    B.alive[:] = 0
    B.touch()
    f = _detector().get_FocalImage(B, RaysPerSource=100, Size=0.02, Pixels=5, Centre=(0.0, 0.0))
    assert not f.intensity.numpy().any() and np.isnan(f.strehl).all() and f.ideal_peak == 0.0 and f.power == 0.0


def test_image_desc_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d\n", sizeof(ArtFocalImageDesc), offsetof(ArtFocalImageDesc, f),
         offsetof(ArtFocalImageDesc, groups), offsetof(ArtFocalImageDesc, reserved), offsetof(ArtFocalImageDesc, seg),
         ART_FOCAL_MAX_GROUPS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    F = _abi.ArtFocalImageDesc
    assert vals == [C.sizeof(F), F.f.offset, F.groups.offset, F.reserved.offset, F.seg.offset, _abi.ART_FOCAL_MAX_GROUPS]
    assert F.f.offset == 0 and F.groups.offset == C.sizeof(_abi.ArtFocalDesc)
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    assert "#define ART_ABI_VERSION %d" % _abi.ART_ABI_VERSION in hdr and _abi.ART_ABI_VERSION == 14
    for name in ("art_focal_image", "art_focal_image_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _abi.PROTOTYPES

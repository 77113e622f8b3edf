"""CPU: the Python layer of the coherent focal field (attosecondraytracing_amd/focal.py, Detector.get_FocalField) against
a NumPy stand-in for art_focal_field on top of the CPU twin backend, and ArtFocalDesc against include/art_hip.h."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import focal_common as fc
from attosecondraytracing_amd import _abi
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)).copy() if n else np.zeros(0)


class NumpyFocalBackend(TwinBackend):
    """art_focal_field's contract in NumPy (tests/focal_common.py); records the last descriptor it was given."""

    def focal_field(self, fdesc, view, w, n):
        self.last = fdesc
        P = np.stack([_host(p, n) for p in (view.ox, view.oy, view.oz)], axis=1) if n else np.zeros((0, 3))
        D = np.stack([_host(p, n) for p in (view.dx, view.dy, view.dz)], axis=1) if n else np.zeros((0, 3))
        alive = _host(view.alive, n, C.c_uint8).astype(bool) if n else np.zeros(0, dtype=bool)
        x = fdesc.x0 + np.arange(fdesc.nx) * fdesc.dx
        y = fdesc.y0 + np.arange(fdesc.ny) * fdesc.dy
        E = fc.field(P, D, _host(view.path, n), alive, None if w is None else w[:n].numpy(), fdesc.k, fdesc.L_ref,
                     fdesc.det.centre[:], fdesc.det.normal[:], fdesc.det.rot[:], x, y,
                     [fdesc.shift[q] for q in range(fdesc.planes)])
        return torch.from_numpy(E)


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyFocalBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _detector(z=0.0):
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, z]), np.array([0.0, 0.0, -1.0]))


def test_defaults_resolve_as_documented(twin):
    import ART.ModuleProcessing as mp
    B = fc.converging_bundle(400, 0.05, 2.0, focus=(0.003, -0.002, 0.0), backend=twin, weights=np.linspace(0.5, 1.5, 400))
    D = _detector()
    f = D.get_FocalField(B, Pixels=9)
    d = twin.last
    airy = mp.ReturnAiryRadius(1e-3, mp.ReturnNumericalAperture(B, 1))
    bb = D.get_PointList2D(B)
    cx, cy = 0.5 * (bb[:, 0].min() + bb[:, 0].max()), 0.5 * (bb[:, 1].min() + bb[:, 1].max())
    assert (d.nx, d.ny, d.planes) == (9, 9, 1) and f.field.shape == (1, 9, 9)
    assert d.x0 == cx - 8 * airy and d.dx == 16 * airy / 8
    assert d.y0 == cy - 8 * airy and d.dy == 16 * airy / 8
    assert np.allclose(f.x, cx + np.linspace(-8 * airy, 8 * airy, 9), rtol=0, atol=1e-15)
    assert np.allclose(f.y, cy + np.linspace(-8 * airy, 8 * airy, 9), rtol=0, atol=1e-15)
    assert d.shift[0] == 0.0 and list(f.shifts) == [0.0]
    assert d.k == 2 * math.pi / 1e-3 and f.wavelength == 1e-3
    assert abs(f.ref_path - D.get_OpticalPaths(B).mean()) <= 1e-15 * 2      # the mean get_Delays subtracts
    assert d.L_ref == f.ref_path
    assert abs(f.amplitude_sum - np.sqrt(np.linspace(0.5, 1.5, 400)).sum()) <= 1e-12 * 400
    assert list(d.det.centre) == list(D.centre) and list(d.det.normal) == list(D.normal)


def test_per_axis_values_shifts_and_ref_path(twin):
    B = fc.converging_bundle(200, 0.05, 2.0, backend=twin)
    D = _detector()
    f = D.get_FocalField(B, Size=(0.02, 0.01), Pixels=(7, 4), Centre=(0.001, -0.002), Shifts=(0.5, -0.25, 0.0),
                         Wavelength=2e-3, RefPath=1.75)
    d = twin.last
    assert f.field.shape == (3, 4, 7) and f.intensity.shape == (3, 4, 7)
    assert np.allclose(f.x, 0.001 + np.linspace(-0.01, 0.01, 7), rtol=0, atol=1e-17)
    assert np.allclose(f.y, -0.002 + np.linspace(-0.005, 0.005, 4), rtol=0, atol=1e-17)
    # Shifts follow Detector.shiftByDistance (away from the optic); the ABI's planes lie at centre + shift * normal
    assert [d.shift[q] for q in range(3)] == [-0.5, 0.25, -0.0]
    assert list(f.shifts) == [0.5, -0.25, 0.0]
    assert d.k == 2 * math.pi / 2e-3 and d.L_ref == 1.75 and f.ref_path == 1.75
    # the oracle's field of the same arguments, and its plane 0 equals a call on a detector moved by shiftByDistance
    E = fc.field_of(B, D, f)
    assert np.abs(f.field.numpy() - E).max() <= 1e-12 * f.amplitude_sum
    D2 = D.copy_detector()
    D2.shiftByDistance(0.5)
    g = D2.get_FocalField(B, Size=(0.02, 0.01), Pixels=(7, 4), Centre=(0.001, -0.002), Wavelength=2e-3, RefPath=1.75)
    assert np.abs(g.field.numpy()[0] - f.field.numpy()[0]).max() <= 1e-10 * f.amplitude_sum


@pytest.mark.parametrize("kw", [dict(Pixels=0), dict(Pixels=2049), dict(Pixels=(4, 4, 4)), dict(Pixels=2.5),
                                dict(Size=-1.0), dict(Size=float("nan")), dict(Size=(1.0, 0.0)),
                                dict(Shifts=[0.0] * 65), dict(Shifts=[0.0, float("inf")]), dict(Shifts=[]),
                                dict(Centre=(0.0, 0.0, 0.0)), dict(Centre=(float("nan"), 0.0)),
                                dict(Wavelength=-1.0), dict(Wavelength=0.0)])
def test_bad_arguments_raise(twin, kw):
    B = fc.converging_bundle(50, 0.05, 2.0, backend=twin)
    kw = dict(dict(Size=0.01), **kw)
    with pytest.raises(ValueError):
        _detector().get_FocalField(B, **kw)


def test_no_wavelength_and_too_small_na_raise(twin):
    B = fc.converging_bundle(50, 0.05, 2.0, backend=twin)
    B.wavelength = None
    with pytest.raises(ValueError, match="wavelength"):
        _detector().get_FocalField(B, Size=0.01)
    assert _detector().get_FocalField(B, Size=0.01, Pixels=3, Wavelength=1e-3).field.shape == (1, 3, 3)
    parallel = fc.converging_bundle(50, 1e-5, 2.0, backend=twin)          # NA 1e-5: ReturnAiryRadius gives 0
    with pytest.raises(ValueError, match="numerical aperture"):
        _detector().get_FocalField(parallel)
    assert _detector().get_FocalField(parallel, Size=0.01, Pixels=3).field.shape == (1, 3, 3)


def test_all_dead_needs_a_centre_and_gives_nan(twin):
    B = fc.converging_bundle(50, 0.05, 2.0, backend=twin)
    B.alive[:] = 0
    B.touch()
    with pytest.raises(ValueError):
        _detector().get_FocalField(B, Size=0.01)
    f = _detector().get_FocalField(B, Size=0.01, Pixels=5, Centre=(0.0, 0.0))
    assert np.all(f.field.numpy() == 0) and np.isnan(f.strehl).all() and np.isnan(f.peak).all()
    assert f.amplitude_sum == 0.0 and f.ref_path == 0.0


def test_strehl_and_peak_on_stand_in_fields():
    from attosecondraytracing_amd.focal import strehl_and_peak
    x, y = np.array([-1.0, 0.0, 1.0, 2.0]), np.array([10.0, 20.0, 30.0])
    I = np.zeros((2, 3, 4))
    I[0, 2, 1] = 9.0
    I[0, 0, 0] = 4.0
    I[1, 1, 3] = 2.5
    I[1, 2, 0] = 2.5          # a tie: the first in row-major order
    s, p = strehl_and_peak(I, x, y, 3.0)
    assert np.array_equal(s, [1.0, 2.5 / 9.0])
    assert np.array_equal(p, [[0.0, 30.0], [2.0, 20.0]])
    s, p = strehl_and_peak(np.zeros((3, 2, 2)), x[:2], y[:2], 0.0)
    assert np.isnan(s).all() and s.shape == (3,) and np.isnan(p).all() and p.shape == (3, 2)


def test_a_perfect_focus_has_strehl_one(twin):
    B = fc.converging_bundle(300, 0.05, 2.0, backend=twin, weights=np.linspace(1.0, 2.0, 300))
    f = _detector().get_FocalField(B, Size=0.02, Pixels=5, Centre=(0.0, 0.0), Shifts=(0.0, 0.3))
    assert abs(f.strehl[0] - 1.0) <= 1e-12 and f.strehl[1] < 0.9
    assert np.array_equal(f.peak[0], [0.0, 0.0])


def test_focal_desc_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(ArtFocalDesc), offsetof(ArtFocalDesc, det),
         offsetof(ArtFocalDesc, k), offsetof(ArtFocalDesc, L_ref), offsetof(ArtFocalDesc, x0), offsetof(ArtFocalDesc, dx),
         offsetof(ArtFocalDesc, y0), offsetof(ArtFocalDesc, dy), offsetof(ArtFocalDesc, nx), offsetof(ArtFocalDesc, ny),
         offsetof(ArtFocalDesc, planes), offsetof(ArtFocalDesc, reserved), offsetof(ArtFocalDesc, shift),
         ART_FOCAL_MAX_PIXELS, ART_FOCAL_MAX_PLANES);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    F = _abi.ArtFocalDesc
    assert vals == [C.sizeof(F), F.det.offset, F.k.offset, F.L_ref.offset, F.x0.offset, F.dx.offset, F.y0.offset,
                    F.dy.offset, F.nx.offset, F.ny.offset, F.planes.offset, F.reserved.offset, F.shift.offset,
                    _abi.ART_FOCAL_MAX_PIXELS, _abi.ART_FOCAL_MAX_PLANES]
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    assert "#define ART_ABI_VERSION %d" % _abi.ART_ABI_VERSION in hdr and _abi.ART_ABI_VERSION >= 13
    for name in ("art_focal_field", "art_focal_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _abi.PROTOTYPES

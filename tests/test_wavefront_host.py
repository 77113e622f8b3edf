"""CPU: the Python layer of the wavefront fit (attosecondraytracing_amd/wavefront.py, Detector.get_Wavefront) against a
NumPy stand-in for art_wavefront on top of the CPU twin backend, its plots under Agg, and ArtWavefrontJob against
include/art_hip.h."""
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
import wavefront_common as wc
from attosecondraytracing_amd import _abi
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)).copy() if n else np.zeros(0)


class NumpyWavefrontBackend(TwinBackend):
    """art_wavefront's contract in NumPy (tests/wavefront_common.py); records the last job table it was given."""

    def wavefront(self, jobs):
        self.last = list(jobs)
        rows = []
        for j in jobs:
            n = j.n
            P = np.stack([_host(p, n) for p in (j.b.ox, j.b.oy, j.b.oz)], axis=1) if n else np.zeros((0, 3))
            D = np.stack([_host(p, n) for p in (j.b.dx, j.b.dy, j.b.dz)], axis=1) if n else np.zeros((0, 3))
            alive = _host(j.b.alive, n, C.c_uint8).astype(bool) if n else np.zeros(0, dtype=bool)
            w = _host(j.w, n) if (j.w and n) else None
            r = wc.rays(P, D, _host(j.b.path, n), alive, w, j.det.centre[:], j.det.normal[:], j.det.rot[:],
                        tuple(j.ref), j.L_ref, tuple(j.pupil))
            for ptr, v in ((j.opd, r["W_all"]), (j.pupil_x, r["x_all"]), (j.pupil_y, r["y_all"])):
                if ptr:
                    np.ctypeslib.as_array((C.c_double * n).from_address(ptr))[:] = np.where(r["used"], v, np.nan)
            rows.append(wc.out_row(r, j.order))
        return torch.from_numpy(np.array(rows))


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyWavefrontBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _detector(z=0.0):
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, z]), np.array([0.0, 0.0, -1.0]))


def _aberrated(twin, coeffs, n=2000, NA=0.05, focus=(0.0, 0.0, 0.0), weights=None):
    """converging_bundle with sum c_nm Z_nm(pupil) added to the paths (pupil: d.e1, d.e2 over the largest radius)."""
    B = fc.converging_bundle(n, NA, 2.0, focus=focus, backend=twin, weights=weights)
    D = _detector()
    d = D._desc()
    rot = np.array(d.rot[:]).reshape(3, 3)
    u = B.data[3:6, :n].numpy().T
    a, b = u @ rot[0], u @ rot[1]
    rho = np.sqrt((a ** 2 + b ** 2).max())
    order = max(k[0] for k in coeffs)
    Z = wc.zernike_matrix(a / rho, b / rho, order)
    keys = [(nn, m) for nn in range(order + 1) for m in range(nn + 1)]
    add = sum(c * Z[keys.index(k)] for k, c in coeffs.items())
    B.data[6, :n] += torch.from_numpy(add)
    B.touch()
    return B, D


def test_defaults_resolve_as_documented(twin):
    B = fc.converging_bundle(500, 0.05, 2.0, focus=(0.002, -0.001, 0.0), backend=twin, weights=np.linspace(0.5, 1.5, 500))
    D = _detector()
    wf = D.get_Wavefront(B)
    j = twin.last[0]
    assert wf.order == 8 and j.order == 8 and len(wf.coefficients) == 45
    assert list(j.ref) == [0.0, 0.0, 0.0] and list(j.pupil) == [0.0, 0.0, 0.0]
    assert wf.centre == (0.0, 0.0) and wf.shift == 0.0 and wf.pupil_centre == (0.0, 0.0)
    assert abs(wf.ref_path - D.get_OpticalPaths(B).mean()) <= 1e-15 * 4 and j.L_ref == wf.ref_path
    u = B.data[3:6, :500].numpy().T
    rot = np.array(D._desc().rot[:]).reshape(3, 3)
    assert abs(wf.pupil_radius - np.sqrt(((u @ rot[0]) ** 2 + (u @ rot[1]) ** 2).max())) <= 1e-15
    assert wf.count == 500 and wf.outside == 0 and wf.wavelength == 1e-3
    assert abs(wf.sum_w - np.linspace(0.5, 1.5, 500).sum()) <= 1e-12
    assert wf.opd is None and wf.pupil is None


def test_coefficient_recovery(twin):
    coeffs = {(2, 0): 3e-5, (2, 1): -2e-5, (3, 1): 1.5e-5, (4, 2): -8e-6, (6, 3): 4e-6, (8, 4): 2e-6}
    B, D = _aberrated(twin, coeffs, weights=np.linspace(0.8, 1.2, 2000))
    wf = D.get_Wavefront(B, Order=8, Wavelength=1e-3)
    big = max(abs(v) for v in coeffs.values())
    for k, v in wf.coefficients.items():      # (piston: W's mean depends on RefPath)
        assert k == (0, 0) or abs(v - coeffs.get(k, 0.0)) <= 1e-10 * big, (k, v)
    assert wf.rms_residual <= 1e-7 * wf.rms
    assert wf.waves[(2, 0)] == pytest.approx(3e-5 / 1e-3, rel=1e-9)
    # per-term rms on the unit disk: defocus 2r^2 - 1 has rms 1/sqrt(3)
    assert wf.term_rms[(2, 1)] == pytest.approx(2e-5 / math.sqrt(3), rel=1e-12)
    assert wf.term_rms[(0, 0)] <= 1e-10 * big
    # the oracle's own least squares on the design matrix
    r = wc.of_bundle(B, D, wf)
    c, res, _, _ = wc.fit(r, 8)
    assert np.abs(np.array(list(wf.coefficients.values())) - c).max() <= 1e-10 * big
    m = wf.map(65)
    assert m.shape == (65, 65) and np.isnan(m[0, 0]) and np.isfinite(m[32, 32])
    assert wf.pv > 0 and np.nanmax(np.abs(wf.map(65, remove=("piston", "tilt", "defocus")))) > 0


@pytest.mark.parametrize("shift", [(0.003, 0.0, 0.0), (0.0, -0.002, 0.0), (0.001, 0.002, -0.05), (0.0, 0.0, 0.08)])
def test_best_reference_point(twin, shift):
    B = fc.converging_bundle(1500, 0.05, 2.0, focus=shift, backend=twin)
    D = _detector()
    wf = D.get_Wavefront(B, Order=4)
    # the focus F in get_FocalField's conventions: X = e1 . (F - C), Y = e2 . (F - C), Shift = -n . (F - C)
    rot = np.array(D._desc().rot[:]).reshape(3, 3)
    F = np.asarray(shift) - D.centre
    want = (rot[0] @ F, rot[1] @ F, -(D.normal @ F))
    X, Y, S = wf.best_focus
    assert np.abs(np.subtract((X, Y, S), want)).max() <= 1e-9, (wf.best_focus, want)
    assert wf.rms_best <= 1e-12 + 1e-9 * wf.rms
    # evaluated at the best point itself the rms is that small, and the fit agrees with the oracle's
    wf2 = D.get_Wavefront(B, Order=4, Centre=(X, Y), Shift=S)
    assert wf2.rms <= 1e-9 * max(wf.rms, 1e-12) + 1e-12
    r = wc.of_bundle(B, D, wf)
    _, _, d, rb = wc.fit(r, 4)
    assert abs(rb - wf.rms_best) <= 1e-12 + 1e-9 * wf.rms


def test_marechal(twin):
    B, D = _aberrated(twin, {(2, 0): 2e-5, (3, 1): 1e-5}, n=1000)
    wf = D.get_Wavefront(B, Wavelength=5e-4)
    assert wf.strehl_marechal == math.exp(-(2 * math.pi * wf.rms_best / 5e-4) ** 2)
    assert 0 < wf.strehl_marechal < 1
    no = D.get_Wavefront(B)
    B.wavelength = None
    nw = D.get_Wavefront(B)
    assert math.isnan(nw.strehl_marechal) and all(math.isnan(v) for v in nw.waves.values())
    assert nw.coefficients == no.coefficients


def test_rays_outside_an_explicit_radius(twin):
    B = fc.converging_bundle(1000, 0.05, 2.0, backend=twin)
    D = _detector()
    full = D.get_Wavefront(B, Order=2)
    wf = D.get_Wavefront(B, Order=2, PupilRadius=0.7 * full.pupil_radius, PupilCentre=(0.001, 0.0), PerRay=True)
    j = twin.last[0]
    assert j.pupil[2] == 0.7 * full.pupil_radius and j.pupil[0] == 0.001
    r = wc.of_bundle(B, D, wf, radius=0.7 * full.pupil_radius)
    assert wf.outside == r["outside"] > 0 and wf.count == 1000 - wf.outside == r["used"].sum()
    assert wf.pupil_radius == 0.7 * full.pupil_radius
    opd = wf.opd.numpy()
    assert np.isnan(opd[~r["used"]]).all() and np.isfinite(opd[r["used"]]).all()
    x, y = wf.pupil.numpy()
    assert (x[r["used"]] ** 2 + y[r["used"]] ** 2 <= 1.0).all()


def test_all_dead_and_empty(twin):
    B = fc.converging_bundle(50, 0.05, 2.0, backend=twin)
    B.alive[:] = 0
    B.touch()
    wf = _detector().get_Wavefront(B, Order=3, RefPath=0.0)
    assert wf.count == 0 and wf.outside == 0 and math.isnan(wf.rms) and math.isnan(wf.rms_best)
    assert all(math.isnan(v) for v in wf.coefficients.values()) and all(math.isnan(v) for v in wf.best_focus)
    assert math.isnan(wf.pupil_radius) and math.isnan(wf.strehl_marechal) and math.isnan(wf.pv)


@pytest.mark.parametrize("kw", [dict(Order=-1), dict(Order=11), dict(Order=2.5), dict(Order=True),
                                dict(Centre=(0.0,)), dict(Centre=(float("nan"), 0.0)), dict(Shift=float("inf")),
                                dict(RefPath=float("nan")), dict(PupilCentre=(0.0, 0.0, 0.0)), dict(PupilRadius=0.0),
                                dict(PupilRadius=-1.0), dict(PupilRadius=float("inf")), dict(Wavelength=0.0),
                                dict(Wavelength=float("nan"))])
def test_bad_arguments_raise(twin, kw):
    B = fc.converging_bundle(50, 0.05, 2.0, backend=twin)
    name = list(kw)[0]
    with pytest.raises(ValueError, match=name):
        _detector().get_Wavefront(B, **kw)


def test_many_requests_one_call(twin):
    B1, D = _aberrated(twin, {(2, 0): 1e-5}, n=300)
    B2 = fc.converging_bundle(700, 0.04, 2.0, backend=twin)
    from attosecondraytracing_amd import wavefront
    calls = []
    orig = twin.wavefront
    twin.wavefront = lambda jobs: calls.append(len(jobs)) or orig(jobs)
    try:
        a, b = wavefront.wavefronts([(B1, D, {"Order": 3}), (B2, D, {"Order": 6, "Shift": 0.1})])
    finally:
        del twin.wavefront
    assert calls == [2] and a.order == 3 and b.order == 6 and b.shift == 0.1
    assert a.coefficients == D.get_Wavefront(B1, Order=3).coefficients


def test_plots_render_under_agg(twin):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    B, D = _aberrated(twin, {(2, 0): 2e-5, (3, 1): 1e-5}, n=800)
    fig = mpl.WavefrontMap(B, D, Order=4, Pixels=33)
    assert fig._art_wavefront.order == 4
    plt.close(fig)

    class Chain:
        def __init__(self, bundle, v):
            self.b, self.loop_variable_value, self.loop_variable_name = bundle, v, "angle"

        def get_output_rays(self):
            return [self.b]

    chains = [Chain(_aberrated(twin, {(2, 0): v * 1e-5}, n=400)[0], v) for v in (0.0, 1.0, 2.0)]
    fig = mpl.WavefrontScan(chains, D, Terms=((2, 0), (3, 1)), Order=3)
    assert [w.coefficients[(2, 0)] for w in fig._art_wavefronts] == pytest.approx([0.0, 1e-5, 2e-5], abs=1e-15)
    plt.close(fig)


def test_wavefront_job_layout_matches_header():
    fields = ["det", "b", "w", "n", "ref", "L_ref", "pupil", "order", "reserved", "opd", "pupil_x", "pupil_y", "out"]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu", sizeof(ArtWavefrontJob));
''' + "".join('  printf(" %%zu", offsetof(ArtWavefrontJob, %s));\n' % f for f in fields) + r'''
  printf(" %d %d %d\n", ART_WAVEFRONT_MAX_ORDER, ART_WAVEFRONT_MAX_COLS, ART_WAVEFRONT_DOUBLES);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    Jt = _abi.ArtWavefrontJob
    assert vals == [C.sizeof(Jt)] + [getattr(Jt, f).offset for f in fields] + [
        _abi.ART_WAVEFRONT_MAX_ORDER, _abi.ART_WAVEFRONT_MAX_COLS, _abi.ART_WAVEFRONT_DOUBLES]
    K = _abi.ART_WAVEFRONT_MAX_COLS
    assert K == (_abi.ART_WAVEFRONT_MAX_ORDER + 1) * (_abi.ART_WAVEFRONT_MAX_ORDER + 2) // 2 + 2
    assert _abi.ART_WAVEFRONT_DOUBLES >= 8 + K * (K + 1) // 2
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    assert "#define ART_ABI_VERSION 14" in hdr and _abi.ART_ABI_VERSION == 14
    for name in ("art_wavefront", "art_wavefront_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _abi.PROTOTYPES

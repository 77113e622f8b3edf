"""CPU: the Python layer of the space-time focal field (attosecondraytracing_amd/pulse.py, Detector.get_FocalPulse)
against a NumPy stand-in for art_focal_spectrum on top of the CPU twin backend, and ArtFocalSpectrumDesc against
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
from attosecondraytracing_amd import _abi
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_FS = 299792458000 * 1e-15        # mm/fs


def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)).copy() if n else np.zeros(0)


class NumpyPulseBackend(TwinBackend):
    """art_focal_spectrum's contract in NumPy: art_focal_field's direct sum (tests/focal_common.py) at every k_j;
    records the last descriptors it was given."""

    def _field(self, fdesc, k, view, w, n):
        P = np.stack([_host(p, n) for p in (view.ox, view.oy, view.oz)], axis=1) if n else np.zeros((0, 3))
        D = np.stack([_host(p, n) for p in (view.dx, view.dy, view.dz)], axis=1) if n else np.zeros((0, 3))
        alive = _host(view.alive, n, C.c_uint8).astype(bool) if n else np.zeros(0, dtype=bool)
        x = fdesc.x0 + np.arange(fdesc.nx) * fdesc.dx
        y = fdesc.y0 + np.arange(fdesc.ny) * fdesc.dy
        return fc.field(P, D, _host(view.path, n), alive, None if w is None else w[:n].numpy(), k, fdesc.L_ref,
                        fdesc.det.centre[:], fdesc.det.normal[:], fdesc.det.rot[:], x, y,
                        [fdesc.shift[q] for q in range(fdesc.planes)])

    def focal_field(self, fdesc, view, w, n):
        self.last = fdesc
        return torch.from_numpy(self._field(fdesc, fdesc.k, view, w, n))

    def focal_spectrum(self, sdesc, view, w, n):
        self.last_spectrum = sdesc
        ks = [sdesc.f.k + j * sdesc.dk for j in range(sdesc.nk)]
        return torch.from_numpy(np.stack([self._field(sdesc.f, k, view, w, n) for k in ks], axis=1))


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyPulseBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _detector(z=0.0):
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, z]), np.array([0.0, 0.0, -1.0]))


def _fwhm_ref(t, I):
    """FWHM of one peak well inside the window: the run of samples >= half around the maximum, its ends interpolated."""
    i = int(np.argmax(I))
    h = I[i] / 2
    a = i
    while I[a - 1] >= h:
        a -= 1
    b = i
    while I[b + 1] >= h:
        b += 1
    left = t[a - 1] + (h - I[a - 1]) / (I[a] - I[a - 1]) * (t[a] - t[a - 1])
    right = t[b] + (I[b] - h) / (I[b] - I[b + 1]) * (t[b + 1] - t[b])
    return right - left


def test_defaults_resolve_as_documented(twin):
    from attosecondraytracing_amd import pulse
    lam, tau = 5e-5, 0.3
    B = fc.converging_bundle(120, 0.05, 2.0, focus=(0.003, -0.002, 0.0), wavelength=lam, backend=twin)
    B.data[6, :60] += 2e-4          # a spread of optical paths: 0.2 um
    B.touch()
    D = _detector()
    p = D.get_FocalPulse(B, tau, Pixels=5)
    sd = twin.last_spectrum
    ops = D.get_OpticalPaths(B)
    T = 16 * tau + 4 * (ops.max() - ops.min()) / C_FS
    assert p.time_window == pytest.approx(T, rel=1e-12) and T > 16 * tau + 2
    w0 = 2 * math.pi * C_FS / lam
    half = math.sqrt(8 * math.log(2) * math.log(1e6)) / tau
    dw = 2 * math.pi / p.time_window
    m = int(half // dw)
    J = len(p.omega)
    assert J == 2 * m + 1 and sd.nk == J and p.spectrum.shape == (1, J, 5, 5) and p.envelope.shape == (1, 256, 5, 5)
    assert p.omega0 == pytest.approx(w0, rel=1e-15) and p.omega[m] == p.omega0
    assert np.allclose(p.omega - w0, (np.arange(J) - m) * dw, rtol=0, atol=1e-12 * w0)
    assert p.omega[-1] - w0 <= half < p.omega[-1] - w0 + dw
    assert sd.f.k == pytest.approx(p.omega[0] / C_FS, rel=1e-15) and sd.dk == pytest.approx(dw / C_FS, rel=1e-15)
    assert np.allclose(p.t, -T / 2 + np.arange(256) * T / 256, rtol=0, atol=1e-12 * T)
    g = np.exp(-(p.omega - w0) ** 2 * tau ** 2 / (8 * math.log(2))) * p.omega / w0
    assert np.allclose(p.weights, g, rtol=1e-14, atol=0)
    # grid, planes, detector and RefPath resolve as get_FocalField's
    f = D.get_FocalField(B, Pixels=5)
    fd = twin.last
    for name in ("x0", "dx", "y0", "dy", "nx", "ny", "planes", "L_ref"):
        assert getattr(sd.f, name) == getattr(fd, name), name
    assert list(sd.f.det.centre) == list(fd.det.centre) and list(sd.f.det.rot) == list(fd.det.rot)
    assert np.array_equal(p.x, f.x) and np.array_equal(p.y, f.y) and p.ref_path == f.ref_path
    assert p.amplitude_sum == f.amplitude_sum


def test_spectrum_slices_are_focal_fields_with_the_weights(twin):
    B = fc.converging_bundle(80, 0.05, 2.0, wavelength=5e-5, backend=twin, weights=np.linspace(0.5, 1.5, 80))
    D = _detector(0.01)
    kw = dict(Size=(0.01, 0.006), Pixels=(5, 3), Centre=(0.0, 0.0), Shifts=(0.0, 0.02), RefPath=2.0)
    p = D.get_FocalPulse(B, 0.5, TimeWindow=6.0, **kw)
    for j in (0, len(p.omega) // 2, len(p.omega) - 1):
        f = D.get_FocalField(B, Wavelength=2 * math.pi * C_FS / p.omega[j], **kw)
        assert np.abs(p.spectrum[:, j].numpy() - p.weights[j] * f.field.numpy()).max() <= 1e-9 * f.amplitude_sum


def test_frequencies_of_weight_zero_still_reach_the_backend(twin):
    """Only the chromatic drivers leave frequencies of weight 0 out of the device call: get_FocalPulse sends them all."""
    B = fc.converging_bundle(12, 0.05, 2.0, wavelength=5e-5, backend=twin)
    p = _detector().get_FocalPulse(B, 0.5, Spectrum=lambda w: np.where(np.arange(len(w)) % 3 == 0, 0.0, 1.0), Size=0.004,
                                   Pixels=3, Centre=(0.0, 0.0), RefPath=2.0, TimeWindow=6.0, Times=8)
    J = len(p.omega)
    zero = p.weights == 0
    assert twin.last_spectrum.nk == J and zero.sum() == (J + 2) // 3 and J > 3
    sp = p.spectrum.numpy()
    assert sp.shape == (1, J, 3, 3) and p.envelope.shape == (1, 8, 3, 3)
    assert not sp[:, zero].any() and np.abs(sp[:, ~zero]).max(axis=(0, 2, 3)).min() > 0


@pytest.mark.parametrize("kw, match", [
    (dict(TimeWindow=4000.0), "wavenumbers"), (dict(DeltaFT=1e-3), "wavenumbers|too short"),
    (dict(Wavelength=1e-3, DeltaFT=1.0), "too short"),
    (dict(DeltaFT=0.0), "DeltaFT"), (dict(DeltaFT=-1.0), "DeltaFT"), (dict(DeltaFT=float("nan")), "DeltaFT"),
    (dict(TimeWindow=0.0), "TimeWindow"), (dict(TimeWindow=float("inf")), "TimeWindow"),
    (dict(Times=0), "Times"), (dict(Times=2.5), "Times"),
    (dict(Spectrum=3.0), "Spectrum"), (dict(Spectrum=lambda w: np.ones(3)), "Spectrum"),
    (dict(Spectrum=lambda w: np.full(len(w), np.nan)), "Spectrum"), (dict(Spectrum=lambda w: 0 * w), "zero"),
    (dict(Pixels=0), "Pixels"), (dict(Shifts=[0.0] * 65), "Shifts")])
def test_bad_arguments_raise(twin, kw, match):
    B = fc.converging_bundle(40, 0.05, 2.0, wavelength=5e-5, backend=twin)
    kw = dict(dict(DeltaFT=0.5, Size=0.01, Pixels=3), **kw)
    with pytest.raises(ValueError, match=match):
        _detector().get_FocalPulse(B, **kw)


def test_the_largest_grid_is_allowed():
    from attosecondraytracing_amd import pulse
    lam, tau = 5e-5, 0.5
    half = pulse.half_span(tau)
    T = (511 + 0.5) * 2 * math.pi / half          # m = 511: 1023 wavenumbers
    assert len(pulse.spectral_grid(lam, tau, T)[1]) == 1023
    with pytest.raises(ValueError, match="1025 wavenumbers"):
        pulse.spectral_grid(lam, tau, (512 + 0.5) * 2 * math.pi / half)


def test_an_in_phase_bundle_has_strehl_one_at_t0(twin):
    B = fc.converging_bundle(150, 0.05, 2.0, wavelength=5e-5, backend=twin, weights=np.linspace(1.0, 2.0, 150))
    p = _detector().get_FocalPulse(B, 0.4, Size=0.004, Pixels=5, Centre=(0.0, 0.0), RefPath=2.0, Shifts=(0.0, 0.05))
    assert abs(p.strehl[0] - 1.0) <= 1e-12 and np.array_equal(p.peak[0], [0.0, 0.0, 0.0])
    assert p.strehl[1] < 0.9
    # the ideal focus: |A| at t = 0 is amplitude_sum, and the pulse front is flat at t = 0
    assert abs(abs(p.envelope.numpy()[0, 128, 2, 2]) - p.amplitude_sum) <= 1e-12 * p.amplitude_sum
    assert abs(p.arrival[0, 2, 2]) <= 1e-9


def test_duration_is_the_fwhm_of_the_transform_of_g(twin):
    B = fc.converging_bundle(100, 0.05, 2.0, wavelength=5e-5, backend=twin)
    kw = dict(Size=0.004, Pixels=3, Centre=(0.0, 0.0), RefPath=2.0, TimeWindow=8.0, Times=512)
    for spectrum in (None, lambda w: np.exp(-(w - w.mean()) ** 2 * 0.5 ** 2 / (8 * math.log(2)) + 0.3j * (w - w.mean()) ** 2)):
        p = _detector().get_FocalPulse(B, 0.5, Spectrum=spectrum, **kw)
        a = np.exp(-1j * (p.omega - p.omega0)[None, :] * p.t[:, None]) @ p.weights / np.abs(p.weights).sum()
        want = _fwhm_ref(p.t, np.abs(a) ** 2)
        assert p.duration[0] == pytest.approx(want, rel=1e-6)
        assert p.duration_integrated[0] == pytest.approx(want, rel=1e-2)       # off-axis pixels differ a little
        if spectrum is None:
            assert p.duration[0] == pytest.approx(0.5, rel=2e-2)                  # the Fourier limit, sampled
            tl = p.duration[0]
        else:
            assert p.duration[0] > 1.5 * tl and p.strehl[0] < 0.7                 # a chirp stretches and dims the pulse


def test_fluence_is_parseval_of_the_spectrum(twin):
    B = fc.converging_bundle(90, 0.05, 2.0, wavelength=5e-5, backend=twin, weights=np.linspace(0.5, 1.0, 90))
    p = _detector(0.02).get_FocalPulse(B, 0.5, Size=0.01, Pixels=(4, 3), Centre=(0.0, 0.0), Times=128)
    assert len(p.omega) <= 128
    S = p.spectrum.numpy()[0] / np.abs(p.weights).sum()
    want = p.time_window * (np.abs(S) ** 2).sum(axis=0)
    assert np.allclose(p.fluence[0], want, rtol=1e-10, atol=0)
    assert np.allclose(p.profile[0], p.intensity[0].sum(axis=(1, 2)), rtol=1e-14)


def test_fwhm_of_stand_in_profiles():
    from attosecondraytracing_amd.pulse import fwhm
    y = np.array([0.0, 1.0, 3.0, 4.0, 3.0, 1.0, 0.0, 0.0])
    assert fwhm(y, 0.5) == pytest.approx((2 * (1 + 1 / 2)) * 0.5)
    assert fwhm(np.roll(y, 5), 0.5) == fwhm(y, 0.5)          # a pulse that wraps round the window
    assert math.isnan(fwhm(np.zeros(8), 1.0)) and math.isnan(fwhm(np.ones(8), 1.0))


def test_all_dead_gives_zeros_and_nan(twin):
    B = fc.converging_bundle(30, 0.05, 2.0, wavelength=5e-5, backend=twin)
    B.alive[:] = 0
    B.touch()
    p = _detector().get_FocalPulse(B, 0.5, Size=0.01, Pixels=3, Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    assert p.time_window == 8.0 and p.amplitude_sum == 0.0
    assert not p.spectrum.numpy().any() and not p.envelope.numpy().any()
    for v in (p.strehl, p.peak, p.duration, p.duration_integrated, p.arrival):
        assert np.isnan(v).all()
    assert not p.fluence.any() and not p.profile.any()


def test_spectrum_desc_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(ArtFocalSpectrumDesc), offsetof(ArtFocalSpectrumDesc, f),
         offsetof(ArtFocalSpectrumDesc, dk), offsetof(ArtFocalSpectrumDesc, nk), offsetof(ArtFocalSpectrumDesc, reserved),
         ART_FOCAL_MAX_WAVENUMBERS, ART_ABI_VERSION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    S = _abi.ArtFocalSpectrumDesc
    assert vals == [C.sizeof(S), S.f.offset, S.dk.offset, S.nk.offset, S.reserved.offset,
                    _abi.ART_FOCAL_MAX_WAVENUMBERS, 14]
    assert _abi.ART_ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    for name in ("art_focal_spectrum", "art_focal_spectrum_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _abi.PROTOTYPES

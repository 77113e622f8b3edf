"""CPU: the Python layer of the chromatic focal pulse (attosecondraytracing_amd/chromatic.py,
Detector.get_ChromaticFocalPulse, OpticalChain.get_ChromaticFocalPulse) against a NumPy stand-in for art_focal_chromatic
(tests/chromatic_common.py) on top of the CPU twin backend; ArtFocalChromaticDesc against include/art_hip.h; and the two
new kernels' resources in the gfx950 code."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import chromatic_common as cc
import focal_common as fc
from attosecondraytracing_amd import _abi
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")
C_FS = 299792458000 * 1e-15        # mm/fs


def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)).copy() if n else np.zeros(0)


def _xyz(view, names, n):
    return np.stack([_host(getattr(view, a), n) for a in names], axis=1) if n else np.zeros((0, 3))


class NumpyChromaticBackend(TwinBackend):
    """art_focal_spectrum's and art_focal_chromatic's contracts in NumPy (tests/focal_common.py, chromatic_common.py);
    records the descriptor and the table of the last chromatic call."""

    def _args(self, fdesc, view, w, n):
        x = fdesc.x0 + np.arange(fdesc.nx) * fdesc.dx
        y = fdesc.y0 + np.arange(fdesc.ny) * fdesc.dy
        alive = _host(view.alive, n, C.c_uint8).astype(bool) if n else np.zeros(0, dtype=bool)
        return (_xyz(view, ("ox", "oy", "oz"), n), _xyz(view, ("dx", "dy", "dz"), n), _host(view.path, n), alive,
                None if w is None else w[:n].numpy()), (fdesc.L_ref, fdesc.det.centre[:], fdesc.det.normal[:],
                                                         fdesc.det.rot[:], x, y, [fdesc.shift[q] for q in range(fdesc.planes)])

    def focal_spectrum(self, sdesc, view, w, n):
        rays, grid = self._args(sdesc.f, view, w, n)
        ks = [sdesc.f.k + j * sdesc.dk for j in range(sdesc.nk)]
        return torch.from_numpy(np.stack([fc.field(*rays, k, *grid) for k in ks], axis=1))

    def focal_chromatic(self, desc, final_view, source_view, w, n, table):
        self.calls = getattr(self, "calls", 0) + 1
        self.last_desc, self.last_table = desc, np.array(table, dtype=float)
        rays, grid = self._args(desc.f, final_view, w, n)
        return torch.from_numpy(cc.field(*rays, _xyz(source_view, ("dx", "dy", "dz"), n), list(desc.axis), self.last_table,
                                         *grid))


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyChromaticBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _detector(z=0.0):
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, z]), np.array([0.0, 0.0, -1.0]))


def _pair(twin, n=90, weights=None, tilt=0.0):
    """An ideal focus and a slot-aligned source bundle: the same cone of directions, leaving one point; `tilt` turns the
    source's cone about y, so that its axis is not +z."""
    from attosecondraytracing_amd.bundle import RayBundle
    B = fc.converging_bundle(n, 0.05, 2.0, wavelength=5e-5, backend=twin, weights=weights)
    d = B.data[3:6, :n].numpy().T.copy()
    c, s = math.cos(tilt), math.sin(tilt)
    d = d @ np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    S = RayBundle.from_arrays(np.zeros((n, 3)), d, wavelength=5e-5, backend=twin)
    return B, S


KW = dict(Size=0.004, Pixels=(5, 3), Centre=(0.0, 0.0), RefPath=2.0, TimeWindow=6.0, Times=64)


def test_the_table_that_reaches_the_backend(twin):
    B, S = _pair(twin, tilt=0.3)
    theta = lambda w: 0.02 + 0.001 * (w - w.min())
    pos = lambda w: 3.0 - 0.5 * (w - w.min())
    p = _detector().get_ChromaticFocalPulse(B, S, 0.5, Divergence=theta, Position=pos, **KW)
    J = len(p.omega)
    t = twin.last_table
    assert t.shape == (J, 4)
    dw = 2 * math.pi / 6.0
    assert np.array_equal(t[:, 0], p.omega[0] / C_FS + np.arange(J) * (dw / C_FS))
    assert np.allclose(t[:, 0], p.omega / C_FS, rtol=1e-14, atol=0)
    assert np.array_equal(t[:, 1], 2.0 / theta(p.omega) ** 2) and np.array_equal(t[:, 2], pos(p.omega))
    assert not t[:, 3].any()
    assert np.array_equal(p.divergence, theta(p.omega)) and np.array_equal(p.position, pos(p.omega))
    # the axis defaults to the source's mean direction, a unit vector about (sin 0.3, 0, cos 0.3)
    a = np.array(twin.last_desc.axis[:])
    assert abs(np.linalg.norm(a) - 1) <= 1e-15 and np.abs(a - [math.sin(0.3), 0.0, math.cos(0.3)]).max() <= 1e-3
    assert np.array_equal(p.axis, a)
    q = _detector().get_ChromaticFocalPulse(B, S, 0.5, Position=-1.5, Axis=(0.0, 0.0, 2.0), **KW)
    assert list(twin.last_desc.axis) == [0.0, 0.0, 1.0]
    assert not twin.last_table[:, 1].any() and (twin.last_table[:, 2] == -1.5).all()
    assert np.isinf(q.divergence).all() and (q.position == -1.5).all()
    # the grid, planes, detector and RefPath resolve as get_FocalPulse's
    f = _detector().get_FocalPulse(B, 0.5, **KW)
    assert np.array_equal(q.x, f.x) and np.array_equal(q.y, f.y) and q.ref_path == f.ref_path
    assert np.array_equal(q.omega, f.omega) and np.array_equal(q.weights, f.weights) and np.array_equal(q.t, f.t)


def test_zero_weight_frequencies_are_left_out_and_their_slices_are_zero(twin):
    from attosecondraytracing_amd import chromatic
    B, S = _pair(twin)
    lam = 5e-5
    comb = chromatic.harmonic_comb(16 * lam, [15, 16, 17], 20.0)
    kw = dict(KW, TimeWindow=40.0, Shifts=(0.0, 0.01))
    p = _detector().get_ChromaticFocalPulse(B, S, 1.5, Position=lambda w: 1e-2 * w, Spectrum=comb, **kw)
    J = len(p.omega)
    keep = np.abs(p.weights) > 0
    assert 0 < keep.sum() < J / 2 and twin.last_table.shape == (keep.sum(), 4)
    assert np.allclose(twin.last_table[:, 0], p.omega[keep] / C_FS, rtol=1e-14, atol=0)
    assert np.array_equal(twin.last_table[:, 2], 1e-2 * p.omega[keep])
    sp = p.spectrum.numpy()
    assert sp.shape == (2, J, 3, 5) and not sp[:, ~keep].any() and np.abs(sp[:, keep]).min() > 0
    assert np.isnan(p.best_focus[~keep]).all() and np.isin(p.best_focus[keep], [0.0, 0.01]).all()
    # the same result as with every frequency in the call: an explicit spectrum that is tiny instead of 0 off the lines
    full = _detector().get_ChromaticFocalPulse(B, S, 1.5, Position=lambda w: 1e-2 * w,
                                               Spectrum=lambda w: comb(w) + 1e-300, **kw)
    assert twin.last_table.shape == (J, 4)
    assert np.abs(full.envelope.numpy() - p.envelope.numpy()).max() <= 1e-12 * p.amplitude_sum
    assert np.abs(full.spectrum.numpy() - sp).max() <= 1e-12 * p.amplitude_sum


def test_amplitude_sum_is_the_ideal_peak_of_the_apodised_source(twin, monkeypatch):
    from attosecondraytracing_amd import chromatic
    w = np.linspace(0.5, 1.5, 90)
    B, S = _pair(twin, weights=w)
    B.alive[::7] = 0
    B.touch()
    S.data[3:6, ::7] = float("nan")            # the source slots of dead rays: whatever they hold
    S.touch()
    theta = lambda om: 0.03 + 0.002 * (om - om.min())
    monkeypatch.setattr(chromatic, "SUM_BLOCK_ELEMENTS", 4 * 90)          # several blocks of frequencies
    p = _detector().get_ChromaticFocalPulse(B, S, 0.5, Divergence=theta, Axis=(0.0, 0.0, 1.0), **KW)
    alive = B.alive[:90].numpy().astype(bool)
    u = cc.source_u(S.data[3:6, :90].numpy().T, [0.0, 0.0, 1.0])[alive]
    Sj = (np.sqrt(w[alive])[None, :] * np.exp(-u[None, :] * (2 / theta(p.omega) ** 2)[:, None])).sum(axis=1)
    want = (np.abs(p.weights) * Sj).sum() / np.abs(p.weights).sum()
    assert p.amplitude_sum == pytest.approx(want, rel=1e-13) and want < 0.9 * np.sqrt(w[alive]).sum()
    # the focus is ideal and the source in phase: the apodised pulse peaks at its own ideal value
    assert p.strehl[0] == pytest.approx(1.0, abs=1e-9)
    assert np.isfinite(p.spectrum.numpy()).all()


def test_neutral_arguments_give_get_FocalPulse_exactly(twin):
    B, S = _pair(twin, weights=np.linspace(1.0, 2.0, 90), tilt=0.2)
    D = _detector(0.01)
    kw = dict(KW, Shifts=(0.0, 0.02))
    f = D.get_FocalPulse(B, 0.5, **kw)
    for extra in (dict(), dict(Position=0.0), dict(Position=lambda w: 0 * w, Axis=(1.0, 0.0, 0.0))):
        p = D.get_ChromaticFocalPulse(B, S, 0.5, **dict(kw, **extra))
        assert p.spectrum.numpy().tobytes() == f.spectrum.numpy().tobytes()
        assert p.envelope.numpy().tobytes() == f.envelope.numpy().tobytes()
        assert p.amplitude_sum == f.amplitude_sum and np.array_equal(p.strehl, f.strehl)
        assert np.array_equal(p.duration, f.duration) and np.array_equal(p.peak, f.peak)


def test_best_focus_follows_the_source_position(twin):
    B, S = _pair(twin, n=300)
    shifts = np.linspace(-0.2, 0.2, 9)
    # 1:1 imaging: a source moved by z downstream moves the focus by z downstream (shiftByDistance's positive sign)
    p = _detector().get_ChromaticFocalPulse(B, S, 0.5, Position=lambda w: np.linspace(-0.15, 0.15, len(w)),
                                            Axis=(0.0, 0.0, 1.0), **dict(KW, Shifts=shifts))
    assert p.best_focus.shape == p.omega.shape and (np.diff(p.best_focus) >= 0).all()
    assert p.best_focus[0] == pytest.approx(-0.15, abs=0.026) and p.best_focus[-1] == pytest.approx(0.15, abs=0.026)


def test_harmonic_comb_and_gaussian_divergence_values():
    from attosecondraytracing_amd import chromatic
    lam, tau = 800e-6, 10.0
    w1 = 2 * math.pi * C_FS / lam
    comb = chromatic.harmonic_comb(lam, [11, 13], tau, Amplitudes=[2.0, 0.5], Phases=[0.0, math.pi / 2])
    width = 4 * math.log(2) / tau
    assert chromatic.line_width(tau) == pytest.approx(width, rel=1e-15)
    om = np.array([11 * w1, 11 * w1 + width / 2, 11 * w1 - 3 * width * (1 - 1e-9), 11 * w1 + 3 * width * (1 + 1e-9), 12 * w1,
                   13 * w1, 13 * w1 - width / 2])
    v = comb(om)
    assert v[0] == 2.0 and abs(v[1]) ** 2 == pytest.approx(2.0, rel=1e-12)        # intensity FWHM = the line width
    assert abs(v[2]) == pytest.approx(2.0 * 2.0 ** -18, rel=1e-6) and v[3] == 0 and v[4] == 0
    assert v[5] == pytest.approx(0.5j, abs=1e-16) and v[6] == pytest.approx(0.5j / math.sqrt(2), abs=1e-12)
    assert comb(np.linspace(11.5 * w1, 12.5 * w1, 50)).tolist() == [0] * 50
    div = chromatic.gaussian_divergence(0.02)
    assert np.allclose(div(np.array([w1, 21 * w1])), [lam / (math.pi * 0.02), lam / 21 / (math.pi * 0.02)], rtol=1e-14)
    div = chromatic.gaussian_divergence(lambda w: 0.02 * w1 / w)          # a waist that shrinks with the order
    assert np.allclose(div(np.array([w1, 21 * w1])), lam / (math.pi * 0.02), rtol=1e-14)
    for bad in (dict(Orders=[]), dict(Orders=[0]), dict(Orders=[11, math.nan]), dict(Amplitudes=[1.0]),
                dict(Phases=[0.0, math.inf]), dict(LineDeltaFT=0.0), dict(FundamentalWavelength=-1.0)):
        with pytest.raises(ValueError):
            chromatic.harmonic_comb(**dict(dict(FundamentalWavelength=lam, Orders=[11, 13], LineDeltaFT=tau), **bad))
    with pytest.raises(ValueError, match="Waist"):
        chromatic.gaussian_divergence(0.0)


@pytest.mark.parametrize("kw, exc, match", [
    (dict(Divergence=0.02), TypeError, "Divergence"), (dict(Position="far"), TypeError, "Position"),
    (dict(Position=1j), TypeError, "Position"), (dict(SourceRays=None), TypeError, "SourceRays"),
    (dict(Divergence=lambda w: 0 * w), ValueError, "Divergence"), (dict(Divergence=lambda w: -1 + 0 * w), ValueError, "Divergence"),
    (dict(Divergence=lambda w: np.full(len(w), np.nan)), ValueError, "Divergence"),
    (dict(Divergence=lambda w: np.ones(3)), ValueError, "Divergence"),
    (dict(Divergence=lambda w: np.full(len(w), 1e-160)), ValueError, "too small"),
    (dict(Position=lambda w: np.full(len(w), np.inf)), ValueError, "Position"),
    (dict(Position=lambda w: np.zeros(2)), ValueError, "Position"), (dict(Position=math.nan), ValueError, "Position"),
    (dict(Axis=(0.0, 0.0, 0.0)), ValueError, "Axis"), (dict(Axis=(1.0, 0.0)), ValueError, "Axis"),
    (dict(Axis=(math.nan, 0.0, 1.0)), ValueError, "Axis"),
    (dict(SourceRays="short"), ValueError, "slot-aligned"),
    (dict(DeltaFT=0.0), ValueError, "DeltaFT"), (dict(Times=0), ValueError, "Times"),
    (dict(Spectrum=lambda w: 0 * w), ValueError, "zero"), (dict(TimeWindow=4000.0), ValueError, "wavenumbers"),
    (dict(Pixels=0), ValueError, "Pixels"), (dict(Shifts=[0.0] * 65), ValueError, "Shifts")])
def test_bad_arguments_raise(twin, kw, exc, match):
    B, S = _pair(twin, n=40)
    calls = getattr(twin, "calls", 0)
    kw = dict(dict(SourceRays=S, DeltaFT=0.5, Size=0.01, Pixels=3), **kw)
    if isinstance(kw["SourceRays"], str):
        kw["SourceRays"] = S.slots(0, 30)
    with pytest.raises(exc, match=match):
        _detector().get_ChromaticFocalPulse(B, **kw)
    assert getattr(twin, "calls", 0) == calls          # refused before the device call


def test_gratings_are_refused():
    import ART.ModuleDetector as mdet
    import ART.ModuleOpticalChain as moc
    import grating_common as gc
    from attosecondraytracing_amd.bundle import RayBundle

    def bundle(grooves):
        b = RayBundle.__new__(RayBundle)
        RayBundle.__init__(b, torch.arange(80, dtype=torch.float64).reshape(8, 10).clone(), torch.ones(10, dtype=torch.uint8),
                           wavelength=30e-6, backend=object(), grooves=torch.zeros(10, dtype=torch.float64) if grooves else None)
        return b

    det = mdet.Detector(np.zeros(3))
    for final, source in ((bundle(True), bundle(False)), (bundle(False), bundle(True))):
        with pytest.raises(NotImplementedError, match="get_SpectralRays"):
            det.get_ChromaticFocalPulse(final, source, 5.0)
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    chain = moc.OpticalChain.__new__(moc.OpticalChain)
    chain._optical_elements = [oe]
    with pytest.raises(NotImplementedError, match="get_ChromaticFocalPulse.*get_SpectralRays"):
        chain.get_ChromaticFocalPulse(det, 5.0)


def test_chain_takes_its_final_and_source_bundles(twin):
    import ART.ModuleDetector as mdet
    import ART.ModuleMirror as mmirror
    import ART.ModuleProcessing as mp
    import ART.ModuleSupport as msupp
    SP = {"Divergence": 0.02, "SourceSize": 0, "Wavelength": 800e-6, "DeltaFT": 1, "NumberRays": 300}
    chain = mp.OEPlacement(SP, [mmirror.MirrorParabolic(100.0, 30.0, msupp.SupportRound(30.0))], [200.0], [0])
    out = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(out, 100.0)
    kw = dict(Divergence=lambda w: 0.015 + 0 * w, Position=0.5, Pixels=3, Size=0.01, TimeWindow=40.0, Times=16)
    a = chain.get_ChromaticFocalPulse(D, 5.0, **kw)
    b = D.get_ChromaticFocalPulse(out, chain.source_rays, 5.0, **kw)
    assert a.envelope.numpy().tobytes() == b.envelope.numpy().tobytes() and a.amplitude_sum == b.amplitude_sum
    assert 0 < a.amplitude_sum < 0.8 * out.n_slots
    with pytest.raises(TypeError):
        chain.get_ChromaticFocalPulse(D, 5.0, Divergance=None)


def test_chromatic_focus_plot_draws(twin):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl, chromatic
    B, S = _pair(twin)
    comb = chromatic.harmonic_comb(16 * 5e-5, [15, 16, 17], 20.0)
    p = _detector().get_ChromaticFocalPulse(B, S, 1.5, Position=lambda w: 1e-2 * w, Spectrum=comb,
                                            **dict(KW, TimeWindow=40.0, Shifts=(0.0, 0.05, -0.05)))
    fig = mpl.ChromaticFocus(p)
    assert fig._art_pulse is p and len(fig.axes) >= 2
    one = _detector().get_ChromaticFocalPulse(B, S, 0.5, **KW)
    assert mpl.ChromaticFocus(one)._art_pulse is one
    plt.close("all")


def test_chromatic_desc_layout_matches_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(ArtFocalChromaticDesc), offsetof(ArtFocalChromaticDesc, f),
         offsetof(ArtFocalChromaticDesc, axis), offsetof(ArtFocalChromaticDesc, nk),
         offsetof(ArtFocalChromaticDesc, reserved), ART_FOCAL_MAX_WAVENUMBERS, ART_ABI_VERSION);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    S = _abi.ArtFocalChromaticDesc
    assert vals == [C.sizeof(S), S.f.offset, S.axis.offset, S.nk.offset, S.reserved.offset,
                    _abi.ART_FOCAL_MAX_WAVENUMBERS, 14]
    assert _abi.ART_ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    for name in ("art_focal_chromatic", "art_focal_chromatic_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _abi.PROTOTYPES
    res, args = _abi.PROTOTYPES["art_focal_chromatic"]
    proto = re.search(r"int art_focal_chromatic\((.*?)\);", hdr, re.S).group(1)
    assert res is C.c_int and len(args) == len(proto.split(",")) == 10
    assert _abi.PROTOTYPES["art_focal_chromatic_scratch_doubles"] == _abi.PROTOTYPES["art_focal_spectrum_scratch_doubles"]


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "art.s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                          stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
        g = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, m.group(2)).group(1))
        res[m.group(1)] = {"vgpr": g("next_free_vgpr"), "lds": g("group_segment_fixed_size"),
                           "scratch": g("private_segment_fixed_size")}
    return res


@pytest.mark.parametrize("kernel", ["k_focal_chromatic_prep", "k_focal_chromatic_field"])
def test_chromatic_kernels_compile_without_scratch(meta, kernel):
    found = [k for k in meta if re.search(r"\d%s[A-Z]" % kernel, k)]
    assert len(found) == 1, found
    m = meta[found[0]]
    assert m["scratch"] == 0, m
    assert m["vgpr"] <= 256, m
    assert m["lds"] <= 80 * 1024, m       # 160 KiB of LDS per CU: two workgroups of the field kernel
    if kernel == "k_focal_chromatic_field":     # the field kernel's LDS footprint, kept
        spec = [k for k in meta if re.search(r"\dk_focal_spectrum_field[A-Z]", k)]
        assert m["lds"] == meta[spec[0]]["lds"]

"""CPU: ArtFocalVectorChromaticDesc and the prototypes of art_focal_vector_chromatic against include/art_hip.h, and the
Python layer on top of them (chromatic.vector_chromatic_focal_pulse, OpticalChain.get_ChromaticFocalPulse with Coatings,
ChromaticFocus) against a NumPy stand-in backend on the CPU twin.

The stand-in keeps the geometry of the contract (tests/vector_pulse_truth.py's direct sum with the paths L + z_j u and
the amplitudes sqrt(w) exp(-u c_j) E_r) but not the coating math, which tests/test_vector_pulse_host.py and the GPU tests
judge: E_r is the input state's transverse part for the ray's source direction, times the complex number n + i kappa
that row j of the material table holds for material 0 of coating 0.  So a material row that does not belong to its table
row shows in the result."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import chromatic_common as cc
import coating_cases as cases
import vector_pulse_truth as vt
from attosecondraytracing_amd import _abi
from test_chromatic_host import _host, _xyz
from test_polarisation_host import _layout
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_FS = 299792458000 * 1e-15        # mm/fs
WL = 13.5e-6


class NumpyVectorBackend(TwinBackend):
    """The stand-in of the module's docstring for art_focal_chromatic (tests/chromatic_common.py),
    art_focal_vector_spectrum and art_focal_vector_chromatic; counts the calls and records the last one's arguments."""

    def __init__(self):
        super().__init__()
        self.calls = {"chromatic": 0, "vector": 0, "vector_chromatic": 0}

    def _grid(self, f):
        x = f.x0 + np.arange(f.nx) * f.dx
        y = f.y0 + np.arange(f.ny) * f.dy
        return (f.L_ref, np.array(f.det.centre[:]), np.array(f.det.normal[:]), np.array(f.det.rot[:]), x, y,
                [f.shift[q] for q in range(f.planes)])

    def focal_chromatic(self, desc, final_view, source_view, w, n, table):
        self.calls["chromatic"] += 1
        self.last_table = np.array(table, dtype=float)
        alive = _host(final_view.alive, n, C.c_uint8).astype(bool)
        return torch.from_numpy(cc.field(_xyz(final_view, ("ox", "oy", "oz"), n), _xyz(final_view, ("dx", "dy", "dz"), n),
                                         _host(final_view.path, n), alive, None if w is None else w[:n].numpy(),
                                         _xyz(source_view, ("dx", "dy", "dz"), n), list(desc.axis), self.last_table,
                                         *self._grid(desc.f)))

    def _vector(self, v, views, materials, axis, table):
        n, K = int(v.n), int(v.n_elems)
        last, src = views[K], views[0]
        alive = _host(last.alive, n, C.c_uint8).astype(bool)
        w = None if not v.w else _host(v.w, n)
        s = _xyz(src, ("dx", "dy", "dz"), n)
        P = np.array(v.pol[:]).reshape(3, 2) @ np.array([1, 1j])
        E = P[None, :] - (s @ P)[:, None] * s
        with np.errstate(invalid="ignore"):
            E = (E / np.sqrt((np.abs(E) ** 2).sum(axis=1))[:, None])[alive]
            u = cc.source_u(s, axis)
        mats = np.asarray(materials, dtype=float)
        out = []
        for j, (k, c, z, _) in enumerate(table):
            r = complex(mats[j, 0, 0, 0], mats[j, 0, 0, 1]) if mats.shape[1] else 1.0
            amp = (E * (r * np.exp(-(u[alive] * c)))[:, None])[:, None, :]
            with np.errstate(invalid="ignore"):
                path = _host(last.path, n) + z * u
            out.append(vt.field(_xyz(last, ("ox", "oy", "oz"), n), _xyz(last, ("dx", "dy", "dz"), n), path, alive, w, amp,
                                [k], *self._grid(v.s.f))[:, 0])
        return torch.from_numpy(np.stack(out, axis=1))

    def focal_vector_spectrum(self, vdesc, views, coatings, materials):
        self.calls["vector"] += 1
        self.last_vector_nk, self.last_vector_materials = int(vdesc.s.nk), np.array(materials, dtype=float)
        k =vdesc.s.f.k + np.arange(vdesc.s.nk) * vdesc.s.dk
        return self._vector(vdesc, views, materials, [0.0, 0.0, 1.0], np.stack([k, 0 * k, 0 * k, 0 * k], axis=1))

    def focal_vector_chromatic(self, vcdesc, views, coatings, materials, table):
        self.calls["vector_chromatic"] += 1
        self.last_table, self.last_materials = np.array(table, dtype=float), np.array(materials, dtype=float)
        self.last_axis, self.last_coatings = list(vcdesc.axis), len(coatings)
        self.last_nk, self.last_bound = int(vcdesc.v.s.nk), int(vcdesc.v.scratch_bound)
        return self._vector(vcdesc.v, views, materials, self.last_axis, self.last_table)


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyVectorBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


@pytest.fixture(scope="module")
def setup(twin):
    """300 rays off one parabola at 13.5 nm, a detector at its focus, and Mo/Si with tabulated materials."""
    import ART.ModuleDetector as mdet
    import ART.ModuleMirror as mmirror
    import ART.ModuleProcessing as mp
    import ART.ModuleSupport as msupp
    SP = {"Divergence": 0.02, "SourceSize": 0, "Wavelength": WL, "DeltaFT": 1, "NumberRays": 300}
    chain = mp.OEPlacement(SP, [mmirror.MirrorParabolic(100.0, 30.0, msupp.SupportRound(30.0))], [200.0], [0])
    out = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(out, 100.0)
    coat = vt.dispersive_copy(cases.mosi(4), WL, 6e-6, 40e-6)
    return chain, D, coat


P = (0.0, 1.0, 0.0)
KW = dict(Pixels=(5, 3), Size=2e-3, TimeWindow=4.0, Times=16, Shifts=(0.0, 0.05))


def _source_axis(chain):
    d = chain.source_rays.data[3:6].numpy().mean(axis=1)
    return d / np.linalg.norm(d)


def _comb():
    from attosecondraytracing_amd import chromatic
    return chromatic.harmonic_comb(15 * WL, [14, 15, 16], 4.0)


# ------------------------------------------------------------------------------------------- the Python layer
def test_only_the_kept_frequencies_reach_the_backend(twin, setup):
    chain, D, coat = setup
    theta = lambda w: 0.02 + 1e-4 * (w - w.min())
    pos = lambda w: 3.0 - 0.01 * (w - w.min())
    before = dict(twin.calls)
    axis = _source_axis(chain)
    p = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, Divergence=theta, Position=pos, Spectrum=_comb(),
                                      Axis=2.0 * axis, ScratchBytes=4096, **KW)
    assert twin.calls == dict(before, vector_chromatic=before["vector_chromatic"] + 1)
    J = len(p.omega)
    keep = np.abs(p.weights) > 0
    assert 3 <= keep.sum() < J - 3
    t = twin.last_table
    assert t.shape == (keep.sum(), 4) and twin.last_nk == keep.sum() and twin.last_bound == 512
    kj = p.omega[0] / C_FS + np.arange(J) * (2 * math.pi / 4.0 / C_FS)
    assert np.array_equal(t[:, 0], kj[keep]) and not t[:, 3].any()
    assert np.array_equal(t[:, 1], (2.0 / theta(p.omega) ** 2)[keep]) and np.array_equal(t[:, 2], pos(p.omega)[keep])
    assert np.abs(np.array(twin.last_axis) - axis).max() <= 1e-15 and twin.last_coatings == 1
    # the materials' rows are those of the kept wavelengths, row for row
    assert twin.last_materials.shape == (keep.sum(), 1, _abi.ART_COATING_MAX_MATERIALS, 2)
    assert np.array_equal(twin.last_materials[:, 0], coat.material_table(2 * math.pi / kj[keep]))
    assert np.ptp(twin.last_materials[:, 0, 0, 0]) > 1e-4           # (they do disperse over the comb)
    assert np.array_equal(p.divergence, theta(p.omega)) and np.array_equal(p.position, pos(p.omega))
    assert np.array_equal(p.axis, twin.last_axis)
    # the skipped slices are 0, the others are not
    sp = p.spectrum.numpy()
    assert sp.shape == (2, J, 3, 3, 5) and p.envelope.shape == (2, 16, 3, 3, 5)
    assert not sp[:, ~keep].any() and np.abs(sp[:, keep]).max(axis=(0, 2, 3, 4)).min() > 0
    # a table outside the material's tabulated range is refused only where a KEPT frequency needs it
    narrow = vt.dispersive_copy(cases.mosi(4), WL, 2 * math.pi / kj[keep].max() * 0.999, 2 * math.pi / kj[keep].min() * 1.001)
    chain.get_ChromaticFocalPulse(D, 0.3, Coatings=narrow, Polarisation=P, Spectrum=_comb(), **KW)
    with pytest.raises(ValueError, match="outside the material's table"):
        chain.get_FocalPulse(narrow, D, 0.3, P, Spectrum=_comb(), **KW)


def test_get_FocalPulse_sends_the_frequencies_of_weight_zero_too(twin, setup):
    """Only the chromatic drivers leave frequencies out: behind the same comb get_FocalPulse sends the whole grid."""
    chain, D, coat = setup
    before = dict(twin.calls)
    p = chain.get_FocalPulse(coat, D, 0.3, P, Spectrum=_comb(), Size=2e-3, Pixels=3, TimeWindow=4.0, Times=8)
    assert twin.calls == dict(before, vector=before["vector"] + 1)
    J = len(p.omega)
    zero = p.weights == 0
    assert 3 < zero.sum() < J - 3
    assert twin.last_vector_nk == J
    assert twin.last_vector_materials.shape == (J, 1, _abi.ART_COATING_MAX_MATERIALS, 2)
    kj = p.omega[0] / C_FS + np.arange(J) * (2 * math.pi / 4.0 / C_FS)
    assert np.array_equal(twin.last_vector_materials[:, 0], coat.material_table(2 * math.pi / kj))
    sp = p.spectrum.numpy()
    assert sp.shape == (1, J, 3, 3, 3) and p.envelope.shape == (1, 8, 3, 3, 3)
    assert not sp[:, zero].any() and np.abs(sp[:, ~zero]).max(axis=(0, 2, 3, 4)).min() > 0


def test_the_same_result_as_with_every_frequency_in_the_call(twin, setup):
    chain, D, coat = setup
    comb = _comb()
    kw = dict(KW, Coatings=coat, Polarisation=P, Position=lambda w: 1e-3 * w, Divergence=lambda w: 0.03 + 0 * w)
    p = chain.get_ChromaticFocalPulse(D, 0.3, Spectrum=comb, **kw)
    full = chain.get_ChromaticFocalPulse(D, 0.3, Spectrum=lambda w: comb(w) + 1e-300, **kw)
    assert twin.last_table.shape == (len(p.omega), 4)
    assert np.abs(full.envelope.numpy() - p.envelope.numpy()).max() <= 1e-12 * p.amplitude_sum
    assert np.abs(full.spectrum.numpy() - p.spectrum.numpy()).max() <= 1e-12 * p.amplitude_sum


def test_without_coatings_the_scalar_call_is_made_as_before(twin, setup):
    chain, D, coat = setup
    before = dict(twin.calls)
    kw = dict(KW, Divergence=lambda w: 0.015 + 0 * w, Position=0.5)
    a = chain.get_ChromaticFocalPulse(D, 0.3, **kw)
    assert twin.calls == dict(before, chromatic=before["chromatic"] + 1)
    b = D.get_ChromaticFocalPulse(chain.get_output_rays()[-1], chain.source_rays, 0.3, **kw)
    from attosecondraytracing_amd import chromatic
    assert type(a) is chromatic.ChromaticFocalPulse and a.spectrum.dim() == 4
    assert a.spectrum.numpy().tobytes() == b.spectrum.numpy().tobytes()
    assert a.envelope.numpy().tobytes() == b.envelope.numpy().tobytes() and a.amplitude_sum == b.amplitude_sum
    c = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=None, **kw)
    assert c.envelope.numpy().tobytes() == b.envelope.numpy().tobytes()


def test_neutral_source_gives_get_FocalPulse_exactly(twin, setup):
    chain, D, coat = setup
    f = chain.get_FocalPulse(coat, D, 0.3, P, **KW)
    for extra in (dict(), dict(Position=0.0), dict(Position=lambda w: 0 * w, Axis=(1.0, 0.0, 0.0))):
        p = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, **dict(KW, **extra))
        assert p.spectrum.numpy().tobytes() == f.spectrum.numpy().tobytes()
        assert p.envelope.numpy().tobytes() == f.envelope.numpy().tobytes()
        assert p.amplitude_sum == f.amplitude_sum and np.array_equal(p.strehl, f.strehl)
        assert np.array_equal(p.duration, f.duration) and np.array_equal(p.longitudinal, f.longitudinal)


def test_amplitude_sum_and_best_focus(twin, setup):
    from attosecondraytracing_amd import chromatic
    chain, D, coat = setup
    B, S = chain.get_output_rays()[-1], chain.source_rays
    n = B.n_slots
    theta = lambda om: 0.03 + 1e-4 * (om - om.min())
    shifts = np.linspace(-0.2, 0.2, 9)
    axis = _source_axis(chain)
    kw = dict(KW, Shifts=shifts, Axis=axis)
    p = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, Divergence=theta, Spectrum=_comb(),
                                      Position=lambda w: np.linspace(-0.15, 0.15, len(w)), **kw)
    keep = np.abs(p.weights) > 0
    alive = B.alive[:n].numpy().astype(bool)
    u = cc.source_u(S.data[3:6, :n].numpy().T, p.axis)[alive]
    w = np.ones(n) if B.intensity is None else B.intensity[:n].numpy()
    Sj = (np.sqrt(w[alive])[None, :] * np.exp(-u[None, :] * (2 / theta(p.omega)[keep] ** 2)[:, None])).sum(axis=1)
    want = (np.abs(p.weights[keep]) * Sj).sum() / np.abs(p.weights).sum()
    assert p.amplitude_sum == pytest.approx(want, rel=1e-13) and want < 0.95 * np.sqrt(w[alive]).sum()
    scalar = chain.get_ChromaticFocalPulse(D, 0.3, Divergence=theta, Spectrum=_comb(), **kw)
    assert p.amplitude_sum == scalar.amplitude_sum                  # (the apodised sum of chromatic_focal_pulse)
    # best_focus: the shift with the largest sum_c |F_c|^2 at the centre pixel, NaN at the skipped frequencies
    assert p.best_focus.shape == p.omega.shape and np.isnan(p.best_focus[~keep]).all()
    on_axis = (np.abs(p.spectrum.numpy()[:, :, :, 1, 2]) ** 2).sum(axis=2)
    assert np.array_equal(p.best_focus[keep], shifts[np.argmax(on_axis[:, keep], axis=0)])
    assert np.ptp(p.best_focus[keep]) > 0                           # (not one plane for all: the argmax is exercised)
    assert 0 < p.strehl.max() <= 1 + 1e-9 and isinstance(p, chromatic.ChromaticVectorFocalPulse)


@pytest.mark.parametrize("kw, exc, match", [
    (dict(Polarisation=None), ValueError, "polarised"), (dict(Polarisation=(1.0, 0.0)), ValueError, "Polarisation"),
    (dict(Coatings=[]), ValueError, "Coatings"), (dict(Coatings=[None]), ValueError, "needs a Coating"),
    (dict(Divergence=0.02), TypeError, "Divergence"), (dict(Position="far"), TypeError, "Position"),
    (dict(Divergence=lambda w: 0 * w), ValueError, "Divergence"),
    (dict(Divergence=lambda w: np.full(len(w), 1e-160)), ValueError, "too small"),
    (dict(Position=lambda w: np.zeros(2)), ValueError, "Position"), (dict(Position=math.nan), ValueError, "Position"),
    (dict(Axis=(0.0, 0.0, 0.0)), ValueError, "Axis"), (dict(Axis=(1.0, 0.0)), ValueError, "Axis"),
    (dict(DeltaFT=0.0), ValueError, "DeltaFT"), (dict(Times=0), ValueError, "Times"),
    (dict(Spectrum=lambda w: 0 * w), ValueError, "zero"), (dict(Pixels=0), ValueError, "Pixels"),
    (dict(Shifts=[0.0] * 65), ValueError, "Shifts"), (dict(ScratchBytes=4), ValueError, "ScratchBytes"),
    (dict(ScratchBytes=16.5), ValueError, "ScratchBytes"), (dict(Polarisation=(0.0, 0.0, 1.0)), ValueError, "parallel"),
    (dict(SourceRays=None), TypeError, "SourceRays"), (dict(Divergance=None), TypeError, "Divergance")])
def test_bad_arguments_raise_before_the_device_call(twin, setup, kw, exc, match):
    chain, D, coat = setup
    before = dict(twin.calls)
    kw = dict(dict(DeltaFT=0.3, Coatings=coat, Polarisation=P, Size=2e-3, Pixels=3, TimeWindow=4.0), **kw)
    if kw["Polarisation"] == (0.0, 0.0, 1.0):                      # along the source's axis: no transverse part on it
        src = chain.source_rays.data[3:6, 0].numpy()
        kw["Polarisation"] = tuple(src)
    with pytest.raises(exc, match=match):
        chain.get_ChromaticFocalPulse(D, kw.pop("DeltaFT"), **kw)
    assert twin.calls == before


def test_polarisation_or_scratch_bytes_without_coatings_are_type_errors(twin, setup):
    chain, D, coat = setup
    before = dict(twin.calls)
    for extra in (dict(Polarisation=P), dict(ScratchBytes=1 << 20), dict(Coatings=None, Polarisation=P)):
        with pytest.raises(TypeError, match="needs Coatings"):
            chain.get_ChromaticFocalPulse(D, 0.3, **dict(KW, **extra))
    with pytest.raises(TypeError):
        chain.get_ChromaticFocalPulse(D, 0.3, coat, **KW)          # (Coatings is given by name)
    assert twin.calls == before


def test_gratings_are_refused_with_coatings_too():
    import ART.ModuleDetector as mdet
    import ART.ModuleOpticalChain as moc
    import grating_common as gc
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    chain = moc.OpticalChain.__new__(moc.OpticalChain)
    chain._optical_elements = [oe]
    with pytest.raises(NotImplementedError, match="get_ChromaticFocalPulse.*get_SpectralRays"):
        chain.get_ChromaticFocalPulse(mdet.Detector(np.zeros(3)), 5.0, Coatings=cases.gold(), Polarisation=P)


def test_chromatic_focus_draws_both_results(twin, setup):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    chain, D, coat = setup
    kw = dict(KW, Shifts=(0.0, 0.05, -0.05), Position=lambda w: 1e-3 * w, Spectrum=_comb())
    vec = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, **kw)
    fig = mpl.ChromaticFocus(vec)
    assert fig._art_pulse is vec and len(fig.axes) >= 2
    mesh = [c for c in fig.axes[0].collections if hasattr(c, "get_array") and c.get_array() is not None][0]
    drawn = np.ma.filled(np.ma.masked_invalid(np.asarray(mesh.get_array(), dtype=float)), 0.0).reshape(-1)
    want = (np.abs(vec.spectrum.numpy()[:, :, :, 1, 2]) ** 2).sum(axis=2)          # [P, J]: sum_c |F_c|^2 on axis
    assert np.isclose(drawn.max(), want.max(), rtol=1e-12) and np.isclose(drawn.sum(), want.sum(), rtol=1e-12)
    sca = chain.get_ChromaticFocalPulse(D, 0.3, **kw)
    assert mpl.ChromaticFocus(sca)._art_pulse is sca
    one = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, **dict(KW, Shifts=None))
    assert mpl.ChromaticFocus(one)._art_pulse is one
    plt.close("all")


# ------------------------------------------------------------------------------------------- the C ABI
def test_layout_matches_header():
    st = _abi.ArtFocalVectorChromaticDesc
    fields = [f[0] for f in st._fields_]
    assert fields == ["v", "axis"]
    assert _layout("ArtFocalVectorChromaticDesc", fields, ["ART_ABI_VERSION"]) == \
        [C.sizeof(st)] + [getattr(st, f).offset for f in fields] + [14]
    assert st.v.offset == 0 and st.axis.offset == C.sizeof(_abi.ArtFocalVectorSpectrumDesc) and _abi.ART_ABI_VERSION == 14


def test_prototypes_match_the_header_text():
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    res, args = _abi.PROTOTYPES["art_focal_vector_chromatic"]
    proto = re.search(r"int art_focal_vector_chromatic\((.*?)\);", hdr, re.S).group(1)
    params = [" ".join(a.split()) for a in proto.split(",")]
    assert params == ["const ArtFocalVectorChromaticDesc* d", "const ArtBundleView* b", "const ArtBundleView* src",
                      "const ArtCoating* coatings_dev", "const ArtCoating* coatings_host",
                      "const ArtCoatingMaterial* materials_host", "const double* table_dev", "const double* table_host",
                      "double* scratch", "double* field", "void* stream"]
    assert res is C.c_int and len(args) == len(params)
    assert args[0]._type_ is _abi.ArtFocalVectorChromaticDesc and args[1]._type_ is args[2]._type_ is _abi.ArtBundleView
    assert args[4]._type_ is _abi.ArtCoating and args[5]._type_ is _abi.ArtCoatingMaterial and args[7] is _abi.c_double_p
    assert all(a is C.c_void_p for a in (args[3], args[6], args[8], args[9], args[10]))     # device pointers, the stream
    assert re.search(r"int64_t art_focal_vector_chromatic_scratch_doubles\(const ArtFocalVectorChromaticDesc\* d\);", hdr)
    res, args = _abi.PROTOTYPES["art_focal_vector_chromatic_scratch_doubles"]
    assert res is C.c_int64 and len(args) == 1 and args[0]._type_ is _abi.ArtFocalVectorChromaticDesc
    doc = hdr[hdr.index("from a CHROMATIC source behind dispersive coatings"):hdr.index("typedef struct ArtFocalVectorChromaticDesc")]
    for text in ("added under ABI 14", "(this order, no fma)", "(sqrt(w_r) * exp(-(u_r * c_j))) * E_r(k_j)",
                 "k_j * (base_r / k + z_j * u_r)", "NOT used", "art_focal_vector_spectrum's bytes", "NaN included",
                 "written, not added to", "no float atomics", "whatever the bound", "| |axis| - 1 | <= 1e-12",
                 "table_host non-NULL", "every c_j finite and", "every z_j finite", "ART_ERR_UNSUPPORTED", "field untouched"):
        assert text in doc, text


def test_python_surface_exists():
    import inspect
    from attosecondraytracing_amd import _lib, chromatic, vector_pulse
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    assert list(inspect.signature(_lib.HipBackend.focal_vector_chromatic).parameters) == \
        ["self", "vcdesc", "views", "coatings", "materials", "table"]
    sig = inspect.signature(chromatic.vector_chromatic_focal_pulse)
    assert list(sig.parameters)[:8] == ["chain", "Coatings", "Detector", "DeltaFT", "Polarisation", "Divergence", "Position",
                                        "Axis"]
    assert sig.parameters["Pixels"].default == 64 and sig.parameters["Times"].default == 256 and "ScratchBytes" in sig.parameters
    assert issubclass(chromatic.ChromaticVectorFocalPulse, vector_pulse.VectorFocalPulse)
    assert inspect.signature(OpticalChain.get_ChromaticFocalPulse).parameters["Coatings"].kind is inspect.Parameter.KEYWORD_ONLY

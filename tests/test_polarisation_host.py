"""CPU: the coating / polarisation oracle of tests/polarisation_common.py against textbook results, coating.Coating,
the Python layer of OpticalChain.get_Polarisation against a NumPy stand-in for art_polarisation on top of the CPU twin
backend, and the ctypes mirror of include/art_hip.h."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import polarisation_common as pcm
from attosecondraytracing_amd import _abi
from attosecondraytracing_amd.coating import Coating
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K13 = 2 * math.pi / 13.5e-6
THETA = np.linspace(0.0, 1.5, 31)


def _tmm(media, thick, s2, k, pol):
    """Characteristic (transfer) matrices, exp(-i w t): M_j = [[cos d, -i sin d / eta], [-i eta sin d, cos d]]."""
    kz = [k * np.sqrt(complex(N) ** 2 - s2 + 0j) for N in media]
    kz = [q if q.imag >= 0 else -q for q in kz]
    eta = [q if pol == "s" else complex(N) ** 2 / q for q, N in zip(kz, media)]
    M = np.eye(2, dtype=complex)
    for j in range(1, len(media) - 1):
        d = kz[j] * thick[j]
        M = M @ np.array([[np.cos(d), -1j * np.sin(d) / eta[j]], [-1j * eta[j] * np.sin(d), np.cos(d)]])
    B, Cc = M @ np.array([1, eta[-1]])
    r = (eta[0] * B - Cc) / (eta[0] * B + Cc)
    return r if pol == "s" else -r          # (p: the admittance form's sign is opposite to r^p's)


def test_single_interface_is_fresnel():
    N = complex(0.97, 0.03)
    s2 = np.sin(THETA) ** 2
    rs, rp = pcm.parratt([1.0, N], [0, 0], [0.0], s2, K13)
    c, q = np.cos(THETA), np.sqrt(N * N - s2)
    assert np.abs(rs - (c - q) / (c + q)).max() < 1e-14
    assert np.abs(rp - (N * N * c - q) / (N * N * c + q)).max() < 1e-14


def test_one_absorbing_layer_is_airy():
    N1, N2, d = complex(0.92, 0.04), complex(0.99, 0.002), 6.5e-6
    for th in THETA:
        s2 = math.sin(th) ** 2
        rs, rp = pcm.parratt([1.0, N1, N2], [0, d, 0], [0.0, 0.0], np.array(s2), K13)
        q0, q1, q2 = (np.sqrt(complex(N) ** 2 - s2) for N in (1.0, N1, N2))
        beta = K13 * d * q1
        for r, (r01, r12) in ((rs, ((q0 - q1) / (q0 + q1), (q1 - q2) / (q1 + q2))),
                              (rp, ((N1 ** 2 * q0 - q1) / (N1 ** 2 * q0 + q1),
                                    (N2 ** 2 * q1 - N1 ** 2 * q2) / (N2 ** 2 * q1 + N1 ** 2 * q2)))):
            e = np.exp(2j * beta)
            assert abs(r - (r01 + r12 * e) / (1 + r01 * r12 * e)) < 1e-13


def test_stack_matches_transfer_matrix():
    mo, si = complex(0.9231, 0.0064), complex(0.999, 0.0018)
    media = [1.0] + [si, mo] * 40 + [si]
    thick = [0.0] + [4.1e-6, 2.8e-6] * 40 + [0.0]
    for th in THETA:
        s2 = math.sin(th) ** 2
        rs, rp = pcm.parratt(media, thick, [0.0] * 81, np.array(s2), K13)
        assert abs(rs - _tmm(media, thick, s2, K13, "s")) < 1e-12
        assert abs(rp - _tmm(media, thick, s2, K13, "p")) < 1e-12


def test_zero_thickness_layers_reduce_to_the_substrate():
    sub = complex(0.95, 0.01)
    s2 = np.sin(THETA) ** 2
    a = pcm.parratt([1.0, complex(0.8, 0.1), complex(0.9, 0.3), sub], [0, 0, 0, 0], [0.0] * 3, s2, K13)
    b = pcm.parratt([1.0, sub], [0, 0], [0.0], s2, K13)
    assert np.abs(a[0] - b[0]).max() < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12


def test_reflectance_bounded_for_absorbing_media():
    rng = np.random.default_rng(1)
    for _ in range(50):
        L = int(rng.integers(0, 6))
        media = [1.0] + [complex(rng.uniform(0.5, 1.5), rng.uniform(0, 0.5)) for _ in range(L + 1)]
        thick = [0.0] + list(rng.uniform(0, 20e-6, L)) + [0.0]
        rs, rp = pcm.parratt(media, thick, list(rng.uniform(0, 1e-6, L + 1)), np.sin(THETA) ** 2, K13)
        assert np.all(np.abs(rs) <= 1 + 1e-14) and np.all(np.abs(rp) <= 1 + 1e-14)


def test_total_external_reflection():
    delta = 0.01
    crit = math.sqrt(2 * delta)                    # grazing angle, to first order
    th = math.pi / 2 - np.linspace(0.1, 0.9, 9) * crit
    rs, rp = pcm.parratt([1.0, 1 - delta], [0, 0], [0.0], np.sin(th) ** 2, K13)
    assert np.abs(np.abs(rs) - 1).max() < 1e-14 and np.abs(np.abs(rp) - 1).max() < 1e-14


def test_normal_incidence_is_isotropic():
    rs, rp = pcm.coating_rs_rp(pcm.mosi(10), np.array([0.0]), K13)
    assert abs(rp[0] + rs[0]) < 1e-14


@pytest.mark.parametrize("make", [pcm.gold, lambda: pcm.mosi(40), Coating.ideal,
                                  lambda: Coating(complex(0.9, 0.1), [(0.97 + 0.02j, 3e-6, 0.0)])])
def test_coating_reflectance_matches_oracle(make):
    c = make()
    rs, rp = c.reflectance(THETA, 13.5e-6)
    o = pcm.coating_rs_rp(c, np.sin(THETA) ** 2, K13)
    assert np.abs(rs - o[0]).max() < 1e-13 and np.abs(rp - o[1]).max() < 1e-13


def test_xuv_form():
    assert Coating((0.01, 0.002)).substrate == complex(0.99, 0.002)


@pytest.mark.parametrize("args", [
    dict(Substrate=float("nan")), dict(Substrate=complex(1, -0.1)), dict(Substrate=(0.1, -0.01)),
    dict(Substrate=1.0, Layers=[(1.0, -1e-6, 0.0)]), dict(Substrate=1.0, Layers=[(1.0, 1e-6, float("inf"))]),
    dict(Substrate=1.0, Roughness=-1.0), dict(Substrate=1.0, Layers=[(1.0, 1e-6, 0.0)] * 257),
    dict(Substrate=1.0, Layers=[(1.0 + 0.01j * k, 1e-6, 0.0) for k in range(7)]),
    dict(Substrate=1.0, Layers=[(1.0, 1e-6)])])
def test_bad_coatings_raise(args):
    with pytest.raises(ValueError):
        Coating(**args)


def test_bad_wavelength_raises():
    with pytest.raises(ValueError):
        pcm.gold().reflectance(0.1, 0.0)


# --------------------------------------------------------------------------------------- the Python layer
def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)).copy() if n else np.zeros(0)


def _coating_of(st):
    """A Coating-like object with the fields the oracle reads, from an ArtCoating."""
    class Cz:
        pass
    c = Cz()
    c.is_ideal = bool(st.ideal)
    mats = [complex(st.materials[m].n, st.materials[m].kappa) for m in range(st.n_materials)]
    c.substrate = mats[st.substrate] if mats else 1.0
    c.layers = [(mats[st.layers[l].material], st.layers[l].thickness, st.layers[l].roughness) for l in range(st.n_layers)]
    c.roughness = st.roughness
    return c


class NumpyPolarisationBackend(TwinBackend):
    """art_polarisation's contract in NumPy (tests/polarisation_common.py); records what it was given."""
    basis = None

    def polarisation(self, jobs, views, coatings):
        self.last = (list(jobs), list(views), list(coatings))
        rows = []
        for j, v in zip(jobs, views):
            n, K = j.n, j.n_elems
            dirs = [np.stack([_host(getattr(v[e], a), n) for a in ("dx", "dy", "dz")], axis=1) if n else np.zeros((0, 3))
                    for e in range(K + 1)]
            a0 = _host(v[0].alive, n, C.c_uint8)
            a = _host(v[K].alive, n, C.c_uint8)
            coats = [None if j.coating[e] < 0 else _coating_of(coatings[j.coating[e]]) for e in range(K)]
            P = None if not j.polarised else np.array([complex(j.pol[2 * q], j.pol[2 * q + 1]) for q in range(3)])
            det = None
            if j.has_det:
                rot = np.array(j.det.rot[:]).reshape(3, 3)
                det = (rot[0], rot[1], np.array(j.det.normal[:]))
            w = _host(j.w, n) if j.w else None
            w0 = _host(j.w0, n) if j.w0 else None
            basis = None if self.basis is None else self.basis(dirs[0])
            r = pcm.run(dirs, a0, a, coats, j.k, P, w, w0, det, basis)
            if n:
                np.ctypeslib.as_array((C.c_double * n).from_address(j.w_out))[:] = r["w_out"]
                if j.field:
                    f = np.ctypeslib.as_array((C.c_double * (6 * n)).from_address(j.field)).reshape(3, n, 2)
                    f[..., 0], f[..., 1] = r["E"].T.real, r["E"].T.imag
            rows.append(r["row"])
        return torch.from_numpy(np.array(rows))


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyPolarisationBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _c3(twin, twist=30.0, n=400):
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    SP = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": n}
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 41e-3 / 2 * 500, 0, 0))
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    tw = twist if isinstance(twist, list) else [twist]
    chains = mp.OEPlacement(SP, [Mask, Tor, Tor], [500, 100, 600], [0, 80, -80], [0, 0, tw], "C3")
    return chains if isinstance(twist, list) else chains[0]


def test_job_table(twin):
    ch = _c3(twin)
    g = pcm.gold()
    pol = ch.get_Polarisation(g, Polarisation=(1, 1j, 0))
    jobs, views, coats = twin.last
    j = jobs[0]
    assert j.n_elems == 3 and list(j.coating[:3]) == [-1, 0, 0] and len(coats) == 1
    assert j.polarised == 1 and list(j.pol) == [1, 0, 0, 1, 0, 0] and j.has_det == 0
    assert j.k == pytest.approx(2 * math.pi / 50e-6, rel=1e-15)
    out = ch.get_output_rays()
    assert views[0][0].dx == ch.source_rays.view().dx and views[0][3].alive == out[-1].view().alive
    assert j.n == out[-1].n_slots
    assert pol.count == int(out[-1].alive.sum()) and 0 < pol.transmission < 100


def test_coating_lists_and_masks(twin):
    ch = _c3(twin)
    g = pcm.gold()
    a = ch.get_Polarisation([None, g, g])
    b = ch.get_Polarisation(g)
    assert np.array_equal(a.throughput.numpy(), b.throughput.numpy())
    for bad in ([g, g, g], [None, None, g], [None, g]):
        with pytest.raises(ValueError):
            ch.get_Polarisation(bad)
    with pytest.raises(ValueError):
        ch.get_Polarisation(g, PerRay=True)            # needs a polarised input
    with pytest.raises(ValueError):
        ch.get_Polarisation(g, Polarisation=(1, 2))
    with pytest.raises(ValueError):
        ch.get_Polarisation(g, Wavelength=-1.0)


def test_unpolarised_is_basis_invariant(twin):
    import ART.ModuleDetector as mdet
    ch = _c3(twin)
    D = mdet.Detector(np.asarray(ch.optical_elements[-1].position, dtype=float))
    D.autoplace(ch.get_output_rays()[-1], 300.0)
    a = ch.get_Polarisation(pcm.mosi(5), Detector=D)

    def rotated(d0):
        u1 = pcm.perp_unit(d0)
        u2 = np.cross(d0, u1)
        t = 0.7
        return [math.cos(t) * u1 + math.sin(t) * u2, -math.sin(t) * u1 + math.cos(t) * u2]
    twin.basis = rotated
    try:
        b = ch.get_Polarisation(pcm.mosi(5), Detector=D)
    finally:
        twin.basis = None
    assert np.allclose(a.throughput.numpy(), b.throughput.numpy(), rtol=1e-13, atol=0)
    assert np.allclose(a.stokes, b.stokes, rtol=1e-12, atol=1e-12 * a.stokes[0])


def test_rays_feed_get_e_transmission(twin):
    import ART.ModuleAnalysisAndPlots as mpl
    ch = _c3(twin)
    pol = ch.get_Polarisation(pcm.gold())
    assert pol.rays.intensity is pol.throughput
    assert mpl.getETransmission(ch.source_rays, pol.rays) == pytest.approx(pol.transmission, rel=1e-12)
    assert pol.transmission < mpl.getETransmission(ch.source_rays, ch.get_output_rays()[-1])


def test_batch_equals_separate_calls(twin):
    from attosecondraytracing_amd.polarisation import polarisations
    chains = _c3(twin, [-60.0, 0.0, 45.0])
    reqs = [(ch, pcm.gold(), {"Polarisation": (0, 1, 0)}) for ch in chains]
    many = polarisations(reqs)
    assert len(twin.last[0]) == 3
    for p, (ch, c, kw) in zip(many, reqs):
        q = ch.get_Polarisation(c, **kw)
        assert np.array_equal(p.throughput.numpy(), q.throughput.numpy()) and p.transmission == q.transmission


# --------------------------------------------------------------------------------------- the C ABI
def _layout(struct, fields, consts=()):
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"art_hip.h\"\nint main(void) {\n"
    src += '  printf("%%zu", sizeof(%s));\n' % struct
    src += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields)
    src += "".join('  printf(" %%d", %s);\n' % c for c in consts)
    src += '  printf("\\n");\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        return [int(v) for v in subprocess.check_output([exe]).split()]


@pytest.mark.parametrize("name", ["ArtCoatingMaterial", "ArtCoatingLayer", "ArtCoating", "ArtPolarisationJob"])
def test_layout_matches_header(name):
    st = getattr(_abi, name)
    fields = [f[0] for f in st._fields_]
    assert _layout(name, fields) == [C.sizeof(st)] + [getattr(st, f).offset for f in fields]


def test_constants_and_version():
    consts = ["ART_COATING_MAX_LAYERS", "ART_COATING_MAX_MATERIALS", "ART_POLARISATION_MAX_ELEMS",
              "ART_POLARISATION_DOUBLES", "ART_ABI_VERSION"]
    assert _layout("ArtCoatingMaterial", [], consts)[1:] == [getattr(_abi, c) for c in consts]
    assert _abi.ART_ABI_VERSION == 14 and _abi.ART_COATING_MAX_LAYERS == 256
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    for name in ("art_polarisation", "art_polarisation_scratch_doubles"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _abi.PROTOTYPES

"""GPU (-m gpu): art_polarisation and OpticalChain.get_Polarisation against the NumPy oracle of
tests/polarisation_common.py on traced histories, a 90-degree periscope, ideal coatings, determinism, batching,
composition with the other analyses, and edge cases."""
import math

import numpy as np
import pytest

import polarisation_common as pcm
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch
    import __graft_entry__
    from attosecondraytracing_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    __graft_entry__.ensure_built()
    _lib._BACKEND = None
    be = _lib.get_backend()
    assert be.name == "hip"
    return be


def _history(chain):
    """Directions of the source and of every bundle of the history, alive bytes, weights: host arrays."""
    src, out = chain.source_rays, chain.get_output_rays()
    bundles = [src] + [out[k] for k in range(len(chain.optical_elements))]
    dirs = [b.data[3:6].cpu().numpy().T.copy() for b in bundles]
    w = lambda b: None if b.intensity is None else b.intensity.cpu().numpy()
    return dirs, src.alive.cpu().numpy(), bundles[-1].alive.cpu().numpy(), w(src), w(bundles[-1])


def _detector(chain):
    import ART.ModuleDetector as mdet
    last = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 300.0)
    d = D._desc()
    rot = np.array(d.rot[:]).reshape(3, 3)
    return D, (rot[0], rot[1], np.array(d.normal[:]))


def _check(pol, chain, coats, P=None, det=None, tol=1e-12):
    from attosecondraytracing_amd.polarisation import resolve_coatings
    dirs, a0, a, w0, w = _history(chain)
    k = 2 * math.pi / chain.get_output_rays()[-1].wavelength
    ref = pcm.run(dirs, a0, a, resolve_coatings(chain.optical_elements, coats), k, P, w, w0, det)
    live = a.astype(bool)
    T = pol.throughput.cpu().numpy()
    wv = np.ones(len(a)) if w is None else w
    assert np.all(T[~live] == 0)
    assert np.all(np.abs(T - ref["w_out"]) <= tol * np.abs(wv * ref["T"]) + 1e-300)
    assert pol.count == int(live.sum())
    assert pol.sum_w_out == pytest.approx(ref["row"][2], rel=tol)
    assert pol.t_min == pytest.approx(ref["row"][3], rel=tol) and pol.t_max == pytest.approx(ref["row"][4], rel=tol)
    if det is not None:
        S0 = ref["row"][5]
        assert np.all(np.abs(np.array(pol.stokes) - ref["row"][5:9]) <= tol * S0)
        assert abs(pol.longitudinal_sum - ref["row"][9]) <= tol * S0
    if pol.field is not None:
        E = pol.field.cpu().numpy().T
        assert np.all(np.abs(E - ref["E"]) <= tol * np.maximum(np.linalg.norm(ref["E"], axis=1), 1e-300)[:, None])
    return ref


@pytest.fixture(scope="module")
def relay4(hip):
    import torch
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=20000)
    g = torch.Generator(device="cpu").manual_seed(3)
    chain.source_rays.intensity = torch.rand(chain.source_rays.n_slots, generator=g, dtype=torch.float64).to(hip.device) + 0.5
    chain.get_output_rays()
    return chain


@pytest.mark.parametrize("P", [None, (0, 0, 1), (1 / math.sqrt(2), 1j / math.sqrt(2), 0)])
def test_relay4_against_oracle(relay4, P):
    D, det = _detector(relay4)
    pol = relay4.get_Polarisation(pcm.gold(), Polarisation=P, Detector=D, PerRay=P is not None)
    _check(pol, relay4, pcm.gold(), P, det)
    assert 0 < pol.transmission < 100


def test_relay4_multilayer_against_oracle(relay4):
    D, det = _detector(relay4)
    pol = relay4.get_Polarisation(pcm.mosi(40), Detector=D)
    _check(pol, relay4, pcm.mosi(40), None, det, tol=1e-10)


@pytest.mark.parametrize("name", ["c3_twisted_chain04", "c4_mixed8", "c2_fxf_chain05"])
def test_golden_chains_against_oracle(hip, name):
    import parity_common as pc
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    from attosecondraytracing_amd.polarisation import resolve_coatings
    scene, arr = load_golden(name)
    src = pc.source_bundle(arr, scene)
    els = pc.build_elements(scene, arr)
    chain = OpticalChain(src, els)
    if src.wavelength is None:
        src.wavelength = 50e-6
    chain.get_output_rays()
    coats = [None if getattr(oe.type, "type", "") == "Mask" else pcm.gold() for oe in els]
    D, det = _detector(chain)
    for P in (None, (0, 1, 1j)):
        pol = chain.get_Polarisation(coats, Polarisation=P, Detector=D, PerRay=P is not None)
        _check(pol, chain, coats, P, det)
    # the oracle on the GOLDEN directions (the reference's trace): the device's history agrees with it to 1e-9
    pol = chain.get_Polarisation(coats, Detector=D)
    K = len(els)
    if all(("out%d_vector" % e) in arr for e in range(K)):
        surv = arr["out%d_number" % (K - 1)]
        idx = {int(v): i for i, v in enumerate(arr["src_number"])}
        rows = [idx[int(v)] for v in surv]
        dirs = [arr["src_vector"][rows]]
        for e in range(K):
            num = arr["out%d_number" % e]
            pos = {int(v): i for i, v in enumerate(num)}
            dirs.append(arr["out%d_vector" % e][[pos[int(v)] for v in surv]])
        dirs = [d / np.linalg.norm(d, axis=1)[:, None] for d in dirs]
        m = len(surv)
        ref = pcm.run(dirs, np.ones(m), np.ones(m), resolve_coatings(els, coats), 2 * math.pi / src.wavelength)
        T = pol.throughput.cpu().numpy()[rows]
        w = np.ones(len(rows)) if src.intensity is None else src.intensity.cpu().numpy()[rows]
        assert np.abs(T - w * ref["T"]).max() <= 1e-9


def _periscope(hip, n=2000):
    """Two plane mirrors at 45 degrees: +z -> +x, then +x -> +y (the second plane of incidence is perpendicular)."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalElement as moe
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    rng = np.random.default_rng(5)
    pts = np.zeros((n, 3))
    pts[:, :2] = rng.uniform(-1, 1, (n, 2))
    vec = np.tile([0.0, 0.0, 1.0], (n, 1))
    src = RayBundle.from_arrays(pts, vec, np.arange(n), np.ones(n), 13.5e-6, backend=hip)
    M = mmirror.MirrorPlane(msupp.SupportRectangle(40, 40))
    m1 = moe.OpticalElement(M, np.array([0.0, 0.0, 100.0]), np.array([-1.0, 0.0, 1.0]) / math.sqrt(2), np.array([0.0, 1.0, 0.0]))
    m2 = moe.OpticalElement(M, np.array([100.0, 0.0, 100.0]), np.array([1.0, -1.0, 0.0]) / math.sqrt(2), np.array([0.0, 0.0, 1.0]))
    return OpticalChain(src, [m1, m2])


def _coplanar_pair(hip, n=500):
    """Two plane mirrors at 45 degrees with the same plane of incidence (x-z): +z -> +x, then +x -> +z."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalElement as moe
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    ch = _periscope(hip, n)
    M = mmirror.MirrorPlane(msupp.SupportRectangle(40, 40))
    m2 = moe.OpticalElement(M, np.array([100.0, 0.0, 100.0]), np.array([1.0, 0.0, -1.0]) / math.sqrt(2),
                            np.array([0.0, 1.0, 0.0]))
    return OpticalChain(ch.source_rays, [ch.optical_elements[0], m2])


def _normal_mirror(hip, n=4000):
    """One plane mirror facing -z, met head on: a quarter of the rays exactly along +z (d_in x d_out = 0), a quarter
    tilted by 1e-14 (|d_in x d_out| ~ 2e-14, below the 1e-12 of the fallback frame), the rest by up to 1e-3."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalElement as moe
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    rng = np.random.default_rng(9)
    pts = np.zeros((n, 3))
    pts[:, :2] = rng.uniform(-1, 1, (n, 2))
    vec = np.tile([0.0, 0.0, 1.0], (n, 1))
    q = n // 4
    vec[q:2 * q, :2] = rng.uniform(-1e-14, 1e-14, (q, 2))
    vec[2 * q:, :2] = rng.uniform(-1e-3, 1e-3, (n - 2 * q, 2))
    src = RayBundle.from_arrays(pts, vec, np.arange(n), np.ones(n), 13.5e-6, backend=hip)
    M = mmirror.MirrorPlane(msupp.SupportRectangle(40, 40))
    el = moe.OpticalElement(M, np.array([0.0, 0.0, 100.0]), np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0]))
    return OpticalChain(src, [el]), q


def test_normal_incidence_against_oracle(hip):
    ch, q = _normal_mirror(hip)
    out = ch.get_output_rays()[-1]
    assert out.alive.cpu().numpy().all()
    dirs, _, _, _, _ = _history(ch)
    m = np.linalg.norm(np.cross(dirs[0], dirs[1]), axis=1)
    assert np.all(m[:2 * q] < 1e-12) and np.all(m[2 * q:] > 1e-12)      # both frames are exercised
    D, det = _detector(ch)
    c = pcm.mosi(40)
    _check(ch.get_Polarisation(c, Detector=D), ch, c, None, det, tol=1e-10)
    Tx = _check(ch.get_Polarisation(c, Polarisation=(1, 0, 0), Detector=D, PerRay=True), ch, c, (1, 0, 0), det,
                tol=1e-10)["T"]
    Ty = _check(ch.get_Polarisation(c, Polarisation=(0, 1j, 0), Detector=D, PerRay=True), ch, c, (0, 1j, 0), det,
                tol=1e-10)["T"]
    # at normal incidence rp = -rs: the mirror is isotropic, whatever frame the fallback picked
    assert np.abs(Tx[:2 * q] - Ty[:2 * q]).max() <= 1e-12 * Tx[:2 * q].max()


def test_periscope(hip):
    ch = _periscope(hip)
    out = ch.get_output_rays()
    assert out[-1].alive.cpu().numpy().all()
    d = out[-1].data[3:6].cpu().numpy().T
    assert np.abs(d - [0, 1, 0]).max() < 1e-12
    c = pcm.gold()
    rs, rp = c.reflectance(math.pi / 4, 13.5e-6)
    expect = abs(rs) ** 2 * abs(rp) ** 2
    # first plane of incidence x-z: s1 = y, p1 = x; a linear input along either comes out along the other's role
    for P, along in (((0, 1, 0), 0), ((1, 0, 0), 2)):
        pol = ch.get_Polarisation(c, Polarisation=P, PerRay=True)
        T = pol.throughput.cpu().numpy()
        assert np.abs(T - expect).max() <= 1e-12 * expect
        E = pol.field.cpu().numpy()
        # s1 = y becomes p2 (along x), p1 = x becomes s2 (along z): each rotated by 90 degrees about the beam
        other = [k for k in range(3) if k not in (along, 1)][0]
        assert np.abs(E[1]).max() < 1e-12
        assert np.abs(E[other]).max() < 1e-12 * math.sqrt(expect)
        assert np.abs(np.abs(E[along]) - math.sqrt(expect)).max() < 1e-12


def test_ideal_coatings(hip, relay4):
    from attosecondraytracing_amd.coating import Coating
    pol = relay4.get_Polarisation(Coating.ideal(), Polarisation=(1, 1j, 0), PerRay=True)
    last = relay4.get_output_rays()[-1]
    live = last.alive.cpu().numpy().astype(bool)
    w = last.intensity.cpu().numpy()
    T = pol.throughput.cpu().numpy()
    assert np.abs(T[live] - w[live]).max() <= 1e-14 * w.max()
    E = pol.field.cpu().numpy().T[live]
    d = last.data[3:6].cpu().numpy().T[live]
    assert np.abs(np.sum(E * d, axis=1)).max() < 1e-13
    # a plane-only chain whose planes of incidence are all equal keeps s as s: two plane mirrors, both planes of
    # incidence x-z (+z -> +x -> +z), s along y at each; an s input stays along y, a p input stays in the x-z plane
    ch = _coplanar_pair(hip)
    d = ch.get_output_rays()[-1].data[3:6].cpu().numpy().T
    assert np.abs(d - [0, 0, 1]).max() < 1e-12
    pol = ch.get_Polarisation(Coating.ideal(), Polarisation=(0, 1, 0), PerRay=True)
    E = pol.field.cpu().numpy()
    assert np.abs(np.abs(E[1]) - 1).max() < 1e-14 and np.abs(E[0]).max() < 1e-14 and np.abs(E[2]).max() < 1e-14
    pol = ch.get_Polarisation(Coating.ideal(), Polarisation=(1, 0, 0), PerRay=True)
    E = pol.field.cpu().numpy()
    assert np.abs(E[1]).max() < 1e-14 and np.abs(np.abs(E[0]) - 1).max() < 1e-13


def test_determinism_and_batching(hip):
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd import polarisation as pmod
    import ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp
    SP = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": 3000}
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 41e-3 / 2 * 500, 0, 0))
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    chains = mp.OEPlacement(SP, [Mask, Tor, Tor], [500, 100, 600], [0, 80, -80],
                            [0, 0, np.linspace(-90, 90, 10).tolist()], "C3")
    c = pcm.gold()
    D, _ = _detector(chains[0])
    reqs = [(ch, c, {"Detector": D}) for ch in chains]
    many = pmod.polarisations(reqs)
    again = pmod.polarisations(reqs)
    for a, b, (ch, _, kw) in zip(many, again, reqs):
        single = ch.get_Polarisation(c, **kw)
        for x in (b, single):
            assert np.array_equal(a.throughput.cpu().numpy(), x.throughput.cpu().numpy())
            assert a.stokes == x.stokes and a.transmission == x.transmission
    # a lazy history gives the same bytes as the full one
    lazy = mp.OEPlacement(SP, [Mask, Tor, Tor], [500, 100, 600], [0, 80, -80], [0, 0, 30.0], "C3")
    full = mp.OEPlacement(SP, [Mask, Tor, Tor], [500, 100, 600], [0, 80, -80], [0, 0, 30.0], "C3")
    lazy.get_output_rays(history="lazy")
    a = lazy.get_Polarisation(c)
    b = full.get_Polarisation(c)
    assert np.array_equal(a.throughput.cpu().numpy(), b.throughput.cpu().numpy())


def test_composition(hip, relay4):
    import ART.ModuleAnalysisAndPlots as mpl
    D, _ = _detector(relay4)
    pol = relay4.get_Polarisation(pcm.gold(), Detector=D)
    w_out = pol.throughput.cpu().numpy()
    assert mpl.getETransmission(relay4.source_rays, pol.rays) == pytest.approx(pol.transmission, rel=1e-12)
    f = D.get_FocalField(pol.rays, Pixels=8, Size=0.01)
    assert f.amplitude_sum == pytest.approx(np.sqrt(w_out).sum(), rel=1e-12)
    # the spot image's intensities sum to sum w_out within the histogram's fixed-point bound n 2^-(S+1)
    h = D.get_Histogram(pol.rays, ("X", "Y"), 64)
    total = float(h.intensity.sum()) + (h.outside[1] or 0.0)
    assert int(h.counts.sum()) + h.outside[0] == pol.count
    assert abs(total - w_out.sum()) <= pol.count * 2.0 ** -(h.shift + 1) + 1e-12 * w_out.sum()


def test_edges(hip, relay4):
    import torch
    # relay4's source runs along +x: a polarisation along it is an error
    with pytest.raises(ValueError):
        relay4.get_Polarisation(pcm.gold(), Polarisation=(1, 0, 0))
    # all slots dead: zeros, no NaN
    D = _detector(relay4)[0]
    last = relay4.get_output_rays()[-1]
    saved = last.alive.clone()
    last.alive.zero_()
    try:
        pol = relay4.get_Polarisation(pcm.gold(), Polarisation=(0, 0, 1), PerRay=True, Detector=D)
    finally:
        last.alive.copy_(saved)
    assert pol.count == 0 and pol.sum_w_out == 0 and pol.t_min == 0 and pol.t_max == 0
    assert not np.isnan(pol.throughput.cpu().numpy()).any() and not torch.isnan(pol.field).any()
    # an n = 0 job beside a full one in one call: zeros for it, the other job's bytes unchanged
    from attosecondraytracing_amd import polarisation as pmod
    c = pcm.gold()
    items = []
    for P in (None, (0, 0, 1)):
        pol_ref = relay4.get_Polarisation(c, Polarisation=P, Detector=D)
        out = relay4.get_output_rays()
        bundles = [relay4.source_rays] + [out[k] for k in range(len(relay4.optical_elements))]
        items.append(((bundles, [c] * 4, None if P is None else np.asarray(P, complex), D, bundles[-1].wavelength,
                       False), pol_ref))
    coat_list, coat_pos = [], {}
    made = [pmod._job(it, coat_list, coat_pos) for it, _ in items]
    made[0][0].n = 0
    rows = hip.polarisation([m[0] for m in made], [m[1] for m in made], [k._struct() for k in coat_list]).cpu().numpy()
    assert np.all(rows[0] == 0)
    ref = items[1][1]
    assert rows[1][2] == ref.sum_w_out and tuple(rows[1][5:9]) == ref.stokes
    assert np.array_equal(made[1][2][0].cpu().numpy(), ref.throughput.cpu().numpy())

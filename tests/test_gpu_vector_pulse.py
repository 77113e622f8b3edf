"""GPU (-m gpu): art_focal_vector_spectrum and the API on top of it (OpticalChain.get_FocalPulse, get_VectorFocalField,
CoatedPulseAtFocus) against the truth of tests/vector_pulse_truth.py (mpmath per ray and frequency, NumPy direct sum),
against get_Polarisation, art_focal_spectrum and Coating.reflectance, and in the limits where the answer is known
exactly.  Bars: 1e-9 amplitude_sum |P| on a focal field (tests/test_gpu_pulse.py's), 1e-12 amplitude_sum between two
device paths of the same sum."""
import ctypes as C
import math
import time

import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import coating_cases as cc
import focal_common as fc
import vector_pulse_truth as vt
from conftest import report

pytestmark = pytest.mark.gpu

C_FS = 299792458000 * 1e-15        # mm/fs
WL = 13.5e-6


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


def mosi_tabulated(periods=40, lo=8e-6, hi=25e-6):
    """coating_cases.mosi(periods) with both materials tabulated (made-up smooth tables through their 13.5 nm values)."""
    return vt.dispersive_copy(cc.mosi(periods), WL, lo, hi)


def _masked_relay4(n):
    """A mask that stops the outer rays, then the four toroids of relay4."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 6.0, 0, 0))
    SP = {"Divergence": 0.02, "SourceSize": 0, "Wavelength": WL, "DeltaFT": 0.5, "NumberRays": n}
    return mp.OEPlacement(SP, [Mask, Tor, Tor, Tor, Tor], [400, 200, 1200, 600, 1200], [0, 80, -80, 80, -80], [0] * 5,
                          "masked relay4")


def _detector_for(chain, distance=600.0):
    import ART.ModuleDetector as mdet
    last = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, distance)
    return D


@pytest.fixture(scope="module")
def relay(hip):
    import torch
    chain = _masked_relay4(10000)
    last = chain.get_output_rays()[-1]
    alive = last.alive.cpu().numpy().astype(bool)
    assert len(alive) == 10000 and 0.2 * len(alive) < alive.sum() < 0.9 * len(alive)       # the mask stops some rays
    g = torch.Generator(device="cpu").manual_seed(3)
    last.intensity = torch.exp(-0.5 * torch.randn(last.n_slots, generator=g, dtype=torch.float64) ** 2).to(hip.device)
    last.touch()
    return {"chain": chain, "D": _detector_for(chain)}


def _bundles(chain):
    from attosecondraytracing_amd import polarisation
    return polarisation.history(chain)


def _sdesc(D, B, k0, dk, nk, **kw):
    from attosecondraytracing_amd import _abi, focal
    fd, x, y, shifts, _, _, _ = focal.focal_desc(D, B, kw.get("Size"), kw.get("Pixels", 16), kw.get("Centre"),
                                                 kw.get("Shifts"), kw.get("Wavelength"), kw.get("RefPath"))
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.f.k, sd.dk, sd.nk = k0, dk, nk
    return sd, x, y, [-s for s in shifts]


def _ks(sd):
    return sd.f.k + np.arange(sd.nk) * sd.dk


def _run(bundles, coats, P, sd, scratch_bytes=None):
    from attosecondraytracing_amd import vector_pulse
    return vector_pulse._vector_spectrum(bundles, coats, np.asarray(P, dtype=complex), sd, 2 * np.pi / _ks(sd), scratch_bytes)


def _truth_field(bundles, coats, P, D, sd, x, y, sh):
    """The truth for the alive slots of bundles[-1] (all of them go through mpmath: keep them few)."""
    d = D._desc()
    Pp, V, L, alive, w = fc.bundle_arrays(bundles[-1])
    idx = np.nonzero(alive)[0]
    dirs = [b.data[3:6, :b.n_slots].cpu().numpy().T for b in bundles]
    amp = vt.amplitudes([[dd[i] for dd in dirs] for i in idx], coats, _ks(sd), P)
    return vt.field(Pp, V, L, alive, w, amp, _ks(sd), sd.f.L_ref, np.array(d.centre[:]), np.array(d.normal[:]),
                    np.array(d.rot[:]), x, y, sh)


def _amp_sum(B):
    from attosecondraytracing_amd import focal
    return focal.amplitude_sum(B)


STATES = {"linear": (0.0, 1.0, 0.0), "circular": (1 / math.sqrt(2), 1j / math.sqrt(2), 0.0)}


# ------------------------------------------------------------------------------------------- against the truth
@pytest.mark.parametrize("state", list(STATES))
def test_random_history_against_the_truth(hip, state):
    """10 000 slots of a made-up history (mirror, mask, mirror, mirror: random unit directions per view), all but 40
    slots dead, so that every alive ray goes through mpmath (40 rays x 5 frequencies x 3 mirrors x 80 layers)."""
    from attosecondraytracing_amd.bundle import RayBundle
    rng = np.random.default_rng(17)
    n = 10000
    keep = np.sort(rng.choice(n, 40, replace=False))

    def dirs(axis, spread):
        u = np.asarray(axis, float)[None, :] + rng.normal(0, spread, (n, 3))
        return u / np.linalg.norm(u, axis=1)[:, None]

    views = [dirs((0, 0, 1), 0.02), dirs((0.3, 0.1, -1), 0.02)]
    views += [views[-1].copy(), dirs((1, 0.2, 0.1), 0.02), dirs((0.05, -0.02, 1), 0.03)]
    pts = -5.0 * views[-1] + rng.normal(0, 2e-4, (n, 3))
    bundles = [RayBundle.from_arrays(rng.normal(0, 1, (n, 3)), v, wavelength=WL, backend=hip) for v in views[:-1]]
    last = RayBundle.from_arrays(pts, views[-1], intensity=rng.uniform(0.2, 2.0, n), wavelength=WL,
                                 path0=rng.normal(0, 3e-6, n), backend=hip)
    dead = np.ones(n, bool)
    dead[keep] = False
    last.alive[hip.from_numpy(dead)] = 0
    last.touch()
    bundles.append(last)
    import ART.ModuleDetector as mdet
    D = mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0]))
    coat = mosi_tabulated()
    coats = [coat, None, cc.gold(), coat]
    k0 = 2 * np.pi / WL
    sd, x, y, sh = _sdesc(D, last, 0.93 * k0, 0.035 * k0, 5, Size=(6e-4, 4e-4), Pixels=(37, 23), Centre=(0.0, 0.0),
                          Shifts=(0.0, 0.02))
    P = STATES[state]
    E = _run(bundles, coats, P, sd).cpu().numpy()
    assert E.shape == (2, 5, 3, 23, 37)
    want = _truth_field(bundles, coats, P, D, sd, x, y, sh)
    err, a = np.abs(E - want).max(), _amp_sum(last)
    report(f"[vector pulse, random history, {state}] |F - truth| = {err:.2e} = {err / a:.1e} amplitude_sum; "
           f"max |F| = {np.abs(want).max() / a:.2e} amplitude_sum")
    assert err <= 1e-9 * a * np.linalg.norm(P), err


@pytest.mark.parametrize("state", list(STATES))
def test_relay4_slice_against_the_truth(relay, state):
    """The 10 000 slots of a masked relay4 (the mask's dead slots stay dead); of the alive rays 48 are kept and the
    others made dead in the final bundle, so that the truth covers every ray of the sum."""
    chain, D = relay["chain"], relay["D"]
    bundles = list(_bundles(chain))
    last = bundles[-1].alias()
    last.alive = bundles[-1].alive.clone()
    alive = last.alive.cpu().numpy().astype(bool)
    rng = np.random.default_rng(5)
    drop = np.nonzero(alive)[0]
    drop = np.setdiff1d(drop, rng.choice(drop, 48, replace=False))
    last.alive[last.backend.from_numpy(drop)] = 0
    last.touch()
    bundles[-1] = last
    coat = mosi_tabulated()
    coats = [None] + [coat] * 4
    k0 = 2 * np.pi / WL
    sd, x, y, sh = _sdesc(D, last, 0.96 * k0, 0.02 * k0, 5, Pixels=(25, 21), Shifts=(-0.5, 0.5))
    P = STATES[state]
    E = _run(bundles, coats, P, sd).cpu().numpy()
    want = _truth_field(bundles, coats, P, D, sd, x, y, sh)
    err, a = np.abs(E - want).max(), _amp_sum(last)
    report(f"[vector pulse, masked relay4 slice, {state}] |F - truth| = {err:.2e} = {err / a:.1e} amplitude_sum; "
           f"max |F| = {np.abs(want).max() / a:.2e} amplitude_sum")
    assert err <= 1e-9 * a * np.linalg.norm(P), err


# ------------------------------------------------------------------------------------------- against the parents
def test_one_frequency_agrees_with_get_polarisation(relay):
    """nk = 1, constant materials: the NumPy direct sum with get_Polarisation's per-ray field as the amplitudes."""
    chain, D = relay["chain"], relay["D"]
    coats = [None, cc.mosi(40), cc.gold(), cc.six_materials(), cc.mosi(40)]
    P = STATES["circular"]
    f = chain.get_VectorFocalField(coats, D, P, Pixels=(24, 21), Shifts=(0.0, 0.4))
    pol = chain.get_Polarisation(coats, Polarisation=P, PerRay=True)
    last = chain.get_output_rays()[-1]
    Pp, V, L, alive, w = fc.bundle_arrays(last)
    amp = pol.field.cpu().numpy().T[alive][:, None, :]
    d = D._desc()
    want = vt.field(Pp, V, L, alive, w, amp, [2 * np.pi / f.wavelength], f.ref_path, np.array(d.centre[:]),
                    np.array(d.normal[:]), np.array(d.rot[:]), f.x, f.y, [-s for s in f.shifts])[:, 0]
    got = f.field.cpu().numpy()
    assert got.shape == (2, 3, 21, 24)
    err, a = np.abs(got - want).max(), f.amplitude_sum
    report(f"[vector pulse, nk = 1 vs get_Polarisation] {err / a:.1e} amplitude_sum; strehl {f.strehl}")
    assert err <= 1e-9 * a, err
    assert np.allclose(f.intensity, (np.abs(got) ** 2).sum(axis=1)) and np.all((f.strehl > 0) & (f.strehl < 1))


def test_get_polarisation_evaluates_tables_at_its_wavelength(relay):
    chain = relay["chain"]
    coat = mosi_tabulated()
    for wl in (WL, 13.1e-6):
        a = chain.get_Polarisation(coat, Polarisation=STATES["circular"], Wavelength=wl, PerRay=True)
        b = chain.get_Polarisation(coat.at(wl), Polarisation=STATES["circular"], Wavelength=wl, PerRay=True)
        assert a.field.cpu().numpy().tobytes() == b.field.cpu().numpy().tobytes() and a.transmission == b.transmission
    assert a.transmission != chain.get_Polarisation(coat, Polarisation=STATES["circular"]).transmission


def test_each_slice_is_the_vector_field_at_its_wavelength(relay):
    chain, D = relay["chain"], relay["D"]
    bundles = _bundles(chain)
    last = bundles[-1]
    coats = [None, cc.mosi(40), cc.gold(), cc.mosi(40), cc.gold()]
    P = STATES["linear"]
    k0 = 2 * np.pi / WL
    kw = dict(Pixels=(40, 36), Shifts=(0.0, 0.3))
    sd, _, _, _ = _sdesc(D, last, 0.95 * k0, 0.013 * k0, 8, **kw)
    E = _run(bundles, coats, P, sd).cpu().numpy()
    a = _amp_sum(last)
    for j, k in enumerate(_ks(sd)):
        f = chain.get_VectorFocalField(coats, D, P, Wavelength=2 * np.pi / k, Size=None, RefPath=sd.f.L_ref,
                                       Centre=None, **kw)
        # (the grid is the bundle's default one at WL: hand it over)
        one, _, _, _ = _sdesc(D, last, k, 0.0, 1, **kw)
        g = _run(bundles, coats, P, one).cpu().numpy()[:, 0]
        err = np.abs(E[:, j] - g).max()
        assert err <= 1e-12 * a, (j, err)
        assert f.field.shape == g.shape


def _collimated(hip, theta, n=400, coat_z=100.0):
    """A collimated bundle (one direction, at `theta` from the normal in the x-z plane) on a plane mirror facing -z;
    the source points lie on one wavefront, so every ray has the same phase anywhere behind the mirror."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalElement as moe
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    rng = np.random.default_rng(2)
    d = np.array([math.sin(theta), 0.0, math.cos(theta)])
    ea, eb = np.array([math.cos(theta), 0.0, -math.sin(theta)]), np.array([0.0, 1.0, 0.0])
    uv = rng.uniform(-1, 1, (n, 2))
    hit0 = np.array([0.0, 0.0, coat_z])
    pts = hit0 - 10.0 * d + uv[:, :1] * ea + uv[:, 1:] * eb
    src = RayBundle.from_arrays(pts, np.tile(d, (n, 1)), np.arange(n), np.ones(n), WL, backend=hip)
    M = mmirror.MirrorPlane(msupp.SupportRectangle(40, 40))
    el = moe.OpticalElement(M, hit0, np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0]))
    chain = OpticalChain(src, [el])
    out = np.array([d[0], 0.0, -d[2]])
    D = mdet.Detector(hit0 + 40.0 * out, hit0 + 50.0 * out, -out)
    return chain, D


def test_ideal_coatings_give_the_scalar_field_times_the_field_vector(hip):
    chain, D = _collimated(hip, 0.3)
    bundles = _bundles(chain)
    last = bundles[-1]
    assert bool(last.alive.all())
    from attosecondraytracing_amd.coating import Coating
    P = STATES["circular"]
    k0 = 2 * np.pi / WL
    sd, _, _, _ = _sdesc(D, last, 0.9 * k0, 0.025 * k0, 9, Size=2e-3, Pixels=(19, 17), Centre=(0.0, 0.0), Shifts=(0.0, 0.2))
    E = _run(bundles, [Coating.ideal()], P, sd).cpu().numpy()
    S = hip.focal_spectrum(sd, last.view(), last.intensity, last.n_slots).cpu().numpy()
    vec = chain.get_Polarisation(Coating.ideal(), Polarisation=P, PerRay=True).field.cpu().numpy()
    assert np.abs(vec - vec[:, :1]).max() <= 1e-15           # (collimated: one field vector)
    d = D._desc()
    U = np.stack([np.array(d.rot[0:3]), np.array(d.rot[3:6]), np.array(d.normal[:])])
    comp = U @ vec[:, 0]
    a = _amp_sum(last)
    err = np.abs(E - S[:, :, None] * comp[None, None, :, None, None]).max()
    report(f"[vector pulse, ideal coatings vs art_focal_spectrum] {err / a:.1e} amplitude_sum")
    assert err <= 1e-12 * a, err


# ------------------------------------------------------------------------------------------- physics, exact by construction
def test_a_spacer_layer_delays_the_pulse_by_its_round_trip(hip):
    """A substrate under a spacer of N = 1 and thickness t reflects as the bare substrate times exp(2 i k t cos th):
    the pulse arrives 2 t cos th / c later and is otherwise the same.  t is chosen so that the delay is 16 samples of the
    time axis (5 fs): the sampled envelope then moves by whole samples and `duration`, interpolated between samples,
    has nothing to differ by but rounding."""
    from attosecondraytracing_amd.coating import Coating
    from coating_truth import cos_incidence
    theta, T, Nt, wl = 0.5, 80.0, 256, 633e-6
    chain, D = _collimated(hip, theta)
    bundles = _bundles(chain)
    a0 = bundles[0].data[3:6, 0].cpu().numpy()
    b0 = bundles[1].data[3:6, 0].cpu().numpy()
    cos_t = float(cos_incidence(a0, b0))
    tau = 16 * T / Nt
    t = tau * C_FS / (2 * cos_t)
    kw = dict(Size=2e-3, Pixels=3, Centre=(0.0, 0.0), Wavelength=wl, TimeWindow=T, Times=Nt)
    P = STATES["linear"]
    bare = chain.get_FocalPulse(Coating(cc.AG), D, 5.0, P, **kw)
    spaced = chain.get_FocalPulse(Coating(cc.AG, [(1.0, t, 0.0)]), D, 5.0, P, **kw)
    shift = spaced.arrival[0, 1, 1] - bare.arrival[0, 1, 1]
    report(f"[vector pulse, spacer layer] arrival moves by {shift:.9f} fs, 2 t cos th / c = {tau:.9f} fs; duration "
           f"{bare.duration[0]:.9f} -> {spaced.duration[0]:.9f} fs")
    assert abs(shift - tau) <= 1e-6 * T, (shift, tau)
    assert spaced.duration[0] == pytest.approx(bare.duration[0], rel=1e-9)


def test_a_multilayer_filters_and_stretches_the_pulse(hip):
    """Collimated, s-polarised: every ray reflects with the same rs(omega_j), so the centre pixel's envelope is
    sum_j g_j rs(omega_j) [mean_r exp(i k_j Phi_r)] e^{-i (omega_j - omega_0) t} / sum |g_j| times amplitude_sum (the
    bracket is 1 but for the rounding of the rays' common phase, taken from the model's own statement in
    focal_common.ray_terms).  A 0.2 fs pulse is wider than the mirror's band: it comes out longer."""
    from attosecondraytracing_amd.pulse import fwhm
    theta = math.radians(5.0)
    chain, D = _collimated(hip, theta)
    coat = mosi_tabulated()
    P = STATES["linear"]                                   # along y: s
    p = chain.get_FocalPulse(coat, D, 0.2, P, Size=2e-3, Pixels=3, Centre=(0.0, 0.0))
    last = chain.get_output_rays()[-1]
    Pp, V, L, alive, w = fc.bundle_arrays(last)
    d = D._desc()
    e2 = np.array(d.rot[3:6])
    assert abs(abs(e2[1]) - 1) <= 1e-12                    # (s lies along the detector's second axis)
    bundles = _bundles(chain)
    from coating_truth import cos_incidence
    cos_t = float(cos_incidence(bundles[0].data[3:6, 0].cpu().numpy(), bundles[1].data[3:6, 0].cpu().numpy()))
    k = p.omega / C_FS
    rs = np.array([coat.reflectance(math.acos(cos_t), 2 * np.pi / kj)[0] for kj in k])
    geo = np.array([np.exp(1j * fc.ray_terms(Pp, V, L, alive, w, kj, p.ref_path, np.array(d.centre[:]),
                                             np.array(d.normal[:]), np.array(d.rot[:]))[1]).mean() for kj in k])
    M = np.exp(-1j * (p.omega - p.omega0)[None, :] * p.t[:, None])
    want = e2[1] * (M @ (p.weights * rs * geo)) / np.abs(p.weights).sum()
    got = p.envelope.cpu().numpy()[0, :, 1, 1, 1] / p.amplitude_sum
    err = np.abs(got - want).max()
    tl = fwhm(np.abs(M @ p.weights) ** 2, p.time_window / len(p.t))
    report(f"[vector pulse, Mo/Si at 5 deg] centre envelope vs host {err:.1e}; |rs|^2 over the grid {np.abs(rs).min() ** 2:.3f}"
           f"..{np.abs(rs).max() ** 2:.3f}; duration {tl:.4f} -> {p.duration[0]:.4f} fs; strehl {p.strehl[0]:.4f}")
    assert err <= 1e-9, err
    assert p.duration[0] > tl
    assert 0 < p.strehl[0] < 1 and abs(p.longitudinal[0]) <= 1e-12


# ------------------------------------------------------------------------------------------- determinism, blocks
def test_same_bytes_on_two_calls_and_for_every_block_size(relay):
    chain, D = relay["chain"], relay["D"]
    bundles = _bundles(chain)
    last = bundles[-1]
    coats = [None] + [mosi_tabulated()] * 4
    P = STATES["circular"]
    k0 = 2 * np.pi / WL
    sd, _, _, _ = _sdesc(D, last, 0.97 * k0, 0.01 * k0, 6, Pixels=(70, 66), Shifts=(0.0, 0.3))
    from attosecondraytracing_amd import _abi
    a = _run(bundles, coats, P, sd).cpu().numpy()
    assert a.tobytes() == _run(bundles, coats, P, sd).cpu().numpy().tobytes()
    # scratch of a block of b frequencies: 5 rows + b (6 rows + the slices' partials); the library's own count for a
    # bound of one double is that of ONE frequency
    d = _abi.ArtFocalVectorSpectrumDesc()
    d.s, d.n_elems, d.n, d.scratch_bound = sd, 5, last.n_slots, 1
    for e in range(5):
        d.coating[e] = -1
    one = last.backend.fn["art_focal_vector_spectrum_scratch_doubles"](C.byref(d))
    d.scratch_bound = 0
    full = last.backend.fn["art_focal_vector_spectrum_scratch_doubles"](C.byref(d))
    stride = (last.n_slots + 63) // 64 * 64
    per_k = (full - 5 * stride) // 6
    assert one == 5 * stride + per_k and full == 5 * stride + 6 * per_k
    for blocks, bound in ((6, 8), (2, 8 * (5 * stride + 3 * per_k)), (1, 8 * full)):
        d.scratch_bound = bound // 8
        got = last.backend.fn["art_focal_vector_spectrum_scratch_doubles"](C.byref(d))
        assert got == 5 * stride + (6 // blocks) * per_k, (blocks, got)
        assert _run(bundles, coats, P, sd, bound).cpu().numpy().tobytes() == a.tobytes(), blocks


def test_empty_and_all_dead_bundles(hip):
    chain, D = _collimated(hip, 0.3, n=300)
    bundles = list(_bundles(chain))
    last = bundles[-1]
    last.alive[:] = 0
    last.touch()
    coat = mosi_tabulated()
    p = chain.get_FocalPulse(coat, D, 0.5, STATES["linear"], Size=0.01, Pixels=(9, 5), Centre=(0.0, 0.0),
                             Shifts=(0.0, 0.1))
    assert p.spectrum.shape[0] == 2 and p.spectrum.shape[2] == 3
    assert not p.spectrum.cpu().numpy().any() and not p.envelope.cpu().numpy().any()
    for v in (p.strehl, p.peak, p.duration, p.duration_integrated, p.arrival, p.longitudinal):
        assert np.isnan(v).all()
    f = chain.get_VectorFocalField(coat, D, STATES["linear"], Size=0.01, Pixels=8, Centre=(0.0, 0.0))
    assert not f.field.cpu().numpy().any() and np.isnan(f.strehl).all()
    empty = [b.slots(0, 0) for b in bundles]
    sd, _, _, _ = _sdesc(D, last, 2 * np.pi / WL, 10.0, 3, Size=0.01, Pixels=8, Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    E = _run(empty, [coat], STATES["linear"], sd)
    assert E.shape == (2, 3, 3, 8, 8) and not E.cpu().numpy().any()


def _set(d, key, v):
    if key in ("nk", "dk"):
        setattr(d.s, key, v)
    elif key in ("k", "nx", "planes", "dx"):
        setattr(d.s.f, key, v)
    elif key == "coating0":
        d.coating[0] = v
    elif key == "pol0":
        d.pol[0] = v
    else:
        setattr(d, key, v)


@pytest.mark.parametrize("over, msg", [
    (dict(nk=0), "nk must"), (dict(nk=1025), "nk must"), (dict(dk=float("nan")), "dk must"),
    (dict(dk=-2500.0), "every k_j"), (dict(planes=64, nk=400), "planes * nk * 3"), (dict(k=0.0), "k must"),
    (dict(nx=0), "nx and ny"), (dict(planes=65), "planes"), (dict(dx=float("nan")), "pitch"),
    (dict(n=-1), "negative ray count"), (dict(n_elems=0), "elements"), (dict(n_elems=65), "elements"),
    (dict(coating0=1), "coating index"), (dict(coating0=-2), "coating index"), (dict(pol0=float("inf")), "input state"),
    (dict(scratch_bound=-1), "scratch_bound"), (dict(views=None), "views is NULL"),
    (dict(materials=None), "table is NULL"), (dict(coatings_dev=None), "table is NULL"),
    (dict(bad_material=(float("nan"), 0.0)), "per-wavenumber table"), (dict(bad_material=(0.9, -1e-3)), "per-wavenumber table"),
    (dict(bad_layers=257), "layers"),
    (dict(field=None), "must not be NULL"), (dict(scratch=None), "must not be NULL")])
def test_invalid_descriptors_launch_nothing(hip, over, msg):
    import torch
    from attosecondraytracing_amd import _abi
    chain, D = _collimated(hip, 0.3, n=256)
    bundles = _bundles(chain)
    last = bundles[-1]
    sd, _, _, _ = _sdesc(D, last, 6000.0, 100.0, 4, Size=0.01, Pixels=8, Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    coat = cc.mosi(4)
    d = _abi.ArtFocalVectorSpectrumDesc()
    d.s, d.n_elems, d.n = sd, 1, last.n_slots
    d.pol[:] = [0, 0, 1, 0, 0, 0]
    d.w = last.intensity.data_ptr()
    views = (_abi.ArtBundleView * 2)(*[b.view() for b in bundles])
    mats = np.stack([coat.material_table(np.full(4, WL))], axis=1)
    over = dict(over)
    if "bad_material" in over:
        mats[2, 0, 1] = over.pop("bad_material")
    struct = coat._struct()
    if "bad_layers" in over:
        struct.n_layers = over.pop("bad_layers")
    cdev, carr, marr = hip.focal_vector_tables(d, views, [struct], mats)
    use_field, use_scratch = over.pop("field", True), over.pop("scratch", True)
    if "coatings_dev" in over:
        cdev = over.pop("coatings_dev")
    for key, v in over.items():
        _set(d, key, v)
    field = torch.full((2 * 4 * 3 * 8 * 8 * 2,), 7.25, dtype=torch.float64, device=hip.device)
    scratch = torch.zeros(1 << 20, dtype=torch.float64, device=hip.device)
    rc = hip.fn["art_focal_vector_spectrum"](C.byref(d), C.byref(views[1]), cdev, carr, marr,
                                             scratch.data_ptr() if use_scratch else None,
                                             field.data_ptr() if use_field else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and msg in hip.last_error(), (rc, hip.last_error())
    assert bool((field == 7.25).all())


def test_api_errors(hip):
    chain, D = _collimated(hip, 0.3, n=64)
    coat = cc.mosi(4)
    with pytest.raises(ValueError, match="polarised"):
        chain.get_FocalPulse(coat, D, 0.5, None)
    with pytest.raises(ValueError, match="parallel"):
        chain.get_VectorFocalField(coat, D, tuple(chain.source_rays.data[3:6, 0].cpu().numpy()), Size=0.01, Pixels=4,
                                   Centre=(0.0, 0.0))
    narrow = vt.dispersive_copy(coat, WL, 13.4e-6, 13.6e-6)
    with pytest.raises(ValueError, match="outside the material's table"):
        chain.get_FocalPulse(narrow, D, 0.2, STATES["linear"], Size=0.01, Pixels=4, Centre=(0.0, 0.0))


def test_coated_pulse_plot_draws(hip):
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    chain, D = _collimated(hip, math.radians(5.0), n=300)
    fig = mpl.CoatedPulseAtFocus(chain, mosi_tabulated(), D, 0.2, STATES["linear"], Size=2e-3, Pixels=9,
                                 Centre=(0.0, 0.0))
    p = fig._art_pulse
    assert p.envelope.shape[1:] == (256, 3, 9, 9) and 0 < p.strehl[0] < 1
    import matplotlib.pyplot as plt
    plt.close("all")


# ------------------------------------------------------------------------------------------- a large case
def test_relay4_1e6_rays_under_mosi(hip):
    """Shape and stability only: relay4 at 1e6 rays, 64 x 64 pixels, the default grid of a 0.3 fs pulse at 13.5 nm,
    40-period Mo/Si (tabulated) on all four mirrors."""
    import torch
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=10 ** 6)
    D = _detector_for(chain)
    coat = mosi_tabulated(lo=6e-6, hi=40e-6)
    kw = dict(Pixels=64, Wavelength=WL)
    P = STATES["linear"]
    p = chain.get_FocalPulse(coat, D, 0.3, P, **kw)             # (warm: allocations, first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p = chain.get_FocalPulse(coat, D, 0.3, P, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    J = len(p.omega)
    assert p.spectrum.shape == (1, J, 3, 64, 64) and p.envelope.shape == (1, 256, 3, 64, 64)
    assert bool(torch.isfinite(torch.view_as_real(p.spectrum)).all()) and np.isfinite(p.intensity).all()
    assert 0 < p.strehl[0] < 1, p.strehl
    report(f"[vector pulse, relay4 1e6 rays x {J} frequencies x 4 x 80 layers, 64 x 64] get_FocalPulse {dt * 1e3:.0f} ms "
           f"(host metrics included); strehl {p.strehl[0]:.3e}, duration {p.duration[0]:.3f} fs, longitudinal "
           f"{p.longitudinal[0]:.2e}")

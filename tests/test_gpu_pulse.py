"""GPU (-m gpu): art_focal_spectrum and the API on top of it (Detector.get_FocalPulse, PulseAtFocus, PulseThroughFocus),
against the NumPy direct sum of tests/focal_common.py at every wavenumber, art_focal_field, the trace's own delays, a
tilted plane wave and an ideal focus."""
import ctypes as C
import math

import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import focal_common as fc

pytestmark = pytest.mark.gpu

C_FS = 299792458000 * 1e-15        # mm/fs


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


@pytest.fixture(scope="module")
def relay4(hip):
    """relay4 traced with 1e5 rays, Gaussian weights on the final bundle, a detector placed 600 mm downstream."""
    import torch
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=10 ** 5)
    last = chain.get_output_rays()[-1]
    g = torch.Generator(device="cpu").manual_seed(7)
    last.intensity = torch.exp(-0.5 * torch.randn(last.n_slots, generator=g, dtype=torch.float64) ** 2).to(hip.device)
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    return {"last": last, "D": D}


def _detector(centre=(0.0, 0.0, 0.0), normal=(0.0, 0.0, -1.0)):
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array(centre, dtype=float), np.array(normal, dtype=float))


def _random_bundle(hip, n, seed, dead=0.3):
    from attosecondraytracing_amd.bundle import RayBundle
    rng = np.random.default_rng(seed)
    u = np.column_stack([rng.normal(0, 0.03, n), rng.normal(0, 0.02, n), np.ones(n)])
    u /= np.linalg.norm(u, axis=1)[:, None]
    P = -5.0 * u + rng.normal(0, 2e-4, (n, 3))
    B = RayBundle.from_arrays(P, u, intensity=rng.uniform(0.2, 2.0, n), wavelength=1e-3, path0=rng.normal(0, 3e-4, n),
                              backend=hip)
    if dead:
        B.alive[hip.from_numpy(rng.random(n) < dead)] = 0
        B.touch()
    return B


def _sdesc(D, B, k0, dk, nk, **kw):
    """An ArtFocalSpectrumDesc with get_FocalField's grid for kw; (desc, x, y, ABI shifts)."""
    from attosecondraytracing_amd import _abi, focal
    fd, x, y, shifts, _, _, _ = focal.focal_desc(D, B, kw.get("Size"), kw.get("Pixels", 16), kw.get("Centre"),
                                                 kw.get("Shifts"), kw.get("Wavelength"), kw.get("RefPath"))
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.f.k, sd.dk, sd.nk = k0, dk, nk
    return sd, x, y, [-s for s in shifts]


def _oracle(B, D, sd, x, y, shifts):
    d = D._desc()
    P, V, L, alive, w = fc.bundle_arrays(B)
    return np.stack([fc.field(P, V, L, alive, w, sd.f.k + j * sd.dk, sd.f.L_ref, np.array(d.centre[:]),
                              np.array(d.normal[:]), np.array(d.rot[:]), x, y, shifts) for j in range(sd.nk)], axis=1)


def _amp_sum(B):
    from attosecondraytracing_amd import focal
    return focal.amplitude_sum(B)


def test_random_bundle_against_the_oracle(hip):
    B = _random_bundle(hip, 3000, 11)
    D = _detector()
    sd, x, y, sh = _sdesc(D, B, 2 * np.pi / 1e-3, 97.0, 7, Size=(0.05, 0.03), Pixels=(37, 23), Shifts=(0.0, -0.1, 0.25))
    E = hip.focal_spectrum(sd, B.view(), B.intensity, B.n_slots)
    assert E.shape == (3, 7, 23, 37) and E.is_cuda
    err = np.abs(E.cpu().numpy() - _oracle(B, D, sd, x, y, sh)).max()
    assert err <= 1e-9 * _amp_sum(B), err


def test_relay4_slice_against_the_oracle(relay4):
    last, D = relay4["last"], relay4["D"]
    B = last.slots(0, 10000)
    k = 2 * np.pi / last.wavelength
    sd, x, y, sh = _sdesc(D, B, 0.98 * k, 0.005 * k, 5, Pixels=(24, 20), Shifts=(-0.5, 0.5))
    E = B.backend.focal_spectrum(sd, B.view(), B.intensity, B.n_slots)
    err = np.abs(E.cpu().numpy() - _oracle(B, D, sd, x, y, sh)).max()
    assert err <= 1e-9 * _amp_sum(B), err


def test_one_wavenumber_is_art_focal_field_bytewise(relay4, hip):
    last, D = relay4["last"], relay4["D"]
    for B, kw in ((last, dict(Pixels=(70, 66), Shifts=(0.0, 0.3))), (_random_bundle(hip, 5000, 12), dict(Size=0.05, Pixels=(37, 23)))):
        sd, _, _, _ = _sdesc(D if B is last else _detector(), B, 0.0, 123.0, 1, **kw)
        sd.f.k = 2 * np.pi / B.wavelength
        f = hip.focal_field(sd.f, B.view(), B.intensity, B.n_slots)
        E = hip.focal_spectrum(sd, B.view(), B.intensity, B.n_slots)
        assert E.shape[1] == 1
        assert E[:, 0].cpu().numpy().tobytes() == f.cpu().numpy().tobytes()


def test_each_slice_is_art_focal_field_at_its_wavenumber(relay4, hip):
    last, D = relay4["last"], relay4["D"]
    k0 = 2 * np.pi / last.wavelength
    sd, _, _, _ = _sdesc(D, last, 0.95 * k0, 0.013 * k0, 8, Pixels=(40, 36), Shifts=(0.0, 0.3))
    E = hip.focal_spectrum(sd, last.view(), last.intensity, last.n_slots).cpu().numpy()
    a = _amp_sum(last)
    for j in range(8):
        one, _, _, _ = _sdesc(D, last, sd.f.k + j * sd.dk, 0.0, 1, Pixels=(40, 36), Shifts=(0.0, 0.3))
        f = hip.focal_field(one.f, last.view(), last.intensity, last.n_slots).cpu().numpy()
        err = np.abs(E[:, j] - f).max()
        assert err <= 1e-12 * a, (j, err)


def test_single_ray_phase_is_linear_in_omega_with_the_delay(hip):
    from attosecondraytracing_amd.bundle import RayBundle
    d = np.array([0.01, -0.02, 1.0])
    B = RayBundle.from_arrays(np.array([[0.3, -0.1, -40.0]]), d[None, :], wavelength=5e-5, path0=np.array([123.4]),
                              backend=hip)
    D = _detector(centre=(0.2, 0.1, 0.0), normal=(0.05, 0.0, -1.0))
    X, Y = D.get_PointList2D(B)[0]
    opl = D.get_OpticalPaths(B)
    ref = opl[0] - 3.1e-4
    tau = D.get_Delays(B)[0] + (opl.mean() - ref) / C_FS            # fs
    assert tau == pytest.approx(3.1e-4 / C_FS, rel=1e-6)
    p = D.get_FocalPulse(B, 0.4, Size=1e-3, Pixels=3, Centre=(X, Y), RefPath=ref)
    E = p.spectrum.cpu().numpy()[0, :, 1, 1]
    resid = [math.remainder(a - w * tau, 2 * np.pi) for a, w in zip(np.angle(E), p.omega)]
    assert np.abs(resid).max() <= 1e-6, np.abs(resid).max()
    # one plane wave: every pixel is as bright, and the centre pixel's envelope peaks at the delay
    assert abs(p.t[np.argmax(p.intensity[0, :, 1, 1])] - tau) <= 0.5 * p.time_window / len(p.t)
    assert abs(p.arrival[0, 1, 1] - tau) <= 1e-6 * p.time_window
    assert 0.98 < p.strehl[0] <= 1 + 1e-12          # the peak falls between two samples of t


def test_tilted_plane_wave_has_a_tilted_pulse_front(hip):
    from attosecondraytracing_amd.bundle import RayBundle
    th = 0.02
    d = np.array([math.sin(th), 0.0, math.cos(th)])
    B = RayBundle.from_arrays(-10 * d[None, :], d[None, :], wavelength=5e-5, backend=hip)
    D = _detector()
    e1 = np.array(D._desc().rot[:3])
    de1 = float(d @ e1)
    assert abs(abs(de1) - math.sin(th)) <= 1e-12
    p = D.get_FocalPulse(B, 0.5, Size=(0.02, 0.004), Pixels=(21, 3), Centre=(0.0, 0.0))
    slope = np.polyfit(p.x, p.arrival[0, 1], 1)[0]
    assert slope == pytest.approx(de1 / C_FS, rel=1e-3), (slope, de1 / C_FS)
    assert np.abs(p.fluence[0] - p.fluence[0, 1, 10]).max() <= 1e-9 * p.fluence[0, 1, 10]


def test_ideal_focus_of_a_transform_limited_pulse(hip):
    lam, tau = 5e-5, 0.5
    B = fc.converging_bundle(20000, 0.05, 10.0, wavelength=lam, backend=hip)
    D = _detector()
    zr = lam / 0.05 ** 2
    kw = dict(Size=0.004, Pixels=9, Centre=(0.0, 0.0), Shifts=(0.0, 5 * zr), Times=512)
    p = D.get_FocalPulse(B, tau, **kw)
    assert p.ref_path == pytest.approx(10.0, abs=1e-12)
    assert p.strehl[0] == pytest.approx(1.0, abs=1e-9)
    assert np.abs(p.peak[0]).max() <= 1e-15
    a = np.exp(-1j * (p.omega - p.omega0)[None, :] * p.t[:, None]) @ p.weights / np.abs(p.weights).sum()
    from attosecondraytracing_amd.pulse import fwhm
    tl = fwhm(np.abs(a) ** 2, p.time_window / len(p.t))
    assert p.duration[0] == pytest.approx(tl, rel=1e-6) and tl == pytest.approx(tau, rel=2e-2)
    assert p.strehl[1] < 0.5
    chirp = lambda w: np.exp(-(w - p.omega0) ** 2 * tau ** 2 / (8 * math.log(2)) + 0.2j * (w - p.omega0) ** 2)
    c = D.get_FocalPulse(B, tau, Spectrum=chirp, **kw)
    assert c.strehl[0] < 0.7 * p.strehl[0] and c.duration[0] > 1.5 * p.duration[0]


def test_two_calls_give_identical_bytes(relay4, hip):
    last, D = relay4["last"], relay4["D"]
    k0 = 2 * np.pi / last.wavelength
    sd, _, _, _ = _sdesc(D, last, k0, 0.01 * k0, 6, Pixels=(70, 66), Shifts=(0.0, 0.3))
    a = hip.focal_spectrum(sd, last.view(), last.intensity, last.n_slots).cpu().numpy()
    b = hip.focal_spectrum(sd, last.view(), last.intensity, last.n_slots).cpu().numpy()
    assert a.tobytes() == b.tobytes()


def test_empty_and_all_dead_bundles(hip):
    D = _detector()
    dead = _random_bundle(hip, 500, 4, dead=0.0)
    dead.alive[:] = 0
    dead.touch()
    p = D.get_FocalPulse(dead, 0.5, Size=0.01, Pixels=(9, 5), Centre=(0.0, 0.0), Shifts=(0.0, 0.1), Wavelength=5e-5)
    assert p.spectrum.shape[0] == 2 and not p.spectrum.cpu().numpy().any() and not p.envelope.cpu().numpy().any()
    for v in (p.strehl, p.peak, p.duration, p.duration_integrated, p.arrival):
        assert np.isnan(v).all()
    sd, _, _, _ = _sdesc(D, dead, 2 * np.pi / 1e-3, 10.0, 3, Size=0.01, Pixels=8, Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    E = hip.focal_spectrum(sd, dead.view(), None, 0)
    assert E.shape == (2, 3, 8, 8) and not E.cpu().numpy().any()


def _bad(sd, key, v):
    if key in ("nk", "dk"):
        setattr(sd, key, v)
    else:
        setattr(sd.f, key, v)


@pytest.mark.parametrize("over, msg", [
    (dict(nk=0), "nk must"), (dict(nk=1025), "nk must"), (dict(dk=float("nan")), "dk must"),
    (dict(dk=float("inf")), "dk must"), (dict(dk=-2500.0), "every k_j"), (dict(planes=64, nk=1024), "planes * nk"),
    (dict(k=0.0), "k must"), (dict(nx=0), "nx and ny"), (dict(planes=65), "planes"), (dict(dx=float("nan")), "pitch"),
    (dict(field=None), "must not be NULL"), (dict(scratch=None), "must not be NULL")])
def test_invalid_descriptors_launch_nothing(hip, over, msg):
    import torch
    B = _random_bundle(hip, 256, 5)
    D = _detector()
    sd, _, _, _ = _sdesc(D, B, 2 * np.pi / 1e-3, 100.0, 4, Size=0.01, Pixels=8, Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    sd.f.k = 6000.0                     # k_3 = 6300; dk = -2500 makes it negative
    over = dict(over)
    use_field, use_scratch = over.pop("field", True), over.pop("scratch", True)
    for key, v in over.items():
        _bad(sd, key, v)
    field = torch.full((2 * 4 * 8 * 8 * 2,), 7.25, dtype=torch.float64, device=hip.device)
    scratch = torch.zeros(1 << 20, dtype=torch.float64, device=hip.device)
    rc = hip.fn["art_focal_spectrum"](C.byref(sd), C.byref(B.view()), B.intensity.data_ptr(), B.n_slots,
                                      scratch.data_ptr() if use_scratch else None,
                                      field.data_ptr() if use_field else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and msg in hip.last_error(), (rc, hip.last_error())
    assert bool((field == 7.25).all())
    assert hip.fn["art_focal_spectrum_scratch_doubles"](8, 8, 1, 0, 10) == -1
    assert hip.fn["art_focal_spectrum_scratch_doubles"](8, 8, 1, 1025, 10) == -1


def test_pulse_plots_draw(hip):
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    B = fc.converging_bundle(3000, 0.05, 10.0, wavelength=5e-5, backend=hip)
    D = _detector()
    fig = mpl.PulseAtFocus(B, D, 0.5, Pixels=17)
    p = fig._art_pulse
    assert p.envelope.shape[1:] == (256, 17, 17) and p.strehl[0] == pytest.approx(1.0, abs=1e-6)
    zr = 5e-5 / 0.05 ** 2
    fig2 = mpl.PulseThroughFocus(B, D, 0.5, Shifts=np.linspace(-4 * zr, 4 * zr, 9), Pixels=9)
    s = fig2._art_pulse.strehl
    assert s.shape == (9,) and np.argmax(s) == 4 and s[4] == pytest.approx(1.0, abs=1e-4)
    import matplotlib.pyplot as plt
    plt.close("all")

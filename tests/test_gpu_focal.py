"""GPU (-m gpu): art_focal_field and the API on top of it (Detector.get_FocalField, FocalSpot, ThroughFocus), against
the NumPy direct sum of tests/focal_common.py, the trace's own optical paths, and the Airy pattern of an ideal focus."""
import ctypes as C
import math
import types

import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import focal_common as fc

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


def _random_bundle(hip, n, seed, dead=0.3, weights=True):
    from attosecondraytracing_amd.bundle import RayBundle
    rng = np.random.default_rng(seed)
    u = np.column_stack([rng.normal(0, 0.03, n), rng.normal(0, 0.02, n), np.ones(n)])
    u /= np.linalg.norm(u, axis=1)[:, None]
    P = -5.0 * u + rng.normal(0, 2e-4, (n, 3))
    w = rng.uniform(0.2, 2.0, n) if weights else None
    B = RayBundle.from_arrays(P, u, intensity=w, wavelength=1e-3, path0=rng.normal(0, 3e-4, n), backend=hip)
    if dead:
        B.alive[hip.from_numpy(rng.random(n) < dead)] = 0
        B.touch()
    return B


def _check_oracle(B, D, f, tol=1e-9):
    E = fc.field_of(B, D, f)
    err = np.abs(f.field.cpu().numpy() - E).max()
    assert err <= tol * f.amplitude_sum, (err, f.amplitude_sum)
    return err


def test_random_bundle_with_dead_slots_and_weights(hip):
    B = _random_bundle(hip, 3000, 1)
    D = _detector()
    f = D.get_FocalField(B, Size=(0.05, 0.03), Pixels=(37, 23), Shifts=(0.0, -0.1, 0.25))
    assert f.field.shape == (3, 23, 37) and f.field.is_cuda
    _check_oracle(B, D, f)
    # several tiles with ragged edges, one plane; no intensities
    B2 = _random_bundle(hip, 1500, 2, weights=False)
    f2 = D.get_FocalField(B2, Size=(0.08, 0.05), Pixels=(130, 70))
    _check_oracle(B2, D, f2)


def test_relay4_slice_against_the_oracle(relay4):
    last, D = relay4["last"], relay4["D"]
    B = last.slots(0, 20000)
    f = D.get_FocalField(B, Pixels=(24, 20), Shifts=(-0.5, 0.0, 0.5))
    _check_oracle(B, D, f)


def test_single_ray_phase_is_the_optical_path(hip):
    from attosecondraytracing_amd.bundle import RayBundle
    d = np.array([0.01, -0.02, 1.0])
    B = RayBundle.from_arrays(np.array([[0.3, -0.1, -40.0]]), d[None, :], wavelength=5e-5, path0=np.array([123.4]),
                              backend=hip)
    D = _detector(centre=(0.2, 0.1, 0.0), normal=(0.05, 0.0, -1.0))
    X, Y = D.get_PointList2D(B)[0]
    opl = D.get_OpticalPaths(B)[0]
    ref = opl - 0.1234567
    f = D.get_FocalField(B, Size=1e-3, Pixels=3, Centre=(X, Y), RefPath=ref)
    k = 2 * np.pi / 5e-5
    got = np.angle(f.field.cpu().numpy()[0, 1, 1])
    want = math.remainder(k * (opl - ref), 2 * np.pi)
    assert abs(math.remainder(got - want, 2 * np.pi)) <= 1e-6
    assert f.strehl[0] == pytest.approx(1.0, abs=1e-12)


def test_parabola_focus_has_strehl_one(hip):
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    feff = 100.0
    SP = {"Divergence": 0, "SourceSize": 2 * 0.1 * feff, "Wavelength": 800e-6, "DeltaFT": 1, "NumberRays": 2000}
    par = mmirror.MirrorParabolic(feff, 30.0, msupp.SupportRound(3 * 0.1 * feff))
    chain = mp.OEPlacement(SP, [par], [2 * feff], [0])
    out = chain.get_output_rays()[-1]
    oe = chain.optical_elements[0]
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    focus = fwd.T @ (np.array([0.0, 0.0, par.p / 2]) - par.get_centre()) + np.asarray(oe.position, float)
    D = _detector(centre=focus, normal=-mp.FindCentralRay(out).vector)
    f = D.get_FocalField(out, Pixels=33, Shifts=(0.0, 1.0))
    assert f.strehl[0] >= 1 - 1e-9, f.strehl
    assert f.strehl[1] < 0.9


def test_ideal_focus_is_an_airy_pattern(hip):
    NA, lam = 0.05, 1e-3
    B = fc.converging_bundle(60000, NA, 10.0, wavelength=lam, backend=hip)
    D = _detector()
    half = 1.5 * lam / NA
    f = D.get_FocalField(B, Size=(2 * half, 1e-4), Pixels=(601, 3), Centre=(0.0, 0.0))
    prof = f.intensity[0, 1] / f.amplitude_sum ** 2
    r = np.abs(f.x)
    assert np.abs(prof - fc.airy(2 * np.pi / lam * NA * r)).max() <= 2e-3
    right = (f.x > 0.4 * lam / NA) & (f.x < 0.8 * lam / NA)
    r_min = f.x[right][np.argmin(prof[right])]
    assert abs(r_min - 0.61 * lam / NA) <= 0.02 * 0.61 * lam / NA
    assert f.strehl[0] == pytest.approx(1.0, abs=1e-9)


def test_planes_agree_with_a_moved_detector(hip):
    B = fc.converging_bundle(2000, 0.05, 0.05, wavelength=1e-3, backend=hip, weights=np.linspace(0.5, 1.0, 2000))
    D = _detector()
    shifts = (-0.03125, 0.0, 0.046875)
    kw = dict(Size=(0.04, 0.03), Pixels=(29, 21), Centre=(0.0, 0.0), RefPath=0.05)
    f = D.get_FocalField(B, Shifts=shifts, **kw)
    for q, s in enumerate(shifts):
        Dq = D.copy_detector()
        Dq.shiftByDistance(s)
        g = Dq.get_FocalField(B, **kw)
        err = np.abs(g.field.cpu().numpy()[0] - f.field.cpu().numpy()[q]).max()
        assert err <= 1e-12 * f.amplitude_sum, (q, err)


def test_two_calls_give_identical_bytes(relay4):
    last, D = relay4["last"], relay4["D"]
    a = D.get_FocalField(last, Pixels=(70, 66), Shifts=(0.0, 0.3))
    b = D.get_FocalField(last, Pixels=(70, 66), Shifts=(0.0, 0.3))
    assert a.field.cpu().numpy().tobytes() == b.field.cpu().numpy().tobytes()


def test_dead_slots_give_the_field_of_the_survivors(hip):
    from attosecondraytracing_amd.bundle import RayBundle
    B = _random_bundle(hip, 4000, 3, dead=0.4)
    D = _detector()
    P, V, L, alive, w = fc.bundle_arrays(B)
    S = RayBundle.from_arrays(P[alive], V[alive], intensity=w[alive], wavelength=1e-3, path0=L[alive], backend=hip)
    kw = dict(Size=0.04, Pixels=(31, 27), Centre=(0.0, 0.0), RefPath=0.0)
    a, b = D.get_FocalField(B, **kw), D.get_FocalField(S, **kw)
    assert a.amplitude_sum == pytest.approx(b.amplitude_sum, rel=1e-14)
    assert np.abs(a.field.cpu().numpy() - b.field.cpu().numpy()).max() <= 1e-11 * a.amplitude_sum


def test_empty_and_all_dead_bundles(hip):
    from attosecondraytracing_amd.focal import FocalField
    D = _detector()
    dead = _random_bundle(hip, 500, 4, dead=0.0)
    dead.alive[:] = 0
    dead.touch()
    f = D.get_FocalField(dead, Size=0.01, Pixels=(9, 5), Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    assert f.field.shape == (2, 5, 9)
    assert np.all(f.field.cpu().numpy() == 0)
    assert np.isnan(f.strehl).all() and f.amplitude_sum == 0.0
    # n = 0: the call writes zeros over whatever the field held
    d = _desc(D)
    field = hip.focal_field(d, dead.view(), None, 0)
    assert field.shape == (2, 8, 8) and not field.cpu().numpy().any()
    e = FocalField(field, np.arange(8.0), np.arange(8.0), (0.0, 0.0), 1e-3, 0.0, 0.0)
    assert np.isnan(e.strehl).all()


def _desc(D, **over):
    from attosecondraytracing_amd import _abi
    d = _abi.ArtFocalDesc()
    d.det = D._desc()
    d.k, d.L_ref, d.x0, d.dx, d.y0, d.dy, d.nx, d.ny, d.planes = 2 * np.pi / 1e-3, 0.0, -0.01, 1e-3, -0.01, 1e-3, 8, 8, 2
    for key, v in over.items():
        if key == "shift1":
            d.shift[1] = v
        else:
            setattr(d, key, v)
    return d


@pytest.mark.parametrize("over, msg", [
    (dict(nx=0), "nx and ny"), (dict(nx=2049), "nx and ny"), (dict(ny=0), "nx and ny"), (dict(ny=2049), "nx and ny"),
    (dict(planes=0), "planes"), (dict(planes=65), "planes"),
    (dict(k=0.0), "k must"), (dict(k=-1.0), "k must"), (dict(k=float("nan")), "k must"), (dict(k=float("inf")), "k must"),
    (dict(dx=float("nan")), "pitch"), (dict(dy=float("inf")), "pitch"), (dict(shift1=float("nan")), "shifts"),
    (dict(field=None), "must not be NULL"), (dict(scratch=None), "must not be NULL")])
def test_invalid_descriptors_launch_nothing(hip, over, msg):
    import torch
    B = _random_bundle(hip, 256, 5)
    D = _detector()
    over = dict(over)
    use_field, use_scratch = over.pop("field", True), over.pop("scratch", True)
    d = _desc(D, **over)
    field = torch.full((2 * 8 * 8 * 2,), 7.25, dtype=torch.float64, device=hip.device)
    scratch = torch.zeros(1 << 20, dtype=torch.float64, device=hip.device)
    rc = hip.fn["art_focal_field"](C.byref(d), C.byref(B.view()), B.intensity.data_ptr(), B.n_slots,
                                   scratch.data_ptr() if use_scratch else None, field.data_ptr() if use_field else None,
                                   hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and msg in hip.last_error(), (rc, hip.last_error())
    assert bool((field == 7.25).all())
    assert hip.fn["art_focal_scratch_doubles"](0, 8, 1, 10) == -1


def test_focal_plots_draw(hip):
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    B = fc.converging_bundle(3000, 0.05, 10.0, wavelength=1e-3, backend=hip)
    D = _detector(centre=(0.0, 0.0, -0.2))
    fig = mpl.FocalSpot(B, D, Pixels=33, Log=True)
    s0 = fig._art_focal.strehl[0]
    fig._art_press(types.SimpleNamespace(key="right"))
    assert fig._art_focal.strehl[0] != s0 and fig._art_focal.field.shape == (1, 33, 33)
    fig2 = mpl.ThroughFocus(B, D, Shifts=np.linspace(0.0, 0.4, 9), Pixels=17)
    s = fig2._art_focal.strehl
    assert s.shape == (9,) and np.argmax(s) == 4 and s[4] == pytest.approx(1.0, abs=1e-4)
    import matplotlib.pyplot as plt
    plt.close("all")

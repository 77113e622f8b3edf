"""GPU (-m gpu): art_wavefront and Detector.get_Wavefront against the NumPy oracle of tests/wavefront_common.py, tied to
the focal field of art_focal_field, and its determinism, batching and edge cases."""
import math

import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import focal_common as fc
import wavefront_common as wc

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


def _relay4(hip, n, weights=True):
    import torch
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=n)
    last = chain.get_output_rays()[-1]
    if weights:
        g = torch.Generator(device="cpu").manual_seed(7)
        last.intensity = torch.exp(-0.5 * torch.randn(last.n_slots, generator=g, dtype=torch.float64) ** 2).to(hip.device)
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    return last, D


@pytest.fixture(scope="module")
def relay4(hip):
    """relay4 traced with 1e5 rays, Gaussian weights on the final bundle, a detector placed 600 mm downstream."""
    last, D = _relay4(hip, 10 ** 5)
    return {"last": last, "D": D}


def _detector():
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0]))


def _aberrated(hip, coeffs, n, NA=0.05):
    """converging_bundle (focus at the origin) with sum c_nm Z_nm(pupil) added to the paths."""
    import torch
    B = fc.converging_bundle(n, NA, 2.0, backend=hip)
    D = _detector()
    rot = np.array(D._desc().rot[:]).reshape(3, 3)
    u = B.data[3:6, :n].cpu().numpy().T
    a, b = u @ rot[0], u @ rot[1]
    rho = np.sqrt((a ** 2 + b ** 2).max())
    order = max(k[0] for k in coeffs)
    Z = wc.zernike_matrix(a / rho, b / rho, order)
    keys = [(nn, m) for nn in range(order + 1) for m in range(nn + 1)]
    B.data[6, :n] += torch.from_numpy(sum(c * Z[keys.index(k)] for k, c in coeffs.items())).to(hip.device)
    B.touch()
    return B, D


def _check_against_oracle(wf, r, order, G=None):
    G = wc.gram(r, order) if G is None else G
    d = np.sqrt(np.outer(np.diag(G), np.diag(G)))
    assert np.all(np.abs(wf.gram - G) <= 1e-12 * d + 1e-300), np.max(np.abs(wf.gram - G) / np.maximum(d, 1e-300))
    c, _, _, _ = wc.fit(r, order)
    got = np.array(list(wf.coefficients.values()))
    assert np.abs(got - c).max() <= 1e-9 * np.abs(c).max()
    assert wf.count == int(r["used"].sum()) and wf.outside == r["outside"]
    assert wf.pupil_radius == pytest.approx(r["rho"], rel=1e-15)
    assert wf.w_range == (r["W"].min(), r["W"].max())


def test_gram_and_coefficients_match_the_oracle(relay4):
    B, D = relay4["last"], relay4["D"]
    wf = D.get_Wavefront(B)
    assert wf.order == 8 and wf.count == len(B)
    _check_against_oracle(wf, wc.of_bundle(B, D, wf), 8)
    # an explicit pupil off the axis, another order and reference point
    wf = D.get_Wavefront(B, Order=10, PupilCentre=(1e-4, -2e-4), PupilRadius=0.8 * wf.pupil_radius, Centre=(0.01, -0.02),
                         Shift=0.5)
    r = wc.of_bundle(B, D, wf, radius=wf.pupil_radius)
    assert r["outside"] > 0
    _check_against_oracle(wf, r, 10)


def test_synthetic_recovery_on_the_device(hip):
    coeffs = {(2, 0): 3e-5, (2, 1): -2e-5, (3, 1): 1.5e-5, (4, 2): -8e-6, (6, 3): 4e-6, (8, 4): 2e-6}
    B, D = _aberrated(hip, coeffs, 3001)                 # not a multiple of the 64-ray chunk
    wf = D.get_Wavefront(B, Order=8)
    big = max(abs(v) for v in coeffs.values())
    for k, v in wf.coefficients.items():
        assert k == (0, 0) or abs(v - coeffs.get(k, 0.0)) <= 1e-10 * big, (k, v)
    assert wf.rms_residual <= 1e-7 * wf.rms and wf.count == 3001


def _phasor_strehl(wf, B):
    import torch
    used = torch.isfinite(wf.opd)
    w = torch.ones_like(wf.opd) if B.intensity is None else B.intensity[:B.n_slots]
    a = torch.where(used, torch.sqrt(torch.where(used, w, 0.0)), 0.0)
    ph = 2 * math.pi / B.wavelength * torch.where(used, wf.opd, 0.0)
    s = torch.complex(a * torch.cos(ph), a * torch.sin(ph)).sum()
    return float(abs(s) ** 2 / a.sum() ** 2)


def _focal_at(D, B, centre, shift, **kw):
    """get_FocalField's one pixel at (X, Y) in the plane of shift (a one-pixel grid lies at Centre - Size / 2)."""
    h = 1e-9
    return D.get_FocalField(B, Size=2 * h, Pixels=1, Centre=(centre[0] + h, centre[1] + h), Shifts=[shift], **kw)


def test_per_ray_error_is_the_focal_field_phase(relay4):
    B, D = relay4["last"], relay4["D"]
    for centre, shift in (((0.0, 0.0), 0.0), ((2e-4, -1e-4), 0.3)):
        wf = D.get_Wavefront(B, Order=6, Centre=centre, Shift=shift, PerRay=True)
        f = _focal_at(D, B, centre, shift, RefPath=wf.ref_path)
        assert _phasor_strehl(wf, B) == pytest.approx(f.strehl[0], rel=1e-6)
        x, y = wf.pupil.cpu().numpy()
        r = wc.of_bundle(B, D, wf)
        assert np.allclose(x[r["used"]], r["x"], rtol=0, atol=1e-15) and np.isnan(x[~r["used"]]).all()
        assert np.allclose(wf.opd.cpu().numpy()[r["used"]], r["W"], rtol=0, atol=1e-15)


def test_marechal_matches_the_focal_strehl_when_weakly_aberrated(hip):
    B, D = _aberrated(hip, {(2, 0): 7.5e-5, (3, 1): 5e-5, (4, 2): 2.5e-5}, 20000)
    wf = D.get_Wavefront(B, Order=6, PerRay=True)
    assert 0.8 < wf.strehl_marechal < 0.99
    X, Y, S = wf.best_focus
    f = _focal_at(D, B, (X, Y), S)
    assert wf.strehl_marechal == pytest.approx(f.strehl[0], rel=0.02)


def test_deterministic_and_batch_equals_single_calls(hip, relay4):
    from attosecondraytracing_amd import wavefront
    B, D = relay4["last"], relay4["D"]
    B2, D2 = _aberrated(hip, {(2, 0): 1e-5, (3, 2): 4e-6}, 3001)
    reqs = [(B, D, {"Order": 8}), (B2, D2, {"Order": 3}), (B, D, {"Order": 8, "Shift": 0.2}),
            (B2, D2, {"Order": 10, "PupilRadius": 0.03})]
    key = lambda w: (w.gram.tobytes(), w.count, w.outside, w.sum_w, w.pupil_radius, w.w_range)
    batch = wavefront.wavefronts(reqs)
    again = wavefront.wavefronts(reqs)
    single = [wavefront.wavefronts([q])[0] for q in reqs]
    for a, b, c in zip(batch, again, single):
        assert key(a) == key(b) == key(c)


def test_empty_and_all_dead(hip):
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd import wavefront
    B = fc.converging_bundle(500, 0.05, 2.0, backend=hip)
    B.alive[:] = 0
    B.touch()
    E = RayBundle.from_arrays(np.zeros((0, 3)), np.zeros((0, 3)), wavelength=1e-3, backend=hip)
    for bundle in (B, E):
        wf = wavefront.wavefronts([(bundle, _detector(), {"Order": 4, "RefPath": 0.0, "PerRay": True})])[0]
        assert wf.count == 0 and wf.outside == 0 and wf.sum_w == 0.0 and not np.any(wf.gram)
        assert math.isnan(wf.rms) and all(math.isnan(v) for v in wf.coefficients.values())
        assert bool(wf.opd.isnan().all())


def test_plots(relay4):
    import matplotlib.pyplot as plt
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    fig = mpl.WavefrontMap(relay4["last"], relay4["D"], Order=6, Pixels=33)
    assert np.isfinite(fig._art_wavefront.rms)
    plt.close(fig)


def test_ten_million_rays(hip):
    """All launches at full size (512 slices): G against the oracle summed over 1e6-ray chunks of the same bundle."""
    B, D = _relay4(hip, 10 ** 7)
    wf = D.get_Wavefront(B, Order=6)
    r = wc.of_bundle(B, D, wf)
    G = np.zeros_like(wf.gram)
    for lo in range(0, len(r["W"]), 10 ** 6):
        part = {k: r[k][lo:lo + 10 ** 6] for k in ("W", "x", "y", "dn", "w")}
        G += wc.gram(part, 6)
    _check_against_oracle(wf, r, 6, G)

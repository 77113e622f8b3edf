"""GPU (-m gpu): art_ray_tubes and OpticalChain.get_RayTubes against the long-double restatement of
tests/tubes_common.py on the device's own traced histories (every scene of the host tests, a KB pair of quadrics through
the stepwise trace, an ExtendedSource), dead rays, determinism, batching, PerRay=False, the re-weighted bundle and what it
does to the focal field of a 10:1 grazing ellipsoid."""
import numpy as np
import pytest

import tubes_common as tb

pytestmark = pytest.mark.gpu
WAVELENGTH = 800e-6


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


def _detector(det):
    import ART.ModuleDetector as mdet
    if det is None:
        return None
    return mdet.Detector(np.asarray(det[0], dtype=float), np.asarray(det[0], dtype=float), np.asarray(det[1], dtype=float))


def _chain(sc):
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    P0, D0 = sc["rays"]
    src = RayBundle.from_arrays(P0, D0, np.arange(len(P0)), sc["w"], WAVELENGTH)
    chain = OpticalChain(src, sc["els"])
    chain.get_output_rays()
    return chain


def _reference(chain, sc, det=None):
    """The restatement on the device's own history: what art_ray_tubes reads."""
    src, out = chain.source_rays, chain.get_output_rays()
    bundles = [src] + [out[k] for k in range(len(chain.optical_elements))]
    hist = [(b.data[0:3].cpu().numpy().T.copy(), b.data[3:6].cpu().numpy().T.copy()) for b in bundles]
    alive = np.logical_and.reduce([b.alive.cpu().numpy() != 0 for b in bundles])
    w = bundles[-1].intensity
    det = sc["det"] if det is None else det
    return tb.run([tb.spec_of(oe) for oe in chain.optical_elements], hist, sc["source"], det,
                  None if w is None else w.cpu().numpy(), alive)


def _per_ray(t):
    return {"solid_angle": t.solid_angle.cpu().numpy(), "area": t.area.cpu().numpy(), "kappa": t.curvature.cpu().numpy(),
            "axis": t.axis.cpu().numpy().T}


def _row(t):
    return np.array([t.count, t.sum_w, t.sum_weight, t.solid_angle_min, t.solid_angle_max, t.sum_area, t.mean_curvature[0],
                     t.mean_curvature[1], t.finite_count, t.asymmetry])


def check(t, ref, name):
    """Per-ray arrays and the sums row against the restatement, the project's parity bar; returns the worst deviation."""
    a = ref["alive"]
    worst = tb.check_against_restatement(_per_ray(t), ref, name)
    worst = max(worst, tb.compare(t.weight.cpu().numpy(), ref["weight"], a, name + " weight"))
    row = ref["row"]
    assert t.count == int(row[0]) == int(a.sum()) and t.finite_count == int(row[9]), name
    kscale = float(np.abs(ref["kappa"][:, ref["finite"]]).max()) if ref["finite"].any() else 1.0
    for got, want, scale in ((t.sum_w, row[1], row[1]), (t.sum_weight, row[2], row[2]), (t.solid_angle_min, row[3], row[4]),
                             (t.solid_angle_max, row[4], row[4]), (t.sum_area, row[5], row[5]),
                             (t.mean_curvature[0], row[6], kscale), (t.mean_curvature[1], row[7], kscale)):
        err = abs(float(got - want)) / float(scale)
        assert err <= tb.PARITY, (name, float(got), float(want))
        worst = max(worst, err)
    assert t.asymmetry <= tb.PARITY and float(row[10]) <= tb.PARITY, (name, t.asymmetry)
    assert t.magnification == t.sum_weight / t.sum_w
    return worst


@pytest.fixture(scope="module")
def runs(hip):
    """name -> (scene, chain, detector, RayTubes, restatement) for the scenes (a) - (e), each traced and analysed once."""
    out = {}
    for name, sc in tb.scenes().items():
        chain = _chain(sc)
        D = _detector(sc["det"])
        out[name] = (sc, chain, D, chain.get_RayTubes(Detector=D, Source=sc["source"]), _reference(chain, sc))
    return out


@pytest.mark.parametrize("name", ["a_toroid", "b_plane", "b_sphere", "b_parabola", "b_ellipsoid", "b_cylinder", "c_kb",
                                  "d_twisted", "e_masked"])
def test_scene_against_restatement(runs, name):
    sc, chain, D, t, ref = runs[name]
    worst = check(t, ref, name)
    print(f"{name}: {t.count} rays, worst deviation from the restatement {worst:.2e}; dOmega'/dmu in "
          f"[{t.solid_angle_min:.4g}, {t.solid_angle_max:.4g}], mean curvatures {t.mean_curvature}")
    if name != "e_masked":
        assert t.count == len(sc["rays"][0])
    if name == "c_kb":                                           # the quadrics went through the stepwise trace
        from attosecondraytracing_amd import ModuleProcessing as mp, _abi
        assert all(mp.element_descriptor(oe, True)[0].flags & _abi.ART_FLAG_QUADRIC for oe in chain.optical_elements)
    c = t.chief
    assert c["solid_angle"] == float(t.solid_angle[0]) and c["curvature"][0] <= c["curvature"][1]
    assert c["foci"][0] == -1.0 / c["curvature"][0]


def test_dead_rays_have_no_weight_and_stay_out_of_the_sums(runs):
    sc, chain, D, t, ref = runs["e_masked"]
    dead = ~ref["alive"]
    assert 100 < dead.sum() < len(dead) - 100 and t.count == int((~dead).sum())
    assert (t.weight.cpu().numpy()[dead] == 0).all() and (t.rays.intensity.cpu().numpy()[dead] == 0).all()
    got = _per_ray(t)
    for key in ("solid_angle", "area"):
        assert np.isnan(got[key][dead]).all() and np.isfinite(got[key][~dead]).all()
    assert np.isnan(got["kappa"][:, dead]).all() and np.isnan(got["axis"][dead]).all()
    w = chain.get_output_rays()[-1].intensity.cpu().numpy()
    assert abs(t.sum_w - w[~dead].sum()) <= 1e-12 * t.sum_w


def test_two_calls_give_identical_bytes_and_per_ray_off_the_same_sums(runs):
    for name in ("d_twisted", "e_masked", "c_kb"):
        sc, chain, D, t, _ = runs[name]
        again = chain.get_RayTubes(Detector=D, Source=sc["source"])
        sums = chain.get_RayTubes(Detector=D, Source=sc["source"], PerRay=False)
        for other in (again, sums):
            assert np.array_equal(_row(other), _row(t))
            assert np.array_equal(other.weight.cpu().numpy(), t.weight.cpu().numpy())
            assert np.array_equal(other.rays.intensity.cpu().numpy(), t.rays.intensity.cpu().numpy())
        for key, v in _per_ray(again).items():
            assert np.array_equal(v, _per_ray(t)[key], equal_nan=True), key
        assert sums.solid_angle is None and sums.curvature is None and sums.foci is None and sums.chief is None


def test_three_chains_in_one_call_equal_three_single_calls(runs):
    from attosecondraytracing_amd import tubes
    names = ["e_masked", "a_toroid", "c_kb"]                     # n = 1001, 1000, 1000; K = 3, 1, 2
    reqs = [(runs[n][1], dict(Detector=runs[n][2], Source=runs[n][0]["source"])) for n in names]
    for name, t in zip(names, tubes.ray_tubes(reqs)):
        single = runs[name][3]
        assert np.array_equal(_row(t), _row(single)), name
        assert np.array_equal(t.weight.cpu().numpy(), single.weight.cpu().numpy())
        for key, v in _per_ray(t).items():
            assert np.array_equal(v, _per_ray(single)[key], equal_nan=True), (name, key)


def test_reweighted_bundle_keeps_the_power(runs):
    for name, (sc, chain, D, t, ref) in runs.items():
        last = chain.get_output_rays()[-1]
        total = float(t.rays.intensity.sum())
        assert abs(total - t.sum_w) <= 1e-12 * t.sum_w, name
        assert t.rays.data.data_ptr() == last.data.data_ptr() and t.rays is not last       # an alias, not a copy
        irr = t.irradiance.cpu().numpy()
        w = np.ones(len(irr)) if last.intensity is None else last.intensity.cpu().numpy()
        a = ref["alive"]
        assert np.allclose(irr[a], w[a] / np.abs(np.asarray(ref["area"][a], dtype=float)), rtol=1e-9)


def test_extended_source_and_inferred_source_kinds(hip):
    """(f): 30 point sources of 300 rays on the toroid of (a); the kind ModuleSource recorded is used."""
    import ART.ModuleSource as msource
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    from attosecondraytracing_amd.bundle import RayBundle
    S = tb.scenes()
    sc = dict(S["a_toroid"], source="point")
    src = msource.ExtendedSource(np.zeros(3), np.array([1.0, 0.0, 0.0]), 0.1, 0.01, 9000, WAVELENGTH)
    assert src.n_slots == 9000 and src.rays_per_source == 300 and src.source_kind == "point"
    chain = OpticalChain(src, sc["els"])
    t = chain.get_RayTubes()
    assert t.count == 9000
    check(t, _reference(chain, sc), "f_extended")
    par = dict(S["b_parabola"])
    wave = msource.PlaneWaveDisk(np.zeros(3), np.array([1.0, 0.0, 0.0]), 10.0, 1000, WAVELENGTH)
    assert wave.source_kind == "plane" and msource.PointSource(np.zeros(3), np.array([1.0, 0, 0]), 0.01, 10).source_kind == "point"
    chain = OpticalChain(wave, par["els"])
    t = chain.get_RayTubes()
    check(t, _reference(chain, par), "plane wave, inferred")
    assert abs(-1.0 / t.mean_curvature[0] - 100.0) < 0.5 and t.count == 999
    anon = OpticalChain(RayBundle.from_arrays(*par["rays"], np.arange(tb.N_RAYS), None, WAVELENGTH), par["els"])
    with pytest.raises(ValueError, match="Source="):
        anon.get_RayTubes()


def test_apodisation_of_a_grazing_ellipsoid_changes_the_focal_spot_not_its_peak(hip):
    """10:1 demagnification at 5 degrees grazing: dOmega'/dOmega = (r1 / r2)^2 varies by more than a factor of two over the
    aperture.  The phases are untouched, so at the stigmatic focus the peak stays where it is and the Strehl ratio stays
    1; the intensity profile around it differs."""
    els, rays, F1, F2 = tb.ellipsoid_scene(1000.0, 100.0, 170.0, 2e-3, support=80.0)
    sc = dict(els=els, rays=rays, source="point", det=None, w=None)
    chain = _chain(sc)
    last = chain.get_output_rays()[-1]
    t = chain.get_RayTubes(Source="point")
    ref = _reference(chain, sc)
    assert t.count == tb.N_RAYS
    check(t, ref, "g_demagnifying")
    P = last.data[0:3].cpu().numpy().T
    r1, r2 = np.linalg.norm(P - F1, axis=1), np.linalg.norm(F2 - P, axis=1)
    assert np.abs(np.abs(t.solid_angle.cpu().numpy()) - (r1 / r2) ** 2).max() <= 1e-9 * ((r1 / r2) ** 2).max()
    assert t.solid_angle_max / t.solid_angle_min > 2.0
    d = F2 / np.linalg.norm(F2)                                  # the chief ray leaves the mirror's centre (the origin)
    D = _detector((F2, -d))
    plain = D.get_FocalField(last, Size=0.4, Pixels=65, Centre=(0.0, 0.0))
    tubed = D.get_FocalField(t.rays, Size=0.4, Pixels=65, Centre=(0.0, 0.0))
    assert np.array_equal(plain.peak, tubed.peak) and np.abs(plain.peak).max() == 0.0
    print(f"Strehl {plain.strehl[0]:.15f} (rays) {tubed.strehl[0]:.15f} (tubes.rays)")
    assert abs(plain.strehl[0] - tubed.strehl[0]) <= 1e-12 and abs(plain.strehl[0] - 1.0) <= 1e-9
    a, b = plain.intensity[0] / plain.intensity[0].sum(), tubed.intensity[0] / tubed.intensity[0].sum()
    l2 = np.linalg.norm(a - b) / np.linalg.norm(a)
    print(f"relative L2 difference of the focal profiles {l2:.3e}; dOmega'/dOmega in [{t.solid_angle_min:.1f}, {t.solid_angle_max:.1f}]")
    assert l2 > 1e-3

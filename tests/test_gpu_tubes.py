"""GPU (-m gpu): art_ray_tubes and OpticalChain.get_RayTubes against the long-double restatement of
tests/tubes_common.py on the device's own traced histories (every scene of the host tests, a KB pair of quadrics through
the stepwise trace, an ExtendedSource), dead rays, determinism, batching, PerRay=False, the re-weighted bundle and what it
does to the focal field of a 10:1 grazing ellipsoid.  Below the second rule: the shapes and edges of the kernels -- one
quadric in two optic frames, bundles of 1 to 70001 slots with dead source slots, guard bands around every output, the
optional arrays one at a time, a ray dead in a middle view only, unequal jobs in one call, more requests than a call
holds, and a detector at and just behind a focus."""
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


def _reference(chain, sc, det=None, specs=None, source=None):
    """The restatement on the device's own history: what art_ray_tubes reads.  det, specs, source: instead of the
    scene's detector, the elements' own descriptions and the scene's seed."""
    src, out = chain.source_rays, chain.get_output_rays()
    bundles = [src] + [out[k] for k in range(len(chain.optical_elements))]
    hist = [(b.data[0:3].cpu().numpy().T.copy(), b.data[3:6].cpu().numpy().T.copy()) for b in bundles]
    alive = np.logical_and.reduce([b.alive.cpu().numpy() != 0 for b in bundles])
    w = bundles[-1].intensity
    det = sc["det"] if det is None else det
    specs = [tb.spec_of(oe) for oe in chain.optical_elements] if specs is None else specs
    return tb.run(specs, hist, source or sc["source"], det, None if w is None else w.cpu().numpy(), alive)


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
    """name -> (scene, chain, detector, RayTubes, restatement) for the scenes (a) - (e) and (h), each traced and analysed
    once."""
    out = {}
    for name, sc in {**tb.scenes(), **tb.scenes_more()}.items():
        chain = _chain(sc)
        D = _detector(sc["det"])
        out[name] = (sc, chain, D, chain.get_RayTubes(Detector=D, Source=sc["source"]), _reference(chain, sc))
    return out


MORE = ["h_rotated_quadric", "h_hyperboloid", "h_convex_sphere", "h_convex_cylinder", "h_convex_quadric", "h_mixed8", "h_c3",
        "h_c2"]
LOSSY = {"h_c3": 673, "h_c2": 490}                               # survivors of the golden chains that lose rays


@pytest.mark.parametrize("name", ["a_toroid", "b_plane", "b_sphere", "b_parabola", "b_ellipsoid", "b_cylinder", "c_kb",
                                  "d_twisted", "e_masked"] + MORE)
def test_scene_against_restatement(runs, name):
    sc, chain, D, t, ref = runs[name]
    worst = check(t, ref, name)
    print(f"{name}: {t.count} rays, worst deviation from the restatement {worst:.2e}; dOmega'/dmu in "
          f"[{t.solid_angle_min:.4g}, {t.solid_angle_max:.4g}], mean curvatures {t.mean_curvature}")
    if name != "e_masked":
        assert t.count == LOSSY.get(name, len(sc["rays"][0]))
    if name in ("c_kb", "h_rotated_quadric", "h_hyperboloid", "h_convex_quadric"):   # quadrics: the stepwise trace
        from attosecondraytracing_amd import ModuleProcessing as mp, _abi
        assert all(mp.element_descriptor(oe, True)[0].flags & _abi.ART_FLAG_QUADRIC for oe in chain.optical_elements)
    if name == "h_mixed8":
        assert len(chain.optical_elements) == 8 and len({type(oe.type).__name__ for oe in chain.optical_elements}) == 3
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


# ------------------------------------------------------------------------------------------- the kernels' shapes and edges
SIZES = [1, 63, 64, 65, 255, 256, 257, 70001]                    # below a wavefront, around it, around a tile, 274 tiles
PAD, GUARD = 512, -7.25
ARRAYS = ("solid_angle", "area", "kappa1", "kappa2", "axis")


def _item(chain, source, det=None, per_ray=True):
    """What tubes._job takes: (history, elements, seed, Detector, PerRay)."""
    from attosecondraytracing_amd import tubes
    from attosecondraytracing_amd.polarisation import history
    return history(chain), list(chain.optical_elements), tubes._SEEDS[source], det, per_ray


def _launch(be, made):
    """One art_ray_tubes call for the jobs `made` (tubes._job's tuples): the rows of sums on the host."""
    return be.ray_tubes(*[[m[q] for m in made] for q in range(4)]).cpu().numpy()


def _as_tubes(row, made, chain):
    """A RayTubes over the arrays tubes._job allocated for a job."""
    from attosecondraytracing_amd import tubes
    return tubes.RayTubes(row, made[4][0], None, made[4][1], chain.get_output_rays()[-1].intensity)


def _bytes(t):
    """Everything a call wrote for one job, as host arrays."""
    out = {"row": _row(t), "weight": t.weight.cpu().numpy()}
    if t.solid_angle is not None:
        out.update(_per_ray(t))
    return out


def _same_bytes(a, b, what):
    a, b = _bytes(a), _bytes(b)
    assert a.keys() == b.keys(), what
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def _dead_slots_carry_nothing(t, dead):
    got = _per_ray(t)
    assert (t.weight.cpu().numpy()[dead] == 0).all()
    assert np.isnan(got["solid_angle"][dead]).all() and np.isnan(got["area"][dead]).all()
    assert np.isnan(got["kappa"][:, dead]).all() and np.isnan(got["axis"][dead]).all()
    assert np.isfinite(got["solid_angle"][~dead]).all() and not np.isnan(t.weight.cpu().numpy()).any()


@pytest.fixture(scope="module")
def sized(hip):
    """n -> (scene, chain, detector, RayTubes, restatement): the masked twisted toroids with n source slots of which every
    7th is dead (slot 0, the chief ray, lives; at n = 1 it is the bundle), each traced and analysed once."""
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    out = {}
    for n in SIZES:
        els, rays, det = tb.twisted(n, mask=True)
        sc = dict(els=els, rays=rays, source="point", det=det, w=0.5 + ((np.arange(n) * 0.6180339887498949) % 1.0))
        src = RayBundle.from_arrays(*rays, np.arange(n), sc["w"], WAVELENGTH)
        src.alive[6::7] = 0
        src.touch()
        chain = OpticalChain(src, els)
        chain.get_output_rays()
        D = _detector(det)
        out[n] = (sc, chain, D, chain.get_RayTubes(Detector=D, Source="point"), _reference(chain, sc))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_bundle_sizes_with_dead_source_slots(sized, n):
    sc, chain, D, t, ref = sized[n]
    assert t.weight.numel() == n and t.axis.shape == (3, n)
    dead = ~ref["alive"]
    assert not dead[0] and dead[6::7].all()
    assert 0 < t.count == int((~dead).sum()) and (t.count < n or n < 64)
    worst = check(t, ref, f"n = {n}")
    _dead_slots_carry_nothing(t, dead)
    _same_bytes(chain.get_RayTubes(Detector=D, Source="point"), t, f"n = {n}, second call")
    print(f"n = {n}: {t.count} rays count, worst deviation from the restatement {worst:.2e}")


def _guarded(be, n, made):
    """Points the job's outputs at [PAD : PAD + n] of tensors filled with GUARD (axis: 3 n slots); returns the tensors and
    their inner parts."""
    import torch
    j = made[0]
    T = {key: torch.full((n * (3 if key == "axis" else 1) + 2 * PAD,), GUARD, dtype=torch.float64, device=be.device)
         for key in ("weight",) + ARRAYS}
    for key, t in T.items():
        setattr(j, key, t.data_ptr() + 8 * PAD)
    return T, {key: t[PAD:t.numel() - PAD] for key, t in T.items()}


@pytest.mark.parametrize("n", [257, 70001])
def test_nothing_is_written_outside_the_n_slots_of_an_output(hip, sized, n):
    """The five per-ray outputs and `weight` lie inside larger tensors: slots >= n of the last tile, and slot n of one row
    of a packed block, must be dropped by the buffer descriptors, not stored."""
    import torch
    from attosecondraytracing_amd import tubes
    sc, chain, D, t, ref = sized[n]
    made = tubes._job(_item(chain, "point", D))
    T, inner = _guarded(hip, n, made)
    rows = _launch(hip, [made])
    for key, big in T.items():
        assert (big[:PAD] == GUARD).all() and (big[-PAD:] == GUARD).all(), key
        assert not (inner[key] == GUARD).any(), key
    arrays = (inner["solid_angle"], inner["area"], torch.stack([inner["kappa1"], inner["kappa2"]]), inner["axis"].reshape(3, n))
    got = tubes.RayTubes(rows[0], inner["weight"], None, arrays, chain.get_output_rays()[-1].intensity)
    worst = check(got, ref, f"n = {n} inside guard bands")
    _dead_slots_carry_nothing(got, ~ref["alive"])
    _same_bytes(got, t, f"n = {n} inside guard bands")
    print(f"n = {n} inside guard bands of {PAD} doubles: worst deviation from the restatement {worst:.2e}")


def test_optional_arrays_one_at_a_time(hip, sized):
    """Each of the five per-ray pointers alone, then all: a NULL array must cost nothing but itself."""
    from attosecondraytracing_amd import tubes
    n = 257
    sc, chain, D, t, ref = sized[n]
    want = _bytes(t)
    pick = lambda b, key: b["kappa"][int(key[-1]) - 1] if key.startswith("kappa") else b[key]
    for only in ARRAYS + (None,):
        made = tubes._job(_item(chain, "point", D))
        for key in ARRAYS:
            if only is not None and key != only:
                setattr(made[0], key, None)
        got = _bytes(_as_tubes(_launch(hip, [made])[0], made, chain))
        assert np.array_equal(got["row"], want["row"]) and np.array_equal(got["weight"], want["weight"]), only
        for key in ARRAYS if only is None else (only,):
            assert np.array_equal(pick(got, key), pick(want, key), equal_nan=True), (only, key)


def test_a_ray_dead_in_a_middle_view_only_does_not_count(runs):
    """h_c3: 50 rays that are alive in the source, after the mask and at the end are marked dead in the bundle after the
    first toroid alone.  `alive in every view`: they drop out of the count and the sums and carry no weight."""
    import torch
    sc, chain, D, t, ref = runs["h_c3"]
    out = chain.get_output_rays()
    assert len(out) == 3
    mid, last = out[1], out[2]
    live = np.flatnonzero(ref["alive"])
    live = live[live != 0]
    chosen = live[np.linspace(0, len(live) - 1, 50).astype(int)]
    assert len(set(chosen)) == 50 and len(set(chosen // 256)) == len(set(live // 256)) > 1     # (in every tile with rays)
    idx = torch.from_numpy(chosen).to(mid.alive.device)
    saved = mid.alive[idx].clone()
    assert (saved != 0).all()
    try:
        mid.alive[idx] = 0
        got = chain.get_RayTubes(Detector=D, Source=sc["source"])
        ref2 = _reference(chain, sc)
        assert (last.alive[idx] != 0).all() and (chain.source_rays.alive[idx] != 0).all() and (out[0].alive[idx] != 0).all()
    finally:
        mid.alive[idx] = saved
    assert got.count == t.count - 50 == int(ref2["alive"].sum())
    assert not ref2["alive"][chosen].any()
    worst = check(got, ref2, "h_c3 with 50 rays dead in the middle view")
    _dead_slots_carry_nothing(got, ~ref2["alive"])
    w = last.intensity.cpu().numpy()
    assert abs((t.sum_w - got.sum_w) - w[chosen].sum()) <= 1e-12 * t.sum_w
    _same_bytes(chain.get_RayTubes(Detector=D, Source=sc["source"]), t, "h_c3 after the bytes were put back")
    print(f"h_c3, 50 rays dead in the middle view only: {got.count} count, worst deviation from the restatement {worst:.2e}")


def test_the_same_quadric_in_another_optic_frame(hip, runs):
    """h_rotated_quadric's surface described again in an optic frame turned by 50 degrees about (1, 2, 3) and shifted by
    (3, -2, 5) mm (tubes_common.reframed): b[0], b[1], c and the element's centre are all set.  Both jobs in one call on
    the same history: each against the restatement of its description, and against the other."""
    from attosecondraytracing_amd import tubes
    sc, chain, D, t, ref = runs["h_rotated_quadric"]
    own, moved = tubes._job(_item(chain, "point", D)), tubes._job(_item(chain, "point", D))
    spec = tb.reframed(tb.spec_of(chain.optical_elements[0]))
    e = moved[2][0]
    fwd = np.asarray(spec["fwd"], dtype=float)
    e.fwd[:], e.bwd[:], e.centre[:] = list(fwd.reshape(9)), list(fwd.T.reshape(9)), list(np.asarray(spec["centre"], dtype=float))
    moved[3][0] = hip._quadric_desc(spec["coeff"])
    assert all(v != 0 for v in list(moved[3][0].q) + list(moved[3][0].b) + [moved[3][0].c] + list(e.centre))
    rows = _launch(hip, [own, moved])
    t_own, t_moved = _as_tubes(rows[0], own, chain), _as_tubes(rows[1], moved, chain)
    _same_bytes(t_own, t, "h_rotated_quadric beside its second description")
    ref2 = _reference(chain, sc, specs=[spec])
    worst = max(check(t_own, ref, "own frame"), check(t_moved, ref2, "moved frame"),
                check(t_moved, ref, "moved frame against the restatement in the own frame"))
    a, one, two = ref["alive"], _per_ray(t_own), _per_ray(t_moved)
    for key in ("solid_angle", "area", "kappa"):
        worst = max(worst, tb.compare(two[key], one[key], a, "the two descriptions: " + key))
    axis = tb.axes_error(two["axis"], one["axis"], a)
    assert axis <= tb.PARITY
    print(f"one quadric in two optic frames: worst deviation {max(worst, axis):.2e}")


@pytest.fixture(scope="module")
def kb257(hip):
    """c_kb's two elliptical cylinders with 257 unweighted rays, read with the plane-wave seed and without a detector."""
    S = tb.scenes()["c_kb"]
    sc = dict(els=S["els"], rays=tb.source_rays("point", 1e-3, 257), source="plane", det=None, w=None)
    chain = _chain(sc)
    return sc, chain, None, chain.get_RayTubes(Source="plane"), _reference(chain, sc)


def test_unequal_jobs_in_one_call_equal_their_single_calls(hip, sized, kb257):
    """1, 70001 and 257 slots and a job of no slots in one grid: the tiles a small job does not have return early, every
    job's partial sums lie at its own stride of the scratch area, and the order of the jobs changes nothing."""
    from attosecondraytracing_amd import tubes
    worst = check(kb257[3], kb257[4], "c_kb, 257 rays, plane seed")
    assert kb257[3].count == 257
    cases = [(sized[1], "point"), (sized[70001], "point"), (kb257, "plane"), (kb257, "plane")]

    def jobs():
        made = [tubes._job(_item(c[1], source, c[2])) for c, source in cases]
        made[3][0].n = 0
        return made

    single = []
    for k, m in enumerate(jobs()):
        row = _launch(hip, [m])[0]
        single.append(_as_tubes(row, m, cases[k][0][1]))
        if k == 3:
            assert row.shape == (16,) and not row.any()
        else:
            _same_bytes(single[k], cases[k][0][3], f"job {k} alone")
    for order in ([0, 1, 2, 3], [1, 3, 2, 0]):
        made = jobs()
        rows = _launch(hip, [made[k] for k in order])
        assert rows.shape == (4, 16) and not rows[order.index(3)].any()
        for pos, k in enumerate(order):
            if k != 3:
                _same_bytes(_as_tubes(rows[pos], made[k], cases[k][0][1]), single[k], f"job {k} at place {pos} of {order}")
    print(f"c_kb, 257 rays, plane seed: worst deviation from the restatement {worst:.2e}")


def test_more_requests_than_one_call_holds(sized):
    from attosecondraytracing_amd import tubes
    sc, chain, D, t, ref = sized[257]
    assert tubes.MAX_JOBS_PER_CALL == 64
    res = tubes.ray_tubes([(chain, dict(Detector=D, Source="point"))] * 65)
    assert len(res) == 65
    for k, other in enumerate(res):
        _same_bytes(other, t, f"request {k} of 65")
    assert len({r.weight.data_ptr() for r in res}) == 65


def test_detector_at_a_focus_and_just_behind_it(runs):
    """b_parabola, a plane wave onto a paraboloid: read at the last hit points, on the plane through the focus normal to
    the chief ray, and 5 mm further.  The detector moves neither the solid angles nor the weights; at the focus the
    areas vanish and the curvatures are whatever rounding makes of 1 / 0 (nothing is clamped), which the row's count and
    means must follow; 5 mm on every wavefront is a sphere about the focus."""
    from attosecondraytracing_amd import tubes
    sc, chain, _, t, ref = runs["b_parabola"]
    last = chain.get_output_rays()[-1]
    Dn = last.data[3:6].cpu().numpy().T
    d, F = Dn[0], np.asarray(sc["focus"], dtype=float)
    at, behind = _detector((F, -d)), _detector((F + 5.0 * d, -d))
    none, focus, five = tubes.ray_tubes([(chain, dict(Detector=det, Source="plane")) for det in (None, at, behind)])
    _same_bytes(none, t, "b_parabola beside two detectors")
    for other in (focus, five):
        assert np.array_equal(other.weight.cpu().numpy(), none.weight.cpu().numpy())
        assert np.array_equal(other.solid_angle.cpu().numpy(), none.solid_angle.cpu().numpy())
        assert (other.count, other.sum_w, other.sum_weight) == (none.count, none.sum_w, none.sum_weight)
    assert none.count == tb.N_RAYS
    area = np.abs(focus.area.cpu().numpy())
    assert area.max() <= tb.PARITY * np.abs(none.area.cpu().numpy()).max() and not np.isnan(focus.weight.cpu().numpy()).any()
    # 5 mm behind the focus: radius 5 / cos(angle to the chief ray) along each ray, 5 mm on the chief ray itself
    ref5 = _reference(chain, sc, det=(behind.centre, behind.normal))
    worst = check(five, ref5, "b_parabola 5 mm behind the focus")
    want = tb.ld(Dn) @ tb.ld(d) / 5
    k = five.curvature.cpu().numpy()
    for q in range(2):
        assert np.abs(tb.ld(k[q]) - want).max() <= tb.PARITY * 0.2
        assert abs(k[q][0] - 0.2) <= tb.PARITY * 0.2
    # at the focus: the row against long-double sums of the device's own per-ray curvatures
    k1, k2 = (tb.ld(v) for v in focus.curvature.cpu().numpy())
    fin = np.isfinite(k1) & np.isfinite(k2)
    assert focus.finite_count == int(fin.sum())
    if fin.any():
        kmax = max(np.abs(k1[fin]).max(), np.abs(k2[fin]).max())
        for got, kk in zip(focus.mean_curvature, (k1, k2)):
            assert abs(tb.LD(got) - kk[fin].sum() / fin.sum()) <= tb.PARITY * kmax, (got, float(kmax))
    else:
        assert focus.mean_curvature == (0.0, 0.0)
    print(f"b_parabola: 5 mm behind the focus worst deviation from the restatement {worst:.2e}; at the focus max |area| "
          f"{area.max():.2e} of {np.abs(none.area.cpu().numpy()).max():.2e}, {int((~fin).sum())} of {len(fin)} rays with "
          f"non-finite curvatures, mean curvatures {focus.mean_curvature}")

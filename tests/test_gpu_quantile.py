"""GPU (-m gpu): art_quantiles against the NumPy restatement of tests/quantile_common.py.

Given keys: every output EQUAL to the restatement (values by bit pattern, the two zeros equal; the sums are integers), over
the sizes at which a tile, a wave or a workgroup is partial, keys that are all equal, keys 1 + i 2^-52 that only the last
digit tells apart, both signs with +-inf and NaN, dead slots, weights of 0, no weight at all, fractions 0, 1, duplicated
and out of order, one and three planes, two calls and two scratch bounds.  Rank sums at thresholds below, above, on a key
and at +-inf.

Detector metrics, on a 4097-ray two-toroid focus and a KB focus with Shifts (-1, 0, 0.5) mm: the restatement works on
get_PointList2D and get_OpticalPaths of a detector moved to each plane (the delay is get_Delays' expression measured from
the mean path the device reports: the zero of the delay cancels in |delay - c|), and every returned radius r must satisfy
    sum q [key < r - eps]  <  T  <=  sum q [key <= r + eps],     |r - restated r| <= eps
with eps = 1e-12 of the largest |X|, |Y| (or |delay|) of the scene over the three planes."""
import numpy as np
import pytest

import focal_common as fc
import quantile_common as qc

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 70001]
FRACTIONS = [0.5, 0.0, 1.0, 0.5, 0.9, 0.1]             # 0, 1, a duplicate, out of order
SHIFTS = (-1.0, 0.0, 0.5)
LIGHT = 299792458000.0


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


def _keys(n, seed=0):
    """[3, n]: both signs with +-inf, NaN and the two zeros among them; all equal; 1 + i 2^-52."""
    rng = np.random.default_rng(seed + n)
    a = rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, size=n)
    a[1::11] = np.inf
    a[2::13] = -np.inf
    a[3::17] = np.nan
    a[4::19] = 0.0
    a[5::23] = -0.0
    return np.stack([a, np.full(n, 3.25), 1.0 + np.arange(n) * 2.0 ** -52])


def _weights(n, seed=0):
    w = np.random.default_rng(100 + seed + n).uniform(0.0, 2.0, size=n)
    w[::7] = 0.0
    return w


def _alive(n):
    return (np.arange(n) % 5 != 4).astype(np.uint8)      # dead slots interleaved; slot 0 alive


def _carrier(hip, n, alive, w):
    """A bundle that only lends its alive flags and intensities to weighted_quantiles."""
    import torch
    from attosecondraytracing_amd.bundle import RayBundle
    B = RayBundle.from_arrays(np.zeros((n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1)), intensity=w, backend=hip)
    if alive is not None:
        B.alive[:n].copy_(torch.from_numpy(np.asarray(alive, dtype=np.uint8)))
        B.touch()
    return B


def _device(hip, keys, fractions, w=None, alive=None, thresholds=None, bound=None):
    from attosecondraytracing_amd import quantile
    keys = np.asarray(keys, dtype=np.float64)
    n = keys.shape[-1]
    rays = _carrier(hip, n, alive, w) if (n > 0 and (alive is not None or w is not None)) else None
    return quantile.weighted_quantiles(hip.from_numpy(keys) if n else hip.empty(0).reshape(keys.shape), fractions, rays=rays,
                                       Thresholds=thresholds, ScratchBound=bound)


def _assert_equal(q, ref, what=""):
    assert qc.same_values(q.values, ref["values"]), (what, q.values, ref["values"])
    assert np.array_equal(q.below, ref["below"]) and np.array_equal(q.upto, ref["upto"]), (what, q.below, ref["below"], q.upto, ref["upto"])
    assert np.array_equal(np.stack([q.total, q.count, q.invalid], axis=1), ref["totals"]), (what, q.total, q.count, q.invalid, ref["totals"])
    if "rank_sums" in ref:
        assert np.array_equal(q.rank_sums, ref["rank_sums"]) and np.array_equal(q.rank_counts, ref["rank_counts"]), what


def _bytes(q):
    parts = [q.values, q.below, q.upto, q.total, q.count, q.invalid] + ([] if q.rank_sums is None else [q.rank_sums, q.rank_counts])
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


@pytest.mark.parametrize("n", SIZES)
def test_given_keys_equal_the_restatement(hip, n):
    keys, w, alive = _keys(n), _weights(n), _alive(n)
    q = _device(hip, keys, FRACTIONS, w, alive)
    _assert_equal(q, qc.restate(keys, w, alive, FRACTIONS, q.shift), f"n = {n}")
    assert q.values.shape == (3, len(FRACTIONS))
    if n >= 63:
        assert q.invalid[0] > 0 and q.invalid[1] == 0 and q.count[0] + q.invalid[0] == int(alive.sum())
        assert np.all(q.below < q.targets) and np.all(q.targets <= q.upto)
    if n == 0:
        assert np.isnan(q.values).all() and not q.total.any() and not q.count.any()


def test_last_digit_decides(hip):
    """keys 1 + i 2^-52, unit weights: the quantile at f is slot ceil(f n) - 1 exactly, whichever pass tells it apart."""
    n = 5000
    keys = 1.0 + np.arange(n) * 2.0 ** -52
    fr = [0.0, 1.0 / n, 0.25, 0.5, 0.75, 1.0 - 1.0 / n, 1.0]
    q = _device(hip, keys, fr)
    _assert_equal(q, qc.restate(keys, None, None, fr, 0))
    assert list(q.values[0]) == [keys[qc.target(n, f) - 1] for f in fr]
    assert list(q.upto[0] - q.below[0]) == [1] * len(fr)


@pytest.mark.parametrize("case", ["no_weights", "all_zero", "all_equal", "one_plane", "all_dead", "all_nan", "subnormal"])
def test_given_key_cases(hip, case):
    n = 1000
    keys, w, alive = _keys(n, 7), _weights(n, 7), _alive(n)
    if case == "no_weights":
        w = None
    elif case == "all_zero":
        w = np.zeros(n)
    elif case == "all_equal":
        keys = np.full((1, n), -2.5)
    elif case == "one_plane":
        keys = keys[0]
    elif case == "all_dead":
        alive = np.zeros(n, dtype=np.uint8)
    elif case == "all_nan":
        keys = np.full((2, n), np.nan)
    elif case == "subnormal":
        keys = np.stack([(np.arange(n) - n // 2) * 5e-324, -(np.arange(n) % 3) * 5e-324])
    q = _device(hip, keys, FRACTIONS, w, alive)
    _assert_equal(q, qc.restate(keys, w, alive, FRACTIONS, q.shift), case)
    if case in ("all_zero", "all_dead", "all_nan"):
        assert np.isnan(q.values).all() and not q.total.any() and not q.below.any() and not q.upto.any()
    if case == "all_nan":
        assert list(q.invalid) == [int(alive.sum())] * 2 and not q.count.any()
    if case == "no_weights":
        assert q.shift == 0 and np.array_equal(q.total, q.count)


def test_two_calls_and_two_scratch_bounds_give_the_same_bytes(hip):
    n = 70001
    keys, w, alive = _keys(n, 3), _weights(n, 3), _alive(n)
    th = [-np.inf, -1.0, 0.0, 3.25, np.inf]
    a = _device(hip, keys, FRACTIONS, w, alive, th)
    b = _device(hip, keys, FRACTIONS, w, alive, th)
    c = _device(hip, keys, FRACTIONS, w, alive, th, bound=1)          # one plane per block
    assert _bytes(a) == _bytes(b) == _bytes(c)
    _assert_equal(a, qc.restate(keys, w, alive, FRACTIONS, a.shift, th))


@pytest.mark.parametrize("n", [1, 65, 257, 70001])
def test_rank_sums_equal_the_restatement(hip, n):
    keys, w, alive = _keys(n, 11), _weights(n, 11), _alive(n)
    finite = keys[0][np.isfinite(keys[0])]
    on_a_key = float(np.sort(finite)[len(finite) // 2]) if len(finite) else 0.5
    per_plane = np.array([sorted([-np.inf, -1e300, on_a_key, 0.0, 1e300, np.inf]),       # below all, on a key, above all, +-inf
                          [-np.inf, 3.0, 3.25, 3.25, 3.5, np.inf],
                          [-np.inf, 0.0, 1.0, 1.0 + (n // 2) * 2.0 ** -52, 2.0, np.inf]])
    q = _device(hip, keys, [0.5], w, alive, per_plane)
    ref = qc.restate(keys, w, alive, [0.5], q.shift, per_plane)
    _assert_equal(q, ref, f"n = {n}")
    assert np.array_equal(q.rank_sums[:, -1], q.total) and np.array_equal(q.rank_counts[:, -1], q.count)
    assert not q.rank_sums[1:, 0].any()
    unweighted = _device(hip, keys, [0.5], None, alive, per_plane)
    _assert_equal(unweighted, qc.restate(keys, None, alive, [0.5], 0, per_plane))
    assert np.array_equal(unweighted.rank_sums, unweighted.rank_counts)


# ------------------------------------------------------------------------------------------------ detector metrics
def _toroid_focus():
    import ART.ModuleDetector as mdet
    import ART.ModuleMirror as mmirror
    import ART.ModuleProcessing as mp
    import ART.ModuleSupport as msupp
    src = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": 4097}
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    chain = mp.OEPlacement(src, [tor, tor], [600, 600], [80, -80], [0, 30.0], "toroids")
    last = chain.get_output_rays()[-1]
    det = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    det.autoplace(last, 600)
    return chain, last, det


def _kb_focus():
    import ART.ModuleDetector as mdet
    import ART.ModuleMirror as mmirror
    import ART.ModuleProcessing as mp
    import ART.ModuleSupport as msupp
    S = msupp.SupportRectangle(150.0, 20.0)
    src = {"Divergence": 1e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": 4097}
    kb = [mmirror.MirrorEllipticalCylinder(S, 1000.0, 400.0, 2.0), mmirror.MirrorEllipticalCylinder(S, 1100.0, 300.0, 2.0)]
    chain = mp.OEPlacement(src, kb, [1000.0, 100.0], [88.0, 88.0], [0.0, 90.0], "KB")
    last = chain.get_output_rays()[-1]
    u = np.array([1.0, 0.0, 0.0])
    for oe in chain.optical_elements:
        u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(chain.optical_elements[-1].position, dtype=float)
    return chain, last, mdet.Detector(pole, pole + 300.0 * u, -u)


@pytest.fixture(scope="module")
def foci(hip):
    """name -> (chain, last bundle, detector, per plane (X, Y, opl) of the alive rays on the moved detector, w)."""
    out = {}
    for name, make in (("toroids", _toroid_focus), ("kb", _kb_focus)):
        chain, last, det = make()
        planes = []
        for s in SHIFTS:
            d = det.copy_detector()
            d.shiftByDistance(s)
            P2 = d.get_PointList2D(last)
            planes.append((P2[:, 0].copy(), P2[:, 1].copy(), d.get_OpticalPaths(last)))
        out[name] = (chain, last, det, planes, last.intensities())
        assert len(planes[0][0]) > 4000
    return out


def _restated_keys(metric, plane, e, p):
    X, Y, opl = plane
    if metric == "radius":
        return np.sqrt((X - e.centre[p, 0]) ** 2 + (Y - e.centre[p, 1]) ** 2)
    if metric == "X":
        return np.abs(X - e.centre[p, 0])
    if metric == "Y":
        return np.abs(Y - e.centre[p, 1])
    return np.abs((opl - e.path_centre[p]) / LIGHT * 1e15 - e.delay_centre[p])


def _scale(metric, planes, e):
    if metric == "Delay":
        return max(np.abs((opl - e.path_centre[p]) / LIGHT * 1e15).max() for p, (_, _, opl) in enumerate(planes))
    return max(max(np.abs(X).max(), np.abs(Y).max()) for X, Y, _ in planes)


def _check_radii(metric, planes, w, e, fractions, what):
    eps = 1e-12 * _scale(metric, planes, e)
    q = qc.fixed_weights(w, e.quantiles.shift, len(planes[0][0]))
    worst = 0.0
    for p, plane in enumerate(planes):
        keys = _restated_keys(metric, plane, e, p)
        v, _, _, (W, valid, _) = qc.select(keys, q, None, fractions)
        assert (W, valid) == (e.quantiles.total[p], e.count[p]), (what, p)
        for k in range(len(fractions)):
            r, T = e.radii[p, k], e.quantiles.targets[p, k]
            lo, hi = int(q[keys < r - eps].sum()), int(q[keys <= r + eps].sum())
            worst = max(worst, abs(r - v[k]) / eps)
            print(f"{what} plane {p} f {fractions[k]}: r {r!r} restated {v[k]!r} |diff| / eps {abs(r - v[k]) / eps:.3g}")
            assert lo < T <= hi, (what, p, k, r, v[k], lo, T, hi, eps)
            assert abs(r - v[k]) <= eps, (what, p, k, r, v[k], eps)
    return worst


@pytest.mark.parametrize("metric", ["radius", "X", "Y", "Delay"])
@pytest.mark.parametrize("name", ["toroids", "kb"])
def test_detector_metrics_against_the_restatement(hip, foci, name, metric):
    chain, last, det, planes, w = foci[name]
    fr = (0.5, 0.8, 0.9)
    e = det.get_EncircledEnergy(last, Fractions=fr, Metric=metric, Shifts=SHIFTS)
    assert e.radii.shape == (3, 3) and np.array_equal(e.shifts, SHIFTS) and np.all(e.radii > 0)
    assert np.array_equal(e.count, [len(planes[0][0])] * 3)
    assert np.allclose(e.power, w.sum(), rtol=1e-12)
    _check_radii(metric, planes, w, e, fr, f"{name} {metric}")
    assert np.array_equal(e.hew, 2 * e.radii[:, 0])
    assert e.best_focus == SHIFTS[int(np.argmin(e.radii[:, 0]))]
    # the default centre is the intensity-weighted centroid
    eps = 1e-12 * _scale(metric, planes, e)
    for p, (X, Y, opl) in enumerate(planes):
        if metric == "Delay":
            delay = (opl - e.path_centre[p]) / LIGHT * 1e15
            print(f"{name} Delay plane {p}: centre {e.delay_centre[p]!r} numpy {(w * delay).sum() / w.sum()!r} eps {eps:.3g}")
            assert abs(e.delay_centre[p] - (w * delay).sum() / w.sum()) <= eps
            assert abs(e.path_centre[p] - opl.mean()) <= 1e-12 * opl.mean()
        else:
            assert abs(e.centre[p, 0] - (w * X).sum() / w.sum()) <= eps and abs(e.centre[p, 1] - (w * Y).sum() / w.sum()) <= eps
    # the chain-level form is the same call
    e2 = chain.get_EncircledEnergy(det, Fractions=fr, Metric=metric, Shifts=SHIFTS)
    assert _bytes(e2.quantiles) == _bytes(e.quantiles) and np.array_equal(e2.centre, e.centre)


@pytest.mark.parametrize("metric", ["radius", "Delay"])
def test_an_explicit_centre_is_used_as_given(hip, foci, metric):
    chain, last, det, planes, w = foci["toroids"]
    X, Y, opl = planes[1]
    auto = det.get_EncircledEnergy(last, Metric=metric, Shifts=SHIFTS)
    centre = 0.37 * auto.radii[1, 0] if metric == "Delay" else (float(np.median(X)), float(np.median(Y)) + 1e-4)
    e = det.get_EncircledEnergy(last, Fractions=(0.5, 0.9), Metric=metric, Centre=centre, Shifts=SHIFTS)
    if metric == "Delay":
        assert np.array_equal(e.delay_centre, [centre] * 3)
    else:
        assert np.array_equal(e.centre, [list(centre)] * 3)
    _check_radii(metric, planes, w, e, (0.5, 0.9), f"given centre {metric}")
    assert not np.array_equal(e.radii[:, 0], auto.radii[:, 0])


@pytest.mark.parametrize("metric", ["radius", "X"])
def test_enclosed_share_at_the_returned_radii(hip, foci, metric):
    chain, last, det, planes, w = foci["kb"]
    fr = (0.5, 0.8, 0.9)
    e = det.get_EncircledEnergy(last, Fractions=fr, Metric=metric, Shifts=SHIFTS)
    eps = 1e-12 * _scale(metric, planes, e)
    smaller = []
    for p, plane in enumerate(planes):
        keys = _restated_keys(metric, plane, e, p)
        smaller.append([keys[keys < e.radii[p, k] - eps].max() for k in range(3)])      # the next smaller distinct key
    Radii = np.unique(np.concatenate([e.radii.ravel(), np.ravel(smaller)]))
    c = det.get_EncircledEnergy(last, Fractions=fr, Radii=Radii, Metric=metric, Centre=e.centre, Shifts=SHIFTS)
    assert np.array_equal(c.radii, e.radii) and c.enclosed.shape == (3, len(Radii))
    assert np.array_equal(c.enclosed, c.quantiles.rank_sums / c.quantiles.total[:, None].astype(float))
    assert np.all(np.diff(c.quantiles.rank_sums, axis=1) >= 0)
    for p in range(3):
        for k, f in enumerate(fr):
            at, under = int(np.searchsorted(Radii, e.radii[p, k])), int(np.searchsorted(Radii, smaller[p][k]))
            assert c.quantiles.rank_sums[p, at] == e.quantiles.upto[p, k]               # the same slots, in integers
            assert c.enclosed[p, at] >= f
            assert c.quantiles.rank_sums[p, under] < e.quantiles.targets[p, k] and c.enclosed[p, under] < f


def test_a_bundle_without_alive_rays(hip, foci):
    import torch
    chain, last, det, planes, w = foci["toroids"]
    dead = last.copy()
    dead.alive.zero_()
    dead.touch()
    e = det.get_EncircledEnergy(dead, Radii=[0.0, 1.0], Shifts=SHIFTS)
    assert np.isnan(e.radii).all() and not e.count.any() and not e.power.any() and e.best_focus is None
    assert np.isnan(e.enclosed).all() and not e.quantiles.rank_sums.any()
    assert torch.equal(last.alive, chain.get_output_rays()[-1].alive) and last.alive.any()


def test_three_bundles_in_one_sequence_equal_three_calls(hip, foci):
    from attosecondraytracing_amd import quantile
    import ART.ModuleDetector as mdet
    w = 0.5 + (np.arange(3001) * 0.6180339887498949) % 1.0
    conv = fc.converging_bundle(3001, 0.05, 40.0, focus=(0.01, -0.02, 0.3), backend=hip, weights=w)
    cdet = mdet.Detector(np.zeros(3), np.zeros(3), np.array([0.0, 0.0, -1.0]))
    jobs = [(foci["toroids"][1], foci["toroids"][2], dict(Shifts=SHIFTS, Radii=[1e-3, 1e-2])),
            (foci["kb"][0], foci["kb"][2], dict(Metric="Delay", Fractions=(0.5, 0.9))),          # a chain: its last bundle
            (conv, cdet, dict(Metric="Y", Shifts=(0.0, 0.2)))]
    together = quantile.encircled_energies(jobs)
    for (rays, det, kw), e in zip(jobs, together):
        rays = rays.get_output_rays()[-1] if hasattr(rays, "get_output_rays") else rays
        single = det.get_EncircledEnergy(rays, **kw)
        assert _bytes(single.quantiles) == _bytes(e.quantiles)
        assert single.centre.tobytes() == e.centre.tobytes() and single.delay_centre.tobytes() == e.delay_centre.tobytes()
    assert together[2].count[0] == 3001 and together[1].metric == "Delay"

"""GPU (-m gpu): art_sensitivities and OpticalChain.get_Sensitivities against the long-double restatement of
tests/sensitivity_common.py on the device's own traced histories, end to end against central differences of device
re-traces built by get_OE_loop_list / get_source_loop_list, and the shapes and edges of the kernels: bundles of 1 to 1000
slots with dead source slots, guard bands around every per-ray output, the optional arrays one at a time and none, a ray
dead in a middle view only, determinism, unequal chains in one call and more requests than a call holds."""
import numpy as np
import pytest

import sensitivity_common as sn
import tubes_common as tb

pytestmark = pytest.mark.gpu
WAVELENGTH = 800e-6
NAMES = list(sn.SCENES) + ["e_masked", "h_c3", "h_rotated_quadric"]


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
    return mdet.Detector(np.asarray(det[0], dtype=float), np.asarray(det[0], dtype=float), np.asarray(det[1], dtype=float))


def _chain(sc, dead=None):
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    P0, D0 = sc["rays"]
    src = RayBundle.from_arrays(P0, D0, np.arange(len(P0)), sc["w"], WAVELENGTH)
    if dead is not None:
        src.alive[dead] = 0
        src.touch()
    chain = OpticalChain(src, sc["els"])
    chain.get_output_rays()
    return chain


def _history(chain):
    src, out = chain.source_rays, chain.get_output_rays()
    return [src] + [out[k] for k in range(len(chain.optical_elements))]


def _device_detector(chain, sc):
    """The scene's detector, or tubes_common.tilted_detector on the chief ray (slot 0) of the device's final bundle."""
    if sc["det"] is not None:
        return sc["det"]
    last = _history(chain)[-1].data[0:6, 0].cpu().numpy()
    return tb.tilted_detector(last[0:3], last[3:6])


def _reference(chain, det, D, origin):
    """The restatement on the device's own history, with the detector's own rot and the device's path."""
    from attosecondraytracing_amd.bundle import ROW_PATH
    bundles = _history(chain)
    hist = [(b.data[0:3].cpu().numpy().T.copy(), b.data[3:6].cpu().numpy().T.copy()) for b in bundles]
    alive = np.logical_and.reduce([b.alive.cpu().numpy() != 0 for b in bundles])
    w = bundles[-1].intensity
    els = chain.optical_elements
    rot = np.array(list(D._desc().rot)).reshape(3, 3)
    return sn.run([tb.spec_of(oe) for oe in els], [sn.axes_of(oe) for oe in els], hist, det, rot,
                  None if w is None else w.cpu().numpy(), alive, origin, bundles[-1].data[ROW_PATH].cpu().numpy())


def check(s, ref, K, name):
    """The table and the per-ray arrays against the restatement, the project's parity bar; returns the worst deviation."""
    a = ref["alive"]
    worst = sn.compare_table(s.table, ref["table"], K, name, ref["span"])
    assert s.count == int(a.sum()), name
    for key in ("dX", "dY", "dL"):
        got = getattr(s, key).cpu().numpy()
        assert got.shape == ref[key].shape, (name, key)
        assert np.isnan(got[:, ~a]).all(), (name, key)
        if a.any():
            worst = max(worst, sn.compare_columns(got, ref[key], a, f"{name} {key}", K))
    return worst


@pytest.fixture(scope="module")
def runs(hip):
    """name -> (scene, chain, (centre, normal), Detector, Sensitivities with PerRay, restatement), each traced and analysed once."""
    S = sn.all_scenes()
    out = {}
    for name in NAMES:
        sc = S[name]
        chain = _chain(sc)
        det = _device_detector(chain, sc)
        D = _detector(det)
        s = chain.get_Sensitivities(D, PerRay=True)
        out[name] = (sc, chain, det, D, s, _reference(chain, det, D, s.origin))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_restatement(runs, name):
    sc, chain, det, D, s, ref = runs[name]
    K = len(chain.optical_elements)
    worst = check(s, ref, K, name)
    print(f"{name}: {s.count} rays, {len(s.names)} degrees of freedom, worst deviation from the restatement {worst:.2e}")
    assert len(s.names) == 6 * (K + 1) == s.dX.shape[0] and s.dX.shape[1] == len(sc["rays"][0])
    if name in ("e_masked", "h_c3"):
        assert 100 < s.count < len(sc["rays"][0]) - 100
    else:
        assert s.count == len(sc["rays"][0])
    if name in ("c_kb", "h_rotated_quadric"):                    # quadrics
        from attosecondraytracing_amd import ModuleProcessing as mp, _abi
        assert all(mp.element_descriptor(oe, True)[0].flags & _abi.ART_FLAG_QUADRIC for oe in chain.optical_elements)
    # the origin is the weighted mean: the first moments about it are rounding of the sums
    T = s.table
    for q in (2, 3, 4):
        assert abs(T[0, q]) <= 1e-9 * np.sqrt(T[0, 1] * T[0, q + 3]), (name, q)
    # the derived quantities from the table
    sw = T[0, 1]
    assert np.allclose(s.centroid, T[1:, 0:2] / sw, rtol=1e-15, atol=0) and np.allclose(s.pointing, T[1:, 9:12] / sw, rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------------------ end to end
def _moments(chain, D):
    """Weighted centroid (mm) and mean path (mm) of a chain's final bundle on the detector, by the fused read-out."""
    st = D.readout(chain.get_output_rays()[-1], store=False)["stats"]
    return np.array([st[9] / st[8], st[10] / st[8], st[11] / st[8]]), int(st[0])


def _fd(chains, D, h):
    """chains at +h, -h, +h/2, -h/2: Richardson-extrapolated central differences of (X, Y, path) and their estimates."""
    m = [_moments(c, D) for c in chains]
    assert len({k for _, k in m}) == 1
    one, two = (m[0][0] - m[1][0]) / (2 * h), (m[2][0] - m[3][0]) / h
    return (4 * two - one) / 3, np.abs(two - one) / 3, m[0][1]


def test_end_to_end_against_central_differences_of_device_retraces(runs):
    """d_twisted loses no ray.  One shift and one rotation per element and one source tilt, the chains moved by the
    package's own loop lists (mm, degrees): centroid and mean path within 10 x the step-halving estimate."""
    sc, chain, det, D, s, ref = runs["d_twisted"]
    n = len(sc["rays"][0])
    fs = 1e15 / 299792458000
    cases = [(0, "shift_normal", 0.05), (0, "pitch", 1e-4), (1, "shift_cross", 0.05), (1, "roll", 1e-4)]
    for k, dof, h in cases:
        rot = not dof.startswith("shift")
        steps = [h, -h, h / 2, -h / 2]
        chains = chain.get_OE_loop_list(k, dof, [float(np.rad2deg(v)) if rot else v for v in steps])
        fd, est, count = _fd(chains, D, h)
        c = s.index(k, dof)
        got = np.array([s.centroid[c, 0], s.centroid[c, 1], s.delay[c] / fs])
        print(f"element {k} {dof}: get_Sensitivities {got}, finite differences {fd}, step-halving estimates {est}")
        assert count == n == s.count and (np.abs(got - fd) <= 10 * est).all(), (k, dof, got, fd, est)
    central, normal = chain._incidence_plane_axes()
    axis = np.cross(central, normal)
    h = 1e-4
    chains = chain.get_source_loop_list("tilt_in_plane", [float(np.rad2deg(v)) for v in (h, -h, h / 2, -h / 2)])
    fd, est, count = _fd(chains, D, h)
    p = s.predict(tilt_source=(axis, float(np.rad2deg(1.0))))
    got = np.array([p["centroid"][0], p["centroid"][1], p["delay"] / fs])
    print(f"source tilt in plane: get_Sensitivities {got}, finite differences {fd}, step-halving estimates {est}")
    assert count == n and (np.abs(got - fd) <= 10 * est).all(), (got, fd, est)


# ------------------------------------------------------------------------------------------- the kernels' shapes and edges
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]                     # below a wavefront, around it, around a tile, four tiles
PAD, GUARD = 512, -7.25
ARRAYS = ("dX", "dY", "dL")


def _bytes(s):
    out = {"table": s.table}
    if s.dX is not None:
        out.update({k: getattr(s, k).cpu().numpy() for k in ARRAYS})
    return out


def _same_bytes(a, b, what):
    a, b = _bytes(a), _bytes(b)
    assert a.keys() == b.keys(), what
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


@pytest.fixture(scope="module")
def sized(hip):
    """n -> (chain, (centre, normal), Detector, Sensitivities, restatement): the masked twisted toroids with n source slots
    of which every 7th is dead (slot 0, the chief ray, lives)."""
    out = {}
    for n in SIZES:
        els, rays, det = tb.twisted(n, mask=True)
        sc = dict(els=els, rays=rays, det=det, w=0.5 + ((np.arange(n) * 0.6180339887498949) % 1.0))
        chain = _chain(sc, dead=slice(6, None, 7))
        D = _detector(det)
        s = chain.get_Sensitivities(D, PerRay=True)
        out[n] = (chain, det, D, s, _reference(chain, det, D, s.origin))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_bundle_sizes_with_dead_source_slots(sized, n):
    chain, det, D, s, ref = sized[n]
    dead = ~ref["alive"]
    assert s.dX.shape == (24, n) and not dead[0] and dead[6::7].all()
    assert 0 < s.count == int((~dead).sum()) and (s.count < n or n < 7)
    worst = check(s, ref, 3, f"n = {n}")
    _same_bytes(chain.get_Sensitivities(D, PerRay=True), s, f"n = {n}, second call")
    print(f"n = {n}: {s.count} rays count, worst deviation from the restatement {worst:.2e}")


def _item(chain, D, per_ray):
    from attosecondraytracing_amd.polarisation import history
    return history(chain), list(chain.optical_elements), D, per_ray


def _launch(be, made):
    return be.sensitivities(*[[m[q] for m in made] for q in range(4)]).cpu().numpy()


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_guard_bands_and_each_optional_array_alone(hip, sized, n):
    """The three per-ray outputs lie inside larger tensors filled with a guard value: slots >= n of the last tile and of the
    last column must be dropped by the buffer descriptors.  Then each array alone, and none: a NULL array costs nothing
    but itself, and the table keeps its bytes."""
    import torch
    from attosecondraytracing_amd import sensitivity
    chain, det, D, s, ref = sized[n]
    want = _bytes(s)
    M = 24
    for only in ARRAYS + ("all", None):
        made = sensitivity._job(_item(chain, D, False), tuple(s.origin))
        big = {}
        for key in ARRAYS:
            if only in (key, "all"):
                big[key] = torch.full((M * n + 2 * PAD,), GUARD, dtype=torch.float64, device=hip.device)
                setattr(made[0], key, big[key].data_ptr() + 8 * PAD)
        table = _launch(hip, [made])
        assert np.array_equal(table, want["table"]), only
        for key, t in big.items():
            assert (t[:PAD] == GUARD).all() and (t[-PAD:] == GUARD).all(), (only, key)
            inner = t[PAD:PAD + M * n].reshape(M, n).cpu().numpy()
            assert not (inner == GUARD).any() and np.array_equal(inner, want[key], equal_nan=True), (only, key)


def test_a_ray_dead_in_a_middle_view_only_does_not_count(runs):
    """h_c3: 50 rays that are alive in the source, after the mask and at the end are marked dead in the bundle after the
    first toroid alone.  They drop out of the count and the sums and read NaN."""
    import torch
    sc, chain, det, D, s, ref = runs["h_c3"]
    out = chain.get_output_rays()
    assert len(out) == 3
    mid, last = out[1], out[2]
    live = np.flatnonzero(ref["alive"])
    chosen = live[np.linspace(0, len(live) - 1, 50).astype(int)]
    assert len(set(chosen)) == 50 and len(set(chosen // 256)) > 1
    idx = torch.from_numpy(chosen).to(mid.alive.device)
    saved = mid.alive[idx].clone()
    assert (saved != 0).all()
    try:
        mid.alive[idx] = 0
        got = chain.get_Sensitivities(D, PerRay=True)
        ref2 = _reference(chain, det, D, got.origin)
        assert (last.alive[idx] != 0).all() and (chain.source_rays.alive[idx] != 0).all() and (out[0].alive[idx] != 0).all()
    finally:
        mid.alive[idx] = saved
    assert got.count == s.count - 50 == int(ref2["alive"].sum()) and not ref2["alive"][chosen].any()
    worst = check(got, ref2, 3, "h_c3 with 50 rays dead in the middle view")
    assert np.array_equal(got.origin, s.origin)                 # (the origin is the final bundle's: only an offset)
    _same_bytes(chain.get_Sensitivities(D, PerRay=True), s, "h_c3 after the bytes were put back")
    print(f"h_c3, 50 rays dead in the middle view only: {got.count} count, worst deviation from the restatement {worst:.2e}")


def test_per_ray_off_gives_the_same_table(runs):
    for name in ("d_twisted", "e_masked"):
        sc, chain, det, D, s, ref = runs[name]
        sums = chain.get_Sensitivities(D)
        assert sums.dX is None and sums.dY is None and sums.dL is None
        assert np.array_equal(sums.table, s.table), name


def test_three_unequal_chains_in_one_call_equal_three_single_calls(runs, sized):
    """K = 3, 1 and 8 with 1001, 1000 and 1000 slots, then 257 and 1 slots beside them, in two orders: every job's partial
    sums lie at its own stride of the scratch area, the tables follow one another, and the order changes nothing."""
    from attosecondraytracing_amd import sensitivity
    cases = [(runs[n][1], runs[n][3], runs[n][4]) for n in ("e_masked", "a_toroid", "h_mixed8")]
    cases += [(sized[n][0], sized[n][2], sized[n][3]) for n in (257, 1)]
    for order in ([0, 1, 2], [2, 4, 0, 3, 1]):
        res = sensitivity.sensitivities([(cases[k][0], dict(Detector=cases[k][1], PerRay=True)) for k in order])
        for pos, k in enumerate(order):
            _same_bytes(res[pos], cases[k][2], f"job {k} at place {pos} of {order}")


def test_more_requests_than_one_call_holds(sized):
    from attosecondraytracing_amd import sensitivity
    chain, det, D, s, ref = sized[257]
    assert sensitivity.MAX_JOBS_PER_CALL == 64
    res = sensitivity.sensitivities([(chain, dict(Detector=D, PerRay=True))] * 65)
    assert len(res) == 65
    for k, other in enumerate(res):
        _same_bytes(other, s, f"request {k} of 65")
    assert len({r.dX.data_ptr() for r in res}) == 65

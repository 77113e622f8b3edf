"""GPU (-m gpu): art_focal_vector_chromatic and OpticalChain.get_ChromaticFocalPulse(Coatings=...) against the truth of
tests/vector_chromatic_common.py (mpmath per ray and frequency, NumPy direct sum), against art_focal_vector_spectrum's
bytes where the contract says bytes, and at the edges.  Bars: 1e-9 amplitude_sum |P| against the truth
(tests/test_gpu_vector_pulse.py's), byte equality between device paths.

Shapes: 65 x 3 pixels (two 64-wide tiles, one partial), 2 planes, 5 table rows, 10 007 slots (no multiple of the 32-ray
chunk; 64 slices of the rays), a made-up history mirror, mask, mirror, mirror under 40-period Mo/Si with tabulated
materials and gold."""
import ctypes as C
import math

import numpy as np
import pytest

import coating_cases as cc
import vector_chromatic_common as vcc
import vector_pulse_truth as vt
from conftest import report

pytestmark = pytest.mark.gpu

WL = 13.5e-6
K0 = 2 * np.pi / WL
N = 10007
AXIS = np.array([0.0, 0.0, 1.0])
STATES = {"linear": (0.0, 1.0, 0.0), "circular": (1 / math.sqrt(2), 1j / math.sqrt(2), 0.0)}
GRID = dict(Size=(6e-4, 4e-5), Pixels=(65, 3), Centre=(0.0, 0.0), Shifts=(0.0, 0.02))
NAN, INF = float("nan"), float("inf")


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


def _detector():
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.array([0.0, 0.0, -50.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0]))


def _history(hip, dead_mask, seed=17, n=N):
    """tests/test_gpu_vector_pulse.py's made-up history: random unit directions per view (the mask does not turn the
    ray), the last bundle converging near the origin; the slots of dead_mask dead in the LAST bundle only."""
    from attosecondraytracing_amd.bundle import RayBundle
    rng = np.random.default_rng(seed)

    def dirs(axis, spread):
        u = np.asarray(axis, float)[None, :] + rng.normal(0, spread, (n, 3))
        return u / np.linalg.norm(u, axis=1)[:, None]

    views = [dirs(AXIS, 0.02), dirs((0.3, 0.1, -1), 0.02)]
    views += [views[-1].copy(), dirs((1, 0.2, 0.1), 0.02), dirs((0.05, -0.02, 1), 0.03)]
    pts = -5.0 * views[-1] + rng.normal(0, 2e-4, (n, 3))
    bundles = [RayBundle.from_arrays(rng.normal(0, 1, (n, 3)), v, wavelength=WL, backend=hip) for v in views[:-1]]
    last = RayBundle.from_arrays(pts, views[-1], intensity=rng.uniform(0.2, 2.0, n), wavelength=WL,
                                 path0=rng.normal(0, 3e-6, n), backend=hip)
    last.alive[hip.from_numpy(np.asarray(dead_mask, dtype=bool))] = 0
    last.touch()
    return bundles + [last]


def _coats():
    coat = vt.dispersive_copy(cc.mosi(40), WL, 8e-6, 25e-6)
    return [coat, None, cc.gold(), coat]


@pytest.fixture(scope="module")
def hist(hip):
    """The history with three slots in ten dead, its coatings and detector."""
    dead = np.random.default_rng(1).random(N) < 0.3
    return {"bundles": _history(hip, dead), "dead": dead, "coats": _coats(), "D": _detector()}


def _sdesc(D, B, k0, dk, nk, **kw):
    from attosecondraytracing_amd import _abi, focal
    kw = dict(GRID, **kw)
    fd, _, _, _, _, _, _ = focal.focal_desc(D, B, kw["Size"], kw["Pixels"], kw["Centre"], kw["Shifts"], None, 5.0)
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.f.k, sd.dk, sd.nk = k0, dk, nk
    return sd


def _progression(sd):
    return sd.f.k + np.arange(sd.nk) * sd.dk


def _neutral(sd):
    k = _progression(sd)
    return np.stack([k, 0 * k, 0 * k, 0 * k], axis=1)


def _spectrum(bundles, coats, P, sd, scratch_bytes=None):
    from attosecondraytracing_amd import vector_pulse
    return vector_pulse._vector_spectrum(bundles, coats, np.asarray(P, dtype=complex), sd, 2 * np.pi / _progression(sd),
                                         scratch_bytes).cpu().numpy()


def _chromatic(bundles, coats, P, sd, table, axis=AXIS, scratch_bytes=None):
    """art_focal_vector_chromatic through the Python layer's one caller: the materials' rows are the table's rows."""
    from attosecondraytracing_amd import _abi, vector_pulse
    table = np.asarray(table, dtype=float)
    one = _abi.ArtFocalSpectrumDesc.from_buffer_copy(sd)
    one.nk = len(table)
    return vector_pulse._vector_spectrum(bundles, coats, np.asarray(P, dtype=complex), one, 2 * np.pi / table[:, 0],
                                         scratch_bytes, chromatic=(axis, table)).cpu().numpy()


def _amp_sum(B):
    from attosecondraytracing_amd import focal
    return focal.amplitude_sum(B)


# a list of wavenumbers that is no progression, with apodisation and source offsets that matter: u ~ 4e-4 for the
# source's 0.02 rad spread per axis, so u c reaches ~0.3 and k z u ~0.6 rad for a typical ray
TABLE = np.array([[0.93 * K0, 0.0, 0.0, 0.0], [0.95 * K0, 300.0, 3e-3, 0.0], [1.02 * K0, 800.0, -2e-3, 0.0],
                  [1.021 * K0, 50.0, 1e-3, 0.0], [0.99 * K0, 0.0, 4e-3, 0.0]])


# ------------------------------------------------------------------------------------------- 1. against the truth
@pytest.mark.parametrize("state", list(STATES))
def test_against_the_truth(hip, state):
    """All but 40 slots dead, so that every alive ray goes through mpmath (40 rays x 5 rows x 3 mirrors)."""
    rng = np.random.default_rng(23)
    dead = np.ones(N, bool)
    dead[rng.choice(N, 40, replace=False)] = False
    bundles, coats, D = _history(hip, dead), _coats(), _detector()
    last = bundles[-1]
    sd = _sdesc(D, last, 0.93 * K0, 0.02 * K0, 5)
    axis = np.array([0.01, -0.005, 1.0])
    axis /= np.linalg.norm(axis)
    P = STATES[state]
    E = _chromatic(bundles, coats, P, sd, TABLE, axis)
    assert E.shape == (2, 5, 3, 3, 65)
    want = vcc.field_of(bundles, D, sd.f, axis, TABLE, coats, P)
    err, a = np.abs(E - want).max(), _amp_sum(last)
    neutral = _chromatic(bundles, coats, P, sd, TABLE * [1.0, 0.0, 0.0, 0.0], axis)
    report(f"[vector chromatic, {state}] |F - truth| = {err:.2e} = {err / a:.1e} amplitude_sum; max |F| = "
           f"{np.abs(want).max() / a:.2e} amplitude_sum; the table moves F by {np.abs(E - neutral).max() / a:.2e}")
    assert np.abs(E - neutral).max() > 1e3 * 1e-9 * a     # (what c_j and z_j do is far above the bar that judges it)
    assert err <= 1e-9 * a * np.linalg.norm(P), err


# ------------------------------------------------------------------------------------------- 2. - 5. bytes
@pytest.fixture(scope="module")
def neutral(hist):
    """The neutral table's field for the circular state, computed once: (sd, table, bytes as an array)."""
    sd = _sdesc(hist["D"], hist["bundles"][-1], 0.94 * K0, 0.03 * K0, 5)
    table = _neutral(sd)
    return sd, table, _chromatic(hist["bundles"], hist["coats"], STATES["circular"], sd, table)


def test_neutral_table_gives_the_vector_spectrum_byte_for_byte(hist, neutral):
    sd, table, E = neutral
    want = _spectrum(hist["bundles"], hist["coats"], STATES["circular"], sd)
    assert E.shape == want.shape == (2, 5, 3, 3, 65) and np.abs(want).max() > 0
    assert E.tobytes() == want.tobytes()
    # ... for any axis (u is multiplied by 0), and twice
    tilted = _chromatic(hist["bundles"], hist["coats"], STATES["circular"], sd, table, np.array([0.6, 0.0, 0.8]))
    assert tilted.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def full(hist):
    """TABLE's field on the shared history, linear state, computed once."""
    sd = _sdesc(hist["D"], hist["bundles"][-1], 0.94 * K0, 0.03 * K0, 5)
    return sd, _chromatic(hist["bundles"], hist["coats"], STATES["linear"], sd, TABLE)


def test_a_comb_pays_for_its_lines_and_changes_nothing(hist, neutral, full):
    for (sd, E), table in ((neutral[::2], neutral[1]), (full, TABLE)):
        P = STATES["circular"] if table is neutral[1] else STATES["linear"]
        rows = [0, 2, 3]
        some = _chromatic(hist["bundles"], hist["coats"], P, sd, table[rows])
        assert some.shape == (2, 3, 3, 3, 65)
        assert some.tobytes() == np.ascontiguousarray(E[:, rows]).tobytes()
        back = _chromatic(hist["bundles"], hist["coats"], P, sd, table[rows[::-1]])
        assert back.tobytes() == np.ascontiguousarray(E[:, rows[::-1]]).tobytes()


def test_the_scratch_bound_does_not_change_the_bytes(hip, hist, full):
    from attosecondraytracing_amd import _abi
    sd, E = full
    last = hist["bundles"][-1]
    d = _abi.ArtFocalVectorChromaticDesc()
    d.v.s, d.v.n_elems, d.v.n, d.v.scratch_bound = sd, 4, N, 1
    d.axis[:] = list(AXIS)
    for e in range(4):
        d.v.coating[e] = -1
    count = lambda: hip.fn["art_focal_vector_chromatic_scratch_doubles"](C.byref(d))
    one = count()
    d.v.scratch_bound = 0
    whole = count()
    stride = (N + 63) // 64 * 64
    per_k = (whole - 6 * stride) // 5                       # six rows of prep (u is the sixth), then 5 wavenumbers
    assert one == 6 * stride + per_k and whole == 6 * stride + 5 * per_k and per_k > 6 * stride
    for nkb, bound in ((1, 8), (2, 8 * (6 * stride + 2 * per_k)), (5, 8 * whole)):
        d.v.scratch_bound = bound // 8
        assert count() == 6 * stride + nkb * per_k, nkb
        got = _chromatic(hist["bundles"], hist["coats"], STATES["linear"], sd, TABLE, scratch_bytes=bound)
        assert got.tobytes() == E.tobytes(), nkb


def test_dead_slots_contribute_nothing_whatever_they_hold(hip, hist, full):
    sd, E = full
    gone = hip.from_numpy(hist["dead"])
    poisoned = []
    for b in hist["bundles"]:
        c = b.copy()
        c.data[:7, :N][:, gone] = NAN
        if b.intensity is not None:
            c.intensity = b.intensity.clone()
            c.intensity[gone] = NAN
        c.touch()
        poisoned.append(c)
    got = _chromatic(poisoned, hist["coats"], STATES["linear"], sd, TABLE)
    assert np.isfinite(got).all() and got.tobytes() == E.tobytes()


# ------------------------------------------------------------------------------------------- 6. edges
def test_no_weights_are_weights_of_one(hip, hist, full):
    import torch
    sd, _ = full
    bundles = list(hist["bundles"])
    ones, none = bundles[-1].alias(), bundles[-1].alias()
    ones.intensity = torch.ones(N, dtype=torch.float64, device=hip.device)
    none.intensity = None
    ones.touch(); none.touch()
    a = _chromatic(bundles[:-1] + [ones], hist["coats"], STATES["linear"], sd, TABLE)
    b = _chromatic(bundles[:-1] + [none], hist["coats"], STATES["linear"], sd, TABLE)
    assert np.abs(a).max() > 0 and a.tobytes() == b.tobytes()


def test_no_slots_give_zeros_and_an_all_mask_chain_runs(hip, hist, full):
    sd, _ = full
    empty = [b.slots(0, 0) for b in hist["bundles"]]
    E = _chromatic(empty, hist["coats"], STATES["linear"], sd, TABLE)
    assert E.shape == (2, 5, 3, 3, 65) and not E.any()
    # every coating index -1: E_r is the input state's transverse part (0, 1, 0) - d_y d over its norm for the source
    # direction d, so E_r . y = sqrt(1 - d_y^2), and the field's y component is art_focal_chromatic's scalar sum to
    # sum_r sqrt(w_r) (1 - sqrt(1 - d_y^2)) at the most (the apodisation is <= 1), plus the two sums' rounding
    masks = _chromatic(hist["bundles"], [None] * 4, STATES["linear"], sd, TABLE)
    assert np.isfinite(masks).all()
    from attosecondraytracing_amd import _abi
    cd = _abi.ArtFocalChromaticDesc()
    cd.f = sd.f
    cd.axis[:] = list(AXIS)
    last, src = hist["bundles"][-1], hist["bundles"][0]
    scalar = hip.focal_chromatic(cd, last.view(), src.view(), last.intensity, N, TABLE).cpu().numpy()
    d = hist["D"]._desc()
    U = np.stack([np.array(d.rot[0:3]), np.array(d.rot[3:6]), np.array(d.normal[:])])
    Fy = np.einsum("qjclx,c->qjlx", masks, U[:, 1])
    alive = ~hist["dead"]
    dy = src.data[4, :N].cpu().numpy()[alive]
    w = last.intensity[:N].cpu().numpy()[alive]
    bound = (np.sqrt(w) * (1 - np.sqrt(1 - dy * dy))).sum() + 1e-12 * _amp_sum(last)
    assert np.abs(scalar).max() > 2 * bound and np.abs(Fy - scalar).max() <= bound


def _set(d, table, key, v):
    if key in ("nk", "dk"):
        setattr(d.v.s, key, v)
    elif key in ("k", "nx", "planes", "dx"):
        setattr(d.v.s.f, key, v)
    elif key == "axis":
        d.axis[:] = list(v)
    elif key in ("k_j", "c_j", "z_j"):
        table[2, "kcz".index(key[0])] = v
    elif key == "coating0":
        d.v.coating[0] = v
    elif key == "pol0":
        d.v.pol[0] = v
    else:
        setattr(d.v, key, v)


BAD = [
    # art_focal_vector_spectrum's
    (dict(nk=0), -1, "nk must"), (dict(nk=1025), -1, "nk must"), (dict(dk=NAN), -1, "dk must"),
    (dict(dk=-2500.0), -1, "every k_j"), (dict(planes=64, nk=400), -1, "planes * nk * 3"), (dict(k=0.0), -1, "k must"),
    (dict(nx=0), -1, "nx and ny"), (dict(planes=65), -1, "planes"), (dict(dx=NAN), -1, "pitch"),
    (dict(n=-1), -1, "negative ray count"), (dict(n=(1 << 28) + 1), -2, "2^28"), (dict(n_elems=0), -1, "elements"),
    (dict(n_elems=65), -1, "elements"), (dict(coating0=1), -1, "coating index"), (dict(coating0=-2), -1, "coating index"),
    (dict(pol0=INF), -1, "input state"), (dict(scratch_bound=-1), -1, "scratch_bound"), (dict(views=None), -1, "views is NULL"),
    (dict(materials=None), -1, "table is NULL"), (dict(coatings_dev=None), -1, "table is NULL"),
    (dict(bad_material=(NAN, 0.0)), -1, "per-wavenumber table"), (dict(bad_material=(0.9, -1e-3)), -1, "per-wavenumber table"),
    (dict(bad_layers=257), -1, "layers"), (dict(field=None), -1, "must not be NULL"), (dict(scratch=None), -1, "must not be NULL"),
    # art_focal_chromatic's on the table and the axis
    (dict(axis=(0.6, 0.0, 0.8 + 1e-9)), -1, "unit vector"), (dict(axis=(0.0, 0.0, 0.0)), -1, "unit vector"),
    (dict(axis=(NAN, 0.0, 1.0)), -1, "unit vector"), (dict(axis=(INF, 0.0, 0.0)), -1, "unit vector"),
    (dict(k_j=0.0), -1, "every k_j"), (dict(k_j=-1.0), -1, "every k_j"), (dict(k_j=NAN), -1, "every k_j"),
    (dict(k_j=INF), -1, "every k_j"), (dict(c_j=-1e-300), -1, "every c_j"), (dict(c_j=NAN), -1, "every c_j"),
    (dict(c_j=INF), -1, "every c_j"), (dict(z_j=NAN), -1, "every z_j"), (dict(z_j=INF), -1, "every z_j"),
    (dict(z_j=-INF), -1, "every z_j"), (dict(table_host=None), -1, "host copy"), (dict(table_dev=None), -1, "device table"),
    (dict(source=None), -1, "source bundle"), (dict(desc=None), -1, "descriptor is NULL")]


@pytest.fixture(scope="module")
def small(hip):
    """256 slots, one coated element: the valid call that every bad argument spoils."""
    import torch
    from attosecondraytracing_amd.bundle import RayBundle
    rng = np.random.default_rng(4)
    n = 256
    d0 = AXIS[None, :] + rng.normal(0, 0.02, (n, 3))
    d0 /= np.linalg.norm(d0, axis=1)[:, None]
    d1 = np.array([0.05, -0.02, 1.0])[None, :] + rng.normal(0, 0.03, (n, 3))
    d1 /= np.linalg.norm(d1, axis=1)[:, None]
    src = RayBundle.from_arrays(np.zeros((n, 3)), d0, wavelength=WL, backend=hip)
    last = RayBundle.from_arrays(-5.0 * d1, d1, intensity=np.ones(n), wavelength=WL, backend=hip)
    return {"bundles": [src, last], "coat": cc.mosi(4), "field": torch.empty(2 * 4 * 3 * 8 * 8 * 2, dtype=torch.float64,
                                                                             device=hip.device),
            "scratch": torch.zeros(1 << 20, dtype=torch.float64, device=hip.device)}


@pytest.mark.parametrize("over, code, msg", BAD)
def test_invalid_arguments_launch_nothing(hip, small, over, code, msg):
    import torch
    from attosecondraytracing_amd import _abi
    bundles, coat = small["bundles"], small["coat"]
    last = bundles[-1]
    sd = _sdesc(_detector(), last, 6000.0, 100.0, 4, Size=0.01, Pixels=8, Shifts=(0.0, 0.1))
    d = _abi.ArtFocalVectorChromaticDesc()
    d.v.s, d.v.n_elems, d.v.n = sd, 1, last.n_slots
    d.v.pol[:] = [0, 0, 1, 0, 0, 0]
    d.v.w = last.intensity.data_ptr()
    d.axis[:] = list(AXIS)
    views = (_abi.ArtBundleView * 2)(*[b.view() for b in bundles])
    table = np.ascontiguousarray(np.stack([6000.0 + 100.0 * np.arange(4), [0, 5, 9, 2], [0, 1e-3, -1e-3, 0], [0] * 4], axis=1))
    mats = np.stack([coat.material_table(np.full(4, WL))], axis=1)
    over = dict(over)
    if "bad_material" in over:
        mats[2, 0, 1] = over.pop("bad_material")
    struct = coat._struct()
    if "bad_layers" in over:
        struct.n_layers = over.pop("bad_layers")
    cdev, carr, marr = hip.focal_vector_tables(d.v, views, [struct], mats)
    use_field, use_scratch = over.pop("field", True), over.pop("scratch", True)
    use_host, use_dev, use_src = over.pop("table_host", True), over.pop("table_dev", True), over.pop("source", True)
    use_desc = over.pop("desc", True)
    if "coatings_dev" in over:
        cdev = over.pop("coatings_dev")
    for key, v in over.items():
        _set(d, table, key, v)
    table_dev = hip.from_numpy(table)
    field, scratch = small["field"], small["scratch"]
    field.fill_(7.25)
    no_src = _abi.ArtBundleView()
    rc = hip.fn["art_focal_vector_chromatic"](
        C.byref(d) if use_desc else None, C.byref(views[1]), C.byref(views[0] if use_src else no_src), cdev, carr, marr,
        table_dev.data_ptr() if use_dev else None, table.ctypes.data_as(_abi.c_double_p) if use_host else None,
        scratch.data_ptr() if use_scratch else None, field.data_ptr() if use_field else None, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == code and msg in hip.last_error(), (rc, hip.last_error())
    assert bool((field == 7.25).all())


def test_the_valid_small_call_runs_and_the_scratch_count_refuses_a_bad_descriptor(hip, small):
    """The call that test_invalid_arguments_launch_nothing spoils is itself accepted; the scratch function returns the
    negative code of a bad descriptor."""
    from attosecondraytracing_amd import _abi
    bundles, coat = small["bundles"], small["coat"]
    sd = _sdesc(_detector(), bundles[-1], 6000.0, 100.0, 4, Size=0.01, Pixels=8, Shifts=(0.0, 0.1))
    table = np.stack([6000.0 + 100.0 * np.arange(4), [0, 5, 9, 2], [0, 1e-3, -1e-3, 0], [0] * 4], axis=1)
    E = _chromatic(bundles, [coat], (0, 1, 0), sd, table)
    assert E.shape == (2, 4, 3, 8, 8) and np.isfinite(E).all() and np.abs(E).max() > 0
    d = _abi.ArtFocalVectorChromaticDesc()
    d.v.s, d.v.n_elems, d.v.n = sd, 1, 256
    d.axis[:] = list(AXIS)
    d.v.coating[0] = -1
    fn = hip.fn["art_focal_vector_chromatic_scratch_doubles"]
    assert fn(C.byref(d)) > 0
    assert fn(None) == -1 and "descriptor is NULL" in hip.last_error()
    for key, v, code in (("nk", 0, -1), ("n_elems", 0, -1), ("n", -1, -1), ("n", (1 << 28) + 1, -2), ("scratch_bound", -1, -1)):
        bad = _abi.ArtFocalVectorChromaticDesc.from_buffer_copy(d)
        _set(bad, None, key, v)
        assert fn(C.byref(bad)) == code, key


# ------------------------------------------------------------------------------------------- 7. the API
def _toroid_pair(n):
    """A mask that stops the outer rays, then two toroids (tests/test_gpu_vector_pulse.py's relay, halved)."""
    import ART.ModuleDetector as mdet
    import ART.ModuleMask as mmask
    import ART.ModuleMirror as mmirror
    import ART.ModuleProcessing as mp
    import ART.ModuleSupport as msupp
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 6.0, 0, 0))
    SP = {"Divergence": 0.02, "SourceSize": 0, "Wavelength": WL, "DeltaFT": 0.5, "NumberRays": n}
    chain = mp.OEPlacement(SP, [Mask, Tor, Tor], [400, 200, 1200], [0, 80, -80], [0] * 3, "masked toroid pair")
    last = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    return chain, D


@pytest.fixture(scope="module")
def api(hip):
    chain, D = _toroid_pair(3001)
    alive = chain.get_output_rays()[-1].alive.cpu().numpy().astype(bool)
    assert 0.2 * len(alive) < alive.sum() < 0.9 * len(alive)            # the mask stops some rays
    coat = vt.dispersive_copy(cc.mosi(40), WL, 6e-6, 40e-6)
    kw = dict(Pixels=(65, 3), Shifts=(0.0, 0.3), TimeWindow=4.0, Times=32)
    return {"chain": chain, "D": D, "coat": coat, "kw": kw, "P": STATES["circular"],
            "pulse": chain.get_FocalPulse(coat, D, 0.3, STATES["circular"], **kw)}


def test_api_neutral_source_gives_get_FocalPulse_byte_for_byte(api):
    chain, D, coat, kw, P, f = (api[k] for k in ("chain", "D", "coat", "kw", "P", "pulse"))
    p = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, **kw)
    assert p.spectrum.shape == f.spectrum.shape and p.spectrum.shape[2:] == (3, 3, 65) and len(p.omega) >= 3
    assert p.spectrum.cpu().numpy().tobytes() == f.spectrum.cpu().numpy().tobytes()
    assert p.envelope.cpu().numpy().tobytes() == f.envelope.cpu().numpy().tobytes()
    assert p.amplitude_sum == f.amplitude_sum and np.array_equal(p.strehl, f.strehl)
    assert np.isinf(p.divergence).all() and not p.position.any() and p.best_focus.shape == p.omega.shape
    small = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, ScratchBytes=8, Position=0.0, **kw)
    assert small.spectrum.cpu().numpy().tobytes() == f.spectrum.cpu().numpy().tobytes()


def test_api_comb_keeps_its_lines_byte_for_byte_and_zeros_elsewhere(api):
    from attosecondraytracing_amd import chromatic
    chain, D, coat, kw, P = (api[k] for k in ("chain", "D", "coat", "kw", "P"))
    # harmonics 14 - 16 of 15 x 13.5 nm (9.3 rad/fs apart), lines of 4 fs: exactly 0 beyond 2.1 rad/fs of a line, on a
    # grid of pi / 2 rad/fs
    comb = chromatic.harmonic_comb(15 * WL, [14, 15, 16], 4.0)
    whole = chain.get_FocalPulse(coat, D, 0.3, P, Spectrum=comb, **kw)
    p = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, Spectrum=comb, **kw)
    keep = np.abs(p.weights) > 0
    assert np.array_equal(p.omega, whole.omega) and np.array_equal(p.weights, whole.weights)
    assert 3 <= keep.sum() < len(keep) - 3
    got, want = p.spectrum.cpu().numpy(), whole.spectrum.cpu().numpy()
    assert got[:, keep].tobytes() == want[:, keep].tobytes()
    assert not got[:, ~keep].any() and np.abs(got[:, keep]).min(axis=(0, 2, 3, 4)).max() > 0
    assert np.isnan(p.best_focus[~keep]).all() and np.isin(p.best_focus[keep], [0.0, 0.3]).all()
    assert np.abs(p.envelope.cpu().numpy() - whole.envelope.cpu().numpy()).max() <= 1e-12 * p.amplitude_sum


def test_api_with_a_real_source_agrees_with_the_entry_point(api):
    import torch
    from attosecondraytracing_amd import _abi, chromatic, focal, polarisation, vector_pulse
    chain, D, coat, kw, P = (api[k] for k in ("chain", "D", "coat", "kw", "P"))
    theta = lambda w: 0.015 + 1e-4 * (w - w.min())
    pos = lambda w: 0.5 - 0.01 * (w - w.min())
    p = chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, Polarisation=P, Divergence=theta, Position=pos, **kw)
    assert isinstance(p, chromatic.ChromaticVectorFocalPulse)
    bundles = polarisation.history(chain)
    last = bundles[-1]
    dw = 2 * math.pi / p.time_window
    k = p.omega[0] / chromatic.C_MM_PER_FS + np.arange(len(p.omega)) * (dw / chromatic.C_MM_PER_FS)
    table = np.stack([k, 2.0 / theta(p.omega) ** 2, pos(p.omega), 0 * k], axis=1)
    fd, _, _, _, _, _, _ = focal.focal_desc(D, last, None, kw["Pixels"], None, kw["Shifts"], None, None)
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.f.k, sd.dk, sd.nk = k[0], dw / chromatic.C_MM_PER_FS, len(k)
    direct = vector_pulse._vector_spectrum(bundles, [None, coat, coat], np.asarray(P, dtype=complex), sd, 2 * np.pi / k, None,
                                           chromatic=(p.axis, table))
    want = (direct * torch.as_tensor(p.weights, device=direct.device)[None, :, None, None, None]).cpu().numpy()
    a = focal.amplitude_sum(last)
    err = np.abs(p.spectrum.cpu().numpy() - want).max()
    report(f"[vector chromatic, API vs entry point] {err / a:.1e} amplitude_sum; amplitude_sum {p.amplitude_sum / a:.3f} of "
           f"the plain sum; strehl {p.strehl}")
    assert err <= 1e-12 * a, err
    assert 0 < p.amplitude_sum < a and np.all((p.strehl > 0) & (p.strehl < 1))
    neutral = api["pulse"].spectrum.cpu().numpy()
    assert np.abs(p.spectrum.cpu().numpy() - neutral).max() > 1e3 * 1e-12 * a     # (the source does something)
    with pytest.raises(ValueError, match="polarised"):
        chain.get_ChromaticFocalPulse(D, 0.3, Coatings=coat, **kw)
    with pytest.raises(TypeError, match="needs Coatings"):
        chain.get_ChromaticFocalPulse(D, 0.3, Polarisation=P, **kw)

"""GPU (-m gpu): art_focal_image and the API on top of it (Detector.get_FocalImage, OpticalChain.get_FocalImage,
SourceImage) against the NumPy sum over groups of tests/image_common.py, the sum of get_FocalField intensities over the
groups, the coherent and the incoherent limit, and the Rayleigh criterion of two mutually incoherent ideal foci.

The error bar on the intensity is 2e-9 * ideal_peak throughout: tests/test_gpu_focal.py holds a group's field E_g to
1e-9 * A_g (A_g the group's sum of amplitudes, |E_g| <= A_g), so | |E_g + d|^2 - |E_g|^2 | <= 2 A_g * 1e-9 A_g to first
order, and the sum over the groups is 2e-9 * sum_g A_g^2 = 2e-9 * ideal_peak."""
import ctypes as C

import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import focal_common as fc
import image_common as ic

pytestmark = pytest.mark.gpu

BAR = 2e-9
SIZES = [1, 31, 32, 33, 64, 500, 2339]       # group edges off, on and just past the 32-ray chunk; 3000 slots in all
DEAD_GROUP = 3                               # every slot of the 33-ray group is dead


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


@pytest.fixture(scope="module")
def grouped(hip):
    """3000 slots, 30 % dead, weights; the groups SIZES with one of them all dead and one gap in the ids."""
    B = _random_bundle(hip, 3000, 1)
    seg = ic.seg_of_sizes(SIZES)
    B.alive[int(seg[DEAD_GROUP]):int(seg[DEAD_GROUP + 1])] = 0
    B.touch()
    return {"B": B, "seg": seg, "ids": ic.ids_of_sizes(SIZES, first=2, gap_after=4), "D": _detector()}


def _check_oracle(B, D, f, seg):
    I = ic.image_of(B, D, f, seg)
    _, _, _, alive, w = fc.bundle_arrays(B)
    ideal = ic.ideal_peak(alive, w, seg)
    assert f.ideal_peak == pytest.approx(ideal, rel=1e-12)
    err = np.abs(f.intensity.cpu().numpy() - I).max()
    print("max |image - oracle| / ideal_peak = %.3e" % (err / ideal))
    assert err <= BAR * ideal, (err, ideal)


def test_groups_against_the_oracle(grouped):
    B, D, seg, ids = grouped["B"], grouped["D"], grouped["seg"], grouped["ids"]
    f = D.get_FocalImage(B, Groups=ids, Size=(0.05, 0.03), Pixels=(37, 23), Shifts=(0.0, -0.1, 0.25))
    assert f.intensity.shape == (3, 23, 37) and f.intensity.is_cuda and f.groups == len(SIZES)
    _check_oracle(B, D, f, seg)
    assert np.all(f.strehl <= 1.0)
    # several tiles with ragged edges, one plane
    f2 = D.get_FocalImage(B, Groups=ids, Size=(0.08, 0.05), Pixels=(130, 70))
    _check_oracle(B, D, f2, seg)


@pytest.mark.parametrize("n, per, pixels", [
    (100, 33, (37, 23)),        # one workgroup per tile and plane walks every group and writes the image itself
    (3000, 100, (37, 23)),      # slices of the groups, folded in slice order; groups of 3 chunks and a part
    (3000, 100, (70, 66)),      # the same over four ragged tiles
    (3000, 1500, (37, 23)),     # two large groups: every group cut into pieces, complex partials per group
    (257, 257, (9, 5))])        # one group of 9 chunks, the last of one ray: three pieces
def test_every_launch_shape_against_the_oracle(hip, n, per, pixels):
    B = _random_bundle(hip, n, 11 + n + per)
    D = _detector()
    f = D.get_FocalImage(B, RaysPerSource=per, Size=(0.05, 0.03), Pixels=pixels, Shifts=(0.0, 0.2))
    seg = np.minimum(np.arange(f.groups + 1) * per, n)
    assert f.groups == -(-n // per)
    _check_oracle(B, D, f, seg)


def test_image_is_the_sum_of_the_groups_focal_field_intensities(grouped):
    B, D, seg, ids = grouped["B"], grouped["D"], grouped["seg"], grouped["ids"]
    kw = dict(Size=(0.05, 0.03), Pixels=(37, 23), Centre=(0.001, -0.002), RefPath=1e-4, Shifts=(0.0, 0.15))
    f = D.get_FocalImage(B, Groups=ids, **kw)
    total = np.zeros(f.intensity.shape)
    for g in range(len(SIZES)):
        total += D.get_FocalField(B.slots(seg[g], seg[g + 1]), **kw).intensity
    assert np.abs(f.intensity.cpu().numpy() - total).max() <= BAR * f.ideal_peak


def test_one_group_is_the_coherent_field(grouped):
    B, D = grouped["B"], grouped["D"]
    kw = dict(Size=(0.05, 0.03), Pixels=(37, 23), Centre=(0.0, 0.0), RefPath=0.0, Shifts=(0.0, 0.15))
    f = D.get_FocalImage(B, Groups=np.zeros(B.n_slots, dtype=np.int64), **kw)
    e = D.get_FocalField(B, **kw)
    assert f.groups == 1 and f.ideal_peak == pytest.approx(e.amplitude_sum ** 2, rel=1e-12)
    assert np.abs(f.intensity.cpu().numpy() - e.intensity).max() <= BAR * f.ideal_peak
    assert f.strehl == pytest.approx(e.strehl, rel=1e-8) and np.array_equal(f.peak, e.peak)


def test_every_slot_its_own_group_gives_the_power_everywhere(hip):
    B = _random_bundle(hip, 500, 6)
    f = _detector().get_FocalImage(B, RaysPerSource=1, Size=(0.05, 0.03), Pixels=(37, 23), Centre=(0.0, 0.0),
                                   Shifts=(0.0, 0.2))
    _, _, _, alive, w = fc.bundle_arrays(B)
    power = w[alive].sum()
    assert f.groups == 500 and f.power == pytest.approx(power, rel=1e-14) and f.ideal_peak == pytest.approx(power, rel=1e-13)
    assert np.abs(f.intensity.cpu().numpy() / power - 1.0).max() <= 1e-12
    assert np.abs(f.strehl - 1.0).max() <= 1e-12


def test_two_incoherent_foci_at_the_rayleigh_distance_show_the_dip(hip):
    from attosecondraytracing_amd.bundle import RayBundle
    NA, lam, n = 0.05, 1e-3, 60000
    sep = 0.305 * lam / NA
    parts = [fc.bundle_arrays(fc.converging_bundle(n, NA, 10.0, focus=(s * sep, 0.0, 0.0), wavelength=lam, backend=hip))
             for s in (-1, 1)]
    B = RayBundle.from_arrays(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                              wavelength=lam, backend=hip)
    D = _detector()
    kw = dict(Size=(3 * lam / NA, 1e-4), Pixels=(601, 3), Centre=(0.0, 0.0), RefPath=10.0)
    f = D.get_FocalImage(B, RaysPerSource=n, **kw)
    assert f.groups == 2 and f.ideal_peak == 2.0 * n * n
    row = f.intensity.cpu().numpy()[0, 1]
    want = 2 * fc.airy(np.array([2 * np.pi / lam * NA * sep]))[0]          # 0.73459: the Rayleigh dip
    print("I(0) / max I = %.6f, 2 airy = %.6f" % (row[300] / row.max(), want))
    assert f.x[300] == pytest.approx(0.0, abs=1e-15)
    assert abs(row[300] / row.max() - want) <= 2e-3
    assert abs(want - 0.73459) <= 1e-4
    assert abs(abs(f.peak[0, 0]) - sep) <= f.x[1] - f.x[0] and row.argmax() != 300
    # summed coherently, the same rays have their maximum between the foci: no dip
    e = D.get_FocalField(B, **kw)
    assert e.intensity[0, 1].argmax() == 300 and e.intensity[0, 1, 300] == pytest.approx(1.469 * n * n, rel=2e-3)


def test_extended_source_through_a_chain(hip):
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    feff = 100.0
    SP = {"Divergence": 0.02, "SourceSize": 0.05, "Wavelength": 800e-6, "DeltaFT": 1, "NumberRays": 9000}
    par = mmirror.MirrorParabolic(feff, 30.0, msupp.SupportRound(3 * 0.1 * feff))
    chain = mp.OEPlacement(SP, [par], [2 * feff], [0])
    assert chain.source_rays.rays_per_source == 300 and chain.source_rays.n_slots == 9000
    out = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(out, 2 * feff)
    f = chain.get_FocalImage(D, Pixels=33)
    g = D.get_FocalImage(out, RaysPerSource=300, Pixels=33)
    assert f.groups == 30 and f.intensity.cpu().numpy().tobytes() == g.intensity.cpu().numpy().tobytes()
    kw = dict(Size=(f.x[-1] - f.x[0], f.y[-1] - f.y[0]), Pixels=33, Centre=(0.5 * (f.x[0] + f.x[-1]), 0.5 * (f.y[0] + f.y[-1])),
              RefPath=f.ref_path)
    total = np.zeros(f.intensity.shape)
    for s in range(30):
        total += D.get_FocalField(out.slots(300 * s, 300 * (s + 1)), **kw).intensity
    assert np.abs(f.intensity.cpu().numpy() - total).max() <= BAR * f.ideal_peak
    assert np.all(f.strehl <= 1.0) and f.power > 0 and np.all(f.rms > 0)


@pytest.mark.parametrize("per", [100, 1500])          # slices of groups; pieces of groups
def test_two_calls_give_identical_bytes(hip, per):
    B = _random_bundle(hip, 3000, 8)
    D = _detector()
    kw = dict(RaysPerSource=per, Size=(0.05, 0.03), Pixels=(70, 66), Centre=(0.0, 0.0), Shifts=(0.0, 0.3))
    a, b = D.get_FocalImage(B, **kw), D.get_FocalImage(B, **kw)
    assert a.intensity.cpu().numpy().tobytes() == b.intensity.cpu().numpy().tobytes()


def test_planes_agree_with_a_moved_detector(hip):
    B = fc.converging_bundle(2000, 0.05, 0.05, wavelength=1e-3, backend=hip, weights=np.linspace(0.5, 1.0, 2000))
    D = _detector()
    kw = dict(RaysPerSource=500, Size=(0.04, 0.03), Pixels=(29, 21), Centre=(0.0, 0.0), RefPath=0.05)
    for s in (-0.03125, 0.046875):
        f = D.get_FocalImage(B, Shifts=(s,), **kw)
        Dq = D.copy_detector()
        Dq.shiftByDistance(s)
        g = Dq.get_FocalImage(B, **kw)
        err = np.abs(g.intensity.cpu().numpy()[0] - f.intensity.cpu().numpy()[0]).max()
        assert err <= 1e-12 * f.ideal_peak, (s, err)


def _desc(D, seg, groups, **over):
    from attosecondraytracing_amd import _abi
    d = _abi.ArtFocalImageDesc()
    f = d.f
    f.det = D._desc()
    f.k, f.L_ref, f.x0, f.dx, f.y0, f.dy, f.nx, f.ny, f.planes = 2 * np.pi / 1e-3, 0.0, -0.01, 1e-3, -0.01, 1e-3, 8, 8, 2
    f.shift[1] = 0.1
    for key, v in over.items():
        setattr(f, key, v)
    d.groups = groups
    d.seg = None if seg is None else seg.data_ptr()
    return d


def test_empty_and_all_dead_bundles(hip):
    import torch
    from attosecondraytracing_amd.image import FocalImage
    D = _detector()
    dead = _random_bundle(hip, 500, 4, dead=0.0)
    dead.alive[:] = 0
    dead.touch()
    f = D.get_FocalImage(dead, RaysPerSource=100, Size=0.01, Pixels=(9, 5), Centre=(0.0, 0.0), Shifts=(0.0, 0.1))
    assert f.intensity.shape == (2, 5, 9) and not f.intensity.cpu().numpy().any()
    assert np.isnan(f.strehl).all() and f.ideal_peak == 0.0 and f.power == 0.0
    # n = 0: the call writes zeros over whatever the image held
    seg = torch.zeros(2, dtype=torch.int64, device=hip.device)
    img = hip.focal_image(_desc(D, seg, 1).f, seg, 1, dead.view(), None, 0)
    assert img.shape == (2, 8, 8) and not img.cpu().numpy().any()
    e = FocalImage(img, np.arange(8.0), np.arange(8.0), (0.0, 0.0), 1e-3, 0.0, 0, 0.0, 0.0)
    assert np.isnan(e.strehl).all() and e.ideal_peak == 0.0


@pytest.mark.parametrize("over, msg", [
    (dict(groups=0), "groups"), (dict(groups=(1 << 20) + 1), "groups"), (dict(seg=None), "seg must not be NULL"),
    (dict(image=None), "image must not be NULL"), (dict(scratch=None), "scratch must not be NULL"),
    (dict(nx=2049), "nx and ny"), (dict(planes=65), "planes"), (dict(k=float("nan")), "k must")])
def test_invalid_descriptors_launch_nothing(hip, over, msg):
    import torch
    B = _random_bundle(hip, 256, 5)
    D = _detector()
    over = dict(over)
    seg = torch.tensor([0, 100, 256], dtype=torch.int64, device=hip.device)
    use_image, use_scratch = over.pop("image", True), over.pop("scratch", True)
    d = _desc(D, over.pop("seg", seg), over.pop("groups", 2), **over)
    image = torch.full((2 * 8 * 8,), 7.25, dtype=torch.float64, device=hip.device)
    scratch = torch.zeros(1 << 20, dtype=torch.float64, device=hip.device)
    rc = hip.fn["art_focal_image"](C.byref(d), C.byref(B.view()), B.intensity.data_ptr(), B.n_slots,
                                   scratch.data_ptr() if use_scratch else None, image.data_ptr() if use_image else None,
                                   hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and msg in hip.last_error(), (rc, hip.last_error())
    assert bool((image == 7.25).all())
    for bad in ((0, 8, 1, 2, 10), (8, 8, 65, 2, 10), (8, 8, 1, 0, 10), (8, 8, 1, (1 << 20) + 1, 10), (8, 8, 1, 2, -1)):
        assert hip.fn["art_focal_image_scratch_doubles"](*bad) == -1


def test_offsets_are_clamped_to_the_bundle(hip):
    """The contract of seg: offsets below 0 and above n are clamped to [0, n], a decreasing pair is an empty group.  The
    call returns 0 and gives the oracle's image of the clamped groups."""
    import torch
    B = _random_bundle(hip, 256, 5)
    D = _detector()
    raw = [-7, 100, 50, 300, 1 << 40]          # groups: [0, 100), empty, [50, 256), empty
    assert ic.clamped_ranges(raw, 256) == [(0, 100), (50, 256)]
    seg = torch.tensor(raw, dtype=torch.int64, device=hip.device)
    d = _desc(D, seg, 4)
    img = hip.focal_image(d.f, seg, 4, B.view(), B.intensity, B.n_slots)
    P, V, L, alive, w = fc.bundle_arrays(B)
    f = d.f
    I = ic.image(P, V, L, alive, w, raw, f.k, f.L_ref, np.array(f.det.centre[:]), np.array(f.det.normal[:]),
                 np.array(f.det.rot[:]), f.x0 + np.arange(8) * f.dx, f.y0 + np.arange(8) * f.dy, [0.0, 0.1])
    assert np.abs(img.cpu().numpy() - I).max() <= BAR * ic.ideal_peak(alive, w, raw)


def test_source_image_draws(hip):
    from attosecondraytracing_amd import ModuleAnalysisAndPlots as mpl
    B = fc.converging_bundle(3000, 0.05, 10.0, wavelength=1e-3, backend=hip)
    D = _detector()
    fig = mpl.SourceImage(B, D, RaysPerSource=1000, Pixels=33, Log=True)
    g, e = fig._art_image, fig._art_focal
    assert g.intensity.shape == (1, 33, 33) and g.groups == 3 and e.field.shape == (1, 33, 33)
    assert np.allclose(g.x, e.x, rtol=0, atol=1e-12) and len(fig.axes) == 4
    import matplotlib.pyplot as plt
    plt.close("all")

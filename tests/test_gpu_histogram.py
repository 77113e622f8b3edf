"""GPU (-m gpu): art_histogram and the API on top of it (Detector.get_Histogram, OpticalChain.get_Footprint, SpotImage,
DelayProfile, MirrorFootprint).  Counts and fixed-point weight sums are compared EXACTLY with numpy.histogramdd /
numpy.histogram on the values the package already returns (get_PointList2D, get_Delays) and with the same integers
formed on the host."""
import ctypes as C
import types

import matplotlib
matplotlib.use("Agg")
import numpy as np
import pytest

import test_plots as tp

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
def golden(hip):
    return tp.build_plot_scene()


@pytest.fixture(scope="module")
def relay4(hip):
    """relay4 traced with 1e6 rays, Gaussian weights on the final bundle, a detector placed 600 mm downstream."""
    import torch
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=10 ** 6)
    last = chain.get_output_rays()[-1]
    n = last.n_slots
    g = torch.Generator(device="cpu").manual_seed(5)
    last.intensity = torch.exp(-0.5 * torch.randn(n, generator=g, dtype=torch.float64) ** 2).to(hip.device)
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    return {"chain": chain, "last": last, "D": D}


def host_flat(sample, edges):
    """numpy.histogramdd's bin of every row of `sample` (row-major flat index), -1 outside or NaN."""
    flat = np.zeros(len(sample), dtype=np.int64)
    ok = np.ones(len(sample), dtype=bool)
    for k, e in enumerate(edges):
        v = sample[:, k]
        j = np.searchsorted(e, v, side="right") - 1
        j[v == e[-1]] = len(e) - 2
        ok &= (j >= 0) & (j < len(e) - 1) & ~np.isnan(v)
        flat = flat * (len(e) - 1) + np.clip(j, 0, len(e) - 2)
    return np.where(ok, flat, -1)


def host_integers(sample, w, edges, shift):
    """(counts, wsums, totals4) formed on the host from q = rint(ldexp(w, shift))."""
    nb = [len(e) - 1 for e in edges]
    flat = host_flat(sample, edges)
    q = np.rint(np.ldexp(w, shift)).astype(np.int64)
    counts = np.zeros(int(np.prod(nb)), dtype=np.int64)
    wsums = np.zeros_like(counts)
    inside = flat >= 0
    np.add.at(counts, flat[inside], 1)
    np.add.at(wsums, flat[inside], q[inside])
    totals = np.array([inside.sum(), (~inside).sum(), q[inside].sum(), q[~inside].sum()], dtype=np.int64)
    return counts.reshape(nb), wsums.reshape(nb), totals


def frame_desc(ndim, bins, lo, hi, M=np.eye(3), T=np.zeros(3)):
    from attosecondraytracing_amd import _abi
    d = _abi.ArtHistogramDesc()
    d.source, d.ndim = _abi.ART_HIST_FRAME, ndim
    for k in range(ndim):
        d.axis[k], d.bins[k], d.lo[k], d.hi[k] = k, bins[k], lo[k], hi[k]
    d.map.rot[:] = [float(v) for v in np.asarray(M, dtype=float).reshape(9)]
    d.map.centre[:] = [float(v) for v in T]
    return d


def run(be, desc, B, n=None, out=None, shift=None):
    n = B.n_slots if n is None else n
    c, ws, t, S = be.histogram(desc, B.view(), B.intensity, n, out=out, shift=shift)
    return c.cpu().numpy(), None if ws is None else ws.cpu().numpy(), t.cpu().numpy(), S


def test_gpu_histogram_bin_rule_on_hand_built_values(hip):
    """FRAME source with M = I, T = 0: the coordinates are the points bit for bit.  Values on interior edges, on lo and
    hi, one ulp outside, NaN, dead slots; 1-D, 2-D and 3-D against numpy.histogramdd."""
    import torch
    from attosecondraytracing_amd.bundle import RayBundle
    rng = np.random.default_rng(3)
    lo, hi, nb = [-1.0, 0.0, 2.0], [1.0, 3.0, 2.5], [4, 3, 5]
    specials = []
    for k in range(3):
        e = np.linspace(lo[k], hi[k], nb[k] + 1)
        specials.append(np.concatenate([e, [np.nextafter(lo[k], -np.inf), np.nextafter(hi[k], np.inf),
                                            np.nextafter(e[1], -np.inf), np.nextafter(e[1], np.inf)],
                                        rng.uniform(lo[k] - 0.2, hi[k] + 0.2, 8)]))
    n = 3000
    P = np.stack([rng.choice(specials[k], n) for k in range(3)], axis=1)
    P[::97] = np.nan                 # NaN in every component: a NaN reaches every coordinate through M (P - T)
    w = rng.uniform(0.1, 2.0, n)
    B = RayBundle.from_arrays(P, np.tile([0.0, 0.0, 1.0], (n, 1)), intensity=w, backend=hip)
    dead = rng.random(n) < 0.2
    B.alive[torch.as_tensor(dead, device=hip.device)] = 0
    live = ~dead
    for ndim in (1, 2, 3):
        edges = [np.linspace(lo[k], hi[k], nb[k] + 1) for k in range(ndim)]
        c, ws, t, S = run(hip, frame_desc(ndim, nb, lo, hi), B)
        ref = np.histogramdd(P[live, :ndim], bins=edges)[0].astype(np.int64)
        hc, hw, ht = host_integers(P[live, :ndim], w[live], edges, S)
        assert np.array_equal(hc, ref)
        assert np.array_equal(c.reshape(nb[:ndim]), ref), ndim
        assert np.array_equal(ws.reshape(nb[:ndim]), hw), ndim
        assert np.array_equal(t, ht), ndim


@pytest.mark.parametrize("which", ["golden", "relay4"])
def test_gpu_detector_histograms_equal_numpys(which, request):
    sc = request.getfixturevalue(which)
    last, D = sc["last"], sc["D"]
    P = D.get_PointList2D(last)
    delays = D.get_Delays(last)
    w = last.intensities()
    for axes, bins, ref_vals in ((("X", "Y"), (64, 48), P), (("Delay",), 100, delays[:, None]),
                                 (("X", "Y", "Delay"), 16, np.column_stack([P, delays]))):
        h = D.get_Histogram(last, axes, bins)
        ref = np.histogramdd(ref_vals, bins=h.edges)[0].astype(np.int64)
        assert np.array_equal(h.counts, ref), axes
        assert h.totals[0] + h.totals[1] == len(last)
        assert h.totals[1] == 0          # the default range holds every alive ray
        if w is None:
            assert h.wsums is None and h.intensity is None
            continue
        hc, hw, ht = host_integers(ref_vals, w, h.edges, h.shift)
        assert np.array_equal(h.wsums, hw) and np.array_equal(h.totals, ht), axes
        fw = np.histogramdd(ref_vals, bins=h.edges, weights=w)[0]
        assert np.all(np.abs(h.intensity - fw) <= h.counts * 2.0 ** -(h.shift + 1) + 1e-12 * np.abs(fw)), axes
    hd = D.get_Histogram(last, "Delay", 100)
    assert np.array_equal(hd.counts, np.histogram(delays, bins=hd.edges[0])[0])


def test_gpu_histogram_is_deterministic_and_accumulates(relay4, hip):
    last, D = relay4["last"], relay4["D"]
    from attosecondraytracing_amd import _abi
    h = D.get_Histogram(last, ("X", "Y"), 256)
    d = _abi.ArtHistogramDesc()
    d.source, d.ndim, d.map = _abi.ART_HIST_DETECTOR, 2, D._desc()
    for k in range(2):
        d.axis[k], d.bins[k], d.lo[k], d.hi[k] = k, 256, h.edges[k][0], h.edges[k][-1]
    a = run(hip, d, last, shift=h.shift)
    b = run(hip, d, last, shift=h.shift)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(a[0].reshape(256, 256), h.counts) and np.array_equal(a[1].reshape(256, 256), h.wsums)
    half = (last.n_slots // 2) // 64 * 64
    first, second = last.slots(0, half), last.slots(half, last.n_slots)
    c, ws, t, S = hip.histogram(d, first.view(), first.intensity, first.n_slots, shift=h.shift)
    hip.histogram(d, second.view(), second.intensity, second.n_slots, out=(c, ws, t), shift=h.shift)
    assert np.array_equal(c.cpu().numpy(), a[0]) and np.array_equal(ws.cpu().numpy(), a[1])
    assert np.array_equal(t.cpu().numpy(), a[2])


@pytest.mark.parametrize("bins", [(64,), (2048, 2048)])
def test_gpu_histogram_both_strategies(relay4, bins):
    """64 bins: the LDS form; 2048 x 2048: the global-atomic form."""
    last, D = relay4["last"], relay4["D"]
    axes = ("X", "Y")[:len(bins)]
    h = D.get_Histogram(last, axes, bins)
    P = D.get_PointList2D(last)[:, :len(bins)]
    assert np.array_equal(h.counts, np.histogramdd(P, bins=h.edges)[0].astype(np.int64))
    _, hw, ht = host_integers(P, last.intensities(), h.edges, h.shift)
    assert np.array_equal(h.wsums, hw) and np.array_equal(h.totals, ht)


def test_gpu_footprint_on_the_second_toroid(golden):
    import ART.ModuleGeometry as mgeo
    chain = golden["chain"]
    oe = chain.optical_elements[2]
    h = chain.get_Footprint(2, Bins=(40, 30))
    P = chain.get_output_rays()[2].points()
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    xy = (P - np.asarray(oe.position, dtype=float)) @ fwd.T
    ref = np.histogramdd(xy[:, :2], bins=h.edges)[0].astype(np.int64)
    near = np.zeros(len(xy), dtype=bool)
    for k in range(2):
        near |= np.min(np.abs(xy[:, k][:, None] - h.edges[k][None, :]), axis=1) <= 1e-9
    assert np.abs(h.counts - ref).sum() <= 2 * near.sum()
    half = np.asarray(oe.type.support._CircumRect(), dtype=float) / 2
    assert h.edges[0][0] == -half[0] and h.edges[1][-1] == half[1]
    assert h.totals[0] + h.totals[1] == len(chain.get_output_rays()[2])


def test_gpu_empty_and_all_dead_bundles(relay4, hip):
    last, D = relay4["last"], relay4["D"]
    c, ws, t, _ = run(hip, frame_desc(2, [8, 8], [-1, -1], [1, 1]), last, n=0)
    assert not c.any() and not ws.any() and not t.any()
    dead = last.copy()
    dead.alive.zero_()
    dead.touch()
    h = D.get_Histogram(dead, ("X", "Delay"), 10)
    assert h.counts.shape == (10, 10) and not h.counts.any() and not h.wsums.any() and not h.totals.any()
    assert h.edges[0][0] == 0.0 and h.edges[0][-1] == 1.0         # numpy's range of no values


def test_gpu_histogram_abi_errors_leave_outputs_untouched(relay4, hip):
    import torch
    from attosecondraytracing_amd import _abi
    last = relay4["last"]
    fn = hip.fn["art_histogram"]
    counts = torch.full((64,), 7, dtype=torch.int64, device=hip.device)
    wsums = torch.full((64,), 7, dtype=torch.int64, device=hip.device)
    totals = torch.full((4,), 7, dtype=torch.int64, device=hip.device)
    w = last.intensity.data_ptr()

    def good():
        return frame_desc(2, [8, 8], [-1.0, -1.0], [1.0, 1.0])

    def case(edit, code, msg, n=last.n_slots, cptr=None, wp=w, wsp=None, tptr=None):
        d = good()
        edit(d)
        rc = fn(C.byref(d), C.byref(last.view()), wp, n, 0, counts.data_ptr() if cptr is None else cptr,
                wsums.data_ptr() if wsp is None else wsp, totals.data_ptr() if tptr is None else tptr, hip.stream_ptr())
        assert rc == code, (msg, rc)
        assert msg in hip.last_error(), (msg, hip.last_error())

    E, U = _abi.ART_ERR_BAD_ARG, _abi.ART_ERR_UNSUPPORTED
    case(lambda d: setattr(d, "source", 2), E, "unknown histogram source")
    case(lambda d: d.axis.__setitem__(1, 4), E, "unknown histogram axis")
    case(lambda d: d.axis.__setitem__(0, -1), E, "unknown histogram axis")
    case(lambda d: setattr(d, "ndim", 0), E, "ndim must be 1, 2 or 3")
    case(lambda d: setattr(d, "ndim", 4), E, "ndim must be 1, 2 or 3")
    case(lambda d: d.bins.__setitem__(0, 0), E, "bins must be >= 1")
    case(lambda d: (d.bins.__setitem__(0, 4097), d.bins.__setitem__(1, 4097)), U, "more than 2^24 histogram bins")
    case(lambda d: d.lo.__setitem__(0, float("nan")), E, "histogram range")
    case(lambda d: d.hi.__setitem__(1, float("inf")), E, "histogram range")
    case(lambda d: d.lo.__setitem__(0, 1.0), E, "histogram range")
    case(lambda d: (d.lo.__setitem__(0, -1e308), d.hi.__setitem__(0, 1e308)), E, "histogram range")
    case(lambda d: d.axis.__setitem__(1, _abi.ART_HAXIS_DELAY), E, "a DELAY axis needs the DETECTOR source")
    case(lambda d: (setattr(d, "source", _abi.ART_HIST_DETECTOR), d.axis.__setitem__(1, 2)), E, "unknown histogram axis")
    case(lambda d: None, E, "negative ray count", n=-1)
    case(lambda d: None, E, "counts/totals4 must not be NULL", cptr=0)
    case(lambda d: None, E, "counts/totals4 must not be NULL", tptr=0)
    case(lambda d: None, E, "weights given but wsums is NULL", wsp=0)
    case(lambda d: setattr(d, "wshift", 1075), E, "wshift outside [-1074, 1074]")
    case(lambda d: setattr(d, "wshift", -1075), E, "wshift outside [-1074, 1074]")
    torch.cuda.synchronize()
    for t in (counts, wsums, totals):
        assert bool((t == 7).all())


def test_gpu_plots_show_the_histograms(relay4, golden):
    import ART.ModuleAnalysisAndPlots as mplots
    last, D = relay4["last"], relay4["D"]
    fig = mplots.SpotImage(last, D, Bins=50)
    h = D.get_Histogram(last, ("X", "Y"), 50)
    assert np.array_equal(np.asarray(fig.axes[0].images[0].get_array()), h.intensity.T)
    assert "μm SD" in fig.axes[0].get_legend().get_texts()[0].get_text()
    step = fig._art_state["step"]
    fig._art_press(types.SimpleNamespace(key="right"))
    D2 = D.copy_detector()
    D2.shiftByDistance(step)
    h2 = D2.get_Histogram(last, ("X", "Y"), 50)
    assert np.array_equal(np.asarray(fig.axes[0].images[0].get_array()), h2.intensity.T)
    assert not np.array_equal(h2.counts, h.counts)

    fig = mplots.DelayProfile(last, D, Bins=80)
    h = D.get_Histogram(last, ("Delay",), 80)
    vals, edges, _ = fig.axes[0].patches[0].get_data()
    assert np.array_equal(vals, h.intensity) and np.array_equal(edges, h.edges[0])
    step = fig._art_state["step"]
    fig._art_press(types.SimpleNamespace(key="right"))
    D2 = D.copy_detector()
    D2.shiftByDistance(step)
    vals, edges, _ = fig.axes[0].patches[0].get_data()
    assert np.array_equal(vals, D2.get_Histogram(last, ("Delay",), 80).intensity)

    chain = golden["chain"]
    fig = mplots.MirrorFootprint(chain, 2, Bins=30)
    hf = chain.get_Footprint(2, 30)
    img = fig._art_hist.counts if hf.intensity is None else hf.intensity
    assert np.array_equal(np.asarray([im for ax in fig.axes for im in ax.images][0].get_array()), img.T)

"""GPU: diffraction gratings (ModuleMirror.Grating, art_trace_grating) against the fp64 oracle of tests/grating_common.py,
which tests/test_grating_host.py holds to a long-double truth (sections 1 to 7: plane, sphere, torus), and against that
long-double truth itself on all six substrates (section 8).  n = 4099 rays (a partial last tile), every 7th input
slot dead, unless a test says otherwise.  Bounds: the project's parity bound (1e-10 of the reference magnitudes for points and
paths, 1e-10 absolute for directions) unless a test states its own."""
import ctypes as C

import numpy as np
import pytest
import torch

import grating_common as gc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module")
def art():
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    import ART.ModuleOpticalChain as moc
    from attosecondraytracing_amd import _abi, _lib
    from attosecondraytracing_amd.bundle import RayBundle

    class A:
        pass
    a = A()
    a.mm, a.ms, a.mp, a.mdet, a.moc, a.abi, a.be, a.RayBundle = mm, ms, mp, mdet, moc, _abi, _lib.get_backend(), RayBundle
    return a


def upload(art, rays, wl):
    P, V, path, alive = rays
    b = art.RayBundle.from_arrays(P, V, wavelength=wl, path0=path)
    b.alive.copy_(torch.from_numpy(alive).to(b.alive.device))
    b.touch()
    return b


def state(b):
    """(point, vector, path, alive) as the DEVICE holds them (pack_rays renormalises the directions)."""
    d = b.data.cpu().numpy()
    return d[0:3].T.copy(), d[3:6].T.copy(), d[6].copy(), b.alive.cpu().numpy().copy()


def result(b):
    d = b.data.cpu().numpy()
    return {"point": d[0:3].T, "vector": d[3:6].T, "path": d[6], "inc": d[7],
            "grooves": np.zeros(d.shape[1]) if b.grooves is None else b.grooves.cpu().numpy(), "alive": b.alive.cpu().numpy() != 0}


def oracle_chain(elements, src, wl):
    """The fp64 oracle through a list of OpticalElements; returns one result dict per element."""
    P, V, path, alive = state(src)
    g = None if src.grooves is None else src.grooves.cpu().numpy()
    out = []
    for oe in elements:
        r = gc.diffract(gc.element_spec(oe), P, V, path, alive, wl, grooves=g)
        live = r["alive"]
        P, V, path, g, alive = (np.where(live[:, None], r["point"], 0.0), np.where(live[:, None], r["vector"], 1.0),
                                np.where(live, r["path"], 0.0), np.where(live, r["grooves"], 0.0), live.astype(np.uint8))
        out.append(r)
    return out


def check_against_oracle(got_bundle, ref, what):
    got = result(got_bundle)
    assert np.array_equal(got["alive"], ref["alive"]), what + ": alive masks differ"
    gc.assert_parity(got, ref, ref["alive"], what)


def raw_grating(art, oe, wls, src, outs, n=None, nw=None, q=None, g_in=None, g_out=None):
    """art_trace_grating through the bare ABI; returns its code."""
    be, abi = art.be, art.abi
    desc, _ = art.mp.element_descriptor(oe, True, be)
    G = oe.type
    wl_host = (C.c_double * len(wls))(*wls)
    varr = (abi.ArtBundleView * len(outs))(*[b.view() for b in outs])
    wl_dev = be.from_numpy(np.asarray(wls, dtype=np.float64))
    v_dev = be.from_numpy(np.frombuffer(bytes(varr), dtype=np.uint8).copy())
    g = abi.ArtGratingDesc()
    g.q[0], g.q[1] = G._groove_vector() if q is None else q
    g.lines_per_mm, g.order, g.nw = G.lines_per_mm, G.order, len(wls) if nw is None else nw
    g.wavelengths, g.outs = wl_dev.data_ptr(), v_dev.data_ptr()
    g.grooves_in = None if g_in is None else g_in.data_ptr()
    g.grooves_out = None if g_out is None else g_out.data_ptr()
    vin = src.view()
    rc = be.fn["art_trace_grating"](C.byref(desc), C.byref(g), wl_host, varr, C.byref(vin), src.n_slots if n is None else n,
                                    be.stream_ptr())
    be.synchronize()
    return rc


def prefilled(art, like, count=1):
    outs = [art.RayBundle.allocate(like.n_slots, like=like) for _ in range(count)]
    for b in outs:
        b.data.fill_(SENTINEL)
        b.alive.fill_(9)
    return outs


def untouched(b):
    return bool((b.data == SENTINEL).all()) and bool((b.alive == 9).all())


# ------------------------------------------------------------------------------------------------ 1. grating equation
@pytest.mark.parametrize("ang", [0.0, 90.0])
@pytest.mark.parametrize("m", [-1, 0, 1])
def test_grating_equation_on_a_plane_substrate(art, m, ang):
    wl, N = 30e-6, 1200.0
    oe = gc.place(gc.plane_grating(N, m, ang), 500.0, 80.0)
    src = upload(art, gc.point_source(5e-3), wl)
    out = art.mp.RayTracingCalculation(src, [oe])[0]
    ref = oracle_chain([oe], src, wl)[0]
    check_against_oracle(out, ref, f"m={m} a={ang}")
    got = result(out)
    live = got["alive"]
    fwd = gc.element_spec(oe)["fwd"]
    u = state(src)[1] @ fwd.T
    v = got["vector"] @ fwd.T
    a = np.deg2rad(ang)
    if live.any():
        assert np.abs(v[live, 0] - u[live, 0] - m * wl * N * np.cos(a)).max() <= 1e-12
        assert np.abs(v[live, 1] - u[live, 1] - m * wl * N * np.sin(a)).max() <= 1e-12
        assert np.abs(np.linalg.norm(got["vector"][live], axis=1) - 1).max() <= 1e-14
    alive_in = state(src)[3] != 0
    if ang == 90.0:
        # conical mount: the component along the grooves (the optic's x axis) is preserved, and every order propagates
        assert np.abs(v[live, 0] - u[live, 0]).max() <= 1e-12
        assert np.array_equal(live, alive_in)
    elif m == 1:
        assert not live.any()            # sin(80 deg) + 0.036 > 1 over the whole cone: evanescent
    else:
        assert np.array_equal(live, alive_in)


# ------------------------------------------------------------------------------------------------------- 2. order zero
@pytest.mark.parametrize("N,m", [(0.0, 1), (1200.0, 0)])
def test_order_zero_is_the_bare_toroid(art, N, m):
    wl = 30e-6
    G = gc.torus_grating(N, m)
    oe = gc.place(G, 237.0, 87.0)
    bare = gc.place(G.Mirror, 237.0, 87.0)
    src = upload(art, gc.point_source(2e-3), wl)
    out = art.mp.RayTracingCalculation(src, [oe])[0]
    ref = art.mp.RayTracingCalculation(src, [bare])[0]
    assert torch.equal(out.alive, ref.alive) and int(ref.alive.sum()) > 0
    live = ref.alive.bool()
    a, b = out.data[:, live].cpu().numpy(), ref.data[:, live].cpu().numpy()
    for row in range(8):
        assert np.abs(a[row] - b[row]).max() <= 1e-14 * max(1.0, np.abs(b[row]).max()), row
    assert ref.grooves is None and out.grooves is not None
    if N == 0.0:
        assert bool((out.grooves == 0).all())


# ------------------------------------------------------------------------------------- 3. flat diffracted wavefront
def test_diffracted_plane_wave_is_flat_with_the_groove_phase(art):
    wl = 800e-6
    oe = gc.place(gc.plane_grating(600.0, 1, 0.0, 60.0), 100.0, 30.0)
    src = upload(art, gc.plane_wave(5.0), wl)
    out = art.mp.RayTracingCalculation(src, [oe])[0]
    E = gc.element_spec(oe)
    guide = gc.diffract(E, np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.zeros(1), np.ones(1), wl)
    assert guide["alive"][0]
    P0, v0 = guide["point"][0], guide["vector"][0]
    det = art.mdet.Detector(P0.copy(), Centre=P0 + 100.0 * v0, Normal=-v0)
    assert len(out) == int((state(src)[3] != 0).sum())
    opl = det.get_OpticalPaths(out)
    g = out.grooves.index_select(0, out.index()).cpu().numpy()
    phase_path = opl + wl * g
    mean = opl.mean()
    print("phase path spread", np.ptp(phase_path), "mean path", mean, "opl range", np.ptp(opl))
    assert np.ptp(phase_path) <= 1e-10 * mean
    # pulse-front tilt: the delays spread by lambda * (groove range) / c, picoseconds
    delays = det.get_Delays(out)
    c = art.mdet.LightSpeed
    tilt_fs = wl * (g.max() - g.min()) / c * 1e15
    print("delay range fs", np.ptp(delays), "lambda * groove range / c", tilt_fs)
    assert abs(np.ptp(delays) - tilt_fs) <= 1e-10 * mean / c * 1e15
    assert np.ptp(delays) > 1000.0
    wf = det.get_Wavefront(out, Order=2)
    print("wavefront rms before fit", wf.rms)
    assert wf.rms < 1e-9
    ff = det.get_FocalField(out, Size=1e-3, Pixels=3, Centre=(0.0, 0.0))
    print("1 - strehl", 1 - ff.strehl[0])
    assert ff.strehl[0] > 1 - 1e-9


# ------------------------------------------------------------------------------------------------- 4. evanescent orders
def test_evanescent_orders_die_and_leave_their_slots_untouched(art):
    wl = 30e-6
    oe = gc.place(gc.plane_grating(500.0, 1, 0.0), 500.0, 80.0)
    src = upload(art, gc.point_source(5e-3), wl)
    ref = oracle_chain([oe], src, wl)[0]
    s = ref["s"][ref["hit"]]
    assert (np.abs(s) >= 1e-9).all() and (s > 0).any() and (s < 0).any()       # about the test's own input
    out, = prefilled(art, src)
    g_out = torch.full((1, src.n_slots), SENTINEL, dtype=torch.float64, device=out.data.device)
    assert raw_grating(art, oe, [wl], src, [out], g_out=g_out) == 0
    got = result(out)
    assert np.array_equal(got["alive"], ref["alive"])
    assert 0 < ref["alive"].sum() < ref["hit"].sum()
    out.grooves = g_out[0]
    gc.assert_parity(result(out), ref, ref["alive"], "evanescent")
    lost = torch.from_numpy(~ref["alive"]).to(out.data.device)
    assert bool((out.data[:, lost] == SENTINEL).all()) and bool((g_out[0, lost] == SENTINEL).all())
    assert bool((out.alive[lost] == 0).all())


# --------------------------------------------------------------------------------------------------- 5. curved substrates
@pytest.fixture(scope="module")
def flat_field(art):
    """Spherical / toroidal grating at 87 deg + a plane mirror placed along the diffracted beam, through OEPlacement."""
    chains = {}
    for name, G in (("sphere", gc.sphere_grating()), ("torus", gc.torus_grating())):
        sp = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": gc.N_RAYS}
        fold = art.mm.MirrorPlane(art.ms.SupportRound(80.0))
        chains[name] = art.mp.OEPlacement(sp, [G, fold], [237.0, 235.0], [87.0, 45.0], [0.0, 0.0], name)
    return chains


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_curved_gratings_through_placement(art, flat_field, name):
    chain = flat_field[name]
    g_el, fold = chain.optical_elements
    # the placement follows the diffracted guide ray: the next optic's centre lies on the oracle's diffracted central ray
    guide = gc.diffract(gc.element_spec(g_el), np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.zeros(1), np.ones(1), 30e-6)
    want = guide["point"][0] + 235.0 * guide["vector"][0]
    assert np.abs(np.asarray(fold.position, dtype=float) - want).max() <= 1e-9
    for wl in (10e-6, 40e-6):
        src = chain.source_rays.alias()
        src.wavelength = wl
        outs = art.mp.RayTracingCalculation(src, chain.optical_elements)
        refs = oracle_chain(chain.optical_elements, src, wl)
        assert refs[0]["alive"].sum() > 0
        for k in range(2):
            check_against_oracle(outs[k], refs[k], f"{name} {wl} element {k}")


def test_evanescent_guide_ray_raises_with_the_grating_equation(art):
    sp = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": 64}
    G = gc.plane_grating(1200.0, 1, 0.0)
    with pytest.raises(ValueError, match="evanescent"):
        art.mp.OEPlacement(sp, [G, art.mm.MirrorPlane(art.ms.SupportRound(80.0))], [500.0, 100.0], [80.0, 45.0], [0.0, 0.0], "x")
    sp["Wavelength"] = None
    with pytest.raises(ValueError, match="wavelength"):
        art.mp.OEPlacement(sp, [G, art.mm.MirrorPlane(art.ms.SupportRound(80.0))], [500.0, 100.0], [80.0, 45.0], [0.0, 0.0], "x")


# --------------------------------------------------------------------------------------------------------- 6. fan-out
def test_fan_out_equals_single_wavelength_calls_bit_for_bit(art):
    wls = [10e-6, 25e-6, 40e-6]
    oe = gc.place(gc.torus_grating(), 237.0, 87.0)
    src = upload(art, gc.point_source(2e-3), None)
    n = src.n_slots
    g_in = torch.linspace(-2.0, 2.0, n, dtype=torch.float64, device=src.data.device)
    fan, single = prefilled(art, src, 3), prefilled(art, src, 3)
    gf = torch.zeros((3, n), dtype=torch.float64, device=src.data.device)
    gs = torch.zeros((3, n), dtype=torch.float64, device=src.data.device)
    assert raw_grating(art, oe, wls, src, fan, g_in=g_in, g_out=gf) == 0
    for j in range(3):
        assert raw_grating(art, oe, [wls[j]], src, [single[j]], g_in=g_in, g_out=gs[j:j + 1]) == 0
    for j in range(3):
        assert torch.equal(fan[j].alive, single[j].alive) and int(fan[j].alive.sum()) > 0
        assert torch.equal(fan[j].data.view(torch.int64), single[j].data.view(torch.int64))
    assert torch.equal(gf.view(torch.int64), gs.view(torch.int64))
    assert not torch.equal(fan[0].data[3], fan[2].data[3])             # the wavelengths do differ


def test_spectral_rays_equal_separate_chains_and_disperse(art, flat_field):
    chain = flat_field["sphere"]
    wls = [20e-6, 30e-6, 40e-6]
    mid = art.mp.RayTracingCalculation(chain.source_rays, chain.optical_elements)[-1]
    det = art.mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    det.autoplace(mid, 100.0)
    fans = chain.get_SpectralRays(wls)
    cents, ocents = [], []
    for wl, b in zip(wls, fans):
        src = chain.source_rays.alias()
        src.wavelength = wl
        one = art.mp.RayTracingCalculation(src, chain.optical_elements)[-1]
        assert b.wavelength == wl and b.grooves is not None
        assert torch.equal(b.alive, one.alive) and int(one.alive.sum()) > 0
        live = one.alive.bool()
        assert torch.equal(b.data[:, live].view(torch.int64), one.data[:, live].view(torch.int64))
        assert torch.equal(b.grooves[live].view(torch.int64), one.grooves[live].view(torch.int64))
        cents.append(det.get_PointList3D(b).mean(axis=0))
        ref = oracle_chain(chain.optical_elements, src, wl)[-1]
        lv = ref["alive"]
        nrm, ctr = np.asarray(det.normal, dtype=float), np.asarray(det.centre, dtype=float)
        t = ((ctr - ref["point"][lv]) @ nrm) / (ref["vector"][lv] @ nrm)
        ocents.append((ref["point"][lv] + t[:, None] * ref["vector"][lv]).mean(axis=0))
    d = cents[2] - cents[0]
    along = [(c - cents[0]) @ d for c in cents]
    assert 0 < along[1] < along[2]                                      # ordered in wavelength
    for j in (1, 2):
        got, want = np.linalg.norm(cents[j] - cents[0]), np.linalg.norm(ocents[j] - ocents[0])
        assert want > 1.0 and abs(got - want) <= gc.PARITY * max(1.0, np.abs(ocents[j]).max())
    # the spectrometer image is the sum of the three spot histograms, formed on the device
    import ART.ModuleAnalysisAndPlots as mplots
    _, h = mplots.SpectrometerImage(chain, det, wls, Bins=64, Show=False)
    assert int(h.counts.sum()) + h.outside[0] == sum(len(b) for b in fans)


# ----------------------------------------------------------------------------------------------------------- 7. edges
def test_empty_and_dead_bundles(art):
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    src = upload(art, gc.point_source(5e-3), 30e-6)
    out, = prefilled(art, src)
    assert raw_grating(art, oe, [30e-6], src, [out], n=0) == 0
    assert untouched(out)
    src.alive.zero_()
    src.touch()
    assert raw_grating(art, oe, [30e-6], src, [out]) == 0
    assert bool((out.alive == 0).all()) and bool((out.data == SENTINEL).all())
    res = art.mp.RayTracingCalculation(src, [oe])[0]
    assert len(res) == 0


def test_bad_arguments_launch_nothing(art):
    abi = art.abi
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    src = upload(art, gc.point_source(5e-3), 30e-6)
    out, = prefilled(art, src)
    assert raw_grating(art, oe, [30e-6], src, [out], nw=abi.ART_GRATING_MAX_WAVELENGTHS + 1) == abi.ART_ERR_BAD_ARG
    assert raw_grating(art, oe, [30e-6], src, [out], nw=0) == abi.ART_ERR_BAD_ARG
    assert raw_grating(art, oe, [30e-6], src, [out], q=(1.0, 1e-3)) == abi.ART_ERR_BAD_ARG
    for bad in (0.0, -30e-6, float("nan"), float("inf")):
        assert raw_grating(art, oe, [bad], src, [out]) == abi.ART_ERR_BAD_ARG
    two = prefilled(art, src, 1) + [src]
    assert raw_grating(art, oe, [30e-6, 31e-6], src, two) == abi.ART_ERR_BAD_ARG        # aliasing needs nw == 1
    assert untouched(out) and untouched(two[0])
    assert raw_grating(art, oe, [30e-6], src, [out], n=(1 << 28) + 1) == abi.ART_ERR_UNSUPPORTED
    assert untouched(out)


def test_other_entries_refuse_a_flagged_element(art):
    abi, be = art.abi, art.be
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    desc, _ = art.mp.element_descriptor(oe, True, be)
    src = upload(art, gc.point_source(5e-3), 30e-6)
    out, = prefilled(art, src)
    n, sp = src.n_slots, be.stream_ptr()
    vin, vout = src.view(), out.view()
    darr, varr = (abi.ArtElementDesc * 2)(desc, desc), (abi.ArtBundleView * 2)(vout, vout)
    assert be.fn["art_trace_element"](C.byref(desc), C.byref(vin), C.byref(vout), n, sp) == abi.ART_ERR_UNSUPPORTED
    assert be.fn["art_trace_chain"](darr, 2, C.byref(vin), varr, n, sp) == abi.ART_ERR_UNSUPPORTED
    assert be.fn["art_trace_chain"](darr, 1, C.byref(vin), varr, n, sp) == abi.ART_ERR_UNSUPPORTED
    image = C.create_string_buffer(int(be.fn["art_scene_bytes"](1, 2)))
    iarr = (abi.ArtBundleView * 1)(vin)
    assert be.fn["art_scene_pack"](darr, 1, 2, iarr, varr, None, C.cast(image, C.c_void_p)) == abi.ART_ERR_UNSUPPORTED
    rays = be.from_numpy(np.array([[0.0, 0, 0, 1, 0, 0, 0, np.nan]]))
    al = be.from_numpy(np.ones(1, dtype=np.uint8))
    assert be.fn["art_trace_guides"](darr, 1, rays.data_ptr(), al.data_ptr(), sp) == abi.ART_ERR_UNSUPPORTED
    be.synchronize()
    assert untouched(out) and int(al[0]) == 1


@pytest.fixture(scope="module")
def toroid_chains(art):
    R, r = art.mm.ReturnOptimalToroidalRadii(600, 80)
    tor = art.mm.MirrorToroidal(R, r, art.ms.SupportRectangle(200, 30))
    G = gc.plane_grating(600.0, 1, 0.0, 120.0)
    sp = {"Divergence": 5e-3, "SourceSize": 0, "Wavelength": 800e-6, "DeltaFT": 0.5, "NumberRays": gc.N_RAYS}
    return art.mp.OEPlacement(sp, [tor, G, tor], [500.0, 200.0, 200.0], [80.0, [29.5, 30.0, 30.5], 80.0], [0.0, 0.0, 0.0], "tgt")


def test_grating_between_two_toroids_eager_lazy_and_many(art, toroid_chains):
    chains = toroid_chains
    assert len(chains) == 3
    refs = [oracle_chain(ch.optical_elements, ch.source_rays, 800e-6) for ch in chains]
    assert refs[1][-1]["alive"].sum() > 0
    ch = chains[1]
    outs = art.mp.RayTracingCalculation(ch.source_rays, ch.optical_elements)
    assert outs[0].grooves is None and outs[1].grooves is not None and outs[2].grooves is outs[1].grooves
    for k in range(3):
        check_against_oracle(outs[k], refs[1][k], f"eager element {k}")
    last = art.mp.RayTracingCalculation(ch.source_rays, ch.optical_elements, history=False)[-1]
    check_against_oracle(last, refs[1][2], "no history")
    lazy = art.mp.RayTracingCalculation(ch.source_rays, ch.optical_elements, history="lazy")
    check_against_oracle(lazy[-1], refs[1][2], "lazy, last")
    check_against_oracle(lazy[1], refs[1][1], "lazy, materialised")
    many = art.mp.RayTracingCalculationMany([c.source_rays for c in chains], [c.optical_elements for c in chains])
    for ci in range(3):
        for k in range(3):
            check_against_oracle(many[ci][k], refs[ci][k], f"many chain {ci} element {k}")
    prog_outs = ch.get_output_rays()
    check_against_oracle(prog_outs[-1], refs[1][2], "chain.get_output_rays")


# ------------------------------------------------------------------ 8. every substrate against the long-double truth
# The scenes of grating_common.scenes_six(): a grating on each of the six surfaces and on the convex sphere and cylinder,
# generic / clipped / straddling the cut-off.  The truth (grating_common.truth, numpy.longdouble) is formed from the state the
# DEVICE holds and seeded by the same substrate traced as a bare mirror (art_trace_element): the grating must hit exactly
# those rays.  Every test first asserts about its own input that no ray is marginal (|s| < 1e-9, or within 1e-9 mm of the
# support's edge); the alive masks are then compared bit for bit.  Bounds: the parity bound -- with s >= 1e-9 the direction's
# conditioning is 1 / (2 sqrt(s)) <= 1.6e4, and the header's own deviation from this truth is below 3e-12
# (tests/test_grating_host.py).
SIX = gc.scenes_six()
GENERIC_SIX = sorted(k for k, sc in SIX.items() if sc["family"] == "generic")
SIZES = [1, 63, 64, 65, 257, 70001]          # around a wavefront, more than one workgroup, a partial last tile


def mirror_trace(art, oe, src):
    """The bare substrate in the pose of `oe` through art_trace_element; returns (bundle, seed): segment lengths, NaN = lost."""
    bare = gc.on_pose(getattr(oe.type, "Mirror", oe.type), oe)
    out = art.mp.RayTracingCalculation(src, [bare], mode="element")[0]
    d, alive = out.data[6].cpu().numpy(), out.alive.cpu().numpy() != 0
    return out, np.where(alive, d - src.data[6].cpu().numpy(), np.nan)


def truth_of(art, oe, src, wl, large=None):
    """(E, truth of `oe` on the device's state of `src`, the same with the large support)."""
    P, V, path, alive = state(src)
    g = None if src.grooves is None else src.grooves.cpu().numpy()
    E = gc.element_spec(oe)
    ref = gc.truth(E, P, V, path, alive, wl, mirror_trace(art, oe, src)[1], grooves=g)
    if large is None or large is oe:
        return E, ref, ref
    return E, ref, gc.truth(gc.element_spec(large), P, V, path, alive, wl, mirror_trace(art, large, src)[1], grooves=g)


def check_against_truth(got, ref, what):
    assert np.array_equal(got["alive"], ref["alive"]), what + ": alive masks differ"
    gc.assert_parity(got, ref, ref["alive"], what)
    dev = gc.worst_deviation(got, ref, ref["alive"])
    print(what, "worst deviation from the truth", " ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    return dev


@pytest.mark.parametrize("name", sorted(SIX))
def test_every_substrate_against_the_long_double_truth(art, name):
    sc = SIX[name]
    src = upload(art, sc["rays"], sc["wl"])
    E, ref, ref_large = truth_of(art, sc["oe"], src, sc["wl"], sc["large"])
    n_hit, n_alive = gc.own_input(sc, E, ref, ref_large, name, alive=state(src)[3])
    assert (n_alive == 0) == (name in gc.EVANESCENT)    # N900_m1_a33: evanescent on the four grazing substrates, alive elsewhere
    out = art.mp.RayTracingCalculation(src, [sc["oe"]])[0]
    got = result(out)
    check_against_truth(got, ref, name)
    if sc["family"] == "cutoff":
        m = ref["alive"]
        dv = np.abs(np.asarray(got["vector"][m] - ref["vector"][m], dtype=float)).max(axis=1)
        print(name, "dv * sqrt(s)", f"{float((dv * np.sqrt(np.asarray(ref['s'][m], dtype=float))).max()):.1e}")


@pytest.mark.parametrize("name", GENERIC_SIX)
def test_the_hit_does_not_depend_on_the_order(art, name):
    """Point, path and incidence angle of a grating are the bare mirror's (the bound of test_order_zero_is_the_bare_toroid);
    the masks are equal wherever the order propagates, and nothing is alive where it does not."""
    sc = SIX[name]
    src = upload(art, sc["rays"], sc["wl"])
    out = art.mp.RayTracingCalculation(src, [sc["oe"]])[0]
    ref, _ = mirror_trace(art, sc["oe"], src)
    assert int(ref.alive.sum()) == int((state(src)[3] != 0).sum())
    if name in gc.EVANESCENT:
        assert int(out.alive.sum()) == 0
        return
    assert torch.equal(out.alive, ref.alive)
    live = ref.alive.bool()
    a, b = out.data[:, live].cpu().numpy(), ref.data[:, live].cpu().numpy()
    for row in (0, 1, 2, 6, 7):
        assert np.abs(a[row] - b[row]).max() <= 1e-14 * max(1.0, np.abs(b[row]).max()), row


def _bytes_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("n", SIZES)
def test_bundle_sizes_sentinels_repeatability_and_aliasing(art, n):
    """The clipped ellipsoid through the bare ABI with nw = 2: slots dead on input and lost rays keep what the outputs held."""
    sc = SIX["ellipsoid_clipped"]
    oe, wls = sc["oe"], [30e-6, 12e-6]
    rays = gc.point_source(gc.SUBSTRATES["ellipsoid"][2], n)
    if n == 1:
        rays = (rays[0], rays[1], rays[2], np.ones(1, dtype=np.uint8))
    src = upload(art, rays, None)
    dev = src.data.device
    g_in = torch.linspace(-2.0, 2.0, n, dtype=torch.float64, device=dev)
    src.grooves = g_in
    alive_in = state(src)[3]
    refs = []
    for wl in wls:
        E, ref, ref_large = truth_of(art, oe, src, wl, sc["large"])
        n_s, n_edge, s_min, d_min = gc.marginal(E, ref, ref_large, alive_in)
        assert n_s == 0 and n_edge == 0, (n_s, n_edge, s_min, d_min)
        refs.append(ref)
    n_hit = int(refs[0]["hit"].sum())
    assert n < 64 or 0 < n_hit < int((alive_in != 0).sum())
    assert n_hit > 0

    def run(source, outs, wl_list, g_out):
        assert raw_grating(art, oe, wl_list, source, outs, g_in=g_in, g_out=g_out) == 0

    outs = prefilled(art, src, 2)
    g_out = torch.full((2, n), SENTINEL, dtype=torch.float64, device=dev)
    run(src, outs, wls, g_out)
    for j in range(2):
        got = result(outs[j])
        got["grooves"] = g_out[j].cpu().numpy()
        check_against_truth(got, refs[j], f"n={n} wavelength {j}")
        lost = torch.from_numpy(~refs[j]["alive"]).to(dev)
        assert bool((outs[j].data[:, lost] == SENTINEL).all()), "a lost ray's slot was written"
        assert bool((g_out[j, lost] == SENTINEL).all()) and bool((outs[j].alive[lost] == 0).all())
    again = prefilled(art, src, 2)
    g_again = torch.full((2, n), SENTINEL, dtype=torch.float64, device=dev)
    run(src, again, wls, g_again)
    for j in range(2):                                                                  # two runs, the same bytes
        assert torch.equal(again[j].alive, outs[j].alive) and _bytes_equal(again[j].data, outs[j].data)
    assert _bytes_equal(g_again, g_out)
    inplace = art.RayBundle.allocate(n, like=src)                                      # nw = 1: the output may alias the input
    inplace.data.copy_(src.data)
    inplace.alive.copy_(src.alive)
    g_one = torch.full((1, n), SENTINEL, dtype=torch.float64, device=dev)
    run(inplace, [inplace], wls[:1], g_one)
    live = outs[0].alive.bool()
    assert torch.equal(inplace.alive, outs[0].alive)
    assert _bytes_equal(inplace.data[:, live], outs[0].data[:, live]) and _bytes_equal(g_one[0, live], g_out[0, live])


def test_widest_fan_out_on_the_convex_sphere(art):
    """nw = ART_GRATING_MAX_WAVELENGTHS at n = 65 with the grating of the cut-off scene: from the whole bundle alive at
    10 nm to none at 40 nm."""
    sc = SIX["convex_sphere_cutoff"]
    oe, nw, n = sc["oe"], art.abi.ART_GRATING_MAX_WAVELENGTHS, 65
    wls = [float(w) for w in np.linspace(10e-6, 40e-6, nw)]
    src = upload(art, gc.point_source(gc.SUBSTRATES["convex_sphere"][2], n), None)
    dev = src.data.device
    P, V, path, alive = state(src)
    E = gc.element_spec(oe)
    seed = mirror_trace(art, oe, src)[1]
    refs = [gc.truth(E, P, V, path, alive, wl, seed) for wl in wls]
    assert np.array_equal(refs[0]["hit"], alive != 0)
    s = np.abs(np.array([np.asarray(r["s"], dtype=float)[r["hit"]] for r in refs]))
    assert s.min() >= gc.MARGIN_S, f"a ray within {gc.MARGIN_S} of the cut-off: {s.min():.2e}"
    counts = [int(r["alive"].sum()) for r in refs]
    assert counts[0] == int((alive != 0).sum()) and counts[-1] == 0 and len(set(counts)) >= 5
    fan = art.RayBundle.allocate_many(n, nw, src)
    for b in fan:
        b.data.fill_(SENTINEL)
        b.alive.fill_(9)
    gf = torch.full((nw, n), SENTINEL, dtype=torch.float64, device=dev)
    assert raw_grating(art, oe, wls, src, fan, g_out=gf) == 0
    got_alive = torch.stack([b.alive for b in fan]).cpu().numpy() != 0
    for j in range(nw):
        assert int(got_alive[j].sum()) == counts[j] and np.array_equal(got_alive[j], refs[j]["alive"]), j
    half = int(np.argmin(np.abs(np.array(counts) - counts[0] / 2)))          # the wavelength that splits the bundle
    assert 0 < counts[half] < counts[0]
    for j in (0, nw // 2, half, nw - 1):
        one, = prefilled(art, src)
        g1 = torch.full((1, n), SENTINEL, dtype=torch.float64, device=dev)
        assert raw_grating(art, oe, [wls[j]], src, [one], g_out=g1) == 0
        assert torch.equal(fan[j].alive, one.alive) and _bytes_equal(fan[j].data, one.data) and _bytes_equal(gf[j], g1[0])
    for j in (nw // 2, half):
        got = result(fan[j])
        got["grooves"] = gf[j].cpu().numpy()
        check_against_truth(got, refs[j], f"fan-out, wavelength {j}")


def _behind(oe_first, guide, distance, incidence_deg, optic):
    """`optic` at `distance` along the guide ray that leaves `oe_first`, at `incidence_deg` in the plane spanned by that ray
    and the first element's normal, major axis in that plane: place() about another axis."""
    P0, v = np.asarray(guide["point"][0], dtype=float), np.asarray(guide["vector"][0], dtype=float)
    a = np.asarray(oe_first.normal, dtype=float)
    a = a - (a @ v) * v
    a /= np.linalg.norm(a)
    th = np.deg2rad(incidence_deg)
    return gc.moe.OpticalElement(optic, P0 + distance * v, -np.cos(th) * v + np.sin(th) * a, np.sin(th) * v + np.cos(th) * a)


def test_two_gratings_in_one_chain(art):
    """A plane grating (600, +1, 33 deg) and a cylinder grating (300, -1, 118 deg) that catches the first one's diffracted
    central ray.  Truth per element, each from the state the device holds in front of it; the last bundle's groove count is
    the sum of the two gratings' own terms."""
    wl = 30e-6
    g1 = gc.place(art.mm.Grating(art.mm.MirrorPlane(art.ms.SupportRectangle(60.0, 10.0)), 600.0, 1, 33.0), 237.0, 75.0)
    one = upload(art, (np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.zeros(1), np.ones(1, dtype=np.uint8)), wl)
    guide = truth_of(art, g1, one, wl)[1]
    assert guide["alive"][0]
    g2 = _behind(g1, guide, 150.0, 75.0, art.mm.Grating(gc.substrate("cylinder"), 300.0, -1, 118.0))
    els = [g1, g2]
    src = upload(art, gc.point_source(2e-3), wl)
    outs = art.mp.RayTracingCalculation(src, els)
    assert src.grooves is None and outs[0].grooves is not None and outs[1].grooves is not outs[0].grooves
    cur, refs = src, []
    for k, oe in enumerate(els):
        E, ref, _ = truth_of(art, oe, cur, wl)
        n_s, n_edge, s_min, d_min = gc.marginal(E, ref, ref, state(cur)[3])
        assert n_s == 0 and n_edge == 0, (k, n_s, n_edge, s_min, d_min)
        check_against_truth(result(outs[k]), ref, f"two gratings, element {k}")
        refs.append(ref)
        cur = outs[k]
    m = refs[1]["alive"]
    assert int(m.sum()) == int((state(src)[3] != 0).sum())
    total = np.asarray(refs[0]["term"] + refs[1]["term"], dtype=np.float64)
    got = outs[1].grooves.cpu().numpy()
    assert float(np.abs(refs[0]["term"][m]).max()) > 1.0 and float(np.abs(refs[1]["term"][m]).max()) > 1.0      # both count
    assert np.abs(got[m] - total[m]).max() <= gc.PARITY * max(1.0, np.abs(total[m]).max())
    last = art.mp.RayTracingCalculation(src, els, history=False)[-1]
    lazy = art.mp.RayTracingCalculation(src, els, history="lazy")
    live = outs[1].alive.bool()
    for what, b in (("history=False", last), ("lazy, last", lazy[-1]), ("lazy, materialised", lazy[0])):
        want = outs[0] if what == "lazy, materialised" else outs[1]
        lv = want.alive.bool()
        assert torch.equal(b.alive, want.alive), what
        assert _bytes_equal(b.data[:, lv], want.data[:, lv]) and _bytes_equal(b.grooves[lv], want.grooves[lv]), what
    assert int(live.sum()) > 0


@pytest.fixture(scope="module")
def placed_six(art):
    """An ellipsoidal and a cylindrical grating, each followed by a plane fold mirror, through OEPlacement."""
    chains = {}
    for name, G, inc in (("ellipsoid", art.mm.Grating(gc.substrate("ellipsoid"), 600.0, 2, 118.0), 80.0),
                         ("cylinder", art.mm.Grating(gc.substrate("cylinder"), 900.0, 1, 33.0), 75.0)):
        sp = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": gc.N_RAYS}
        fold = art.mm.MirrorPlane(art.ms.SupportRound(80.0))
        chains[name] = art.mp.OEPlacement(sp, [G, fold], [237.0, 235.0], [inc, 45.0], [0.0, 0.0], name)
    return chains


@pytest.mark.parametrize("name", ["ellipsoid", "cylinder"])
def test_ellipsoidal_and_cylindrical_gratings_through_placement(art, placed_six, name):
    chain = placed_six[name]
    g_el, fold = chain.optical_elements
    wl = 30e-6
    one = upload(art, (np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), np.zeros(1), np.ones(1, dtype=np.uint8)), wl)
    guide = truth_of(art, g_el, one, wl)[1]
    assert guide["alive"][0]
    want = np.asarray(guide["point"][0] + 235.0 * guide["vector"][0], dtype=float)
    assert np.abs(np.asarray(fold.position, dtype=float) - want).max() <= 1e-9
    src = chain.source_rays
    outs = art.mp.RayTracingCalculation(src, chain.optical_elements)
    cur = src
    for k, oe in enumerate(chain.optical_elements):
        E, ref, _ = truth_of(art, oe, cur, wl)
        n_s, n_edge, s_min, d_min = gc.marginal(E, ref, ref, state(cur)[3])
        assert n_s == 0 and n_edge == 0, (k, n_s, n_edge, s_min, d_min)
        assert ref["alive"].sum() > 0
        check_against_truth(result(outs[k]), ref, f"{name} through placement, element {k}")
        cur = outs[k]

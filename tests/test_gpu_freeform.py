"""GPU: freeform and aspheric mirrors (ModuleMirror.MirrorFreeform / MirrorEvenAsphere, art_trace_freeform) against the
long-double truth of tests/freeform_common.py.  Bounds: the project's parity bound (1e-10 of the reference magnitudes for
points and paths, 1e-10 absolute for directions and angles), alive masks bit-exact (tests/test_freeform_host.py shows that
no ray of any scene is marginal and that every candidate converges well inside the device's step limit)."""
import ctypes as C

import numpy as np
import pytest
import torch

import focal_common as fo
import freeform_common as fc
import quadric_common as qc

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 70001]          # around a wavefront, more than one workgroup, a partial last tile
WL = 30e-6
SENTINEL = -7.25
LD = qc.LD


@pytest.fixture(scope="module")
def art():
    import ART.ModuleMirror as mm
    import ART.ModuleMask as mk
    import ART.ModuleSupport as ms
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    import ART.ModuleOpticalChain as moc
    from attosecondraytracing_amd import _abi, _lib
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.graph import SceneProgram

    class A:
        pass
    a = A()
    a.mm, a.mk, a.ms, a.mp, a.mdet, a.moc, a.abi, a.be, a.RayBundle = mm, mk, ms, mp, mdet, moc, _abi, _lib.get_backend(), RayBundle
    a.SceneProgram = SceneProgram
    return a


def upload(art, rays):
    P, V, path, alive = rays
    b = art.RayBundle.from_arrays(P, V, wavelength=WL, path0=path)
    b.alive.copy_(torch.from_numpy(np.ascontiguousarray(alive)).to(b.alive.device))
    b.touch()
    return b


def state(b):
    """(point, vector, path, alive) as the DEVICE holds them (packing renormalises the directions)."""
    d = b.data.cpu().numpy()
    return d[0:3].T.copy(), d[3:6].T.copy(), d[6].copy(), b.alive.cpu().numpy().copy()


def result(b):
    d = b.data.cpu().numpy()
    return {"point": d[0:3].T, "vector": d[3:6].T, "path": d[6], "inc": d[7], "alive": b.alive.cpu().numpy() != 0}


def check_against_truth(got_bundle, ref, what):
    got = result(got_bundle)
    assert np.array_equal(got["alive"], ref["alive"]), what + ": alive masks differ"
    worst = qc.assert_parity(got, ref, ref["alive"], what)
    print(f"{what}: {int(ref['alive'].sum())} alive, worst deviation from the truth {worst:.2e} of the scene's magnitudes")
    return worst


def same_bytes(a, b):
    live = b.alive.bool()
    return torch.equal(a.alive, b.alive) and torch.equal(a.data[:, live], b.data[:, live])


def figure_on_device(art, M):
    table, R, N = M._freeform_figure()
    return (art.be.from_numpy(table), R, N)


# ------------------------------------------------------------------------------------------- 1. scenes against the truth
SCENES = fc.scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_against_truth(art, name):
    oe, rays = SCENES[name]
    src = upload(art, rays)
    out = art.mp.RayTracingCalculation(src, [oe])[0]
    ref = fc.trace(fc.element_spec(oe), *state(src))
    check_against_truth(out, ref, name)


@pytest.mark.parametrize("n", SIZES)
def test_bundle_sizes_sentinels_and_repeatability(art, n):
    """Scene (a) at every size: slots dead on input and lost rays keep what the output held."""
    oe = SCENES["a_ellipsoid_2deg"][0]
    rays = qc.point_source(1.5e-3, n)
    if n == 1:
        rays = (rays[0], rays[1], rays[2], np.ones(1, dtype=np.uint8))
    src = upload(art, rays)
    out = art.RayBundle.allocate(n, like=src)
    out.data.fill_(SENTINEL)
    out.alive.fill_(9)
    desc, _ = art.mp.element_descriptor(oe, True, art.be)
    fig = figure_on_device(art, oe.type)
    co = oe.type._base_coefficients()
    art.be.trace_freeform(desc, co, fig, src.view(), out.view(), n)
    art.be.synchronize()
    ref = fc.trace(fc.element_spec(oe), *state(src))
    check_against_truth(out, ref, f"n={n}")
    assert n < 64 or 0 < ref["alive"].sum() < (rays[3] != 0).sum()
    lost = torch.from_numpy(~ref["alive"]).to(out.data.device)
    assert bool((out.data[:, lost] == SENTINEL).all()), "a lost ray's slot was written"
    assert bool((out.alive[lost] == 0).all())
    again = art.RayBundle.allocate(n, like=src)
    again.data.fill_(SENTINEL)
    art.be.trace_freeform(desc, co, fig, src.view(), again.view(), n)
    art.be.synchronize()
    assert torch.equal(again.alive, out.alive) and torch.equal(again.data, out.data)      # two runs, the same bytes
    inplace = art.RayBundle.allocate(n, like=src)                                          # out may alias in
    inplace.data.copy_(src.data)
    inplace.alive.copy_(src.alive)
    art.be.trace_freeform(desc, co, fig, inplace.view(), inplace.view(), n)
    art.be.synchronize()
    assert same_bytes(inplace, out)


@pytest.mark.parametrize("name", ["a_ellipsoid_2deg", "b_ellipsoid_45deg", "f_twice_on_the_sheet_zero", "f_second_candidate_zero",
                                  "f_support_recthole_zero"])
def test_zero_figure_against_art_trace_quadric(art, name):
    """The same bundle through art_trace_quadric and through art_trace_freeform with a zero figure on the same base: masks
    equal, values to 1e-13 of the scene's magnitudes (the one Newton step is a rounding error)."""
    oe, rays = SCENES[name]
    base = fc.base_element(oe)
    flat = fc.on_pose(art.mm.MirrorFreeform(oe.type.Base, []), oe)
    src = upload(art, rays)
    a = result(art.mp.RayTracingCalculation(src, [flat])[0])
    b = result(art.mp.RayTracingCalculation(src, [base])[0])
    assert np.array_equal(a["alive"], b["alive"]) and b["alive"].any()
    m = b["alive"]
    worst = 0.0
    for key, rel in (("point", True), ("path", True), ("vector", False), ("inc", False)):
        scale = max(1.0, float(np.abs(b[key][m]).max())) if rel else 1.0
        err = float(np.abs(a[key][m] - b[key][m]).max())
        assert err <= 1e-13 * scale, f"{name} {key}: {err:.3e}"
        worst = max(worst, err / scale)
    print(f"{name}: zero figure against art_trace_quadric {worst:.2e} of the scene's magnitudes")


# --------------------------------------------------------------------------------------------------- 2. the KB chain (h)
def test_kb_chain_full_and_lazy_history_truth_and_wavefront(art):
    els, focus, u2 = fc.kb_elements()
    src = upload(art, qc.point_source(1e-3))
    chain = art.moc.OpticalChain(src, els, "figured KB")
    full = chain.get_output_rays()
    lazy_chain = art.moc.OpticalChain(src, els, "figured KB, lazy")
    lazy = lazy_chain.get_output_rays(history="lazy")
    assert same_bytes(lazy[-1], full[-1]) and same_bytes(lazy[0], full[0])
    cur = state(chain.source_rays)
    for k, oe in enumerate(chain.optical_elements):
        ref = fc.trace(fc.element_spec(oe), *cur)
        check_against_truth(full[k], ref, f"KB mirror {k}")
        cur = (ref["point"], ref["vector"], ref["path"], ref["alive"].astype(np.uint8))
    assert ref["alive"].sum() > 500
    # the wavefront error about the ideal focus: W = path + d . (F - p) about its mean, from the truth's last bundle
    m = ref["alive"]
    W = ref["path"][m] + (ref["vector"][m] * (np.asarray(focus, dtype=LD) - ref["point"][m])).sum(1)
    rms = float(np.sqrt(((W - W.mean()) ** 2).mean()))
    det = art.mdet.Detector(np.asarray(els[-1].position, dtype=float), np.asarray(focus, dtype=float), -u2)
    wf = det.get_Wavefront(full[-1], Order=4, Centre=(0.0, 0.0))
    print(f"figured KB: wavefront rms {wf.rms:.6e} mm on the device, {rms:.6e} mm from the truth, relative {abs(wf.rms / rms - 1):.2e}")
    assert wf.count == int(m.sum()) and rms > 1e-7
    assert abs(wf.rms - rms) <= 1e-6 * rms


def test_freeform_mixed_with_a_toroid_and_a_mask_is_traced_stepwise(art):
    mask = art.mk.Mask(art.ms.SupportRoundHole(30.0, 1.5, 0.0, 0.0))
    S = art.ms.SupportRectangle(200.0, 30.0)
    A = art.mm.MirrorFreeform(art.mm.MirrorEllipticalCylinder(S, 1000.0, 2000.0, 3.0), [fc.cubic_figure(S, 2e-5)])
    R, r = art.mm.ReturnOptimalToroidalRadii(600.0, 87.0)
    T = art.mm.MirrorToroidal(R, r, S)
    sp = {"Divergence": 5e-3, "SourceSize": 0, "Wavelength": WL, "DeltaFT": 0.5, "NumberRays": 4099}
    ch = art.mp.OEPlacement(sp, [mask, A, T], [400.0, 600.0, 200.0], [0.0, 87.0, 87.0], [0.0, 0.0, 0.0], "mixed")
    src, els = ch.source_rays, ch.optical_elements
    ref, cur = [], src
    for oe in els:
        cur = art.mp.RayTracingCalculation(cur, [oe])[0]
        ref.append(cur)
    assert 0 < len(ref[-1]) < int((src.alive != 0).sum())
    for k, (a, b) in enumerate(zip(art.mp.RayTracingCalculation(src, els, history=True), ref)):
        assert same_bytes(a, b), f"history=True, element {k}"
    assert same_bytes(art.mp.RayTracingCalculation(src, els, history=False)[-1], ref[-1])
    prog = art.SceneProgram([src], [els])
    assert prog._stepwise and prog.graph is None
    for a, b in zip(prog.run()[0], ref):
        assert same_bytes(a, b)
    for a, b in zip(ch.get_output_rays(), ref):
        assert same_bytes(a, b)
    # the guide ray followed the REAL reflected central ray: the figure has a slope at the pole (-3A / R per mm)
    slope = -3 * 2e-5 / S._CircumCirc()
    n_flat = np.asarray(els[1].normal, dtype=float)
    u_in = np.array([1.0, 0.0, 0.0])
    d_flat = u_in - 2 * u_in.dot(n_flat) * n_flat
    d_real = np.asarray(els[2].position, dtype=float) - np.asarray(els[1].position, dtype=float)
    d_real /= np.linalg.norm(d_real)
    turn = np.linalg.norm(np.cross(d_flat, d_real))
    assert abs(turn - 2 * abs(slope)) <= 1e-2 * 2 * abs(slope)


# ------------------------------------------------------------------------------------------- 3. an analysis behind the trace
def test_strehl_behind_a_figured_ellipsoid_against_the_truths_coherent_sum(art):
    """Scene (b) at 30 nm: get_FocalField's Strehl ratio at the base's image focus against the same coherent sum formed in
    NumPy (focal_common.field) from the TRUTH's bundle.  focal_common states no bound of its own: 1e-9 absolute."""
    oe, rays = SCENES["b_ellipsoid_45deg"]
    src = upload(art, rays)
    out = art.mp.RayTracingCalculation(src, [oe])[0]
    ref = fc.trace(fc.element_spec(oe), *state(src))
    u = np.array([0.0, 0.0, 1.0])                                   # 45 degrees grazing: +x turns into +z
    focus = np.asarray(oe.position, dtype=float) + 400.0 * u
    det = art.mdet.Detector(np.asarray(oe.position, dtype=float), focus, -u)
    f = det.get_FocalField(out, Size=2e-3, Pixels=5, Centre=(0.0, 0.0))
    d = det._desc()
    E = fo.field(np.asarray(ref["point"], dtype=float), np.asarray(ref["vector"], dtype=float), np.asarray(ref["path"], dtype=float),
                 ref["alive"], None, 2 * np.pi / f.wavelength, f.ref_path, np.array(d.centre[:]), np.array(d.normal[:]),
                 np.array(d.rot[:]), f.x, f.y, [-s for s in f.shifts])
    strehl = float((np.abs(E[0]) ** 2).max()) / float(ref["alive"].sum()) ** 2
    print(f"figured ellipsoid at 30 nm: Strehl {f.strehl[0]:.12f} on the device, {strehl:.12f} from the truth, "
          f"difference {abs(f.strehl[0] - strehl):.2e}")
    assert 0 < strehl < 1
    assert abs(f.strehl[0] - strehl) <= 1e-9


# ------------------------------------------------------------------------------------------------- 4. refusals on the device
def test_other_entry_points_refuse_a_freeform_on_the_device(art):
    be, abi = art.be, art.abi
    oe, rays = SCENES["b_ellipsoid_45deg"]
    src = upload(art, rays)
    out = art.RayBundle.allocate(src.n_slots, like=src)
    out.data.fill_(SENTINEL)
    out.alive.fill_(9)
    desc, _ = art.mp.element_descriptor(oe, True, be)
    vin, vout = src.view(), out.view()
    darr, varr = (abi.ArtElementDesc * 1)(desc), (abi.ArtBundleView * 1)(vout)
    n, sp = src.n_slots, be.stream_ptr()
    guides = be.from_numpy(np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]]))
    galive = be.from_numpy(np.ones(1, dtype=np.uint8))
    image = C.create_string_buffer(int(be.fn["art_scene_bytes"](1, 1)))
    q = abi.ArtQuadricDesc()
    q.q[0], q.b[2] = 0.01, -0.5
    calls = {"art_trace_element": lambda: be.fn["art_trace_element"](C.byref(desc), C.byref(vin), C.byref(vout), n, sp),
             "art_trace_chain": lambda: be.fn["art_trace_chain"](darr, 1, C.byref(vin), varr, n, sp),
             "art_trace_grating": lambda: be.fn["art_trace_grating"](C.byref(desc), None, None, None, C.byref(vin), n, sp),
             "art_trace_quadric": lambda: be.fn["art_trace_quadric"](C.byref(desc), C.byref(q), C.byref(vin), C.byref(vout), n, sp),
             "art_scene_pack": lambda: be.fn["art_scene_pack"](darr, 1, 1, (abi.ArtBundleView * 1)(vin), varr, None,
                                                               C.cast(image, C.c_void_p)),
             "art_trace_guides": lambda: be.fn["art_trace_guides"](darr, 1, guides.data_ptr(), galive.data_ptr(), sp)}
    for name, call in calls.items():
        assert call() == abi.ART_ERR_UNSUPPORTED, name
        assert "art_trace_freeform" in be.last_error(), name
    be.synchronize()
    assert bool((out.data == SENTINEL).all()) and bool((out.alive == 9).all())

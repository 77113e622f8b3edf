"""GPU: general quadric mirrors (ModuleMirror.MirrorQuadric / MirrorConic, art_trace_quadric) against the long-double truth
of tests/quadric_common.py.  Bounds: the project's parity bound (1e-10 of the reference magnitudes for points and paths,
1e-10 absolute for directions and angles), alive masks bit-exact (tests/test_quadric_host.py shows that no ray of any
scene is marginal); the stigmatic tests state their own."""
import ctypes as C

import numpy as np
import pytest
import torch

import quadric_common as qc

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 70001]          # around a wavefront, more than one workgroup, a partial last tile
WL = 50e-6
SENTINEL = -7.25


@pytest.fixture(scope="module")
def art():
    import ART.ModuleMirror as mm
    import ART.ModuleMask as mk
    import ART.ModuleSupport as ms
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd import _abi, _lib, coating
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.graph import SceneProgram

    class A:
        pass
    a = A()
    a.mm, a.mk, a.ms, a.mp, a.mdet, a.abi, a.be, a.RayBundle = mm, mk, ms, mp, mdet, _abi, _lib.get_backend(), RayBundle
    a.coating, a.SceneProgram = coating, SceneProgram
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


def stepwise(art, src, elements):
    """The element-by-element trace: one call per element."""
    outs, cur = [], src
    for oe in elements:
        cur = art.mp.RayTracingCalculation(cur, [oe])[0]
        outs.append(cur)
    return outs


# ------------------------------------------------------------------------------------------- 1. scenes against the truth
SCENES = qc.scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_against_truth(art, name):
    oe, rays = SCENES[name]
    src = upload(art, rays)
    out = art.mp.RayTracingCalculation(src, [oe])[0]
    ref = qc.trace(qc.element_spec(oe), *state(src))
    check_against_truth(out, ref, name)


def _sized(n):
    """An off-axis ellipsoid behind a holed round support; rays on both sides of the edge and of the hole."""
    M = SCENES["support_roundhole"][0].type
    return qc.place(M, 400.0, 45.0), qc.point_source(0.06, n)


@pytest.mark.parametrize("n", SIZES)
def test_bundle_sizes_and_repeatability(art, n):
    oe, rays = _sized(n)
    if n == 1:
        rays = (rays[0], rays[1], rays[2], np.ones(1, dtype=np.uint8))
    src = upload(art, rays)
    out = art.RayBundle.allocate(n, like=src)
    out.data.fill_(SENTINEL)
    out.alive.fill_(9)
    desc, _ = art.mp.element_descriptor(oe, True, art.be)
    art.be.trace_quadric(desc, oe.type._quadric_coefficients(), src.view(), out.view(), n)
    art.be.synchronize()
    ref = qc.trace(qc.element_spec(oe), *state(src))
    check_against_truth(out, ref, f"n={n}")
    lost = torch.from_numpy(~ref["alive"]).to(out.data.device)
    assert bool((out.data[:, lost] == SENTINEL).all()), "a lost ray's slot was written"
    assert bool((out.alive[lost] == 0).all())
    again = art.RayBundle.allocate(n, like=src)
    again.data.fill_(SENTINEL)
    art.be.trace_quadric(desc, oe.type._quadric_coefficients(), src.view(), again.view(), n)
    art.be.synchronize()
    assert torch.equal(again.alive, out.alive) and torch.equal(again.data, out.data)      # two runs, the same bytes
    # in place (out may alias in), as the history-free trace uses it
    inplace = art.RayBundle.allocate(n, like=src)
    inplace.data.copy_(src.data)
    inplace.alive.copy_(src.alive)
    art.be.trace_quadric(desc, oe.type._quadric_coefficients(), inplace.view(), inplace.view(), n)
    art.be.synchronize()
    assert same_bytes(inplace, out)


# ------------------------------------------------------------------------------------------------- 2. stigmatic imaging
def _source(div, size, n=4099):
    return {"Divergence": div, "SourceSize": size, "Wavelength": WL, "DeltaFT": 0.5, "NumberRays": n}


def _focus(chain, q):
    """The lab point `q` behind the last element along the reflected central ray, and that ray's direction: the central
    ray leaves the source along +x and is mirrored at every element's normal (nothing here looks at the major axis)."""
    u = np.array([1.0, 0.0, 0.0])
    for oe in chain.optical_elements:
        n = np.asarray(oe.normal, dtype=float)
        u = u - 2 * u.dot(n) * n
    return np.asarray(chain.optical_elements[-1].position, dtype=float) + q * u, u


def _stigmatic(art, chain, q, total, what):
    """Spot radius about the focus and spread of the optical paths on a detector through it; both <= 1e-10 * total."""
    last = chain.get_output_rays()[-1]
    assert len(last) > 0.5 * chain.source_rays.n_slots, what + ": most rays must reach the focus"
    F, u = _focus(chain, q)
    det = art.mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float), F, -u)
    r = np.linalg.norm(det.get_PointList2D(last), axis=1).max()
    spread = np.ptp(det.get_OpticalPaths(last))
    print(f"{what}: spot radius {r:.3e} mm, path spread {spread:.3e} mm (bound {1e-10 * total:.3e})")
    assert r <= 1e-10 * total and spread <= 1e-10 * total
    return det, last


def _strehl(det, last, eps, what):
    """At a stigmatic focus every ray arrives in phase: Strehl >= 1 - (k eps)^2 for path errors bounded by eps."""
    ff = det.get_FocalField(last, Size=1e-4, Pixels=3, Centre=(0.0, 0.0))
    k = 2 * np.pi / WL
    print(f"{what}: 1 - Strehl = {1 - ff.strehl[0]:.3e} (bound {(k * eps) ** 2:.3e})")
    assert ff.strehl[0] >= 1 - (k * eps) ** 2


def test_stigmatic_ellipsoid_point_to_point(art):
    M = art.mm.MirrorConic(art.ms.SupportRound(25.0), 700.0, 250.0, 10.0)
    chain = art.mp.OEPlacement(_source(5e-3, 0), [M], [700.0], [80.0], [0.0], "ellipsoid")
    det, last = _stigmatic(art, chain, 250.0, 950.0, "ellipsoid 700 -> 250 at 10 deg")
    _strehl(det, last, 1e-10 * 950.0, "ellipsoid")


def test_stigmatic_paraboloid_collimated_to_point(art):
    M = art.mm.MirrorConic(art.ms.SupportRectangle(130.0, 20.0), np.inf, 300.0, 2.0)
    chain = art.mp.OEPlacement(_source(0, 4.0), [M], [100.0], [88.0], [0.0], "paraboloid")
    det, last = _stigmatic(art, chain, 300.0, 400.0, "paraboloid -> 300 at 2 deg")
    _strehl(det, last, 1e-10 * 400.0, "paraboloid")


def test_stigmatic_wolter_pair(art):
    """Paraboloid (focus 600 mm behind it) then, 200 mm downstream, a hyperboloid that takes the converging beam --
    virtual object 400 mm behind it -- to a real focus at 150 mm."""
    S = art.ms.SupportRectangle(130.0, 20.0)
    P = art.mm.MirrorConic(S, np.inf, 600.0, 2.0)
    H = art.mm.MirrorHyperboloidal(S, -400.0, 150.0, 2.0)
    chain = art.mp.OEPlacement(_source(0, 4.0), [P, H], [100.0, 200.0], [88.0, 88.0], [0.0, 0.0], "wolter")
    det, last = _stigmatic(art, chain, 150.0, 450.0, "Wolter-I, 600 / -400 -> 150 at 2 deg")
    assert len(last) == chain.source_rays.n_slots                     # the two mirrors are far enough apart: no ray is lost
    _strehl(det, last, 1e-10 * 450.0, "Wolter-I")


def test_stigmatic_elliptical_cylinder_in_its_plane_of_incidence(art):
    """A cylinder focuses onto a LINE (along y, the lab's normal of the plane of incidence): in the projection onto the
    xz plane every ray passes through the focus, and since the normal has no y component a ray keeps v_y, so its
    projected path -- path * sqrt(1 - v_y^2) -- is the constant p + q."""
    M = art.mm.MirrorEllipticalCylinder(art.ms.SupportRectangle(130.0, 20.0), 1000.0, 300.0, 2.0)
    chain = art.mp.OEPlacement(_source(1.5e-3, 0), [M], [1000.0], [88.0], [0.0], "ellcyl")
    last = chain.get_output_rays()[-1]
    assert len(last) > 0.5 * chain.source_rays.n_slots
    F, u = _focus(chain, 300.0)
    assert abs(F[1]) < 1e-9 and abs(u[1]) < 1e-12
    got = result(last)
    live = got["alive"]
    P, v, path = got["point"][live], got["vector"][live], got["path"][live]
    w = np.hypot(v[:, 0], v[:, 2])                                  # |projection of v|
    dx, dz = F[0] - P[:, 0], F[2] - P[:, 2]
    r = np.abs(dx * v[:, 2] - dz * v[:, 0]) / w                     # distance of the projected ray from the projected focus
    s = (dx * v[:, 0] + dz * v[:, 2]) / (w * w)                     # ray parameter where the projection reaches the focus
    proj = (path + s) * w
    total = 1300.0
    print(f"elliptical cylinder: projected spot {r.max():.3e} mm, projected path spread {np.ptp(proj):.3e} mm (bound {1e-10 * total:.3e})")
    assert r.max() <= 1e-10 * total and np.ptp(proj) <= 1e-10 * total
    assert abs(proj.mean() - total) <= 1e-10 * total
    assert np.abs(v[:, 1]).max() > 1e-4                             # the bundle does have out-of-plane rays


# ------------------------------------------------------------------- 3. cross-checks against the reference-derived kinds
def test_quadric_sphere_against_mirror_spherical(art):
    R, S = 400.0, art.ms.SupportRound(12.0)
    quad = art.mm.MirrorQuadric(S, np.eye(3) / (2 * R), [0.0, 0.0, -0.5])
    ref = art.mm.MirrorSpherical(R, S)
    sp = _source(0.03, 0)
    a = art.mp.OEPlacement(sp, [quad], [500.0], [25.0], [30.0], "quadric sphere")
    b = art.mp.OEPlacement(sp, [ref], [500.0], [25.0], [30.0], "sphere")
    oa, ob = a.get_output_rays()[0], b.get_output_rays()[0]
    ra, rb = result(oa), result(ob)
    assert np.array_equal(ra["alive"], rb["alive"]) and 0 < rb["alive"].sum() < (b.source_rays.alive != 0).sum().item()
    worst = qc.assert_parity(ra, rb, rb["alive"], "quadric sphere against MirrorSpherical")
    print(f"quadric sphere against MirrorSpherical: worst {worst:.2e}")


def test_conic_ellipsoid_against_mirror_ellipsoidal(art):
    """The same surface in two frames: MirrorEllipsoidal lives in the ellipse's centre frame, MirrorConic in the pole
    frame.  The conic element gets the pose that puts its pole, tangent and normal where the ellipsoid's are.  The supports
    are generous (their xy planes differ, so an edge would cut the two differently): the masks compare the dead inputs."""
    import ART.ModuleOpticalElement as moe
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    p, q, off = 400.0, 250.0, 60.0
    S = art.ms.SupportRound(60.0)
    E = art.mm.MirrorEllipsoidal(S, f_object=p, f_image=q, OffAxisAngle=off)
    K = art.mm.MirrorConic(S, p, q, 90.0 - off / 2)
    Cc = np.asarray(E.get_centre(), dtype=float)
    n = np.asarray(E.get_normal(Cc), dtype=float)
    t = np.cross([0.0, 1.0, 0.0], n)
    cf = np.sqrt(E.a ** 2 - E.b ** 2)
    assert t.dot(np.array([-cf, 0.0, 0.0]) - Cc) < 0                # the object focus is the one at -x of the ellipse frame
    normal, major = np.array([-0.3, 0.2, 0.9]), np.array([0.9, 0.1, 0.3])
    normal /= np.linalg.norm(normal)
    major = major - major.dot(normal) * normal
    major /= np.linalg.norm(major)
    pos = np.array([300.0, -20.0, 40.0])
    oeE = moe.OpticalElement(E, pos, normal, major)
    fwd, _ = mgeo.frame_maps(oeE.normal, oeE.majoraxis)
    oeK = moe.OpticalElement(K, pos, fwd.T @ n, fwd.T @ t)
    F1 = pos + fwd.T @ (np.array([-cf, 0.0, 0.0]) - Cc)             # the object focus in the lab: a point source there
    m = 2053
    a_, b_ = qc._vogel(m, 0.05)
    axis = (pos - F1) / np.linalg.norm(pos - F1)
    e1 = np.cross(axis, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    V = axis[None, :] + a_[:, None] * e1 + b_[:, None] * e2
    rays = (np.tile(F1, (m, 1)), V / np.linalg.norm(V, axis=1)[:, None], np.zeros(m), qc._alive(m))
    src = upload(art, rays)
    ra = result(art.mp.RayTracingCalculation(src, [oeK])[0])
    rb = result(art.mp.RayTracingCalculation(src, [oeE])[0])
    assert np.array_equal(ra["alive"], rb["alive"]) and np.array_equal(rb["alive"], rays[3] != 0)
    worst = qc.assert_parity(ra, rb, rb["alive"], "conic ellipsoid against MirrorEllipsoidal")
    print(f"conic ellipsoid against MirrorEllipsoidal: worst {worst:.2e}")


# ------------------------------------------------------------------------------------------- 4. chains, every trace mode
@pytest.fixture(scope="module")
def kb_chains(art):
    """[Mask, elliptical cylinder, toroid, elliptical cylinder (crossed)]; the last distance is a loop list of two."""
    mask = art.mk.Mask(art.ms.SupportRoundHole(30.0, 1.5, 0.0, 0.0))
    A = art.mm.MirrorEllipticalCylinder(art.ms.SupportRectangle(200.0, 30.0), 1000.0, 2000.0, 3.0)
    R, r = art.mm.ReturnOptimalToroidalRadii(600.0, 87.0)
    T = art.mm.MirrorToroidal(R, r, art.ms.SupportRectangle(200.0, 30.0))
    B = art.mm.MirrorEllipticalCylinder(art.ms.SupportRectangle(200.0, 30.0), 1200.0, 800.0, 3.0)
    return art.mp.OEPlacement(_source(5e-3, 0), [mask, A, T, B], [400.0, 600.0, 200.0, [200.0, 210.0]],
                              [0.0, 87.0, 87.0, 87.0], [0.0, 0.0, 0.0, 90.0], "kb")


def test_chain_with_conics_in_every_trace_mode(art, kb_chains):
    ch = kb_chains[0]
    src, els = ch.source_rays, ch.optical_elements
    ref = stepwise(art, src, els)
    n_in, n_out = int((src.alive != 0).sum()), len(ref[-1])
    assert 0 < n_out < n_in                                           # the mask cuts, the mirrors pass
    for k, (a, b) in enumerate(zip(art.mp.RayTracingCalculation(src, els, history=True), ref)):
        assert same_bytes(a, b), f"history=True, element {k}"
    last = art.mp.RayTracingCalculation(src, els, history=False)
    assert last[:-1] == [None] * 3 and same_bytes(last[-1], ref[-1])
    lazy = art.mp.RayTracingCalculation(src, els, history="lazy")
    assert same_bytes(lazy[-1], ref[-1]) and same_bytes(lazy[1], ref[1]) and same_bytes(lazy[2], ref[2])
    prog = art.SceneProgram([src], [els])
    assert prog._stepwise and prog.graph is None
    for a, b in zip(prog.run()[0], ref):
        assert same_bytes(a, b)
    for a, b in zip(ch.get_output_rays(), ref):
        assert same_bytes(a, b)
    with pytest.raises(ValueError):
        art.SceneProgram([src], [els], history=False)


_ANA = {"verbose": False, "plot_Render": False, "plot_SpotDiagram": False, "plot_DelaySpotDiagram": False,
        "plot_IntensitySpotDiagram": False, "plot_IncidenceSpotDiagram": False, "plot_DelayGraph": False,
        "plot_IntensityGraph": False, "plot_IncidenceGraph": False, "plot_DelayMirrorProjection": False,
        "plot_IntensityMirrorProjection": False, "plot_IncidenceMirrorProjection": False, "DrawAiryAndFourier": True,
        "save_results": False}


def test_chain_list_through_artmain(art, kb_chains):
    import ARTmain
    assert len(kb_chains) == 2
    det = {"ReflectionNumber": -1, "ManualDetector": False, "DistanceDetector": 800.0, "AutoDetectorDistance": False,
           "OptFor": "intensity"}
    kept = ARTmain.main(list(kb_chains), _source(5e-3, 0), det, dict(_ANA))
    for k, ch in enumerate(kb_chains):
        ref = stepwise(art, ch.source_rays, ch.optical_elements)
        outs = kept["OpticalChain"][k].get_output_rays()
        assert same_bytes(outs[-1], ref[-1]) and same_bytes(outs[1], ref[1])
        assert np.isfinite(kept["SpotSizeSD"][k]) and np.isfinite(kept["DurationSD"][k])
        assert 0 < kept["ETransmission"][k] < 100
    assert not same_bytes(kb_chains[0].get_output_rays()[-1], kb_chains[1].get_output_rays()[-1])


def test_analyses_run_behind_conics(art, kb_chains):
    ch = kb_chains[0]
    last = ch.get_output_rays()[-1]
    det = art.mdet.Detector(np.asarray(ch.optical_elements[-1].position, dtype=float))
    det.autoplace(last, 800.0)
    pol = ch.get_Polarisation(art.coating.Coating.ideal(), Detector=det)
    assert pol.count == len(last) and abs(pol.t_min - 1) <= 1e-12 and abs(pol.t_max - 1) <= 1e-12
    wf = det.get_Wavefront(last, Order=4)
    assert np.isfinite(wf.rms)
    h = det.get_Histogram(last, Bins=16)
    assert int(h.counts.sum()) == len(last) and h.outside[0] == 0


# ------------------------------------------------------------------------------------------------- 5. refusals on the device
def test_other_entry_points_refuse_a_quadric_on_the_device(art):
    be, abi = art.be, art.abi
    oe, rays = SCENES["ellipsoid_45deg"]
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
    calls = {"art_trace_element": lambda: be.fn["art_trace_element"](C.byref(desc), C.byref(vin), C.byref(vout), n, sp),
             "art_trace_chain": lambda: be.fn["art_trace_chain"](darr, 1, C.byref(vin), varr, n, sp),
             "art_trace_grating": lambda: be.fn["art_trace_grating"](C.byref(desc), None, None, None, C.byref(vin), n, sp),
             "art_scene_pack": lambda: be.fn["art_scene_pack"](darr, 1, 1, (abi.ArtBundleView * 1)(vin), varr, None,
                                                               C.cast(image, C.c_void_p)),
             "art_trace_guides": lambda: be.fn["art_trace_guides"](darr, 1, guides.data_ptr(), galive.data_ptr(), sp)}
    for name, call in calls.items():
        assert call() == abi.ART_ERR_UNSUPPORTED, name
        assert "art_trace_quadric" in be.last_error(), name
    be.synchronize()
    assert bool((out.data == SENTINEL).all()) and bool((out.alive == 9).all())
    # a plain mirror in the same pose goes through art_trace_element as ever
    plane = qc.place(art.mm.MirrorPlane(oe.type.support), 400.0, 45.0)
    assert len(art.mp.RayTracingCalculation(src, [plane])[0]) > 0

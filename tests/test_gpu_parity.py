"""GPU (-m gpu): the HIP kernels, called through the C ABI (libart_hip.so via ctypes), against (i) the golden
vectors the reference produced and (ii) the CPU oracle on seeded inputs, plus size-independent properties at
BASELINE sizes.  Tolerances: survivor indices bit-exact; positions, directions, optical paths 1e-10 relative;
delays 1e-10 of the mean travel time (BASELINE.json north_star)."""
import numpy as np
import pytest

from conftest import chain_golden_names, load_golden, report
import parity_common as pc

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


@pytest.mark.parametrize("mode", ["element", "chain"])
@pytest.mark.parametrize("name", chain_golden_names())
def test_gpu_chain_matches_reference(hip, name, mode):
    import ART.ModuleProcessing as mp
    scene, a = load_golden(name)
    els = pc.build_elements(scene, a)
    src = pc.source_bundle(a, scene)
    out = mp.RayTracingCalculation(src, els, IgnoreDefects=scene.get("IgnoreDefects", True), mode=mode)
    w = pc.check_outputs(out, a, scene)
    _GOLDEN_WORST.setdefault(mode, {})
    for k, v in w.items():
        if v > _GOLDEN_WORST[mode].get(k, (0.0, ""))[0]:
            _GOLDEN_WORST[mode][k] = (v, name)


_GOLDEN_WORST = {}


def test_gpu_golden_summary(hip):
    """Not a check of its own: puts the worst errors of the golden chains (above) into the end-of-run summary."""
    for mode, w in _GOLDEN_WORST.items():
        report(f"[parity goldens, {mode} mode] " + "  ".join(f"{k} {v:.2e} ({n})" for k, (v, n) in sorted(w.items())))


@pytest.mark.parametrize("name", [n for n in chain_golden_names() if not n.startswith("frame_")])
def test_gpu_detector_matches_reference(hip, name):
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    import ART.ModuleAnalysisAndPlots as mplots
    scene, a = load_golden(name)
    if "detector" not in scene:
        pytest.skip("no detector in fixture")
    els = pc.build_elements(scene, a)
    src = pc.source_bundle(a, scene)
    last = mp.RayTracingCalculation(src, els, IgnoreDefects=scene.get("IgnoreDefects", True))[-1]
    d = scene["detector"]
    scale = max(1.0, np.abs(a["det_points3d"]).max())
    if name != "autofocus_c3":
        D = mdet.Detector(np.array(els[-1].position, float))
        D.autoplace(last, d["distance"])
        assert np.abs(D.centre - d["centre"]).max() <= 1e-10 * scale
        assert np.abs(D.normal - d["normal"]).max() <= 1e-10
    D = mdet.Detector(np.array(d["refpoint"]), np.array(d["centre"]), np.array(d["normal"]))
    assert np.abs(D.get_PointList3D(last) - a["det_points3d"]).max() <= 1e-10 * scale
    assert np.abs(D.get_PointList2D(last) - a["det_points2d"]).max() <= 1e-10 * scale
    assert np.abs(D.get_PointList2DCentre(last) - a["det_points2dcentre"]).max() <= 1e-10 * scale
    mean_t_fs = np.mean(D.get_OpticalPaths(last)) / mdet.LightSpeed * 1e15
    assert np.abs(D.get_Delays(last) - a["det_delays"]).max() <= 1e-10 * mean_t_fs
    spot, dur = mplots.GetResultSummary(D, last, False)
    assert abs(spot - scene["SpotSizeSD"]) <= 1e-9 * scale
    assert abs(dur - scene["DurationSD"]) <= 1e-10 * mean_t_fs
    assert abs(mplots.getETransmission(src, last) - scene["ETransmission"]) <= 1e-9


def _c3_chain(n, twist=30.0):
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    SourceProperties = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5,
                        "NumberRays": n}
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 41e-3 / 2 * 500, 0, 0))
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    return mp.OEPlacement(SourceProperties, [Mask, Tor, Tor], [500, 100, 600], [0, 80, -80], [0, 0, twist], "c3")


def test_gpu_vs_oracle_seeded_c3(hip):
    """1e5 seeded rays through the C3 scene: HIP vs the CPU oracle (same inputs)."""
    from oracle import art_oracle as orc
    n = 100_000
    chain = _c3_chain(n)
    out = chain.get_output_rays()
    src = chain.source_rays
    B = orc.make_bundle(src.data[0:3].cpu().numpy().T, src.data[3:6].cpu().numpy().T, np.arange(n),
                        src.intensity.cpu().numpy(), 50e-6)
    els = []
    for oe in chain.optical_elements:
        o = oe.type
        kind = "mask" if o.type == "Mask" else "torus"
        params = {"R": o.majorradius, "r": o.minorradius} if kind == "torus" else {}
        sk = {1: "roundhole", 2: "rect"}[o.support._abi_kind]
        els.append(orc.Element(orc.Optic(kind, orc.Support(sk, o.support._abi_params()), params, [], o.type),
                               np.asarray(oe.position, float), oe.normal, oe.majoraxis))
    ref = orc.ray_tracing_calculation(B, els)
    worst = [0.0, 0.0, 0.0]
    for o, q in zip(out, ref):
        assert np.array_equal(o.numbers(), q.number)
        scale = max(1.0, np.abs(q.point).max())            # 1e-10 of max|ref|, not of a fixed length
        e = (np.abs(o.points() - q.point).max() / scale, np.abs(o.vectors() - q.vector).max(),
             np.abs(o.paths_total() - q.path.sum(axis=1)).max() / q.path.sum(axis=1).mean())
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] <= 1e-10 and e[1] <= 1e-10 and e[2] <= 1e-10, e
    report(f"[parity c3 1e5 vs oracle] worst rel err: pos {worst[0]:.2e} dir {worst[1]:.2e} path {worst[2]:.2e}")


def test_gpu_full_size_properties(hip):
    """BASELINE size (1e7 rays, C3 scene): size-independent properties instead of a CPU comparison.
    (a) a contiguous sub-range traced alone gives bit-identical results to the same slots of the full run
        (rays are independent: sharding is exact); (b) survivors' directions are unit vectors; (c) every hit
        point of the last toroid lies on the torus implicit surface; (d) chain mode == element mode bitwise."""
    import torch
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd.bundle import RayBundle
    n = 10_000_000
    chain = _c3_chain(n)
    src = chain.source_rays
    els = chain.optical_elements
    out_c = mp.RayTracingCalculation(src, els, mode="chain")
    out_e = mp.RayTracingCalculation(src, els, mode="element")
    for a, b in zip(out_c, out_e):
        assert torch.equal(a.alive, b.alive)
        m = a.alive.bool()
        scale = max(1.0, float(b.data[0:3, m].abs().max()))
        assert float((a.data[0:3, m] - b.data[0:3, m]).abs().max()) <= 1e-13 * scale
        assert float((a.data[3:6, m] - b.data[3:6, m]).abs().max()) <= 1e-13
        assert float((a.data[6:8, m] - b.data[6:8, m]).abs().max()) <= 1e-13 * scale
    last = out_c[-1]
    m = last.alive.bool()
    assert abs(int(m.sum().item()) / n - 0.673) < 0.01      # SURVEY: mask passes 67.3 %
    d = last.data[3:6, m]
    assert float((d.pow(2).sum(0) - 1).abs().max()) < 1e-14
    # (a) shard [3e6, 4e6)
    lo, hi = 3_000_000, 4_000_000
    sub = RayBundle(src.data[:, lo:hi].contiguous(), src.alive[lo:hi].contiguous(), None,
                    src.intensity[lo:hi].contiguous(), src.wavelength, None, src.backend)
    out_s = mp.RayTracingCalculation(sub, els)
    assert torch.equal(out_s[-1].alive, last.alive[lo:hi])
    ms = out_s[-1].alive.bool()
    assert torch.equal(out_s[-1].data[:, ms], last.data[:, lo:hi][:, ms])
    # (c) implicit surface residual in the optic frame of the last toroid
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    oe = els[-1]
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    P = last.data[0:3, m][:, ::97].cpu().numpy().T
    Po = (P - np.asarray(oe.position, float)) @ fwd.T + oe.type.get_centre()
    R, r = oe.type.majorradius, oe.type.minorradius
    res = (np.sqrt(Po[:, 0] ** 2 + Po[:, 2] ** 2) - R) ** 2 + Po[:, 1] ** 2 - r ** 2
    assert np.abs(res).max() <= 1e-8        # ~ r * 2e-11 mm normal distance


def test_gpu_compaction_and_reductions(hip):
    import torch
    be = hip
    g = torch.Generator().manual_seed(3)
    for n in (1, 63, 64, 2048, 2049, 1_000_003):
        alive = (torch.rand(n, generator=g) < 0.37).to(torch.uint8).to(be.device)
        idx, c = be.compact(alive, n)
        ref = torch.nonzero(alive, as_tuple=False).reshape(-1)
        assert c == ref.numel()
        assert torch.equal(idx, ref)
    n = 1_000_003
    X = torch.randn(n, generator=g, dtype=torch.float64).to(be.device)
    Y = torch.randn(n, generator=g, dtype=torch.float64).to(be.device)
    O = (torch.rand(n, generator=g, dtype=torch.float64) + 1000).to(be.device)
    W = torch.rand(n, generator=g, dtype=torch.float64).to(be.device)
    s = be.detector_stats(alive, X, Y, O, W, n)
    m = alive.bool()
    assert s[0] == int(m.sum())
    assert abs(s[1] - float(O[m].sum())) <= 1e-12 * abs(float(O[m].sum()))
    assert s[2] == float(X[m].min()) and s[3] == float(X[m].max())
    assert s[4] == float(Y[m].min()) and s[5] == float(Y[m].max())
    assert abs(s[9] - float((W * X)[m].sum())) <= 1e-10 * float((W * X.abs())[m].sum())
    assert abs(s[11] - float((W * O)[m].sum())) <= 1e-12 * float((W * O)[m].sum())
    mo = be.detector_moments(alive, X, Y, O, W, n, 0.1, -0.2, 1000.5)
    assert abs(mo[1] - float((W * (X - 0.1) ** 2)[m].sum())) <= 1e-11 * mo[1]
    assert abs(mo[3] - float((W * (O - 1000.5) ** 2)[m].sum())) <= 1e-11 * mo[3]
    s2 = be.detector_stats(alive, X, Y, O, W, n)
    assert np.array_equal(s, s2), "reductions must be deterministic"

    # n == 0 through the raw ABI (the wrappers return early): the exact bytes each entry writes for an empty bundle
    import ctypes as C
    from attosecondraytracing_amd import _abi
    from attosecondraytracing_amd.bundle import RayBundle
    sp, red = be.stream_ptr(), be._red_scratch().data_ptr()
    bundle, alive0, w_out = RayBundle.allocate(1, backend=be), be.zeros(1, torch.uint8), be.empty(1)
    d, view = _abi.ArtDetectorDesc(), bundle.view()
    axis = (C.c_double * 3)(0.0, 0.0, 1.0)
    ident = [np.inf if k in (2, 4, 12) else (-np.inf if k in (3, 5, 13) else 0.0) for k in range(24)]

    def empty_call(size, call):
        out = torch.full((size,), float("nan"), dtype=torch.float64, device=be.device)
        assert call(out.data_ptr()) == _abi.ART_OK
        return out.cpu().numpy().view(np.uint64)

    bits = lambda v: np.asarray(v, dtype=np.float64).view(np.uint64)
    a0 = alive0.data_ptr()
    assert np.array_equal(empty_call(16, lambda o: be.fn["art_detector_stats"](a0, None, None, None, None, 0, red, o, sp)),
                          bits(ident[:16]))
    assert np.array_equal(empty_call(24, lambda o: be.fn["art_detector_readout"](
        C.byref(d), C.byref(_abi.ArtBundleView()), None, 0, 0.0, 0.0, 0.0, None, None, None, None, None, None, red, o, sp)),
        bits(ident))
    assert np.array_equal(empty_call(8, lambda o: be.fn["art_detector_moments"](a0, None, None, None, None, 0, 0.0, 0.0, 0.0,
                                                                                  red, o, sp)), bits(np.zeros(8)))
    assert np.array_equal(empty_call(8, lambda o: be.fn["art_bundle_sums"](C.byref(view), None, 0, red, o, sp)),
                          bits(np.zeros(8)))
    assert np.array_equal(empty_call(33, lambda o: be.fn["art_detector_scan_moments"](
        C.byref(d), C.byref(_abi.ArtBundleView()), None, 0, 0.0, 0.0, red, o, sp)), bits(np.zeros(33)))
    assert np.array_equal(empty_call(2, lambda o: be.fn["art_bundle_max_angle"](C.byref(view), axis, 0, red, o, sp)),
                          bits(np.zeros(2)))
    assert be.fn["art_gaussian_intensity"](C.byref(view), axis, 0.5, 0, red, w_out.data_ptr(), sp) == _abi.ART_OK


def test_gpu_sources_match_oracle(hip):
    import ART.ModuleSource as msource
    from oracle import art_oracle as orc
    n = 20000
    S = np.array([1.0, -2.0, 3.0])
    ax = np.array([0.3, -0.2, 0.9])
    b = msource.ApplyGaussianIntensityToRayList(msource.PointSource(S, ax, 0.05, n, 50e-6))
    q = orc.apply_gaussian_intensity(orc.point_source(S, ax, 0.05, n))
    assert np.abs(b.points() - q.point).max() <= 1e-12
    assert np.abs(b.vectors() - q.vector).max() <= 1e-12
    assert np.abs(b.intensities() - q.intensity).max() <= 1e-10
    b = msource.ApplyGaussianIntensityToRayList(msource.PlaneWaveDisk(S, ax, 12.0, n, 50e-6))
    q = orc.apply_gaussian_intensity(orc.plane_wave_disk(S, ax, 12.0, n))
    assert len(b) == n - 1
    assert np.abs(b.points() - q.point).max() <= 1e-10 * 12
    assert np.abs(b.vectors() - q.vector).max() <= 1e-12
    assert np.abs(b.intensities() - q.intensity).max() <= 1e-10


def test_gpu_strided_source_shards(hip):
    """art_make_source_strided: rank r's strided shard of a source is every world-th ray of the full source, bit for bit."""
    import torch
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd import sharding, ModuleGeometry as mgeo
    n_total, world = 1_000_003, 4
    rot = mgeo.rotation_matrix(np.array([0.0, 0.0, 1.0]), np.array([0.3, -0.5, 0.8]))
    for kind, size in ((0, 0.03), (1, 12.0)):
        full = RayBundle.allocate(n_total, backend=hip)
        hip.make_source(kind, size, rot, np.array([1.0, 2.0, 3.0]), 0, n_total, n_total, full.view())
        for rk in range(world):
            first, step, n = sharding.shard_spec(n_total, rk, world, "strided")
            part = RayBundle.allocate(n, backend=hip)
            hip.make_source(kind, size, rot, np.array([1.0, 2.0, 3.0]), first, n, n_total, part.view(), step=step)
            assert torch.equal(part.data[0:7], full.data[0:7, rk::world]) and bool(part.alive.all())
    with pytest.raises(RuntimeError):
        hip.make_source(0, 0.03, rot, np.zeros(3), 3, 10, 39, RayBundle.allocate(10, backend=hip).view(), step=4)   # 3 + 9*4 = 39 is not < 39


def test_gpu_extended_source_matches_reference(hip):
    """ExtendedSource on the device (art_make_extended_source) against the reference's list, numbering included."""
    import ART.ModuleSource as msource
    _, a = load_golden("geometry_units")
    b = msource.ExtendedSource(np.array([0.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]), 0.1, 0.02, 9000)
    b = msource.ApplyGaussianIntensityToRayList(b, 1 / np.e ** 2)
    assert np.array_equal(b.numbers(), a["src_extended_number"])
    assert np.abs(b.points() - a["src_extended_point"]).max() <= 1e-12
    assert np.abs(b.vectors() - a["src_extended_vector"]).max() <= 1e-13
    assert np.abs(b.intensities() - a["src_extended_intensity"]).max() <= 1e-11


def test_gpu_fuzz_differential(hip):
    """300 random scenes (every optic x aperture kind, arbitrary poses) on the GPU against the pinned oracle."""
    import fuzz_common as fz
    st = {}
    res = fz.run_differential(list(range(300)) + list(fz.REGRESSION_SEEDS), stats=st)     # (seed 65 is in range(300) too)
    assert res["scenes_with_hits"] >= 250, res
    report(f"[gpu fuzz, {st['scenes']} scenes] local error vs long-double truth: " + "  ".join(f"{k} {v:.1e}" for k, v in st["local_worst"].items())
           + f"; adjudicated by truth: seeds {sorted(set(st['adjudicated_seeds']))}, product {st['adjudicated_worst']['product']:.1e} vs oracle "
           f"{st['adjudicated_worst']['oracle']:.1e}")
    assert fz.run_detector_fuzz(range(150)) >= 200
    fz.run_source_fuzz(range(100))


def test_gpu_exchange_kernels(hip):
    """art_exchange_pack / art_exchange_fold (the per-step multi-GPU exchange) against torch, incl. a fold over
    several fake ranks."""
    import torch
    from attosecondraytracing_amd import sharding, _lib
    be = _lib.get_backend()
    n = 100_003
    g = torch.Generator(device="cpu").manual_seed(5)
    X, Y, O = (torch.randn(n, generator=g, dtype=torch.float64).to(be.device) for _ in range(3))
    alive = (torch.rand(n, generator=g) > 0.3).to(torch.uint8).to(be.device)
    stats = torch.randn(24, generator=g, dtype=torch.float64).to(be.device)
    ex = sharding.Exchange(be, n, sample=1000)
    st, smp = ex(stats, X, Y, O, alive)
    assert torch.equal(st, stats) and smp.shape == (1, ex.k, 4) and ex.k == 1000
    ref = torch.stack([X[ex.slots], Y[ex.slots], O[ex.slots], alive[ex.slots].to(torch.float64)], dim=1)
    assert torch.equal(smp[0], ref)
    ex0 = sharding.Exchange(be, n, sample=0)            # statistics only
    st0, smp0 = ex0(stats, X, Y, O, alive)
    assert torch.equal(st0, stats) and smp0.shape == (1, 0, 4)
    # fold over 5 fake ranks
    world, stride = 5, 24 + 8
    recv = torch.randn(world * stride, generator=g, dtype=torch.float64).to(be.device)
    out = torch.empty(24, dtype=torch.float64, device=be.device)
    be.exchange_fold(recv, world, stride, out)
    allv = recv.view(world, stride)[:, :24].cpu()
    want = allv[0].clone()
    for r in range(1, world):
        want = want + allv[r]
    for sl in (2, 4, 12):
        want[sl] = allv[:, sl].min()
    for sl in (3, 5, 13):
        want[sl] = allv[:, sl].max()
    assert torch.equal(out.cpu(), want)
    with pytest.raises(RuntimeError):
        be.exchange_fold(recv, 0, stride, out)
    # a shard above 2^24 slots (a float32 linspace of sample slots rounds n-1 up to n there): the last sampled slot is
    # n-1, and the packed sample is exactly those slots
    del X, Y, O, alive
    n = 2 ** 25 + 3
    X = torch.arange(n, dtype=torch.float64, device=be.device)
    alive = torch.ones(n, dtype=torch.uint8, device=be.device)
    ex = sharding.Exchange(be, n, sample=20000)
    assert int(ex.slots[-1]) == n - 1 and int(ex.slots.max()) < n and ex.k == 20000
    st, smp = ex(stats, X, X, X, alive)
    assert torch.equal(smp[0][:, 0], ex.slots.to(torch.float64)) and bool((smp[0][:, 3] == 1).all())
    # empty and all-dead shards give the reduction identities, which fold away
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd.bundle import RayBundle
    D = mdet.Detector(np.zeros(3), np.array([0.0, 0.0, 10.0]), np.array([0.0, 0.0, -1.0]))
    dead = RayBundle.allocate(1000, backend=be)
    dead.data.zero_()
    dead.alive.zero_()
    for B in (dead, RayBundle.allocate(0, backend=be)):
        s = D.readout(B)["stats"]
        assert s[0] == 0 and s[1] == 0 and s[2] == np.inf and s[3] == -np.inf and s[12] == np.inf and s[13] == -np.inf
    both = torch.cat([torch.as_tensor(s, device=be.device), stats])
    be.exchange_fold(both, 2, 24, out)
    want = stats.clone()
    assert torch.equal(out[[2, 3, 4, 5, 12, 13]], want[[2, 3, 4, 5, 12, 13]]) and out[0] == want[0]


def test_gpu_plain_c_consumer_of_the_abi(hip, tmp_path):
    """examples/c_abi_demo.c: gcc (C, not C++), the HIP runtime for memory, include/art_hip.h for everything else --
    no Python and no PyTorch between the caller and libart_hip.so."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = "/opt/rocm"
    if not (shutil.which("gcc") and os.path.isdir(rocm + "/include/hip")):
        pytest.skip("gcc or the HIP headers are not available")
    exe = str(tmp_path / "c_abi_demo")
    lib = os.path.join(root, "attosecondraytracing_amd", "libart_hip.so")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_abi_demo.c"),
                           "-L" + rocm + "/lib", "-lamdhip64", lib, "-lm", "-Wl,-rpath," + rocm + "/lib", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "C_ABI_DEMO_OK" in r.stdout, r.stdout + r.stderr


def test_gpu_step_captured_in_a_hip_graph(hip):
    """A trace + read-out step captured with graph.CapturedStep replays to the same bits as eager launches, and a
    replay picks up rays written in place into the captured source bundle."""
    import torch
    import bench
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd import _lib
    from attosecondraytracing_amd.graph import CapturedStep
    be = _lib.get_backend()
    n = 50_000
    chain, _ = bench.build_scene(3)
    els = chain.optical_elements
    src = bench.device_source(n, 0, n, be)
    det = mdet.Detector(np.asarray(els[-1].position, dtype=float))
    det.autoplace(mp.RayTracingCalculation(src, els)[-1], 600.0)

    def step():
        o = mp.RayTracingCalculation(src, els)
        return o, det.readout(o[-1], sync=False)

    o, r = step()
    want_stats, want_X = r["stats_dev"].clone(), r["X"].clone()
    cap = CapturedStep(step)
    go, gr = cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(gr["stats_dev"], want_stats) and torch.equal(gr["X"], want_X)
    assert torch.equal(go[0].data, o[0].data) and torch.equal(go[-1].alive, o[-1].alive)
    # other rays through the same captured scene: every second ray switched off in place
    src.alive[::2] = 0
    cap.replay()
    torch.cuda.synchronize()
    assert int(gr["stats_dev"][0].item()) == n // 2
    eager = step()[1]["stats_dev"]
    assert torch.equal(gr["stats_dev"], eager)


def test_gpu_error_paths(hip):
    """Bad arguments come back as error codes with a message, never as a crash."""
    import ctypes as C
    from attosecondraytracing_amd import _abi
    be = hip
    d = _abi.ArtElementDesc()
    d.kind = 99
    v = _abi.ArtBundleView()
    rc = be.fn["art_trace_element"](C.byref(d), C.byref(v), C.byref(v), 10, None)
    assert rc == _abi.ART_ERR_BAD_ARG and b"kind" in be.fn["art_last_error"]()
    d.kind = 0
    rc = be.fn["art_trace_element"](C.byref(d), C.byref(v), C.byref(v), 10, None)
    assert rc == _abi.ART_ERR_BAD_ARG


def test_gpu_smoke_entry(hip):
    import __graft_entry__ as g
    g.smoke()


def test_gpu_oeplacement_and_sources_match_reference(hip):
    """Scene construction end to end on the GPU (device-generated sources + device Gaussian weights + 1-ray
    alignment traces) against the reference's poses and source bundles."""
    import ART.ModuleProcessing as mp
    for name in ("c1_singleparabola", "c2_fxf_chain05", "c3_twisted_chain09", "c4_mixed8", "c5_zernike_withdefects"):
        scene, a = load_golden(name)
        pl = scene.get("placement") or scene.get("placement_before_roll")
        optics = [pc.build_optic(e, a) for e in scene["elements"]]
        SP = dict(pl["SourceProperties"])
        SP["NumberRays"] = int(SP["NumberRays"])
        chain = mp.OEPlacement(SP, optics, list(pl["DistanceList"]), list(pl["IncidenceAngleList"]),
                               list(pl["IncidencePlaneAngleList"]), "t")
        if "placement" in scene:
            for oe, e in zip(chain.optical_elements, scene["elements"]):
                scale = max(1.0, np.abs(np.array(e["position"])).max())
                assert np.abs(np.asarray(oe.position, float) - e["position"]).max() <= 1e-10 * scale
                assert np.abs(oe.normal - e["normal"]).max() <= 1e-10
                assert np.abs(oe.majoraxis - e["majoraxis"]).max() <= 1e-10
        src = chain.source_rays
        assert np.array_equal(src.numbers(), a["src_number"])
        assert np.abs(src.points() - a["src_point"]).max() <= 1e-10 * max(1.0, np.abs(a["src_point"]).max())
        assert np.abs(src.vectors() - a["src_vector"]).max() <= 1e-12
        assert np.abs(src.intensities() - a["src_intensity"]).max() <= 1e-10


def test_gpu_autofocus_matches_reference(hip):
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    scene, a = load_golden("autofocus_c3")
    els = pc.build_elements(scene, a)
    last = mp.RayTracingCalculation(pc.source_bundle(a, scene), els)[-1]
    d = scene["detector"]
    det = mdet.Detector(np.array(d["refpoint"]), np.array(d["centre"]), np.array(d["normal"]))
    for key, (dist, spot, dur) in scene["autofocus"].items():
        optfor, weighted = key.rsplit("_", 1)
        D, s, t = mp.FindOptimalDistance(det, last, optfor, None, 3, bool(int(weighted)), False)
        assert abs(D.get_distance() - dist) <= 1e-9 * dist, key
        if not np.isnan(spot):
            assert abs(s - spot) <= 1e-9 * max(spot, 1e-3), key
        assert abs(t - dur) <= 1e-7 * max(dur, 1e-3), key


def test_gpu_edge_cases(hip):
    import edge_cases
    edge_cases.run_edge_cases()


def test_gpu_launch_chunking(hip, monkeypatch):
    import edge_cases
    edge_cases.run_chunking(monkeypatch.setenv)
    edge_cases.run_readout_chunking(monkeypatch.setenv)


def test_gpu_source_misalignment_helpers(hip):
    """shift_source / tilt_source (ART/ModuleOpticalChain.py:219-369) go through art_transform_bundle."""
    import ART.ModuleOpticalChain as moc
    scene, a = load_golden("c2_fxf_chain05")
    chain = moc.OpticalChain(pc.source_bundle(a, scene), pc.build_elements(scene, a), "misalign")
    p0, v0 = chain.source_rays.points(), chain.source_rays.vectors()
    chain.shift_source(np.array([0.0, 0.0, 2.0]), 0.5)
    assert np.abs(chain.source_rays.points() - (p0 + [0, 0, 0.5])).max() <= 1e-15
    assert np.abs(chain.source_rays.vectors() - v0).max() <= 5e-16    # re-normalised like the Ray setter
    chain.tilt_source(np.array([0.0, 1.0, 0.0]), 0.1)
    th = np.deg2rad(0.1)
    Rm = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    assert np.abs(chain.source_rays.vectors() - v0 @ Rm.T).max() <= 1e-15
    assert np.abs(chain.source_rays.points() - (p0 + [0, 0, 0.5])).max() <= 1e-15     # tilt leaves origins alone
    assert len(chain.get_output_rays()[-1]) > 0


def _oracle_elements(chain):
    """Oracle description of the product's elements (kinds, parameters, supports, Zernike defects, poses)."""
    from oracle import art_oracle as orc
    kinds = {0: "plane", 1: "sphere", 2: "parabola", 3: "torus", 4: "ellipsoid", 5: "cylinder", 6: "mask"}
    sups = {0: "round", 1: "roundhole", 2: "rect", 3: "recthole", 4: "rectrecthole"}
    els = []
    for oe in chain.optical_elements:
        o = oe.type
        base = getattr(o, "Mirror", o)
        kind = kinds[o._abi_kind]
        params = {}
        if kind in ("sphere", "cylinder"):
            params = {"R": base.radius}
        elif kind == "parabola":
            params = {"feff": base.feff, "offaxis_rad": base.offaxisangle, "p": base.p}
        elif kind == "torus":
            params = {"R": base.majorradius, "r": base.minorradius}
        elif kind == "ellipsoid":
            params = {"a": base.a, "b": base.b, "offaxis_rad": base._offaxisangle}
        defects = [orc.ZernikeDefect(dict(d.coefficients), d.R) for d in getattr(o, "DeformationList", [])]
        els.append(orc.Element(orc.Optic(kind, orc.Support(sups[o.support._abi_kind], o.support._abi_params()), params,
                                         defects, o.type), np.asarray(oe.position, float), oe.normal, oe.majoraxis))
    return els


@pytest.mark.parametrize("scene", ["c3", "mixed8", "c5_zernike"])
def test_gpu_full_size_sampled_against_oracle(hip, scene):
    """BASELINE sizes (1e7 / 1.25e7 rays): 20 000 randomly chosen slots of the full-size GPU run against the CPU
    oracle tracing exactly those rays (rays are independent, so a slot-wise comparison is exact) -- catches
    indexing, stride and launch-geometry errors that small cases cannot."""
    import torch
    import ART.ModuleProcessing as mp
    from oracle import art_oracle as orc
    sys_path = __import__("sys").path
    root = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    if root not in sys_path:
        sys_path.insert(0, root)
    from tools import sweep
    ignore = True
    if scene == "c3":
        chain = _c3_chain(10_000_000)
        src = chain.source_rays
    elif scene == "mixed8":
        els, div = sweep.scene_mixed8(0)
        src = sweep.point_source(12_500_000, div, hip)

        class _C:  # minimal holder
            optical_elements = els
        chain = _C()
    else:
        class _C:
            optical_elements = sweep.scene_c5(0, False)
        chain = _C()
        src = sweep.plane_source(10_000_000, 20.0, hip)
        ignore = False
    out = mp.RayTracingCalculation(src, chain.optical_elements, IgnoreDefects=ignore)
    n = src.n_slots
    rng = np.random.default_rng(123)
    slots = np.sort(rng.choice(n, 20_000, replace=False))
    st = torch.from_numpy(slots).to(hip.device)
    host = src.data.index_select(1, st).cpu().numpy()
    B = orc.make_bundle(host[0:3].T, host[3:6].T, slots, np.ones(len(slots)))
    ref = orc.ray_tracing_calculation(B, _oracle_elements(chain), IgnoreDefects=ignore)
    worst = [0.0, 0.0, 0.0, 0.0]
    for o, q in zip(out, ref):
        alive = o.alive.index_select(0, st).cpu().numpy().astype(bool)
        assert np.array_equal(slots[alive], q.number), "survivors differ on the sampled slots"
        d = o.data.index_select(1, st).cpu().numpy()[:, alive]
        scale = max(1.0, np.abs(q.point).max())            # 1e-10 of max|ref|: ~25-100 mm for C5
        e = (np.abs(d[0:3].T - q.point).max() / scale, np.abs(d[3:6].T - q.vector).max(),
             np.abs(d[6] - q.path.sum(axis=1)).max() / max(q.path.sum(axis=1).mean(), 1.0),
             np.abs(d[7] - q.incidence).max())
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] <= 1e-10, f"position error {e[0]:.3e} of max|ref| = {scale:.1f} mm"
        assert e[1] <= 1e-10, f"direction error {e[1]:.3e}"
        assert e[2] <= 1e-10, f"path error {e[2]:.3e}"
        assert e[3] <= 1e-9, f"incidence error {e[3]:.3e}"
    report(f"[parity {scene} full size, 20000 slots vs oracle] worst rel err: pos {worst[0]:.2e} dir {worst[1]:.2e} "
          f"path {worst[2]:.2e} inc {worst[3]:.2e} rad")
    assert len(ref[-1]) > 5_000


@pytest.mark.parametrize("name", ["c2_fxf_chain05", "c3_twisted_chain04"])
def test_gpu_torus_hit_distance_vs_long_double_truth(hip, name):
    """The kernels' hardware-seeded reciprocal / rsqrt paths against an 80-bit truth (tests/test_accuracy_truth.py)."""
    from test_accuracy_truth import check_against_truth
    check_against_truth(name)


@pytest.mark.parametrize("name", chain_golden_names())
def test_gpu_every_element_vs_long_double_truth(hip, name):
    """Every optic kind, the deformations and the reflection of the HIP kernels against tests/truth_common.py."""
    from test_accuracy_truth import check_every_element_against_truth
    check_every_element_against_truth(name)


# ------------------------------------------------------------------------------------------------ scene table
def test_gpu_batched_loop_lists_match_reference(hip):
    """Many chains in ONE launch (art_scene_pack / art_trace_scene): the reference's loop-list chains C2 (chains 0/5/10
    of 11) and C3 (chains 0/4/9 of 10, ART/ModuleProcessing.py:203-239) from one batched call each, against their
    fixtures and bit-for-bit against the single-chain launches."""
    import scene_cases
    for names in (("c2_fxf_chain00", "c2_fxf_chain05", "c2_fxf_chain10"),
                  ("c3_twisted_chain00", "c3_twisted_chain04", "c3_twisted_chain09")):
        w = scene_cases.run_batched_goldens(names)
        report(f"[parity batched {names[0][:2]}] worst rel err: " + " ".join(f"{k} {v:.2e}" for k, v in w.items()))


def test_gpu_batched_variants(hip):
    import scene_cases
    scene_cases.run_batched_variants()


def test_gpu_scene_program_replays(hip):
    """graph.SceneProgram: pose updates rewrite the device-resident table, the captured HIP graph is replayed."""
    import scene_cases
    scene_cases.run_program_updates()
    scene_cases.run_program_history_off()
    scene_cases.run_chain_list_cache()


def test_gpu_scene_program_placement_look_is_opt_in_and_bounded(hip, monkeypatch):
    """graph.SceneProgram._tune_placement: off by default; when asked for, the program times its own launch into a few
    candidate allocations of its output bundles and keeps the fastest (the first one unless another is 3 % faster) --
    same results bit for bit; a failed allocation or a memory cap ends the look with what there is."""
    import torch
    import bench
    from attosecondraytracing_amd.graph import SceneProgram
    chain, _ = bench.build_scene(3)
    els = chain.optical_elements
    n = 2_000_000                                        # 3 x 65 B x 2e6 = 390 MB of outputs: above the look's threshold
    src = bench.device_source(n, 0, n, hip)
    monkeypatch.delenv("ART_PLACEMENT_TRIES", raising=False)
    first = SceneProgram([src], [els])
    assert first.placement is None                       # default: the first allocation, no look
    ref = [(b.alive.clone(), b.data.clone()) for b in first.run()[0]]

    def same(prog):
        outs = prog.run()[0]
        torch.cuda.synchronize()
        for (al, da), y in zip(ref, outs):
            assert torch.equal(al, y.alive) and torch.equal(da.view(torch.int64), y.data.view(torch.int64))

    tuned = SceneProgram([src], [els], placement_tries=4)
    pl = tuned.placement
    assert pl["tries"] == 4 and len(pl["launch_ms"]) == 4 and pl["allocation_failed"] is False
    assert pl["launch_ms"][pl["chosen"]] <= 1.03 * min(pl["launch_ms"]) and pl["gain_vs_first"] >= 1.0
    assert pl["passes"] in (1, 2)
    same(tuned)
    # the environment switch does the same
    monkeypatch.setenv("ART_PLACEMENT_TRIES", "2")
    assert SceneProgram([src], [els]).placement["tries"] == 2
    monkeypatch.delenv("ART_PLACEMENT_TRIES")
    # a memory cap below one candidate: no look, first block kept
    monkeypatch.setenv("ART_PLACEMENT_MEM_CAP", "1000000")
    capped = SceneProgram([src], [els], placement_tries=4)
    assert capped.placement["tries"] == 1 and capped.placement["chosen"] == 0
    same(capped)
    monkeypatch.delenv("ART_PLACEMENT_MEM_CAP")
    # the third candidate's allocation fails: the look goes on with two
    real, calls = SceneProgram._alloc_outputs, {"n": 0}

    def failing(self):
        calls["n"] += 1
        if calls["n"] >= 3:
            raise torch.OutOfMemoryError("no room (test)")
        return real(self)

    monkeypatch.setattr(SceneProgram, "_alloc_outputs", failing)
    short = SceneProgram([src], [els], placement_tries=4)
    assert short.placement["tries"] == 2 and short.placement["allocation_failed"] is True
    same(short)
    monkeypatch.setattr(SceneProgram, "_alloc_outputs", real)
    small = SceneProgram([bench.device_source(1000, 0, 1000, hip)], [els], placement_tries=4)
    assert small.placement is None                       # small bundles are not worth the look


def test_gpu_scene_grid_shapes_give_identical_results(hip, monkeypatch):
    """A scene whose chains share their input is launched chain-interleaved (grid (chains, tiles)), with the input loaded
    through the caches while it fits them; ART_SCENE_ORDER / ART_SCENE_KEEP force the other forms: all three give the same
    bundles and read-outs bit for bit (the grid shape and the cache policy change the dispatch order, not the work), for an
    odd ray count, chains with a mask (two-rays-per-lane body) and without (one-ray body), with fused read-outs."""
    import torch
    import bench
    import ART.ModuleDetector as mdet
    import ART.ModuleProcessing as mp
    lists_m, kind_m, dist_m = bench.scene_c3()                      # mask + 2 toroids, 10 chains
    relay, _ = bench.build_scene(3)
    lists_p = [relay.optical_elements] * 4                          # no mask: the one-ray body, 4 chains
    for lists, kind, dist, n in ((lists_m[:5], kind_m, dist_m, 300_001), (lists_p, ("point", 0.02), 600.0, 200_003)):
        src = bench.device_source(n, 0, n, hip, kind)
        dets = []
        for els in lists:
            d = mdet.Detector(np.asarray(els[-1].position, dtype=float))
            d.autoplace(mp.RayTracingCalculation(src, els, history=False)[-1], dist)
            dets.append(d)
        ref = None
        for order, keep in (("tile", "0"), ("chain", "0"), ("chain", "1")):
            monkeypatch.setenv("ART_SCENE_ORDER", order)
            monkeypatch.setenv("ART_SCENE_KEEP", keep)
            outs = mp.RayTracingCalculationMany([src] * len(lists), lists, detectors=dets)
            got = [(b.alive.clone(), b.data.clone()) for o in outs for b in o]
            ros = [torch.stack([d.readout(o[-1], sync=False)[k] for k in ("X", "Y", "opl")]).clone() for d, o in zip(dets, outs)]
            stats = [d.readout(o[-1], sync=False)["stats_dev"].clone() for d, o in zip(dets, outs)]
            if ref is None:
                ref = (got, ros, stats)
                continue
            for (a0, d0), (a1, d1) in zip(ref[0], got):
                live = a0.bool()
                assert torch.equal(a0, a1) and torch.equal(d0[:, live].view(torch.int64), d1[:, live].view(torch.int64)), (order, keep)
            for r0, r1, o in zip(ref[1], ros, outs):
                live = o[-1].alive.bool()
                assert torch.equal(r0[:, live].view(torch.int64), r1[:, live].view(torch.int64)), (order, keep)
            for s0, s1 in zip(ref[2], stats):
                assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)), (order, keep)      # same partials, same fold order


def test_gpu_list_analysis(hip):
    """ARTmain.analyse_chain_list on the device (art_analyse_bundles, blockIdx.y = chain): ONE analysis call and one copy
    back for a whole loop list; identical to run_ART chain by chain; against the per-ray read-out reduced on the host."""
    import scene_cases
    scene_cases.run_list_analysis(rays=200_003)


@pytest.mark.parametrize("name", ["analysis_c2", "analysis_c3"])
def test_gpu_list_analysis_matches_the_reference_for_every_chain(hip, name):
    """art_analyse_bundles + the moment-form autofocus against the reference's FindOptimalDistance / GetResultSummary /
    getETransmission for all 11 C2 and all 10 C3 chains (fixtures from the reference itself, not from the twin)."""
    import scene_cases
    w = scene_cases.run_analysis_goldens(name)
    report(f"[analysis goldens {name}] vs the reference, worst over all chains: " + "  ".join(f"{k} {float(v):.1e}" for k, v in w.items()))


def test_gpu_analysis_rows_match_numpy(hip):
    """Every slot of art_analyse_bundles' output rows (sums, placed detector, 32 moments, kink shifts, largest angle,
    bounding box) against a PURE-NumPy restatement of the reference's definitions (oracle/art_oracle.py: detector_autoplace,
    analysis_row -- ART/ModuleDetector.py:109-137, :191-279, ART/ModuleProcessing.py:464-482, :536-566; no kernel code on
    that side), for an auto-placed, a manual and a sums-only job, odd ray count."""
    import torch
    import bench
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd import _abi, analysis
    from oracle import art_oracle as orc
    lists, kind, dist = bench.scene_c3()
    n = 100_003
    src = bench.device_source(n, 0, n, hip, kind)
    src.intensity = torch.rand(n, dtype=torch.float64, device=hip.device) + 0.5
    B = mp.RayTracingCalculation(src, lists[3])[-1]
    det = mdet.Detector(np.asarray(lists[3][-1].position, dtype=float))
    det.autoplace(B, dist)
    man = det.copy_detector()
    man.shiftByDistance(3.0)
    reqs = [(B, _abi.ART_JOB_AUTOPLACE, dist), (B, _abi.ART_JOB_MANUAL, man), (src, _abi.ART_JOB_SUMS, None)]
    rows = hip.analyse_bundles([analysis._job(b, m_, a_) for b, m_, a_ in reqs], n).cpu().numpy()

    def oracle_bundle(b):
        a = b.alive.bool().cpu().numpy()
        d = b.data.cpu().numpy()
        return orc.make_bundle(d[0:3].T[a], d[3:6].T[a], np.nonzero(a)[0], b.intensity.cpu().numpy()[a], 50e-6), d[6][a]
    for j, (b, mode, arg) in enumerate(reqs):
        g = rows[j]
        Bo, path = oracle_bundle(b)
        Bo.path = path[:, None]
        assert g[0] == len(Bo) > 0
        if j == 2:
            r = orc.analysis_row(Bo, orc.Detector(np.zeros(3), np.array([0.0, 0.0, 1.0]), np.zeros(3)), 0.0)
            assert np.abs(g[1:4] - r["sum_point"]).max() <= 1e-12 * g[0] * 2000.0 and np.abs(g[4:7] - r["sum_vector"]).max() <= 1e-12 * g[0]
            assert abs(g[7] - r["sum_w"]) <= 1e-12 * r["sum_w"]
            assert not g[10:53].any() and g[53] == -np.inf and g[54] == np.inf
            continue
        # the detector: placed like Detector.autoplace (oracle: detector_autoplace), or the manual one, bit for bit
        Do = orc.detector_autoplace(Bo, dist) if mode == _abi.ART_JOB_AUTOPLACE else orc.Detector(man.centre, man.normal, man.refpoint)
        assert np.abs(g[10:13] - Do.centre).max() <= 1e-11 * 2000.0 and np.abs(g[13:16] - Do.normal).max() <= 1e-12
        assert np.abs(g[16:19] - Do.refpoint).max() <= 1e-11 * 2000.0
        # everything else on the DEVICE's detector and centres (a provisional centre is a free parameter of the sums): the
        # path about co = g[19], X and Y about the mean ray's hit (g[62], g[63]) -- exactly 0 when auto-placing
        Dg = orc.Detector(g[10:13].copy(), g[13:16].copy(), g[16:19].copy())
        r = orc.analysis_row(Bo, Dg, g[19], cxy=g[62:64])
        assert (mode != _abi.ART_JOB_AUTOPLACE or not g[62:64].any()) and np.abs(g[62:64]).max() <= 1e-3
        assert abs(g[19] - r["mean_opl"]) <= 0.5                                  # the path centre is near the mean path
        assert np.abs(g[1:4] - r["sum_point"]).max() <= 1e-12 * g[0] * 2000.0 and np.abs(g[4:7] - r["sum_vector"]).max() <= 1e-12 * g[0]
        assert abs(g[7] - r["sum_w"]) <= 1e-12 * r["sum_w"] and abs(g[8] - r["sum_path"]) <= 1e-12 * r["sum_path"]
        span = max(abs(g[56:60]).max(), 1e-3)                                   # |X|, |Y| on the detector
        osp = max(g[61] - g[60], 1e-6)                                          # spread of the optical path
        m_g, m_r = g[20:52], r["moments"]
        assert m_g[0] == m_r[0] and abs(m_g[16] - m_r[16]) <= 1e-12 * m_r[16]
        for base in (0, 16):
            wsum = m_r[base]
            for k, scale in enumerate((span, span, osp + abs(g[19] - (g[60] + g[61]) / 2))):
                o = base + 1 + 5 * k
                # (the NumPy side's slopes are differences of two read-outs 1 mm apart: 1e-13 of the coordinate each)
                tol = 1e-10 * wsum * np.array([scale, 1.0, scale * scale, scale, 1.0]) + 1e-13
                assert (np.abs(m_g[o:o + 5] - m_r[o:o + 5]) <= tol).all(), (j, base, k, m_g[o:o + 5], m_r[o:o + 5])
        assert abs(g[55] - r["max_angle"]) <= 1e-12 and np.abs(g[56:62] - r["bbox"]).max() <= 1e-11 * 2000.0
        for k, key in ((53, "kink_below"), (54, "kink_above")):
            assert g[k] == r[key] or abs(g[k] - r[key]) <= 1e-9 * abs(r[key])       # kink shifts (~ the detector distance)


def test_gpu_list_analysis_edges(hip):
    import scene_cases
    scene_cases.run_list_analysis_edges()


def test_gpu_guide_rays(hip):
    """art_trace_guides == the element kernel bit for bit (the alignment rays of OEPlacement's loop lists)."""
    import scene_cases
    scene_cases.run_guides()


def test_gpu_lockstep_placement(hip):
    """OEPlacement's loop lists placed in lockstep (art_trace_guides) == every value placed alone, bit for bit."""
    import scene_cases
    scene_cases.run_lockstep_placement()


def test_gpu_loop_list_prefix_sharing(hip):
    """Loop lists from OEPlacement share the trace of their common prefix (mask + first toroid in C2 / C3)."""
    import scene_cases
    scene_cases.run_prefix_sharing()


def test_gpu_fused_readout(hip):
    """The detector read-out fused behind the tracing launch (art_trace_chain_readout, scene read-outs): per-ray values
    bit-identical to the separate art_detector_readout, statistics to rounding, Detector.readout reuses it."""
    import scene_cases
    scene_cases.run_fused_readout()


def test_gpu_fused_readout_full_size(hip):
    """relay4 at the headline size (1e7 rays x 4 toroids): fused == separate read-out; and the chunked-launch limit."""
    import torch
    import bench
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    chain, _ = bench.build_scene(4)
    els = chain.optical_elements
    src = bench.device_source(10_000_000, 0, 10_000_000, hip)
    plain = mp.RayTracingCalculation(src, els)
    D = mdet.Detector(np.asarray(els[-1].position, dtype=float))
    D.autoplace(plain[-1], 600.0)
    want = D.readout(plain[-1], sync=False)
    out = mp.RayTracingCalculation(src, els, detector=D)
    got = D.readout(out[-1], sync=False)
    assert got["X"] is out[-1]._fused_readout[2]["X"]
    for x, y in zip(out, plain):
        assert torch.equal(x.alive, y.alive) and torch.equal(x.data, y.data)
    for k in ("X", "Y", "opl"):
        assert torch.equal(got[k], want[k])
    g, w = got["stats_dev"].cpu().numpy(), want["stats_dev"].cpu().numpy()
    assert g[0] == w[0] == 10_000_000 and all(g[k] == w[k] for k in (2, 3, 4, 5, 12, 13))
    rel = max(abs(g[k] - w[k]) / abs(w[k]) for k in (1, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21) if w[k] != 0)
    report(f"[fused read-out relay4 1e7] statistics vs separate read-out: max rel diff {rel:.1e} (summation order)")
    assert rel <= 1e-11
    # the partials are folded in a fixed order: a second launch (by-value and scene-table form) gives the same bits
    again = D.readout(mp.RayTracingCalculation(src, els, detector=D)[-1], sync=False)["stats_dev"]
    assert torch.equal(again.view(torch.int64), got["stats_dev"].view(torch.int64))
    many = mp.RayTracingCalculationMany([src], [els], detectors=[D])[0]
    assert torch.equal(D.readout(many[-1], sync=False)["stats_dev"].view(torch.int64), got["stats_dev"].view(torch.int64))


def test_gpu_fused_readout_fold_boundary(hip):
    """The fused read-out's partial statistics are folded by one launch up to 8192 per-wave partials (524 288 rays) and
    by two above: both sides of the boundary, and a scene launch of two chains, against the separate read-out."""
    import torch
    import bench
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    chain, _ = bench.build_scene(2)
    els = chain.optical_elements
    for n in (8192 * 64, 8192 * 64 + 1, 8193 * 64, 300_001):
        src = bench.device_source(n, 0, n, hip)
        plain = mp.RayTracingCalculation(src, els)
        D = mdet.Detector(np.asarray(els[-1].position, dtype=float))
        D.autoplace(plain[-1], 600.0)
        want = D.readout(plain[-1], sync=False)["stats_dev"].cpu().numpy()
        outs = [mp.RayTracingCalculation(src, els, detector=D)] + mp.RayTracingCalculationMany([src, src], [els, els], detectors=[D, D])
        for out in outs:
            got = D.readout(out[-1], sync=False)
            assert got["X"] is out[-1]._fused_readout[2]["X"]
            g = got["stats_dev"].cpu().numpy()
            assert g[0] == want[0] == n and all(g[k] == want[k] for k in (2, 3, 4, 5, 12, 13)) and g[22] == 0.0 and g[23] == 0.0
            for k in (1, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21):
                assert abs(g[k] - want[k]) <= 1e-11 * abs(want[k]), (n, k, g[k], want[k])


def test_gpu_batched_full_size_c2(hip):
    """BASELINE C2 size: 11 chains x 1e6 rays in one launch == 11 single launches, bit for bit."""
    import torch
    import ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp, ART.ModuleProcessing as mp
    SP = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": 1_000_000}
    Mask = mmask.Mask(msupp.SupportRoundHole(20, 14e-3 * 500, 0, 0))
    R, r = mmirror.ReturnOptimalToroidalRadii(500, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(150, 32))
    chains = mp.OEPlacement(SP, [Mask, Tor, Tor], [400, 100, np.linspace(300, 700, 11).tolist()], [0, 80, -80], [0, 0, 0],
                            "C2")
    assert len(chains) == 11
    many = mp.RayTracingCalculationMany([c.source_rays for c in chains], [c.optical_elements for c in chains])
    for c, o in zip(chains, many):
        for x, y in zip(o, mp.RayTracingCalculation(c.source_rays, c.optical_elements)):
            assert torch.equal(x.alive, y.alive)
            m = x.alive.bool()
            assert torch.equal(x.data[:, m], y.data[:, m])
        assert 0.4 < len(o[-1]) / 1e6 < 0.6          # SURVEY: C2 1e6 -> 4.9e5


@pytest.mark.parametrize("rpl", ["1", "2"])
def test_gpu_dropped_store_pairs_touch_nothing(hip, monkeypatch, rpl):
    """The fused kernels store pairs of neighbouring slots with one 16-byte access and drop a pair of dead rays through
    the range check of the buffer descriptor (offset 2^31).  Output arrays pre-filled with a sentinel: a pair of dead
    slots keeps the sentinel in all eight streams, live slots -- slots 0 and 1 of every stream in particular, where a
    wrapped-around offset would land -- equal the per-element kernel's 8-byte stores bit for bit.  The ray count is ODD
    and every row is padded (bundle.RayBundle._rows): the GUARD slots behind the last ray of every stream -- where the
    second half of the last 16-byte store, or the second byte of a 16-bit alive access, would land -- keep the sentinel
    too, for both bodies of the fused kernel (one ray per lane / two rays per lane)."""
    import torch
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd.bundle import RayBundle
    import bench
    monkeypatch.setenv("ART_CHAIN_RPL", rpl)
    element_lists, _, _ = bench.scene_c3()
    els = element_lists[3]
    n = 100_001
    src = bench.device_source(n, 0, n, hip, ("point", 0.025))
    ref = mp.RayTracingCalculation(src, els, mode="element")
    descs = [mp.element_descriptor(oe, True, hip)[0] for oe in els]
    outs = RayBundle.allocate_many(n, len(els), src, hip)
    sentinel = torch.tensor([0x7FF8DEADBEEF0123], dtype=torch.int64, device=hip.device).view(torch.float64)
    rows, flags = outs[0].data._base, outs[0].alive._base          # [m, 8, pitch] and [m, pitch]: the whole allocations
    assert rows.shape[-1] > n and flags.shape[-1] > n               # padded: guard slots exist behind every stream
    rows[:] = sentinel
    flags.fill_(7)
    hip.trace_chain(descs, src.view(), [b.view() for b in outs], n)
    torch.cuda.synchronize()
    assert bool((rows[..., n:].view(torch.int64) == sentinel.view(torch.int64)).all()), "a store landed behind a stream's end"
    assert bool((flags[..., n:] == 7).all()), "an alive byte landed behind the array's end"
    lost = 0
    for k, (b, r) in enumerate(zip(outs, ref)):
        assert torch.equal(b.alive, r.alive)
        live = r.alive.bool()
        assert torch.equal(b.data[:, live].view(torch.int64), r.data[:, live].view(torch.int64))
        assert bool(live[0]) and bool(live[1])
        assert torch.equal(b.data[:, :2].view(torch.int64), r.data[:, :2].view(torch.int64))
        pad = torch.cat([live, torch.zeros(n % 2, dtype=torch.bool, device=hip.device)]).view(-1, 2)
        dead_pair = (~pad.any(dim=1)).repeat_interleave(2)[:n]
        lost += int(dead_pair.sum())
        assert bool((b.data[:, dead_pair].view(torch.int64) == sentinel.view(torch.int64)).all()), k
    assert lost > 10_000        # the mask stops a third of the rays: whole pairs among them


def test_gpu_zernike_any_order_and_any_number_of_defects(hip):
    """Order 16 (unrolled Horner tables), orders 20 / 30 / 48 (the recurrence kernel, private-memory rows), a recurrence
    element inside a chain, seven defects on one mirror: against the oracle and the long-double truth."""
    import zernike_cases
    for name, w in zernike_cases.run_high_order().items():
        report(f"[zernike {name}, local error vs long-double truth] " + "  ".join(f"{k} {v:.1e}" for k, v in w.items()))


def test_gpu_two_rays_per_lane_body(hip, monkeypatch):
    """The experiment body of the fused kernels (ART_CHAIN_RPL=2, read by the library at every launch: two neighbouring
    slots per lane, 16-byte accesses straight from registers, no LDS staging) gives the shipped body's results bit for bit:
    golden chains, an odd ray count (16-bit alive accesses at the tail), the scene launch and the fused read-out."""
    import torch
    import bench
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    element_lists, _, _ = bench.scene_c3()
    for n in (100_001, 4096, 77):
        src = bench.device_source(n, 0, n, hip, ("point", 0.025))
        D = None
        outs = {}
        for rpl in ("1", "2"):
            monkeypatch.setenv("ART_CHAIN_RPL", rpl)
            plain = mp.RayTracingCalculation(src, element_lists[2])
            if D is None:
                D = mdet.Detector(np.asarray(element_lists[2][-1].position, dtype=float))
                D.autoplace(plain[-1], 600.0)
            fused = mp.RayTracingCalculation(src, element_lists[2], detector=D)
            ro = D.readout(fused[-1], sync=False)
            many = mp.RayTracingCalculationMany([src, src], [element_lists[2], element_lists[7]], detectors=[D, D])
            outs[rpl] = (plain, fused, ro, many)
            torch.cuda.synchronize()
        a, b = outs["1"], outs["2"]
        for x, y in list(zip(a[0], b[0])) + list(zip(a[1], b[1])) + [(p, q) for ca, cb in zip(a[3], b[3]) for p, q in zip(ca, cb)]:
            assert torch.equal(x.alive, y.alive)
            live = x.alive.bool()
            assert torch.equal(x.data[:, live].view(torch.int64), y.data[:, live].view(torch.int64))
        live = a[1][-1].alive.bool()
        for k in ("X", "Y", "opl"):
            assert torch.equal(a[2][k][live].view(torch.int64), b[2][k][live].view(torch.int64))
        sa, sb = a[2]["stats_dev"].cpu().numpy(), b[2]["stats_dev"].cpu().numpy()
        assert sa[0] == sb[0] and all(sa[k] == sb[k] for k in (2, 3, 4, 5, 12, 13))
        assert np.abs(sa - sb).max() <= 1e-11 * max(1.0, np.abs(sa).max())

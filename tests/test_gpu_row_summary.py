"""GPU (-m gpu): scene launches with row summaries attached (include/art_hip.h: art_bundle_row_summary -- the one-ray
scene kernels skip the rows of their input that hold one value in every slot) against the same launches without
(ART_ROW_SUMMARY=0, read per launch): every bundle, X / Y / opl and the 24 statistics bit for bit.  And the summary
itself: what it reports constant, and that it follows its bundle through a captured graph."""
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 257, 1037, 4099]        # a lone ray, a ragged wave, one tile + 1, ragged tiles
OX, OY, OZ, DX, DY, DZ, PATH, ALIVE, W = (1 << j for j in range(9))      # bits of the summary's `differs` word
DIR = DX | DY | DZ                      # what varies in a point source with uniform weights


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
def scenes(hip):
    """name -> (elements, source kind, wavelength, IgnoreDefects, detector): a point source through 2 toroids (k_trace_scene)
    and a plane source through one parabola with a Zernike defect (k_trace_scene1)."""
    import bench
    import ART.ModuleMirror as mmirror, ART.ModuleSupport as msupp, ART.ModuleDefects as mdef, ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    els = bench.build_scene(2)[0].optical_elements
    src = bench.device_source(1037, 0, 1037, hip, ("point", 0.02))
    det = mdet.Detector(np.asarray(els[-1].position, dtype=float))
    det.autoplace(mp.RayTracingCalculation(src, els, history=False)[-1], 600.0)
    out = {"point": (els, ("point", 0.02), 50e-6, True, det)}
    S = msupp.SupportRectangle(40, 40)
    Z = mdef.Zernike(S, {(2, 1): 1e-4, (3, 1): 5e-5, (4, 2): 2e-5, (3, 3): -3e-5, (5, 2): 1e-5})
    SP = {"Divergence": 0, "SourceSize": 40, "Wavelength": 800e-6, "DeltaFT": 0, "NumberRays": 1000}
    ch = mp.OEPlacement(SP, [mmirror.DeformedMirror(mmirror.MirrorParabolic(25.4, 0, S), [Z])], [15], [8.0], Description="plane")
    e1 = ch.optical_elements
    nrm = np.array([0.9, -0.1, 0.05])
    det1 = mdet.Detector(np.zeros(3), np.asarray(e1[0].position, float) + np.array([-20.0, 3.0, 1.0]), nrm / np.linalg.norm(nrm))
    out["plane"] = (e1, ("plane", 19.0), 800e-6, False, det1)
    return out


def _source(be, scene, n, weights="uniform"):
    import torch
    import bench
    _, kind, wl, _, _ = scene
    src = bench.device_source(n, 0, n, be, kind, wl)          # (its intensity: ones)
    if weights == "gauss":
        src.intensity = be.gaussian_intensity_central(src.view(), 1 / np.e ** 2, n) if n > 1 else \
            torch.full((n,), 0.5, dtype=torch.float64, device=be.device)
    elif weights is None:
        src.intensity = None
    return src


def _program(src, scene, history=True, readout="full", capture=False):
    from attosecondraytracing_amd.graph import SceneProgram
    els, _, _, ign, det = scene
    return SceneProgram([src], [els], IgnoreDefects=ign, capture=capture, history=history,
                        detectors=None if readout == "none" else [det], readout_lite=(readout == "lite"))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64).clone()


def _poison(prog):
    """Overwrite everything a run writes, so that a run that skipped something cannot pass on the previous run's bytes."""
    for outs in prog.outputs:
        for b in outs:
            if b is not None:
                b.data.fill_(7.0)
                b.alive.fill_(9)
    for ro in prog.readouts or []:
        for k in ("X", "Y", "opl", "stats_dev"):
            ro[k].fill_(7.0)


def _snapshot(prog):
    """Everything a run produced: alive bytes of every slot, the rows of the alive slots (dead slots are not written),
    X / Y / opl of the last bundle's alive slots, the 24 statistics -- as bit patterns."""
    res = []
    for ci, outs in enumerate(prog.outputs):
        for b in outs:
            if b is not None:
                res += [b.alive.clone(), _bits(b.data[:, b.alive.bool()])]
        if prog.readouts is not None:
            ro, live = prog.readouts[ci], outs[-1].alive.bool()
            res += [_bits(ro[k][live]) for k in ("X", "Y", "opl")] + [_bits(ro["stats_dev"])]
    return res


def _run(prog, monkeypatch, summaries):
    if summaries:
        monkeypatch.delenv("ART_ROW_SUMMARY", raising=False)
    else:
        monkeypatch.setenv("ART_ROW_SUMMARY", "0")
    _poison(prog)
    prog.run()
    monkeypatch.delenv("ART_ROW_SUMMARY", raising=False)
    return _snapshot(prog)


def _same(a, b, what):
    import torch
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, k)


def _differs(summary):
    """(`differs` word, slot count, nine patterns) of one summary tensor."""
    raw = summary.cpu().numpy()
    return int(raw[0:4].view(np.uint32)[0]), int(raw[8:16].view(np.int64)[0]), raw[16:88].view(np.uint64).copy()


def _both(prog, monkeypatch, what):
    ref = _run(prog, monkeypatch, False)
    got = _run(prog, monkeypatch, True)
    _same(ref, got, what)
    return ref


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["point", "plane"])
def test_gpu_summarised_scene_launch_is_the_plain_one_bit_for_bit(hip, scenes, monkeypatch, name, n):
    scene = scenes[name]
    const_rows = (OX | OY | OZ) if name == "point" else (DX | DY | DZ)
    for weights in (None, "uniform", "gauss"):
        src = _source(hip, scene, n, weights)
        for history in (True, False):
            for readout in ("full", "lite", "none"):
                prog = _program(src, scene, history, readout)
                ref = _both(prog, monkeypatch, (name, n, weights, history, readout))
                d, cnt, c = _differs(prog._summaries[0])
                assert cnt == n and (d & (const_rows | PATH | ALIVE)) == 0, (name, n, hex(d))
                if n > 64:
                    assert (d & ~W & 0x1ff) != 0, (name, hex(d))          # (some row does vary: the mask is not trivially empty)
                w_varies = weights is None or (weights == "gauss" and n > 1)
                assert bool(d & W) == w_varies, (name, n, weights, hex(d))
                assert c[7] == 1 and c[6] == 0                           # alive = 1, path = +0.0
                if readout != "none":
                    stats = prog.readouts[0]["stats_dev"].cpu().numpy()
                    assert stats[0] == float(int(prog.outputs[0][-1].alive.sum()))
                    if name == "point":
                        assert stats[0] == n                             # every ray survives: no slot beyond n counted
                assert len(ref) > 0


def test_gpu_every_one_ray_scene_body(hip, scenes, monkeypatch):
    """The other builds of the one-ray body: 6 waves per SIMD, the general defect body, the 5-wave special one."""
    for name, env in (("point", {"ART_CHAIN_WAVES": "6"}), ("plane", {"ART_CHAIN_SPECIAL": "0"}),
                      ("plane", {"ART_CHAIN_SPECIAL": "1", "ART_CHAIN_SPECIAL_WAVES": "5"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for n in (257, 1037):
            prog = _program(_source(hip, scenes[name], n), scenes[name])
            _both(prog, monkeypatch, (name, env, n))
        for k in env:
            monkeypatch.delenv(k)


def test_gpu_sums_tail_of_a_one_shot_scene_launch(hip, scenes, monkeypatch):
    """RayTracingCalculationMany forms the summaries from the second trace of an unchanged source on."""
    import torch
    import ART.ModuleProcessing as mp
    els, _, _, ign, _ = scenes["point"]
    for n in (257, 1037):
        src = _source(hip, scenes["point"], n)
        srcs = [src, src.copy()]                              # (two inputs: the one-ray body)

        def trace():
            outs = mp.RayTracingCalculationMany(srcs, [els, els], IgnoreDefects=ign, history=False, sums=True)
            return [t for o in outs for t in (o[-1].alive.clone(), _bits(o[-1].data[:, o[-1].alive.bool()]),
                                              _bits(o[-1].fused_sums()[:9]))]
        first = trace()
        assert getattr(src, "_row_summary", None) is None      # a single trace is not worth the pass over the source
        second = trace()
        assert src._row_summary is not None and _differs(src._row_summary[1])[0] == DIR
        monkeypatch.setenv("ART_ROW_SUMMARY", "0")
        plain = trace()
        monkeypatch.delenv("ART_ROW_SUMMARY")
        _same(plain, first, n)
        _same(plain, second, n)
        assert float(second[2][0].view(torch.float64)) == n


def _mutations():
    """name, row bit, what to do to a uniform-weight point source of 1037 rays; every one makes that row non-constant."""
    import torch

    def first(src):
        src.data[0, 0] = 0.25

    def last(src):
        src.data[1, src.n_slots - 1] = 0.25

    def slot64(src):
        src.data[6, 64] = 0.125

    def minus_zero(src):
        src.data[2].zero_()
        src.data[2, 700] = -0.0

    def weight(src):
        src.intensity[64] = 2.0

    def weight_last(src):
        src.intensity[src.n_slots - 1] = torch.nextafter(src.intensity[0], src.intensity[0] + 1)

    return [("first slot", OX, first), ("last slot", OY, last), ("slot 64", PATH, slot64), ("-0.0 among +0.0", OZ, minus_zero),
            ("weight of slot 64", W, weight), ("last weight, one ulp", W, weight_last)]


def test_gpu_summary_reports_what_differs(hip, scenes, monkeypatch):
    import torch
    scene, n = scenes["point"], 1037
    for what, bit, change in _mutations():
        src = _source(hip, scene, n)
        prog = _program(src, scene)
        prog.run()
        assert _differs(prog._summaries[0])[0] == DIR, what
        change(src)
        _both(prog, monkeypatch, what)
        assert _differs(prog._summaries[0])[0] == (DIR | bit), what
    # one NaN pattern in every slot IS constant (patterns are compared, not values) ...
    src = _source(hip, scene, n)
    src.data[6].fill_(float("nan"))
    prog = _program(src, scene)
    _both(prog, monkeypatch, "NaN row")
    d, _, c = _differs(prog._summaries[0])
    assert d == DIR and c[6] == int(torch.tensor(float("nan"), dtype=torch.float64).view(torch.int64))
    # ... and two NaN patterns are not
    src.data[6, 5] = torch.tensor(0x7FF8000000000001, dtype=torch.int64).view(torch.float64)
    _both(prog, monkeypatch, "two NaN patterns")
    assert _differs(prog._summaries[0])[0] == (DIR | PATH)
    # no slots, no arrays: nothing is proven
    buf = torch.zeros(hip.row_summary_bytes(), dtype=torch.uint8, device=hip.device)
    hip.bundle_row_summary(src.view(), None, 0, buf)
    assert _differs(buf)[:2] == (0x1ff, 0)
    hip.bundle_row_summary(src.view(), None, n, buf)
    assert _differs(buf)[:2] == (DIR | PATH | W, n)


def test_gpu_dead_slots(hip, scenes, monkeypatch):
    scene, n = scenes["point"], 1037
    src = _source(hip, scene, n)
    prog = _program(src, scene)
    _both(prog, monkeypatch, "all alive")
    assert prog.readouts[0]["stats_dev"][0].item() == n          # the count: no lane of the last tile's tail resurrected
    assert int(prog.outputs[0][0].alive.sum()) == n and int(prog.outputs[0][-1].alive.sum()) == n
    src.alive[::3] = 0
    _both(prog, monkeypatch, "some dead")
    assert _differs(prog._summaries[0])[0] & ALIVE
    assert prog.readouts[0]["stats_dev"][0].item() == n - len(range(0, n, 3))
    src.alive.zero_()                                            # a constant 0
    _both(prog, monkeypatch, "all dead")
    d, _, c = _differs(prog._summaries[0])
    assert not d & ALIVE and c[7] == 0
    assert prog.readouts[0]["stats_dev"][0].item() == 0 and int(prog.outputs[0][-1].alive.sum()) == 0


@pytest.mark.parametrize("xmap", ["0", "-1", "3"])
def test_gpu_rounded_up_grids_stay_inert(hip, scenes, monkeypatch, tmp_path, xmap):
    """ART_XCD_MAP rounds the grid up to whole groups of tiles (8, or 32 with runs of 4): the padding workgroups lie beyond n
    and a constant alive = 1 must not wake them.  The mapping is read once per loaded library, so each value gets a copy of
    the library of its own, loaded beside the default one."""
    import __graft_entry__
    from attosecondraytracing_amd import _lib
    lib = str(tmp_path / ("libart_xmap_%s.so" % xmap.replace("-", "m")))
    shutil.copy(__graft_entry__.HIP_LIB, lib)
    monkeypatch.setenv("ART_XCD_MAP", xmap)
    be = _lib.HipBackend(lib)
    for name in ("point", "plane"):
        for n in (257, 1037, 4099):
            src = _source(be, scenes[name], n)
            assert src.backend is be
            prog = _program(src, scenes[name])
            _both(prog, monkeypatch, (xmap, name, n))
            if name == "point":
                assert prog.readouts[0]["stats_dev"][0].item() == n
    # the XCD-grouped scene grid (chains that share an input, padded to 8 tiles per chain) with the one-ray defect body
    from attosecondraytracing_amd.graph import SceneProgram
    els, _, _, ign, det = scenes["plane"]
    src = _source(be, scenes["plane"], 1037)
    prog = SceneProgram([src] * 3, [els] * 3, IgnoreDefects=ign, capture=False, detectors=[det] * 3)
    _both(prog, monkeypatch, "xcd-grouped")


def test_gpu_slot_ranges(hip, scenes, monkeypatch):
    """A program over src.slots(256, 1037): the range is a bundle of its own with a summary of its own."""
    import torch
    for name in ("point", "plane"):
        src = _source(hip, scenes[name], 1037)
        part = src.slots(256, 1037)
        prog = _program(part, scenes[name])
        _both(prog, monkeypatch, name)
        assert _differs(prog._summaries[0])[1] == 1037 - 256
        whole = _program(src, scenes[name])
        ref = _run(whole, monkeypatch, False)
        full, got = whole.outputs[0][-1], prog.outputs[0][-1]
        live = got.alive.bool()
        assert torch.equal(got.alive, full.alive[256:1037]) and int(live.sum()) > 0      # the range of the whole trace
        assert torch.equal(_bits(got.data[:, live]), _bits(full.data[:, 256:1037][:, live]))
        # a summary formed over fewer slots than the launch covers is not used: a one-slot summary (every row "constant")
        # in the place of the whole bundle's changes nothing
        _same(ref, _run(whole, monkeypatch, True), name)
        whole._summaries[0].copy_(src.slots(0, 1).row_summary()[1])
        assert _differs(whole._summaries[0])[:2] == (0, 1)
        _same(ref, _run(whole, monkeypatch, True), (name, "short summary"))


def test_gpu_summary_follows_its_source_through_a_captured_graph(hip, scenes, monkeypatch):
    import torch
    import bench
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    scene, n = scenes["point"], 1037
    src = _source(hip, scene, n)
    prog = _program(src, scene, capture=True)
    assert prog.graph is not None
    address = prog._summaries.data_ptr()

    def check(what, expect):
        _poison(prog)
        prog.run()
        got = _snapshot(prog)
        monkeypatch.setenv("ART_ROW_SUMMARY", "0")                   # a fresh program, every row loaded
        fresh = _program(src, scene, capture=False)
        fresh.run()
        monkeypatch.delenv("ART_ROW_SUMMARY")
        _same(_snapshot(fresh), got, what)
        assert prog._summaries.data_ptr() == address                  # the buffer the graph holds
        assert _differs(prog._summaries[0])[0] == expect, (what, hex(_differs(prog._summaries[0])[0]))

    check("as built", DIR)
    src.data[0, 5] = 1.0
    check("one element written", DIR | OX)
    other = bench.device_source(n, 0, n, hip, ("point", 0.03))
    other.data[0:3] += torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float64, device=hip.device)   # another source point
    src.data.copy_(other.data)
    check("data.copy_", DIR)
    assert _differs(prog._summaries[0])[2][0] == int(_bits(src.data[0, 0:1])[0]) == int(_bits(other.data[0, 7:8])[0])
    # (in place: a captured program reads the weight tensor it was built with, as it reads the source's arrays)
    src.intensity.copy_(hip.gaussian_intensity_central(src.view(), 1 / np.e ** 2, n))
    check("non-uniform intensity", DIR | W)
    src.intensity.fill_(0.5)
    check("uniform intensity again", DIR)
    rot = mgeo.rotation_matrix(np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    hip.make_source(0, 0.015, rot, np.array([0.5, -0.25, 0.125]), 0, n, n, src.view())      # a library kernel, a raw view
    src.touch()
    check("make_source into the same bundle", DIR)
    assert _differs(prog._summaries[0])[2][0] == int(_bits(src.data[0, 0:1])[0]) != int(_bits(other.data[0, 0:1])[0])

"""CPU: diffraction gratings -- the oracle against the long-double truth, the header's per-ray function (compiled with
g++) against the truth on all six substrates, the host shell (Grating, RayBundle.grooves, refusals), the ABI mirror, and
the device code's resource usage (no scratch memory)."""
import ctypes as C
import os
import pickle
import re
import shutil
import subprocess

import numpy as np
import pytest

import grating_common as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = gc.scenes()


# ------------------------------------------------------------------------------------------ oracle, truth, header
@pytest.mark.parametrize("name", sorted(SCENES))
def test_fp64_oracle_agrees_with_long_double_truth(name):
    assert gc.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    oe, (P, V, path, alive), wl = SCENES[name]
    E = gc.element_spec(oe)
    ref = gc.diffract(E, P, V, path, alive, wl, T=gc.LD)
    res = gc.diffract(E, P, V, path, alive, wl, T=np.float64)
    clear = np.abs(np.asarray(ref["s"], dtype=float)) > 1e-9            # (the evanescent scene has none closer, see below)
    assert (res["alive"] == ref["alive"])[clear].all()
    assert ref["hit"].sum() > 0
    gc.assert_parity(res, ref, ref["alive"] & res["alive"], name)


def test_evanescent_scene_straddles_the_cut_off_with_a_margin():
    oe, (P, V, path, alive), wl = SCENES["evanescent"]
    ref = gc.diffract(gc.element_spec(oe), P, V, path, alive, wl, T=gc.LD)
    s = np.asarray(ref["s"], dtype=float)[ref["hit"]]
    assert (np.abs(s) >= 1e-9).all() and (s > 0).any() and (s < 0).any()


HARNESS = r'''
#include <cstdio>
#include <vector>
#include "art_device.h"
// in: 36 doubles (kind, support kind, fwd[9], pos[3], centre[3], sp[6], mp[4], qx, qy, N, m, wavelength, n, 3 unused), then
// n rows of 9 doubles (point, vector, path, alive, grooves).  out: n rows of 10 (ray[8], grooves, alive).
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  double h[36];
  if (!f || fread(h, 8, 36, f) != 36) return 2;
  ArtElementDesc e = {};
  e.kind = (int)h[0]; e.support_kind = (int)h[1];
  for (int i = 0; i < 9; ++i) e.fwd[i] = h[2 + i];
  for (int i = 0; i < 3; ++i) { e.pos[i] = h[11 + i]; e.centre[i] = h[14 + i]; }
  for (int i = 0; i < 6; ++i) e.sp[i] = h[17 + i];
  for (int i = 0; i < 4; ++i) e.mp[i] = h[23 + i];
  art::prepare_element(e);
  const long n = (long)h[32];
  std::vector<double> in(9 * n), out(10 * n);
  if (fread(in.data(), 8, 9 * n, f) != (size_t)(9 * n)) return 3;
  for (long i = 0; i < n; ++i) {
    const double* r = &in[9 * i];
    art::Ray ray = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], 0.0};
    double g = r[8];
    const bool ok = r[7] != 0.0 && art::grating_ray(e, h[27], h[28], h[29], (int)h[30], h[31], ray, g);
    const double o[10] = {ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, ray.path, ray.inc, g, ok ? 1.0 : 0.0};
    for (int k = 0; k < 10; ++k) out[10 * i + k] = o[k];
  }
  FILE* w = fopen(argv[2], "wb");
  fwrite(out.data(), 8, 10 * n, w);
  fclose(w);
  return 0;
}
'''


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    td = tmp_path_factory.mktemp("grating_harness")
    src, exe = td / "h.cpp", td / "h"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DART_HOST_TWIN", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "attosecondraytracing_amd", "csrc"), "-o", str(exe), str(src)])
    return td, str(exe)


KIND_NUMBER = {"plane": 0, "sphere": 1, "parabola": 2, "torus": 3, "ellipsoid": 4, "cylinder": 5}     # include/art_hip.h


def run_header(harness, tag, E, rays, wl, g_in, N=None, m=None):
    """grating_ray of the header on every ray of a scene; rows of (ray[8], grooves, alive).  N = 0: the bare mirror."""
    td, exe = harness
    P, V, path, alive = rays
    n = len(P)
    sp = list(E["support"][1:]) + [0.0] * 6
    head = ([KIND_NUMBER[E["kind"]], 0 if E["support"][0] == "round" else 2] + list(E["fwd"].reshape(9))
            + list(E["pos"]) + list(E["centre"]) + sp[:6] + (E["mp"] + [0.0] * 4)[:4]
            + [E["q"][0], E["q"][1], E["N"] if N is None else N, E["m"] if m is None else m, wl, n, 0, 0, 0])
    rows = np.column_stack([P, V, path, alive.astype(float), g_in])
    fin, fout = str(td / (tag + ".in")), str(td / (tag + ".out"))
    with open(fin, "wb") as f:
        f.write(np.asarray(head, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, dtype=np.float64).reshape(n, 10)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_header_function_agrees_with_long_double_truth(harness, name):
    oe, (P, V, path, alive), wl = SCENES[name]
    E = gc.element_spec(oe)
    n = len(P)
    g_in = np.linspace(-3.0, 3.0, n)
    out = run_header(harness, name, E, (P, V, path, alive), wl, g_in)
    ref = gc.diffract(E, P, V, path, alive, wl, grooves=g_in, T=gc.LD)
    clear = np.abs(np.asarray(ref["s"], dtype=float)) > 1e-9
    got_alive = out[:, 9] != 0
    assert (got_alive == ref["alive"])[clear].all()
    res = {"point": out[:, 0:3], "vector": out[:, 3:6], "path": out[:, 6], "inc": out[:, 7], "grooves": out[:, 8]}
    gc.assert_parity(res, ref, ref["alive"] & got_alive, name)
    lost = ~got_alive                                   # a lost ray keeps its state and its groove count
    assert (out[lost, 0:3] == P[lost]).all() and (out[lost, 8] == g_in[lost]).all()


# ---------------------------------------------------------------- the six substrates: header and oracle against the truth
SIX = gc.scenes_six()
THREE_KIND = sorted(k for k, sc in SIX.items() if sc["substrate"] in ("plane", "sphere", "torus"))     # what `diffract` knows


def mirror_seed(harness, tag, E, rays):
    """Which rays the bare substrate catches and their segment lengths (NaN: lost), from the header with N = 0."""
    P, V, path, alive = rays
    out = run_header(harness, tag, E, rays, 30e-6, np.zeros(len(P)), N=0.0, m=0)
    return np.where(out[:, 9] != 0, out[:, 6] - path, np.nan)


def six_truth(harness, name, g_in=None):
    sc = SIX[name]
    E, EL = gc.element_spec(sc["oe"]), gc.element_spec(sc["large"])
    P, V, path, alive = sc["rays"]
    ref = gc.truth(E, P, V, path, alive, sc["wl"], mirror_seed(harness, name + "_m", E, sc["rays"]), grooves=g_in)
    ref_large = ref if sc["large"] is sc["oe"] else gc.truth(EL, P, V, path, alive, sc["wl"],
                                                             mirror_seed(harness, name + "_ml", EL, sc["rays"]))
    return sc, E, ref, ref_large


@pytest.mark.parametrize("name", sorted(SIX))
def test_header_function_agrees_with_long_double_truth_on_every_substrate(harness, name):
    assert gc.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    P, V, path, alive = SIX[name]["rays"]
    g_in = np.linspace(-3.0, 3.0, len(P))
    sc, E, ref, ref_large = six_truth(harness, name, g_in)
    n_hit, n_alive = gc.own_input(sc, E, ref, ref_large, name)
    if sc["family"] == "clipped":
        assert n_hit == gc.CLIPPED_HITS[sc["substrate"]]
    assert (n_alive == 0) == (name in gc.EVANESCENT)    # N900_m1_a33: evanescent on the four grazing substrates, alive elsewhere
    out = run_header(harness, name, E, sc["rays"], sc["wl"], g_in)
    got_alive = out[:, 9] != 0
    assert np.array_equal(got_alive, ref["alive"]), name + ": alive masks differ"
    res = {"point": out[:, 0:3], "vector": out[:, 3:6], "path": out[:, 6], "inc": out[:, 7], "grooves": out[:, 8]}
    gc.assert_parity(res, ref, ref["alive"], name)
    dev = gc.worst_deviation(res, ref, ref["alive"])
    print(name, "worst deviation from the truth", {k: f"{v:.1e}" for k, v in dev.items()})
    if sc["family"] == "cutoff":
        m = ref["alive"]
        dv = np.abs(np.asarray(res["vector"][m] - ref["vector"][m], dtype=float)).max(axis=1)
        print(name, "dv * sqrt(s)", f"{float((dv * np.sqrt(np.asarray(ref['s'][m], dtype=float))).max()):.1e}")
    lost = ~got_alive                                   # a lost ray keeps its state and its groove count
    assert (out[lost, 0:3] == P[lost]).all() and (out[lost, 8] == g_in[lost]).all()


@pytest.mark.parametrize("name", THREE_KIND)
def test_fp64_oracle_agrees_with_long_double_truth_on_its_three_substrates(harness, name):
    """`diffract` in fp64 (the oracle of the older GPU tests) against the truth seeded by the bare mirror."""
    assert gc.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    sc, E, ref, ref_large = six_truth(harness, name)
    gc.own_input(sc, E, ref, ref_large, name)
    P, V, path, alive = sc["rays"]
    res = gc.diffract(E, P, V, path, alive, sc["wl"], T=np.float64)
    assert np.array_equal(res["hit"], ref["hit"]) and np.array_equal(res["alive"], ref["alive"])
    gc.assert_parity(res, ref, ref["alive"], name)
    # The two long-double forms of the same equation, written independently (the literal root b^2 - c of `diffract` against
    # the stable root of truth_common).  Both round at 1.1e-19; the literal root of the sphere loses R^2 / (t sqrt(disc)) ~ 1e5
    # of that and a direction at the cut-off another 1.6e4: 1e-13 of the magnitudes is three decades above both.
    full = gc.diffract(E, P, V, path, alive, sc["wl"], T=gc.LD)
    assert np.array_equal(full["alive"], ref["alive"])
    m = ref["alive"]
    for key in ("point", "vector", "path", "inc", "grooves", "s"):
        if m.any():
            assert float(np.abs(full[key][m] - ref[key][m]).max()) <= 1e-13 * max(1.0, float(np.abs(ref[key][m]).max())), key


# ------------------------------------------------------------------------------------------------------- host shell
def _mirrors():
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    S = ms.SupportRound(10.0)
    return mm, ms, [mm.MirrorPlane(S), mm.MirrorSpherical(100.0, S), mm.MirrorSpherical(-100.0, S),
                    mm.MirrorParabolic(50.0, 30.0, S), mm.MirrorToroidal(300.0, 20.0, S),
                    mm.MirrorEllipsoidal(S, SemiMajorAxis=200.0, SemiMinorAxis=100.0, OffAxisAngle=30.0),
                    mm.MirrorCylindrical(100.0, S)]


def test_grating_wraps_every_mirror_and_delegates():
    mm, ms, mirrors = _mirrors()
    for M in mirrors:
        G = mm.Grating(M, 1200.0, Order=-1, GrooveAngle=90.0)
        assert "Mirror" in G.type and G.type == M.type
        assert G.support is M.support and G._abi_kind == M._abi_kind
        assert np.array_equal(G.get_centre(), M.get_centre())
        assert list(G._abi_params()) == list(M._abi_params())
        assert G._groove_vector() == (0.0, 1.0)
        assert len(G.get_grid3D(200)) == len(M.get_grid3D(200))
        assert hash(G) != hash(mm.Grating(M, 1200.0, Order=1, GrooveAngle=90.0))
    q = mm.Grating(mirrors[0], 100.0, GrooveAngle=30.0)._groove_vector()
    assert abs(q[0] ** 2 + q[1] ** 2 - 1) < 1e-15 and abs(q[1] - 0.5) < 1e-15


def test_grating_validation_and_refused_substrates():
    mm, ms, mirrors = _mirrors()
    import ART.ModuleMask as mk
    import ART.ModuleDefects as md
    with pytest.raises(ValueError):
        mm.Grating(mk.Mask(ms.SupportRound(5.0)), 1200.0)
    D = mm.DeformedMirror(mirrors[0], [md.Zernike(mirrors[0].support, {(2, 0): 1e-5})])
    with pytest.raises(ValueError):
        mm.Grating(D, 1200.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mm.Grating(mirrors[0], bad)
    with pytest.raises(ValueError):
        mm.Grating(mirrors[0], 1200.0, Order=0.5)
    with pytest.raises(ValueError):
        mm.Grating(mirrors[0], 1200.0, GrooveAngle=float("nan"))


def test_descriptor_carries_the_grating_flag():
    from attosecondraytracing_amd import ModuleProcessing as mp, _abi
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    d, _ = mp._build_descriptor(oe, True, None)
    assert d.flags & _abi.ART_FLAG_GRATING and d.grating is oe.type
    bare = gc.place(oe.type.Mirror, 500.0, 80.0)
    d0, _ = mp._build_descriptor(bare, True, None)
    assert not d0.flags & _abi.ART_FLAG_GRATING
    assert bytes(d)[16:] == bytes(d0)[16:]             # everything but the flags word is the substrate's


def _host_bundle(n=10, grooves=True):
    import torch
    from attosecondraytracing_amd.bundle import RayBundle
    b = RayBundle.__new__(RayBundle)
    RayBundle.__init__(b, torch.arange(8 * n, dtype=torch.float64).reshape(8, n).clone(), torch.ones(n, dtype=torch.uint8),
                       wavelength=30e-6, backend=object(), grooves=torch.arange(n, dtype=torch.float64) * 0.25 if grooves else None)
    return b


def test_bundle_grooves_survive_slicing_pickling_and_copies():
    import torch
    b = _host_bundle()
    s = b.slots(2, 7)
    assert torch.equal(s.grooves, b.grooves[2:7])
    r = pickle.loads(pickle.dumps(b))
    assert torch.equal(r.grooves, b.grooves) and r.wavelength == b.wavelength
    assert b.alias().grooves is b.grooves
    plain = _host_bundle(grooves=False)
    assert plain.grooves is None and plain.slots(0, 4).grooves is None
    assert pickle.loads(pickle.dumps(plain)).grooves is None
    assert plain.phase_ref_offset() == 0.0
    assert abs(b.phase_ref_offset() - 30e-6 * float(b.grooves.mean())) < 1e-18


def test_pulse_analyses_refuse_bundles_behind_a_grating():
    import ART.ModuleDetector as mdet
    import ART.ModuleOpticalChain as moc
    b = _host_bundle()
    det = mdet.Detector(np.zeros(3))
    with pytest.raises(NotImplementedError, match="get_SpectralRays"):
        det.get_FocalPulse(b, 5.0)
    oe = gc.place(gc.plane_grating(1200.0, -1, 0.0), 500.0, 80.0)
    chain = moc.OpticalChain.__new__(moc.OpticalChain)
    chain._optical_elements = [oe, oe]
    with pytest.raises(NotImplementedError, match="get_SpectralRays"):
        chain.get_FocalPulse(None, det, 5.0, np.array([0, 1, 0]))
    with pytest.raises(NotImplementedError, match="get_SpectralRays"):
        chain.get_VectorFocalField(None, det, np.array([0, 1, 0]))
    with pytest.raises(NotImplementedError, match="more than one grating"):
        chain.get_SpectralRays([30e-6])
    chain._optical_elements = [gc.place(oe.type.Mirror, 500.0, 80.0)]
    with pytest.raises(ValueError):
        chain.get_SpectralRays([30e-6])


def test_tracing_a_grating_needs_a_wavelength():
    from attosecondraytracing_amd import ModuleProcessing as mp, _abi
    d = _abi.ArtElementDesc()
    d.flags = _abi.ART_FLAG_GRATING
    with pytest.raises(ValueError, match="wavelength"):
        mp._trace_one(None, d, None, None, 0, None, None)


# -------------------------------------------------------------------------------------------------------------- ABI
def test_grating_desc_matches_the_header_and_the_library_exports_the_entry(tmp_path):
    from attosecondraytracing_amd import _abi
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import __graft_entry__ as g
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d\n", sizeof(ArtGratingDesc), offsetof(ArtGratingDesc, q),
         offsetof(ArtGratingDesc, lines_per_mm), offsetof(ArtGratingDesc, order), offsetof(ArtGratingDesc, nw),
         offsetof(ArtGratingDesc, wavelengths), offsetof(ArtGratingDesc, outs), offsetof(ArtGratingDesc, grooves_in),
         offsetof(ArtGratingDesc, grooves_out), ART_FLAG_GRATING, ART_GRATING_MAX_WAVELENGTHS);
  return 0;
}'''
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _abi.ArtGratingDesc
    assert vals == [C.sizeof(D), D.q.offset, D.lines_per_mm.offset, D.order.offset, D.nw.offset, D.wavelengths.offset,
                    D.outs.offset, D.grooves_in.offset, D.grooves_out.offset, _abi.ART_FLAG_GRATING,
                    _abi.ART_GRATING_MAX_WAVELENGTHS]
    if g._stale(g.HIP_LIB, g.HIP_DEPS):
        g.build()
    lib = C.CDLL(g.HIP_LIB)
    assert hasattr(lib, "art_trace_grating") and "art_trace_grating" in _abi.PROTOTYPES


def test_scene_pack_refuses_a_grating_on_the_host():
    """art_scene_pack is pure host code: the refusal can be checked without a device."""
    from attosecondraytracing_amd import _abi
    import torch  # noqa: F401
    import __graft_entry__ as g
    if g._stale(g.HIP_LIB, g.HIP_DEPS):
        g.build()
    fn = _abi.bind(C.CDLL(g.HIP_LIB))
    e = (_abi.ArtElementDesc * 1)()
    e[0].kind, e[0].flags = _abi.ART_PLANE, _abi.ART_FLAG_GRATING
    v = _abi.ArtBundleView(*([8] * 9))
    ins, outs = (_abi.ArtBundleView * 1)(v), (_abi.ArtBundleView * 1)(v)
    image = C.create_string_buffer(int(fn["art_scene_bytes"](1, 1)))
    assert fn["art_scene_pack"](e, 1, 1, ins, outs, None, C.cast(image, C.c_void_p)) == _abi.ART_ERR_UNSUPPORTED
    e[0].flags = 0
    assert fn["art_scene_pack"](e, 1, 1, ins, outs, None, C.cast(image, C.c_void_p)) >= 0


# ---------------------------------------------------------------------------------------------------- device code
def test_grating_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "dev.o"), src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    blocks = re.split(r"remark: Function Name: ", p.stdout)
    mine = [b for b in blocks if "k_trace_grating" in b.split("[", 1)[0]]
    assert len(mine) == 1, "the kernel's resource remarks were not found"
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0])
    assert m and int(m.group(1)) == 0, mine[0]
    assert re.search(r"VGPRs Spill: 0", mine[0]) and re.search(r"SGPRs Spill: 0", mine[0])

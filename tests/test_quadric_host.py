"""CPU: general quadric mirrors -- the coefficient builders, the header's per-ray function (compiled with g++) against
the long-double truth of tests/quadric_common.py on every scene, the candidate rules one by one, the host shell
(validation, refused substrates, descriptor flag, refusals that need no device), the ABI mirror, and the device code's
resource usage (no scratch memory, no LDS)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import quadric_common as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = qc.scenes()
LD = qc.LD


@pytest.fixture(scope="module")
def truth():
    assert qc.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    return {name: qc.trace(qc.element_spec(oe), *rays) for name, (oe, rays) in SCENES.items()}


# ------------------------------------------------------------------------------------------------ coefficient builders
def _mods():
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    return mm, ms


CONICS = [(1000.0, 300.0, 2.0), (20000.0, 500.0, 0.5), (400.0, 400.0, 45.0), (250.0, 700.0, 90.0), (np.inf, 300.0, 2.0),
          (np.inf, 300.0, 45.0), (300.0, np.inf, 2.0), (-800.0, 250.0, 3.0), (300.0, -900.0, 20.0), (800.0, -250.0, 3.0)]


def _foci(p, q, deg):
    th = np.deg2rad(LD(deg))
    ct, st = (LD(0), LD(1)) if deg == 90 else (np.cos(th), np.sin(th))
    F1 = None if np.isinf(p) else LD(abs(p)) * (np.array([-ct, 0, st]) if p > 0 else np.array([ct, 0, -st]))
    F2 = None if np.isinf(q) else LD(abs(q)) * (np.array([ct, 0, st]) if q > 0 else np.array([-ct, 0, -st]))
    return F1, F2, ct, st


@pytest.mark.parametrize("cyl", [False, True])
@pytest.mark.parametrize("p,q,deg", CONICS)
def test_conic_coefficients_pole_gradient_and_focal_property(p, q, deg, cyl):
    """c == 0.0 and grad F(0) = (0, 0, -1) exactly; points of the surface (found in long double from the fp64
    coefficients, by Newton in z from the pole's tangent plane) satisfy the defining distance property of the two foci.
    Bound: the ten coefficients are rounded to fp64 (relative 2^-53 each); at a surface point every term of F is at most
    |P| (they balance 2 b.P = -z and |grad F| ~ 1), so the rounded surface lies within 10 * 2^-53 |P| of the ideal one
    and a focal distance sum moves by at most twice that: 2.3e-15 |P| <= 2.3e-15 * scale, taken as 4e-15 * scale with
    scale = the larger finite conjugate distance (the long-double arithmetic of the check itself is at 1e-19)."""
    mm, ms = _mods()
    M = mm.MirrorConic(ms.SupportRound(10.0), p, q, deg, Cylindrical=cyl)
    co = M._quadric_coefficients()
    assert co[9] == 0.0 and tuple(co[6:9]) == (0.0, 0.0, -0.5)
    assert "Mirror" in M.type and np.array_equal(M.get_centre(), np.zeros(3))
    assert np.allclose(M.get_normal(np.zeros(3)), [0, 0, 1], atol=0)
    c = [LD(v) for v in co]
    scale = max(abs(v) for v in (p, q) if np.isfinite(v))
    ext = min(0.02 * scale, 30.0)
    x = np.linspace(-ext, ext, 41).astype(LD)[:, None] + np.zeros((1, 5), dtype=LD)
    y = np.linspace(-2.0, 2.0, 5).astype(LD)[None, :] + np.zeros((41, 1), dtype=LD)
    z = np.asarray(M._sag(x.astype(float), y.astype(float)), dtype=LD)
    assert np.isfinite(z.astype(float)).all()
    for _ in range(4):          # Newton in long double on the fp64 coefficients, from the fp64 sag
        F = c[0] * x * x + c[1] * y * y + c[2] * z * z + 2 * (c[3] * x * y + c[4] * x * z + c[5] * y * z) + 2 * c[8] * z
        dF = 2 * (c[2] * z + c[4] * x + c[5] * y + c[8])
        assert (dF < 0).all()                       # the sheet that faces +z
        z = z - F / dF
    yy = 0 * y if cyl else y                         # a cylinder: y drops out of every distance
    P = np.stack([x, yy, z], axis=-1)
    F1, F2, ct, st = _foci(p, q, deg)
    dist = lambda Fk: np.sqrt(((P - Fk) ** 2).sum(-1))
    if np.isinf(p):
        err = dist(F2) - (LD(q) - (ct * x - st * z))          # |P - F| = f - d.P, d = (cos, 0, -sin)
    elif np.isinf(q):
        err = dist(F1) - (LD(p) + (ct * x + st * z))          # |P - F| = f + d.P, d = (cos, 0, +sin)
    elif p < 0 or q < 0:
        err = (dist(F1) - dist(F2)) - (LD(abs(p)) - LD(abs(q)))
    else:
        err = (dist(F1) + dist(F2)) - (LD(p) + LD(q))
    worst = float(np.abs(err).max())
    print(f"focal property p={p} q={q} deg={deg} cyl={cyl}: {worst:.3e} mm (bound {4e-15 * scale:.3e})")
    assert worst <= 4e-15 * scale


def test_named_constructors_and_the_raw_form():
    mm, ms = _mods()
    S = ms.SupportRectangle(60.0, 10.0)
    a = mm.MirrorEllipticalCylinder(S, 1000.0, 300.0, 2.0)
    assert a._quadric_coefficients() == mm.MirrorConic(S, 1000.0, 300.0, 2.0, Cylindrical=True)._quadric_coefficients()
    assert a._quadric_coefficients()[1] == 0.0 and a.type == "Elliptical Cylinder Mirror"
    b = mm.MirrorParabolicCylinder(S, 300.0, 2.0)
    assert b._quadric_coefficients() == mm.MirrorConic(S, np.inf, 300.0, 2.0, Cylindrical=True)._quadric_coefficients()
    b2 = mm.MirrorParabolicCylinder(S, 300.0, 2.0, Collimating=True)
    assert b2._quadric_coefficients() == mm.MirrorConic(S, 300.0, np.inf, 2.0, Cylindrical=True)._quadric_coefficients()
    h = mm.MirrorHyperboloidal(S, -800.0, 250.0, 3.0)
    assert h._quadric_coefficients() == mm.MirrorConic(S, -800.0, 250.0, 3.0)._quadric_coefficients()
    hc = mm.MirrorHyperbolicCylinder(S, -800.0, 250.0, 3.0)
    assert hc._quadric_coefficients()[1] == 0.0 and "Mirror" in hc.type
    assert len({hash(a), hash(b), hash(b2), hash(h), hash(hc)}) == 5            # the hash covers the coefficients
    # the raw form: a sphere of radius R through the origin, |P|^2 / (2R) - z, given at another scale
    R = 250.0
    raw = mm.MirrorQuadric(S, 3.0 * np.eye(3) / (2 * R), [0.0, 0.0, -1.5])
    assert raw._quadric_coefficients() == (1 / (2 * R),) * 3 + (0.0,) * 3 + (0.0, 0.0, -0.5, 0.0)
    x, y = np.array([0.0, 3.0, -20.0]), np.array([0.0, 4.0, 1.0])
    assert np.allclose(raw._sag(x, y), R - np.sqrt(R * R - x * x - y * y), rtol=0, atol=1e-13)
    assert np.isnan(raw._sag(np.array([300.0]), np.array([0.0]))).all()         # no surface under that point
    n = raw.get_normal(np.array([3.0, 4.0, raw._sag(np.array([3.0]), np.array([4.0]))[0]]))
    assert np.allclose(n, np.array([-3.0, -4.0, R - (R - np.sqrt(R * R - 25.0))]) / R, atol=1e-15)
    assert len(raw.get_grid3D(200)) > 100


def test_validation_and_refused_substrates():
    mm, ms = _mods()
    import ART.ModuleDefects as md
    S = ms.SupportRound(10.0)
    for bad in (0.0, -1.0, 90.5, float("nan")):
        with pytest.raises(ValueError):
            mm.MirrorConic(S, 100.0, 100.0, bad)
    for p, q in ((0.0, 100.0), (100.0, 0.0), (np.inf, np.inf), (-100.0, -50.0), (np.inf, -50.0)):
        with pytest.raises(ValueError):
            mm.MirrorConic(S, p, q, 10.0)
    with pytest.raises(ValueError, match="MirrorPlane"):
        mm.MirrorConic(S, 100.0, -100.0, 10.0)
    with pytest.raises(ValueError):
        mm.MirrorHyperboloidal(S, 100.0, 50.0, 10.0)
    with pytest.raises(ValueError):
        mm.MirrorEllipticalCylinder(S, 100.0, -50.0, 10.0)
    with pytest.raises(ValueError):
        mm.MirrorParabolicCylinder(S, np.inf, 10.0)
    I = np.eye(3) / 100.0
    for Q, b, c in ((I, [0, 0, 0.5], 0.0), (I, [0.1, 0, -0.5], 0.0), (I, [0, 0, -0.5], 1e-3), (I, [0, 0, 0.0], 0.0),
                    (I + np.array([[0, 1e-3, 0], [0, 0, 0], [0, 0, 0]]), [0, 0, -0.5], 0.0), (I * np.nan, [0, 0, -0.5], 0.0)):
        with pytest.raises(ValueError):
            mm.MirrorQuadric(S, Q, b, c)
    M = mm.MirrorConic(S, 100.0, 100.0, 10.0)
    with pytest.raises(ValueError):
        mm.DeformedMirror(M, [md.Zernike(S, {(2, 0): 1e-5})])
    with pytest.raises(ValueError):
        mm.Grating(M, 1200.0)


def test_descriptor_carries_the_quadric_flag():
    from attosecondraytracing_amd import ModuleProcessing as mp, _abi
    mm, ms = _mods()
    oe = SCENES["ellcyl_2deg"][0]
    d, _ = mp._build_descriptor(oe, True, None)
    assert d.flags == _abi.ART_FLAG_QUADRIC and d.quadric is oe.type and d.grating is None and d.kind == _abi.ART_PLANE
    assert mp._STEPWISE_FLAGS & _abi.ART_FLAG_QUADRIC
    plane = qc.place(mm.MirrorPlane(oe.type.support), 1000.0, 2.0)
    d0, _ = mp._build_descriptor(plane, True, None)
    assert d0.flags == 0 and d0.quadric is None
    assert bytes(d)[16:] == bytes(d0)[16:]             # everything but the flags word is a plane mirror's in that pose

    class Recorder:
        def trace_quadric(self, desc, coefficients, vin, vout, n):
            self.got = (desc, tuple(coefficients), vin, vout, n)

    r = Recorder()
    assert mp._trace_one(r, d, "in", "out", 5, None, "g") == "g"
    assert r.got == (d, oe.type._quadric_coefficients(), "in", "out", 5)


# ---------------------------------------------------------------------------------------------- header against truth
def test_no_ray_of_any_scene_is_marginal(truth):
    """Mask equality is only meaningful when no ray sits on a decision boundary: no candidate hit within 1e-9 mm of a
    support edge, no root within 1e-9 of the 1e-12 threshold, no discriminant within 1e-9 (relative) of zero."""
    for name, (oe, rays) in SCENES.items():
        t = truth[name]
        live = rays[3] != 0
        roots = np.asarray(t["roots"], dtype=float)[live]
        assert (np.abs(roots[np.isfinite(roots)] - qc.T_MIN) >= qc.MARGIN).all(), name
        assert (t["edge"][live] >= qc.MARGIN).all(), name
        assert (np.abs(np.asarray(t["disc_rel"], dtype=float))[live] >= qc.MARGIN).all(), name
        assert (np.bincount(t["count"], minlength=3)[3:] == 0).all()


HARNESS = r'''
#include <cstdio>
#include <vector>
#include "art_device.h"
// in: 36 doubles (support kind, fwd[9], pos[3], centre[3], sp[6], q[6], b[3], c, n, 3 unused), then n rows of 8 doubles
// (point, vector, path, alive).  out: n rows of 9 (ray[8], alive).
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  double h[36];
  if (!f || fread(h, 8, 36, f) != 36) return 2;
  ArtElementDesc e = {};
  e.kind = ART_PLANE; e.support_kind = (int)h[0]; e.flags = ART_FLAG_QUADRIC;
  for (int i = 0; i < 9; ++i) e.fwd[i] = h[1 + i];
  for (int i = 0; i < 3; ++i) { e.pos[i] = h[10 + i]; e.centre[i] = h[13 + i]; }
  for (int i = 0; i < 6; ++i) e.sp[i] = h[16 + i];
  ArtQuadricDesc Q = {};
  for (int i = 0; i < 6; ++i) Q.q[i] = h[22 + i];
  for (int i = 0; i < 3; ++i) Q.b[i] = h[28 + i];
  Q.c = h[31];
  art::prepare_element(e);
  const long n = (long)h[32];
  std::vector<double> in(8 * n), out(9 * n);
  if (fread(in.data(), 8, 8 * n, f) != (size_t)(8 * n)) return 3;
  for (long i = 0; i < n; ++i) {
    const double* r = &in[8 * i];
    art::Ray ray = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], -7.25};
    const bool ok = r[7] != 0.0 && art::quadric_trace(e, Q, ray);
    const double o[9] = {ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, ray.path, ray.inc, ok ? 1.0 : 0.0};
    for (int k = 0; k < 9; ++k) out[9 * i + k] = o[k];
  }
  FILE* w = fopen(argv[2], "wb");
  fwrite(out.data(), 8, 9 * n, w);
  fclose(w);
  return 0;
}
'''

SUPPORT_CODE = {"round": 0, "roundhole": 1, "rect": 2, "recthole": 3, "rectrecthole": 4}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    td = tmp_path_factory.mktemp("quadric_harness")
    src, exe = td / "h.cpp", td / "h"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DART_HOST_TWIN", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "attosecondraytracing_amd", "csrc"), "-o", str(exe), str(src)])
    return td, str(exe)


@pytest.fixture(scope="module")
def header(harness):
    """name -> what the header function makes of the scene: rows [n, 9] (ray[8], alive), computed once."""
    td, exe = harness
    out = {}
    for name, (oe, (P, V, path, alive)) in SCENES.items():
        E = qc.element_spec(oe)
        n = len(P)
        head = ([SUPPORT_CODE[E["support"][0]]] + list(E["fwd"].reshape(9)) + list(E["pos"]) + list(E["centre"])
                + (list(E["support"][1:]) + [0.0] * 6)[:6] + list(E["coeff"]) + [n, 0, 0, 0])
        fin, fout = str(td / (name + ".in")), str(td / (name + ".out"))
        with open(fin, "wb") as f:
            f.write(np.asarray(head, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(np.column_stack([P, V, path, alive.astype(float)]), dtype=np.float64).tobytes())
        subprocess.check_call([exe, fin, fout])
        out[name] = np.fromfile(fout, dtype=np.float64).reshape(n, 9)
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_header_function_agrees_with_long_double_truth(header, truth, name):
    out, ref = header[name], truth[name]
    P = SCENES[name][1][0]
    got_alive = out[:, 8] != 0
    assert np.array_equal(got_alive, ref["alive"])
    res = {"point": out[:, 0:3], "vector": out[:, 3:6], "path": out[:, 6], "inc": out[:, 7]}
    worst = qc.assert_parity(res, ref, ref["alive"], name)
    print(f"{name}: {int(got_alive.sum())} of {len(P)} alive, worst deviation from the truth {worst:.2e} of the scene's magnitudes")
    lost = ~got_alive                                   # a lost ray keeps its state
    assert (out[lost, 0:3] == P[lost]).all() and (out[lost, 7] == -7.25).all()
    if got_alive.any():
        assert np.abs(np.linalg.norm(out[got_alive, 3:6], axis=1) - 1).max() <= 4e-16


# --------------------------------------------------------------------------------------- the candidate rules, one by one
def test_rule_two_candidates_the_closer_one_wins(header, truth):
    t = truth["twice_on_the_sheet"]
    live = SCENES["twice_on_the_sheet"][1][3] != 0
    assert (t["count"][live] == 2).all() and t["alive"][live].all()
    roots = np.asarray(t["roots"], dtype=float)
    got = header["twice_on_the_sheet"]
    assert np.allclose(got[live, 6], roots[live].min(axis=1), rtol=1e-13, atol=0)       # path0 = 0: the path IS t
    assert (roots[live].max(axis=1) - roots[live].min(axis=1) > 10.0).all()


def test_rule_negative_discriminant_loses_the_ray(header, truth):
    t = truth["miss"]
    assert (t["nroots"] == 0).all() and (np.asarray(t["disc_rel"], dtype=float) < 0).all()
    assert not header["miss"][:, 8].any()


def test_rule_far_side_of_a_closed_ellipse_is_rejected(header, truth):
    """From inside the ellipsoid: the root behind the start never counts; going down the ray lands on the accepted sheet,
    going up it meets only the far side (dF/dz > 0) and is lost."""
    t, (oe, rays) = truth["from_inside"], SCENES["from_inside"]
    live, down = rays[3] != 0, rays[1][:, 2] < 0
    roots = np.asarray(t["roots"], dtype=float)
    assert (roots.min(axis=1) < 0).all() and (roots.max(axis=1) > 0).all()
    assert np.array_equal(header["from_inside"][:, 8] != 0, live & down)
    assert (live & down).any() and (live & ~down).any()


def test_rule_roots_at_or_below_the_threshold_do_not_count(header, truth):
    t, (oe, rays) = truth["start_on_the_surface"], SCENES["start_on_the_surface"]
    live = rays[3] != 0
    roots = np.asarray(t["roots"], dtype=float)
    assert np.abs(roots.min(axis=1) + 1e-6).max() < 1e-9            # every ray starts 1e-6 mm past a surface point
    got = header["start_on_the_surface"]
    alive = got[:, 8] != 0
    assert np.array_equal(alive, t["alive"]) and alive.any() and (live & ~alive).any()
    assert (got[alive, 6] > 1.0).all()                              # the hit is the OTHER root, never the start


def test_rule_axis_parallel_ray_on_a_parabola_has_one_root(header, truth):
    t, (oe, rays) = truth["along_the_axis"], SCENES["along_the_axis"]
    assert (np.asarray(t["qa"], dtype=float) == 0.0).all() and (t["nroots"] == 1).all()
    got = header["along_the_axis"]
    alive = got[:, 8] != 0
    assert np.array_equal(alive, t["alive"]) and alive.any() and ((rays[3] != 0) & ~alive).any()
    f = 50.0                                                        # z = (x^2 + y^2) / (4 f): every ray goes to (0, 0, f)
    P, V = got[alive, 0:3], got[alive, 3:6]
    s = (f - P[:, 2]) / V[:, 2]
    assert np.abs(P[:, :2] + s[:, None] * V[:, :2]).max() <= 1e-12


def test_rule_support_edges_and_holes(header, truth):
    n_alive = {}
    for k in ("round", "roundhole", "rect", "recthole", "rectrecthole"):
        t = truth["support_" + k]
        live = SCENES["support_" + k][1][3] != 0
        n_alive[k] = int(t["alive"].sum())
        assert 0 < n_alive[k] < int(live.sum())                     # rays on both sides of the outer edge
        assert np.array_equal(header["support_" + k][:, 8] != 0, t["alive"])
    assert n_alive["roundhole"] < n_alive["round"] and n_alive["recthole"] < n_alive["rect"]
    assert n_alive["rectrecthole"] < n_alive["rect"]


# -------------------------------------------------------------------------------------------------------------- ABI
def _lib():
    from attosecondraytracing_amd import _abi
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import __graft_entry__ as g
    if g._stale(g.HIP_LIB, g.HIP_DEPS):
        g.build()
    return _abi, C.CDLL(g.HIP_LIB)


def test_quadric_desc_matches_the_header_and_the_library_exports_the_entry(tmp_path):
    _abi, lib = _lib()
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %u %d %d\n", sizeof(ArtQuadricDesc), offsetof(ArtQuadricDesc, q), offsetof(ArtQuadricDesc, b),
         offsetof(ArtQuadricDesc, c), ART_FLAG_QUADRIC, ART_NUM_KINDS, ART_ABI_VERSION);
  return 0;
}'''
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _abi.ArtQuadricDesc
    assert vals == [C.sizeof(D), D.q.offset, D.b.offset, D.c.offset, _abi.ART_FLAG_QUADRIC, 7, _abi.ART_ABI_VERSION]
    assert vals[0] == 80 and _abi.ART_FLAG_QUADRIC == 8
    assert hasattr(lib, "art_trace_quadric") and "art_trace_quadric" in _abi.PROTOTYPES


def test_entry_points_refuse_on_the_host_what_they_can():
    """Argument validation comes before any device work: these calls return without touching a GPU."""
    _abi, lib = _lib()
    fn = _abi.bind(lib)
    e = (_abi.ArtElementDesc * 1)()
    e[0].kind, e[0].flags = _abi.ART_PLANE, _abi.ART_FLAG_QUADRIC
    v = _abi.ArtBundleView(*([8] * 9))
    ins, outs = (_abi.ArtBundleView * 1)(v), (_abi.ArtBundleView * 1)(v)
    image = C.create_string_buffer(int(fn["art_scene_bytes"](1, 1)))
    assert fn["art_scene_pack"](e, 1, 1, ins, outs, None, C.cast(image, C.c_void_p)) == _abi.ART_ERR_UNSUPPORTED
    for call in (lambda: fn["art_trace_element"](e, C.byref(v), C.byref(v), 4, None),
                 lambda: fn["art_trace_chain"](e, 1, C.byref(v), outs, 4, None),
                 lambda: fn["art_trace_grating"](e, None, None, None, C.byref(v), 4, None),
                 lambda: fn["art_trace_guides"](e, 1, 8, 8, None)):
        assert call() == _abi.ART_ERR_UNSUPPORTED
        assert b"art_trace_quadric" in fn["art_last_error"]()
    e[0].flags = 0
    assert fn["art_scene_pack"](e, 1, 1, ins, outs, None, C.cast(image, C.c_void_p)) >= 0
    # art_trace_quadric's own validation
    e[0].flags = _abi.ART_FLAG_QUADRIC
    q = _abi.ArtQuadricDesc()
    q.q[0], q.b[2] = 0.01, -0.5
    tq = fn["art_trace_quadric"]
    assert tq(e, C.byref(q), C.byref(v), C.byref(v), 0, None) == _abi.ART_OK
    assert tq(e, C.byref(q), C.byref(v), C.byref(v), -1, None) == _abi.ART_ERR_BAD_ARG
    assert tq(None, C.byref(q), C.byref(v), C.byref(v), 0, None) == _abi.ART_ERR_BAD_ARG
    assert tq(e, None, C.byref(v), C.byref(v), 0, None) == _abi.ART_ERR_BAD_ARG
    assert tq(e, C.byref(q), None, C.byref(v), 0, None) == _abi.ART_ERR_BAD_ARG
    assert tq(e, C.byref(q), C.byref(v), None, 0, None) == _abi.ART_ERR_BAD_ARG
    hole = _abi.ArtBundleView(*([8] * 8 + [None]))
    assert tq(e, C.byref(q), C.byref(hole), C.byref(v), 4, None) == _abi.ART_ERR_BAD_ARG
    for bad in (float("nan"), float("inf")):
        q.c = bad
        assert tq(e, C.byref(q), C.byref(v), C.byref(v), 0, None) == _abi.ART_ERR_BAD_ARG
    q.c = 0.0
    q.q[0], q.b[2] = 0.0, 0.0
    assert tq(e, C.byref(q), C.byref(v), C.byref(v), 0, None) == _abi.ART_ERR_BAD_ARG       # no surface
    q.b[2] = -0.5
    e[0].n_defects, e[0].zern = 1, 8
    assert tq(e, C.byref(q), C.byref(v), C.byref(v), 0, None) == _abi.ART_ERR_BAD_ARG       # defects


# ---------------------------------------------------------------------------------------------------- device code
def test_quadric_kernel_compiles_for_gfx950_without_scratch_and_lds(tmp_path):
    """Read from the code object's metadata (the compiler's resource remarks), not from instructions."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "dev.o"), src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    blocks = re.split(r"remark: Function Name: ", p.stdout)
    mine = [b for b in blocks if "k_trace_quadric" in b.split("[", 1)[0]]
    assert len(mine) == 1, "the kernel's resource remarks were not found"
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0])
    assert m and int(m.group(1)) == 0, mine[0]
    m = re.search(r"LDS Size \[bytes/block\]: (\d+)", mine[0])
    assert m and int(m.group(1)) == 0, mine[0]
    assert re.search(r"VGPRs Spill: 0", mine[0]) and re.search(r"SGPRs Spill: 0", mine[0])

"""CPU: freeform and aspheric mirrors -- the figure and table builders, the header's per-ray function (compiled with g++)
against the long-double truth of tests/freeform_common.py on every scene, the identities that tie it to the conics, the
first-order physics at a stigmatic focus, the host shell (validation, refused wrappers, descriptor flag, routing, refusals
that need no device), the ABI mirror, and the device code's resource usage (no scratch memory, no LDS, no spills)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import freeform_common as fc
import quadric_common as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = fc.scenes()
LD = qc.LD


def _mods():
    import ART.ModuleDefects as md
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    return mm, ms, md


@pytest.fixture(scope="module")
def truth():
    assert qc.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    return {name: fc.trace(fc.element_spec(oe), *rays) for name, (oe, rays) in SCENES.items()}


# ------------------------------------------------------------------------------------------------------- constructors
def test_polynomial_and_its_dense_table():
    mm, ms, md = _mods()
    from attosecondraytracing_amd import _abi
    S = ms.SupportRectangle(60.0, 10.0)
    P = md.Polynomial(S, {(3, 0): 4e-5, (1, 0): -3e-5, (0, 2): 5e-6, (2, 1): 1e-6})
    assert P.R == S._CircumCirc() and P.max_order == 3
    t = P._dense_table()
    D, Z = _abi.ART_ZERN_DIM, _abi.ART_ZERN_DIM ** 2
    assert t.shape == (_abi.ART_ZERN_STRIDE,) and t[0] == P.R and t[1] == 3
    at = lambda block, p, q: t[2 + block * Z + p * D + q]
    assert at(0, 3, 0) == 4e-5 and at(0, 1, 0) == -3e-5 and at(0, 0, 2) == 5e-6 and at(0, 2, 1) == 1e-6
    assert at(1, 2, 0) == 3 * 4e-5 and at(1, 0, 0) == -3e-5 and at(1, 1, 1) == 2 * 1e-6        # dA/dx = (p+1) A[p+1][q]
    assert at(2, 0, 1) == 2 * 5e-6 and at(2, 2, 0) == 1e-6                                     # dA/dy = (q+1) A[p][q+1]
    assert np.count_nonzero(t[2:]) == 4 + 3 + 2
    x, y = 7.0, -2.0
    xi, eta = x / P.R, y / P.R
    h = 4e-5 * xi ** 3 - 3e-5 * xi + 5e-6 * eta ** 2 + 1e-6 * xi * xi * eta
    assert abs(P.get_offset([x, y, 0.0]) - h) <= 1e-19
    n = P.get_normal([x, y, 0.0])
    assert abs(-n[0] - (12e-5 * xi ** 2 - 3e-5 + 2e-6 * xi * eta) / P.R) <= 1e-19 and n[2] == 1.0
    assert abs(-n[1] - (1e-5 * eta + 1e-6 * xi * xi) / P.R) <= 1e-19
    assert hash(P) == hash(md.Polynomial(S, dict(P.coefficients))) != hash(md.Polynomial(S, {(3, 0): 4e-5}))
    assert md.Polynomial(S, {(1, 1): 1.0}, Radius=8.0).R == 8.0 and P.RMS() > 0 and P.PV() > 0
    for bad in ({(9, 8): 1.0}, {(-1, 0): 1.0}, {(0.5, 0): 1.0}, {(1, 0): np.nan}):
        with pytest.raises(ValueError):
            md.Polynomial(S, bad)
    with pytest.raises(ValueError):
        md.Polynomial(S, {(1, 0): 1.0}, Radius=0.0)


def test_freeform_validation_and_refused_wrappers():
    mm, ms, md = _mods()
    S = ms.SupportRound(10.0)
    base = mm.MirrorConic(S, 100.0, 100.0, 10.0)
    ok = mm.MirrorFreeform(base, [md.Zernike(S, {(16, 4): 1e-6}), md.Polynomial(S, {(2, 0): 1e-6}), md.Polynomial(S, {(0, 0): 1e-3}, Radius=3.0)])
    assert ok._fig_N == 16 and ok._fig_R == 10.0 and "Mirror" in ok.type and not hasattr(ok, "_quadric_coefficients")
    with pytest.raises(ValueError, match="order 17"):
        mm.MirrorFreeform(base, [md.Zernike(S, {(17, 1): 1e-6})])
    with pytest.raises(ValueError, match="Fourrier"):
        mm.MirrorFreeform(base, [md.Fourrier(S, 1e-6, smallest=2.0)])
    with pytest.raises(ValueError, match="radii"):
        mm.MirrorFreeform(base, [md.Polynomial(S, {(2, 0): 1e-6}), md.Polynomial(S, {(2, 0): 1e-6}, Radius=7.0)])
    with pytest.raises(TypeError):
        mm.MirrorFreeform(mm.MirrorSpherical(100.0, S), [])
    with pytest.raises(TypeError):
        mm.MirrorFreeform(base, md.Polynomial(S, {(2, 0): 1e-6}))
    for wrap in (lambda M: mm.DeformedMirror(M, [md.Zernike(S, {(2, 0): 1e-5})]), lambda M: mm.Grating(M, 1200.0)):
        with pytest.raises(ValueError):
            wrap(ok)
        with pytest.raises(ValueError):
            wrap(base)
    for bad in (lambda: mm.MirrorEvenAsphere(S, 0.0), lambda: mm.MirrorEvenAsphere(S, 100.0, Coefficients=[1e-9] * 8),
                lambda: mm.MirrorEvenAsphere(S, 100.0, Conic=np.inf)):
        with pytest.raises(ValueError):
            bad()
    assert hash(ok) != hash(mm.MirrorFreeform(base, [md.Polynomial(S, {(2, 0): 1e-6})]))
    assert len(ok.get_grid3D(200)) > 100


@pytest.mark.parametrize("R,k,alphas", [(100.0, -1.0, ()), (250.0, 0.0, (1e-9, -3e-13)), (-180.0, -2.5, (2e-9,)),
                                        (np.inf, 0.0, (1e-8, 1e-12, -1e-16)), (90.0, 0.7, (1e-10, 0, 0, 0, 0, 0, 1e-24))])
def test_even_asphere_base_and_figure_against_its_closed_form(R, k, alphas):
    """Base sag (from the fp64 coefficients, by the stable root) plus the figure table, both evaluated in long double,
    against z = c r^2 / (1 + sqrt(1 - (1 + k) c^2 r^2)) + sum alpha_i r^(2i+2): 1e-15 relative.  Each coefficient is one
    rounding of its long-double value (1.1e-16 relative; the normalisation radius is a power of two), all terms of one
    alpha have its sign, and the base's coefficients share the one rounded 1 / (2R)."""
    mm, ms, md = _mods()
    S = ms.SupportRound(18.0)
    M = mm.MirrorEvenAsphere(S, R, Conic=k, Coefficients=alphas)
    assert isinstance(M, mm.MirrorFreeform) and "Mirror" in M.type
    th = np.linspace(0, 2 * np.pi, 13)[:-1]
    r = np.linspace(0.5, 18.0, 9)
    x, y = (r[:, None] * np.cos(th)).ravel().astype(LD), (r[:, None] * np.sin(th)).ravel().astype(LD)
    r2 = x * x + y * y
    c = LD(0) if np.isinf(R) else 1 / LD(R)
    want = c * r2 / (1 + np.sqrt(1 - (1 + LD(k)) * c * c * r2))
    poly = sum(LD(a) * r2 ** (i + 1) for i, a in enumerate(alphas, start=1)) if alphas else 0 * r2
    q = [LD(v) for v in M._base_coefficients()]
    # base: q0 (x^2 + y^2) + q2 z^2 - z = 0 on the sheet through the origin
    rr = q[0] * x * x + q[1] * y * y
    base = 2 * rr / (1 + np.sqrt(1 - 4 * q[2] * rr))
    fig = M._figure(x, y)
    assert fig.dtype == LD
    for got, ref, what in ((base, want, "base"), (fig, poly, "figure")):
        scale = np.abs(ref)
        err = np.abs(got - ref)
        print(f"even asphere R={R} k={k}: {what} worst {float((err / np.where(scale > 0, scale, 1)).max()):.2e} relative")
        assert (err <= 1e-15 * scale).all(), what
    # the fp64 _sag itself: the stable root (about six roundings) plus the Horner sum
    total = np.asarray(M._sag(x.astype(float), y.astype(float)), dtype=LD)
    assert (np.abs(total - (want + poly)) <= 2e-15 * (np.abs(want) + np.abs(poly)) + 1e-300).all()


def test_sag_and_normal_against_finite_differences_of_phi():
    """Phi(x, y, z) = F(x, y, z - h) from the truth's pieces, in long double: Phi vanishes on _sag (to fp64 rounding of the
    sag, |dPhi/dz| ~ 1) and get_normal is -grad Phi / |grad Phi| by central differences (step 1e-6 mm: truncation
    ~ 1e-12 h''' , rounding 1e-19 / 1e-6)."""
    for name in ("a_ellipsoid_2deg", "b_ellipsoid_45deg", "c_order16", "e_parabola_0"):
        oe = SCENES[name][0]
        M, E = oe.type, fc.element_spec(oe)
        q = [LD(v) for v in E["coeff"]]

        def phi(x, y, z):
            h = fc.figure(E, x, y)[0]
            zp = z - h
            return (q[0] * x * x + q[1] * y * y + q[2] * zp * zp + 2 * (q[3] * x * y + q[4] * x * zp + q[5] * y * zp)
                    + 2 * (q[6] * x + q[7] * y + q[8] * zp) + q[9])

        ext = 0.45 * np.asarray(M.support._CircumRect(), dtype=float)
        x = np.array([-0.9, -0.3, 0.0, 0.4, 0.8]) * ext[0]
        y = np.array([0.7, -0.5, 0.0, 0.2, -0.9]) * ext[1]
        z = M._sag(x, y)
        assert np.abs(phi(x.astype(LD), y.astype(LD), z.astype(LD))).max() <= 4e-16 * max(1.0, np.abs(z).max())
        d = LD(1e-6)
        for xi, yi, zi in zip(x, y, z):
            X, Y, Z = (np.array([v], dtype=LD) for v in (xi, yi, zi))
            g = np.array([(phi(X + d, Y, Z) - phi(X - d, Y, Z))[0], (phi(X, Y + d, Z) - phi(X, Y - d, Z))[0],
                          (phi(X, Y, Z + d) - phi(X, Y, Z - d))[0]], dtype=LD) / (2 * d)
            n = np.asarray(-g / np.sqrt((g * g).sum()), dtype=float)
            assert np.abs(M.get_normal(np.array([xi, yi, zi])) - n).max() <= 1e-11, name
    assert np.array_equal(SCENES["a_ellipsoid_2deg"][0].type.get_centre(), np.zeros(3))


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_descriptor_carries_the_freeform_flag_only_and_the_trace_routes():
    from attosecondraytracing_amd import ModuleProcessing as mp, _abi
    mm, ms, md = _mods()
    oe = SCENES["a_ellipsoid_2deg"][0]
    d, _ = mp._build_descriptor(oe, True, None)
    assert d.flags == _abi.ART_FLAG_FREEFORM and d.freeform is oe.type and d.quadric is None and d.grating is None
    assert d.kind == _abi.ART_PLANE and d.n_defects == 0 and d.n_grid == 0
    assert mp._STEPWISE_FLAGS & _abi.ART_FLAG_FREEFORM
    base = fc.base_element(oe)
    d0, _ = mp._build_descriptor(base, True, None)
    assert d0.flags == _abi.ART_FLAG_QUADRIC and d0.freeform is None        # a conic's descriptor is what it was
    assert bytes(d)[16:] == bytes(d0)[16:]

    class Recorder:
        uploads = 0

        def from_numpy(self, a):
            self.uploads += 1
            return ("dev", a.copy())

        def trace_freeform(self, desc, coefficients, figure, vin, vout, n):
            self.got = (desc, tuple(coefficients), figure, vin, vout, n)

    r = Recorder()
    assert mp._trace_one(r, d, "in", "out", 5, None, "g") == "g"
    assert mp._trace_one(r, d, "in", "out", 5, None, "g") == "g" and r.uploads == 1
    desc, co, (tab, R, N), vin, vout, n = r.got
    assert desc is d and co == oe.type._base_coefficients() and (vin, vout, n) == ("in", "out", 5)
    assert tab[0] == "dev" and np.array_equal(tab[1], oe.type._freeform_figure()[0]) and (R, N) == (oe.type._fig_R, 3)


def _lib():
    from attosecondraytracing_amd import _abi
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import __graft_entry__ as g
    if g._stale(g.HIP_LIB, g.HIP_DEPS):
        g.build()
    return _abi, C.CDLL(g.HIP_LIB)


def test_figure_desc_matches_the_header_and_the_library_exports_the_entry(tmp_path):
    _abi, lib = _lib()
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %u %d %d %d\n", sizeof(ArtFigureDesc), offsetof(ArtFigureDesc, table), offsetof(ArtFigureDesc, radius),
         offsetof(ArtFigureDesc, order), sizeof(ArtQuadricDesc), ART_FLAG_FREEFORM, ART_ZERN_STRIDE, ART_ZERN_MAX_ORDER, ART_ABI_VERSION);
  return 0;
}'''
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _abi.ArtFigureDesc
    assert vals == [C.sizeof(D), D.table.offset, D.radius.offset, D.order.offset, C.sizeof(_abi.ArtQuadricDesc),
                    _abi.ART_FLAG_FREEFORM, _abi.ART_ZERN_STRIDE, _abi.ART_ZERN_MAX_ORDER, _abi.ART_ABI_VERSION]
    assert vals[4] == 80 and _abi.ART_FLAG_FREEFORM == 16 and _abi.ART_ABI_VERSION == 14
    assert hasattr(lib, "art_trace_freeform") and "art_trace_freeform" in _abi.PROTOTYPES


def test_entry_points_refuse_on_the_host_what_they_can():
    """Argument validation comes before any device work: these calls return without touching a GPU."""
    _abi, lib = _lib()
    fn = _abi.bind(lib)
    e = (_abi.ArtElementDesc * 1)()
    e[0].kind, e[0].flags = _abi.ART_PLANE, _abi.ART_FLAG_FREEFORM
    v = _abi.ArtBundleView(*([8] * 9))
    ins, outs = (_abi.ArtBundleView * 1)(v), (_abi.ArtBundleView * 1)(v)
    image = C.create_string_buffer(int(fn["art_scene_bytes"](1, 1)))
    q = _abi.ArtQuadricDesc()
    q.q[0], q.b[2] = 0.01, -0.5
    assert fn["art_scene_pack"](e, 1, 1, ins, outs, None, C.cast(image, C.c_void_p)) == _abi.ART_ERR_UNSUPPORTED
    for call in (lambda: fn["art_trace_element"](e, C.byref(v), C.byref(v), 4, None),
                 lambda: fn["art_trace_chain"](e, 1, C.byref(v), outs, 4, None),
                 lambda: fn["art_trace_grating"](e, None, None, None, C.byref(v), 4, None),
                 lambda: fn["art_trace_quadric"](e, C.byref(q), C.byref(v), C.byref(v), 4, None),
                 lambda: fn["art_trace_guides"](e, 1, 8, 8, None)):
        assert call() == _abi.ART_ERR_UNSUPPORTED
        assert b"art_trace_freeform" in fn["art_last_error"]()
    # art_trace_freeform's own validation
    f = _abi.ArtFigureDesc(8, 10.0, 4, 0)
    tf = fn["art_trace_freeform"]
    args = lambda **kw: [kw.get("e", e), kw.get("q", C.byref(q)), kw.get("f", C.byref(f)), kw.get("i", C.byref(v)),
                         kw.get("o", C.byref(v)), kw.get("n", 0), None]
    assert tf(*args()) == _abi.ART_OK
    assert tf(*args(n=-1)) == _abi.ART_ERR_BAD_ARG
    for k in "eqfio":
        assert tf(*args(**{k: None})) == _abi.ART_ERR_BAD_ARG, k
    hole = _abi.ArtBundleView(*([8] * 8 + [None]))
    assert tf(*args(i=C.byref(hole), n=4)) == _abi.ART_ERR_BAD_ARG
    for bad in (float("nan"), float("inf")):
        q.c = bad
        assert tf(*args()) == _abi.ART_ERR_BAD_ARG
    q.c = 0.0
    q.q[0], q.b[2] = 0.0, 0.0
    assert tf(*args()) == _abi.ART_ERR_BAD_ARG                                   # no surface
    q.b[2] = -0.5                                                                # (a plane base is one)
    assert tf(*args()) == _abi.ART_OK
    for order in (-1, 17):
        assert tf(*args(f=C.byref(_abi.ArtFigureDesc(8, 10.0, order, 0)))) == _abi.ART_ERR_BAD_ARG
    for order in (0, 16):
        assert tf(*args(f=C.byref(_abi.ArtFigureDesc(8, 10.0, order, 0)))) == _abi.ART_OK
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert tf(*args(f=C.byref(_abi.ArtFigureDesc(8, radius, 4, 0)))) == _abi.ART_ERR_BAD_ARG
    assert tf(*args(f=C.byref(_abi.ArtFigureDesc(None, 10.0, 4, 0)))) == _abi.ART_ERR_BAD_ARG
    for flags in (_abi.ART_FLAG_FREEFORM | _abi.ART_FLAG_QUADRIC, _abi.ART_FLAG_FREEFORM | _abi.ART_FLAG_GRATING):
        e[0].flags = flags
        assert tf(*args()) == _abi.ART_ERR_BAD_ARG
    e[0].flags = _abi.ART_FLAG_FREEFORM
    e[0].n_defects, e[0].zern = 1, 8
    assert tf(*args()) == _abi.ART_ERR_BAD_ARG                                   # defects


# ---------------------------------------------------------------------------------------------- header against truth
HARNESS = r'''
#include <cstdio>
#include <vector>
#include "art_device.h"
// in: 36 doubles (support kind, fwd[9], pos[3], centre[3], sp[6], q[6], b[3], c, n, 3 unused), the figure table
// (ART_ZERN_STRIDE doubles), then n rows of 8 doubles (point, vector, path, alive).  out: n rows of 10 (ray[8], alive,
// Newton steps).
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  double h[36];
  if (!f || fread(h, 8, 36, f) != 36) return 2;
  ArtElementDesc e = {};
  e.kind = ART_PLANE; e.support_kind = (int)h[0]; e.flags = ART_FLAG_FREEFORM;
  for (int i = 0; i < 9; ++i) e.fwd[i] = h[1 + i];
  for (int i = 0; i < 3; ++i) { e.pos[i] = h[10 + i]; e.centre[i] = h[13 + i]; }
  for (int i = 0; i < 6; ++i) e.sp[i] = h[16 + i];
  ArtQuadricDesc Q = {};
  for (int i = 0; i < 6; ++i) Q.q[i] = h[22 + i];
  for (int i = 0; i < 3; ++i) Q.b[i] = h[28 + i];
  Q.c = h[31];
  art::prepare_element(e);
  std::vector<double> fig(ART_ZERN_STRIDE);
  if (fread(fig.data(), 8, ART_ZERN_STRIDE, f) != (size_t)ART_ZERN_STRIDE) return 4;
  const long n = (long)h[32];
  std::vector<double> in(8 * n), out(10 * n);
  if (fread(in.data(), 8, 8 * n, f) != (size_t)(8 * n)) return 3;
  for (long i = 0; i < n; ++i) {
    const double* r = &in[8 * i];
    art::Ray ray = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], -7.25};
    int steps = 0;
    const bool ok = r[7] != 0.0 && art::freeform_trace(e, Q, (const double*)fig.data(), ray, &steps);
    const double o[10] = {ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, ray.path, ray.inc, ok ? 1.0 : 0.0, (double)steps};
    for (int k = 0; k < 10; ++k) out[10 * i + k] = o[k];
  }
  FILE* w = fopen(argv[2], "wb");
  fwrite(out.data(), 8, 10 * n, w);
  fclose(w);
  return 0;
}
'''

SUPPORT_CODE = {"round": 0, "roundhole": 1, "rect": 2, "recthole": 3, "rectrecthole": 4}


@pytest.fixture(scope="module")
def run_header(tmp_path_factory):
    """(oe, rays, tag) -> rows [n, 10] (ray[8], alive, Newton steps) of the header function."""
    td = tmp_path_factory.mktemp("freeform_harness")
    src, exe = td / "h.cpp", td / "h"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DART_HOST_TWIN", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "attosecondraytracing_amd", "csrc"), "-o", str(exe), str(src)])

    def run(oe, rays, tag):
        P, V, path, alive = rays
        E = fc.element_spec(oe)
        n = len(P)
        head = ([SUPPORT_CODE[E["support"][0]]] + list(E["fwd"].reshape(9)) + list(E["pos"]) + list(E["centre"])
                + (list(E["support"][1:]) + [0.0] * 6)[:6] + list(E["coeff"]) + [n, 0, 0, 0])
        fin, fout = str(td / (tag + ".in")), str(td / (tag + ".out"))
        with open(fin, "wb") as f:
            f.write(np.asarray(head, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(oe.type._freeform_figure()[0], dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(np.column_stack([P, V, path, np.asarray(alive).astype(float)]), dtype=np.float64).tobytes())
        subprocess.check_call([str(exe), fin, fout])
        return np.fromfile(fout, dtype=np.float64).reshape(n, 10)
    return run


@pytest.fixture(scope="module")
def header(run_header):
    return {name: run_header(oe, rays, name) for name, (oe, rays) in SCENES.items()}


def as_result(out):
    return {"point": out[:, 0:3], "vector": out[:, 3:6], "path": out[:, 6], "inc": out[:, 7], "alive": out[:, 8] != 0}


def test_no_ray_of_any_scene_is_marginal_and_every_ray_converges_early(truth):
    """Mask equality and parity only mean something when no ray sits on a decision: no candidate's refined hit within
    1e-9 mm of a support edge, no base root or refined t within 1e-9 of the 1e-12 threshold, no discriminant within 1e-9
    (relative) of zero, no |dPhi/dz| or |dF/dz| below 1e-9 -- and every candidate of the truth meets its 1e-17 tolerance at
    least two steps before the device's limit."""
    worst = 0
    for name, (oe, rays) in SCENES.items():
        t = truth[name]
        live = rays[3] != 0
        c = t["cand"][live]
        base = qc.trace(_base_spec(oe), *rays)
        roots = np.asarray(base["roots"], dtype=float)[live]
        assert (np.abs(roots[np.isfinite(roots)] - qc.T_MIN) >= qc.MARGIN).all(), name
        assert (np.abs(np.asarray(base["disc_rel"], dtype=float))[live] >= qc.MARGIN).all(), name
        assert (t["edge"][live][c] >= qc.MARGIN).all(), name
        assert (np.abs(np.asarray(t["t"], dtype=float)[live][c] - qc.T_MIN) >= qc.MARGIN).all(), name
        assert (np.abs(np.asarray(t["phi_z"], dtype=float)[live][c]) >= qc.MARGIN).all(), name
        steps = t["steps"][live][c]
        assert (steps >= 1).all() and (steps <= fc.MAX_STEPS - 2).all(), name
        worst = max(worst, int(steps.max()) if steps.size else 0)
    print(f"the truth's slowest candidate meets 1e-17 at step {worst}; the device allows {fc.MAX_STEPS}")
    assert sum(int((truth[n]["taken"] == 1).sum()) for n in SCENES) > 100          # the second candidate is exercised
    assert (truth["g_piston"]["cand"][:, 0] & ~truth["g_piston"]["ok"][:, 0])[SCENES["g_piston"][1][3] != 0].sum() > 100


def _base_spec(oe):
    return qc.element_spec(fc.base_element(oe))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_header_function_agrees_with_long_double_truth(header, truth, name):
    out, ref = header[name], truth[name]
    P = SCENES[name][1][0]
    got = as_result(out)
    assert np.array_equal(got["alive"], ref["alive"])
    worst = qc.assert_parity(got, ref, ref["alive"], name)
    a = got["alive"]
    print(f"{name}: {int(a.sum())} of {len(P)} alive, worst deviation from the truth {worst:.2e} of the scene's magnitudes, "
          f"Newton steps mean {out[a, 9].mean() if a.any() else 0:.2f} max {int(out[a, 9].max()) if a.any() else 0}")
    lost = ~a                                           # a lost ray keeps its state
    assert (out[lost, 0:3] == P[lost]).all() and (out[lost, 7] == -7.25).all()
    if a.any():
        assert np.abs(np.linalg.norm(out[a, 3:6], axis=1) - 1).max() <= 4e-16
        assert out[a, 9].max() <= fc.MAX_STEPS - 2


def test_kb_chain_of_figured_cylinders(run_header):
    """Scene (h): the header function chained through both mirrors against the truth chained through both."""
    els, focus, u2 = fc.kb_elements()
    rays = qc.point_source(1e-3)
    cur_t, cur_h = rays, rays
    for k, oe in enumerate(els):
        t = fc.trace(fc.element_spec(oe), *cur_t)
        h = as_result(run_header(oe, cur_h, f"kb{k}"))
        assert np.array_equal(h["alive"], t["alive"])
        qc.assert_parity(h, t, t["alive"], f"KB mirror {k}")
        cur_t = (t["point"], t["vector"], t["path"], t["alive"].astype(np.uint8))
        cur_h = (h["point"], h["vector"], h["path"], h["alive"].astype(np.uint8))
    assert cur_t[3].sum() > 0.8 * (rays[3] != 0).sum()


# ---------------------------------------------------------------------------------------------------------- identities
def _close(a, b, mask, bound, what):
    """Alive masks equal; points, paths within `bound` of the scene's magnitudes; directions and incidence absolute."""
    assert np.array_equal(a["alive"], b["alive"]), what
    f = lambda v: np.asarray(v, dtype=LD)
    worst = 0.0
    for key, rel in (("point", True), ("path", True), ("vector", False), ("inc", False)):
        x, y = f(a[key])[mask], f(b[key])[mask]
        if x.size == 0:
            continue
        scale = max(1.0, float(np.abs(y).max())) if rel else 1.0
        err = float(np.abs(x - y).max())
        assert err <= bound * scale, f"{what} {key}: {err:.3e} > {bound * scale:.3e}"
        worst = max(worst, err / scale)
    return worst


def test_plane_plus_paraboloid_figure_is_the_parabolic_conic_and_the_even_asphere(header, truth):
    """Scene (e): z = r^2 / (4 f) as the figure of a plane, as MirrorConic(S, inf, f, 90) and as
    MirrorEvenAsphere(S, 2 f, Conic=-1): points and paths agree to 1e-13 mm, at every tilt."""
    mm, ms, md = _mods()
    conic = qc.identity_pose(mm.MirrorConic(ms.SupportRound(20.0), np.inf, fc.PARABOLA_F, 90.0))
    for name, tilt in fc.PARABOLA_TILTS.items():
        rays = SCENES["e_" + name][1]
        ref = qc.trace(qc.element_spec(conic), *rays)
        m = ref["alive"]
        assert m.sum() > 100
        for who, res in (("truth", truth["e_" + name]), ("header", as_result(header["e_" + name])),
                         ("truth, asphere", truth["e_asphere_" + name.split("_")[1]]),
                         ("header, asphere", as_result(header["e_asphere_" + name.split("_")[1]]))):
            assert np.array_equal(res["alive"], m), who
            dp = float(np.abs(np.asarray(res["point"], dtype=LD)[m] - ref["point"][m]).max())
            dl = float(np.abs(np.asarray(res["path"], dtype=LD)[m] - ref["path"][m]).max())
            print(f"{name} ({who}) against the parabolic conic: points {dp:.2e} mm, paths {dl:.2e} mm")
            assert dp <= 1e-13 and dl <= 1e-13, who


@pytest.mark.parametrize("name", sorted(n for n in SCENES if n.endswith("_zero")))
def test_zero_figure_is_the_quadric(header, truth, name):
    oe, rays = SCENES[name]
    ref = qc.trace(_base_spec(oe), *rays)
    for who, res in (("truth", truth[name]), ("header", as_result(header[name]))):
        worst = _close(res, ref, ref["alive"], 1e-13, f"{name} ({who})")
        print(f"{name} ({who}) against quadric_trace's truth: {worst:.2e}")


def test_zernike_figure_and_its_monomials_are_one_surface(header, truth):
    for who, a, b in (("truth", truth["d_zernike"], truth["d_monomials"]),
                      ("header", as_result(header["d_zernike"]), as_result(header["d_monomials"]))):
        worst = _close(a, b, b["alive"], 1e-13, "zernike against monomials (" + who + ")")
        print(f"zernike against monomials ({who}): {worst:.2e}")
    A, B = SCENES["d_zernike"][0].type, SCENES["d_monomials"][0].type
    assert np.abs(A._fig_A - B._fig_A).max() <= 1e-20 and A._fig_R == B._fig_R and A._fig_N >= B._fig_N


# ------------------------------------------------------------------------------------------------ first-order physics
@pytest.mark.parametrize("name,q,grazing", [("a_ellipsoid_2deg", 300.0, 2.0), ("b_ellipsoid_45deg", 400.0, 45.0)])
def test_path_to_the_stigmatic_focus_changes_by_minus_two_h_cos_incidence(header, truth, name, q, grazing):
    """At the base's image focus every path is p + q; a height h shortens it by 2 h cos(incidence) to first order.  Bound:
    1e-2 of max |OPD|.  What is left -- the lateral slide of the hit, z against the normal, and the deflected ray's
    second-order miss of the focus in |F - P| -- measures 3.8e-3 on (a) and 2.1e-3 on (b)."""
    oe, rays = SCENES[name]
    g = np.deg2rad(LD(grazing))
    focus = np.asarray(oe.position, dtype=LD) + LD(q) * np.array([np.cos(2 * g), LD(0), np.sin(2 * g)])
    flat = qc.trace(_base_spec(oe), *rays)
    E = fc.element_spec(oe)
    for who, res in (("truth", truth[name]), ("header", as_result(header[name]))):
        m = res["alive"] & flat["alive"]
        assert m.sum() > 400
        P = np.asarray(res["point"], dtype=LD)
        opd = (np.asarray(res["path"], dtype=LD) + qc._norm(P - focus))[m] - qc.optical_path_to(flat, focus)[m]
        local = truth[name]["local"][m]
        h = fc.figure(E, local[:, 0], local[:, 1])[0]
        model = -2 * h * np.cos(np.asarray(truth[name]["inc"], dtype=LD)[m])
        resid = float(np.abs(opd - model).max() / np.abs(opd).max())
        print(f"{name} ({who}): max |OPD| {float(np.abs(opd).max()):.3e} mm, residual of -2 h cos(inc) {resid:.2e} of it")
        assert resid <= 1e-2


# ---------------------------------------------------------------------------------------------------- device code
def test_freeform_kernel_compiles_for_gfx950_without_scratch_lds_and_spills(tmp_path):
    """Read from the compiler's resource remarks, not from instructions."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "attosecondraytracing_amd", "csrc", "art_kernels.hip")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "dev.o"), src],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    blocks = re.split(r"remark: Function Name: ", p.stdout)
    mine = [b for b in blocks if "k_trace_freeform" in b.split("[", 1)[0]]
    assert len(mine) == 1, "the kernel's resource remarks were not found exactly once"
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0])
    assert m and int(m.group(1)) == 0, mine[0]
    m = re.search(r"LDS Size \[bytes/block\]: (\d+)", mine[0])
    assert m and int(m.group(1)) == 0, mine[0]
    assert re.search(r"VGPRs Spill: 0", mine[0]) and re.search(r"SGPRs Spill: 0", mine[0]), mine[0]
    assert len([b for b in blocks if "k_trace_quadric" in b.split("[", 1)[0]]) == 1

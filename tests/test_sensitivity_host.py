"""CPU: alignment sensitivities -- the long-double restatement of tests/sensitivity_common.py against Richardson-extrapolated
central differences of re-traces whose elements and sources were moved by the package's own methods, the header's per-ray
functions (csrc/art_tubes.h compiled with g++) against the restatement, closed forms and invariances (plane mirror, sphere,
a common shift of everything, rays lost at a mask), the ABI mirror, the entry point's host-side refusals, the Python
layer's argument errors and the linearity of predict."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import sensitivity_common as sn
import tubes_common as tb
from test_tubes_host import element_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tb.LD
# every ray of the one- and two-element scenes; every 4th of the eight elements' 54 degrees of freedom (the chief ray first)
EVERY = {"h_mixed8": 4}
NAMES = list(sn.SCENES) + ["b_plane", "e_masked"]


@pytest.fixture(scope="module")
def scenes():
    assert tb.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    S = sn.all_scenes()
    return {name: sn.prepare(S[name], EVERY.get(name, 1)) for name in NAMES}


# ------------------------------------------------------------------------------- restatement against finite differences
STEP = {0: 0.05, 1: 1e-4}                                        # mm, rad


@pytest.mark.parametrize("name", sn.SCENES)
def test_restatement_agrees_with_richardson_extrapolated_central_differences(scenes, name):
    """Every column of every group: the change of the detector hit point, the final direction and the path, within
    10 x the step-halving estimate of the finite differences, per quantity over the bundle and the three columns of a
    group that share a unit."""
    sc = scenes[name]
    a, K = sc["alive"], len(sc["els"])
    exact = sn.run(sc["specs"], sc["axes"], sc["hist"], sc["det"], sc["rot"], sc["w"], a)   # (on the long-double history)
    for g in range(K + 1):
        for unit in (0, 1):
            err, est, big = np.zeros(3), np.zeros(3), np.zeros(3)
            for i in range(3 * unit, 3 * unit + 3):
                c = sn.COLS * g + i
                fd, e = sn.fd_column(sc["els"], *sc["rays"], sc["det"], sc["plan"], g, i, STEP[unit])
                got = (exact["dXlab"][c], exact["dD"][c], exact["dL"][c])
                for q in range(3):
                    assert np.isfinite(fd[q][a]).all(), (name, g, i)
                    err[q] = max(err[q], np.abs(got[q] - fd[q])[a].max())
                    est[q] = max(est[q], e[q][a].max())
                    big[q] = max(big[q], np.abs(fd[q][a]).max())
            print(f"{name} group {g} per {('mm', 'rad')[unit]}: |restatement - finite differences| {err}, step-halving "
                  f"estimates {est}, largest entries {big}")
            assert (err <= 10 * est).all(), (name, g, unit, err, est)


# -------------------------------------------------------------------------------------------- header against restatement
HARNESS = r'''
#include <cstdio>
#include <vector>
#include "art_tubes.h"
// in: 17 doubles (n, K, det centre[3], det normal[3], det rot[9]); K x 32 doubles per element as test_tubes_host's harness;
// (K + 1) blocks of n rows (point, direction).  out: [6 (K + 1)][n] rows of 9 (dX, dY, dL, dD'[3], dX_lab[3]).
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  double h[17];
  if (!f || fread(h, 8, 17, f) != 17) return 2;
  const long n = (long)h[0];
  const int K = (int)h[1];
  std::vector<artt::Surface> S(K);
  for (int k = 0; k < K; ++k) {
    double v[32];
    if (fread(v, 8, 32, f) != 32) return 3;
    ArtElementDesc e = {};
    ArtQuadricDesc Q = {};
    e.kind = (int)v[0]; e.flags = (unsigned)v[1];
    for (int i = 0; i < 9; ++i) e.fwd[i] = v[2 + i];
    for (int i = 0; i < 3; ++i) { e.pos[i] = v[11 + i]; e.centre[i] = v[14 + i]; }
    for (int i = 0; i < 4; ++i) e.mp[i] = v[17 + i];
    for (int i = 0; i < 6; ++i) Q.q[i] = v[21 + i];
    for (int i = 0; i < 3; ++i) Q.b[i] = v[27 + i];
    Q.c = v[30];
    artt::load_surface(&e, &Q, S[k]);
  }
  const int M = 6 * (K + 1);
  std::vector<double> H((size_t)(K + 1) * n * 6), out((size_t)M * n * 9);
  if (fread(H.data(), 8, H.size(), f) != H.size()) return 4;
  for (long r = 0; r < n; ++r)
    for (int g = 0; g <= K; ++g)
      for (int i = 0; i < 6; ++i) {
        const int first = g ? g - 1 : 0;
        const double* at = &H[((size_t)first * n + r) * 6];
        artt::Column c;
        if (g == 0) artt::seed_source(i, at + 3, c);
        else artt::clear(c);
        for (int k = first; k < K; ++k) {
          const double* nx = &H[((size_t)(k + 1) * n + r) * 6];
          artt::Hit hit;
          artt::hit_of(S[k], at + 3, at, nx, hit);
          if (k == g - 1) {
            double sv[3], th[3];
            artt::motion(S[k], i, nx, sv, th);
            artt::step_moved(S[k], hit, at + 3, sv, th, c);
          } else {
            artt::step_path(S[k], hit, at + 3, c);
          }
          at = nx;
        }
        double dX, dY;
        artt::readout_column(at + 3, at, h + 2, h + 5, h + 8, c, dX, dY);
        double* o = &out[((size_t)(6 * g + i) * n + r) * 9];
        o[0] = dX; o[1] = dY; o[2] = c.dL;
        for (int q = 0; q < 3; ++q) { o[3 + q] = c.dD[q]; o[6 + q] = c.dP[q]; }
      }
  FILE* w = fopen(argv[2], "wb");
  fwrite(out.data(), 8, out.size(), w);
  fclose(w);
  return 0;
}
'''


@pytest.fixture(scope="module")
def header(scenes, tmp_path_factory):
    """name -> [M, n, 9] of the header's functions on the scene's fp64 history."""
    td = tmp_path_factory.mktemp("sens_harness")
    src, exe = td / "h.cpp", td / "h"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DART_HOST_TWIN", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "attosecondraytracing_amd", "csrc"), "-o", str(exe), str(src)])
    out = {}
    for name, sc in scenes.items():
        n, K = len(sc["rays"][0]), len(sc["els"])
        head = [n, K] + list(sc["det"][0]) + list(sc["det"][1]) + list(np.asarray(sc["rot"]).reshape(9))
        fin, fout = str(td / (name + ".in")), str(td / (name + ".out"))
        with open(fin, "wb") as f:
            f.write(np.asarray(head, dtype=np.float64).tobytes())
            for oe in sc["els"]:
                f.write(np.asarray(element_row(oe), dtype=np.float64).tobytes())
            for P, D in sc["hist64"]:
                f.write(np.ascontiguousarray(np.column_stack([P, D]), dtype=np.float64).tobytes())
        subprocess.check_call([str(exe), fin, fout])
        out[name] = np.fromfile(fout, dtype=np.float64).reshape(sn.COLS * (K + 1), n, 9)
    return out


def test_header_functions_agree_with_the_restatement(scenes, header):
    for name, sc in scenes.items():
        got, ref, a, K = header[name], sc["ref"], sc["alive"], len(sc["els"])
        worst = {"dX": sn.compare_columns(got[:, :, 0], ref["dX"], a, name + " dX", K),
                 "dY": sn.compare_columns(got[:, :, 1], ref["dY"], a, name + " dY", K),
                 "dL": sn.compare_columns(got[:, :, 2], ref["dL"], a, name + " dL", K),
                 "dD": sn.compare_columns(got[:, :, 3:6], ref["dD"], a, name + " dD", K),
                 "dXlab": sn.compare_columns(got[:, :, 6:9], ref["dXlab"], a, name + " dXlab", K)}
        print(f"{name}: header against restatement {worst}")


# ------------------------------------------------------------------------------------------------------- closed forms
def both(scenes, header, name):
    ref = scenes[name]["ref"]
    yield "restatement", {k: ref[k] for k in ("dX", "dY", "dL", "dD", "dXlab")}
    h = header[name]
    yield "header", {"dX": tb.ld(h[:, :, 0]), "dY": tb.ld(h[:, :, 1]), "dL": tb.ld(h[:, :, 2]), "dD": tb.ld(h[:, :, 3:6]),
                     "dXlab": tb.ld(h[:, :, 6:9])}


def test_plane_mirror_closed_forms(scenes, header):
    """b_plane, 45 degrees: shifts in the mirror's plane and yaw change nothing; pitch and roll turn every ray by
    2 r x D' (2 rad/rad and 2 cos(incidence) rad/rad on the chief ray)."""
    sc = scenes["b_plane"]
    Dp = sc["hist"][-1][1]
    r = sc["axes"][0]
    for who, res in both(scenes, header, "b_plane"):
        col = lambda i: 6 + i
        for key in ("dXlab", "dD", "dL"):
            per_mm, per_rad = np.abs(res[key][col(2)]).max(), np.abs(res[key][[col(3), col(4)]]).max()
            for i, scale in ((0, per_mm), (1, per_mm), (5, per_rad)):
                assert np.abs(res[key][col(i)]).max() <= 1e-10 * max(scale, 1e-300), (who, key, i)
        for i in (3, 4):
            want = 2 * np.cross(r[i - 3][None, :], Dp)
            assert np.abs(res["dD"][col(i)] - want).max() <= 1e-10 * 2, (who, i)
        turn = lambda i: np.sqrt(tb._dot(res["dD"][col(i)], res["dD"][col(i)]))[0]
        assert abs(turn(4) - 2) <= 1e-10 * 2 and abs(turn(3) - 2 * np.cos(np.deg2rad(LD(45)))) <= 1e-10 * 2, who


def test_normal_shift_changes_the_path_by_two_cosines(scenes):
    """The chief ray of b_plane onto a detector perpendicular to the outgoing beam: |dL| = 2 cos(45 degrees) per mm, and
    shorter for a mirror that moves towards the light."""
    sc = scenes["b_plane"]
    P, D = (np.asarray(v[0], dtype=float) for v in sc["hist"][-1])
    det = (P + 150.0 * D, -D)
    res = sn.run(sc["specs"], sc["axes"], sc["hist"], det, sn.detector_rot(det[1]), None, sc["alive"])
    want = 2 * np.cos(np.deg2rad(LD(45)))
    assert abs(res["dL"][6 + 2][0] + want) <= 1e-10 * want


def test_sphere_rotations_are_shifts_of_its_centre_of_curvature(scenes, header):
    """A rotation about r_i through the position is a rotation about the centre of curvature, which changes nothing, plus
    the shift r_i x (centre of curvature - position)."""
    sc = scenes["b_sphere"]
    s, r = sc["specs"][0], sc["axes"][0]
    to_centre = -(s["centre"] @ s["fwd"])                         # fwd^T (0 - centre): the optic frame's origin from pos
    assert abs(np.sqrt(to_centre @ to_centre) - 1000) < 1e-6
    for who, res in both(scenes, header, "b_sphere"):
        for key in ("dX", "dY", "dL", "dD"):
            scale = np.abs(res[key][9:12]).max()
            for i in range(3):
                coeff = r @ np.cross(r[i], to_centre)
                want = sum(coeff[j] * res[key][6 + j] for j in range(3))
                assert np.abs(res[key][9 + i] - want).max() <= 1e-10 * scale, (who, key, i)


@pytest.mark.parametrize("name", list(sn.SCENES) + ["e_masked"])
def test_a_common_shift_of_everything_is_a_detector_moved_the_other_way(scenes, header, name):
    sc = scenes[name]
    a, K = sc["alive"], len(sc["els"])
    e = tb.ld([0.3, -0.5, 0.8])
    nd, Dp = tb.ld(sc["det"][1]), sc["hist64"][-1][1]
    slide = (nd @ e) / (tb.ld(Dp) @ nd)
    want = {"dXlab": e[None, :] - tb.ld(Dp) * slide[:, None], "dL": -slide, "dD": np.zeros((len(a), 3), dtype=LD)}
    for who, res in both(scenes, header, name):
        for key, target in want.items():
            total = sum(e[i] * res[key][i] for i in range(3))
            for k in range(K):
                coeff = sc["axes"][k] @ e
                total = total + sum(coeff[j] * res[key][6 * (k + 1) + j] for j in range(3))
            scale = max(np.abs(res[key][u][a]).max() for u in range(6 * (K + 1)) if u % 6 < 3)
            assert np.abs(total - target)[a].max() <= 1e-10 * scale, (name, who, key)


def test_rays_dead_in_any_view_stay_out(scenes):
    sc = scenes["e_masked"]
    ref, a = sc["ref"], sc["alive"]
    assert 100 < a.sum() < len(a) - 100 and ref["table"][0, 0] == a.sum()
    w = tb.ld(sc["w"])
    assert abs(ref["table"][0, 1] - w[a].sum()) <= 1e-15 * w.sum()
    assert np.isnan(ref["dX"][:, ~a]).all() and np.isfinite(ref["dX"][:, a]).all()
    # a mask that moves changes nothing behind it
    for key in ("dX", "dY", "dL", "dD"):
        scale = np.abs(ref[key][:, a]).max()
        assert np.abs(ref[key][12:18][:, a]).max() <= 1e-10 * scale, key


# ------------------------------------------------------------------------------------------------------------ plumbing
def _lib():
    from attosecondraytracing_amd import _abi
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import __graft_entry__ as g
    if g._stale(g.HIP_LIB, g.HIP_DEPS):
        g.build()
    return _abi, C.CDLL(g.HIP_LIB)


def test_sensitivity_job_matches_the_header(tmp_path):
    _abi, lib = _lib()
    fields = [n for n, _ in _abi.ArtSensitivityJob._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "art_hip.h"\nint main(void) {\n  printf("%zu", sizeof(ArtSensitivityJob));\n'
           + "".join(f'  printf(" %zu", offsetof(ArtSensitivityJob, {n}));\n' for n in fields)
           + '  printf(" %d %d %d\\n", ART_SENS_DOUBLES, ART_SENS_COLS, ART_ABI_VERSION);\n  return 0;\n}\n')
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    J = _abi.ArtSensitivityJob
    assert vals == [C.sizeof(J)] + [getattr(J, n).offset for n in fields] + [_abi.ART_SENS_DOUBLES, _abi.ART_SENS_COLS,
                                                                             _abi.ART_ABI_VERSION]
    assert _abi.ART_ABI_VERSION == 14 and _abi.ART_SENS_DOUBLES == 16 and _abi.ART_SENS_COLS == 6
    for name, (res, args) in ((n, _abi.PROTOTYPES[n]) for n in ("art_sensitivities", "art_sensitivities_scratch_doubles")):
        assert hasattr(lib, name)
    assert _abi.PROTOTYPES["art_sensitivities_scratch_doubles"] == (C.c_int64, [C.POINTER(J), C.c_int32])
    assert _abi.PROTOTYPES["art_sensitivities"] == (C.c_int, [C.c_void_p, C.POINTER(J), C.c_int32, C.c_void_p, C.c_void_p,
                                                              C.c_void_p])


def test_entry_point_refuses_on_the_host_what_it_can():
    """Argument validation comes before any device work: these calls return without touching a GPU."""
    _abi, lib = _lib()
    fn = _abi.bind(lib)
    K = 2
    elems = (_abi.ArtElementDesc * K)()
    for e in elems:
        e.kind = _abi.ART_TORUS
    quad = (_abi.ArtQuadricDesc * K)()
    good = _abi.ArtDetectorDesc()
    good.normal[:] = [0.0, 0.6, 0.8]

    def job(**kw):
        j = _abi.ArtSensitivityJob()
        j.views, j.elems, j.n_elems, j.n, j.det = 8, C.addressof(elems), K, 1000, good
        for k, v in kw.items():
            setattr(j, k, v)
        return (_abi.ArtSensitivityJob * 1)(j)

    sd, rt = fn["art_sensitivities_scratch_doubles"], fn["art_sensitivities"]
    per_tile = 8 + 12 * 6                                        # row 0 and six columns per workgroup
    assert sd(job(), 1) == 3 * 4 * per_tile and sd(job(n=0), 1) == 3 * per_tile
    for bad in (dict(n=-1), dict(n_elems=0), dict(n_elems=65), dict(views=None), dict(elems=None)):
        assert sd(job(**bad), 1) == _abi.ART_ERR_BAD_ARG, bad
        assert rt(8, job(**bad), 1, 8, 8, None) == _abi.ART_ERR_BAD_ARG, bad
    assert sd(job(n=(1 << 28) + 1), 1) == _abi.ART_ERR_UNSUPPORTED
    assert sd(None, 1) == _abi.ART_ERR_BAD_ARG and sd(job(), 0) == _abi.ART_ERR_BAD_ARG
    assert sd(job(), _abi.ART_TUBE_MAX_JOBS + 1) == _abi.ART_ERR_BAD_ARG
    for args in ((None, job(), 1, 8, 8, None), (8, None, 1, 8, 8, None), (8, job(), 1, None, 8, None), (8, job(), 1, 8, None, None)):
        assert rt(*args) == _abi.ART_ERR_BAD_ARG
    d = _abi.ArtDetectorDesc()                                   # no detector: a zero normal
    assert sd(job(det=d), 1) == _abi.ART_ERR_BAD_ARG and b"detector" in fn["art_last_error"]()
    d.normal[:] = [0.0, 0.0, 2.0]
    assert sd(job(det=d), 1) == _abi.ART_ERR_BAD_ARG
    d.normal[:] = [0.0, 0.6, 0.8]
    d.centre[0] = float("nan")
    assert sd(job(det=d), 1) == _abi.ART_ERR_BAD_ARG
    assert sd(job(origin=(C.c_double * 3)(0.0, float("inf"), 0.0)), 1) == _abi.ART_ERR_BAD_ARG
    elems[1].kind = 7
    assert sd(job(), 1) == _abi.ART_ERR_BAD_ARG
    elems[1].kind = _abi.ART_PLANE
    for setup, word in ((dict(flags=_abi.ART_FLAG_GRATING), b"grating"), (dict(flags=_abi.ART_FLAG_FREEFORM), b"freeform"),
                        (dict(flags=_abi.ART_FLAG_PERTURBED_NORMAL), b"defects"), (dict(n_defects=1), b"defects"),
                        (dict(n_grid=1), b"defects")):
        for k, v in setup.items():
            setattr(elems[1], k, v)
        assert sd(job(), 1) == _abi.ART_ERR_UNSUPPORTED and rt(8, job(), 1, 8, 8, None) == _abi.ART_ERR_UNSUPPORTED
        msg = fn["art_last_error"]()
        assert b"element 1" in msg and word in msg, msg
        for k in setup:
            setattr(elems[1], k, 0)
    elems[0].flags = _abi.ART_FLAG_QUADRIC
    assert sd(job(), 1) == _abi.ART_ERR_BAD_ARG                  # a quadric without the table
    assert sd(job(quadrics=C.addressof(quad)), 1) == 3 * 4 * per_tile


def _chain(els, **src):
    return types.SimpleNamespace(optical_elements=els, source_rays=types.SimpleNamespace(**src))


def test_python_layer_argument_errors():
    """Raised before the history is touched: no device needed."""
    import ART.ModuleDefects as md
    import ART.ModuleDetector as mdet
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    from attosecondraytracing_amd import sensitivity
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    S = ms.SupportRound(10.0)
    plane = tb.qc.identity_pose(mm.MirrorPlane(S))
    det = mdet.Detector(np.zeros(3), np.zeros(3), np.array([0.0, 0.0, 1.0]))
    with pytest.raises(TypeError, match="Source"):
        sensitivity.sensitivities([(_chain([plane]), dict(Detector=det, Source="point"))])
    with pytest.raises(TypeError, match="need a Detector"):
        sensitivity.sensitivities([(_chain([plane]), dict())])
    with pytest.raises(TypeError, match="no centre and normal"):
        sensitivity.sensitivity(_chain([plane]), mdet.Detector(np.zeros(3)))
    with pytest.raises(ValueError, match="optical elements"):
        sensitivity.sensitivity(_chain([]), det)
    conic = mm.MirrorConic(S, 100.0, 100.0, 10.0)
    for optic, word in ((mm.DeformedMirror(mm.MirrorPlane(S), [md.Zernike(S, {(2, 0): 1e-5})]), "defects"),
                        (mm.Grating(mm.MirrorPlane(S), 1200.0), "grating"),
                        (mm.MirrorFreeform(conic, [md.Polynomial(S, {(2, 0): 1e-6})]), "freeform")):
        with pytest.raises(NotImplementedError, match="element 1 .*" + word):
            sensitivity.sensitivity(_chain([plane, tb.qc.identity_pose(optic)]), det)
    assert OpticalChain.get_Sensitivities.__defaults__ == (False,)


def test_result_follows_the_table_and_predict_is_linear(scenes):
    """A Sensitivities built on the host from the restatement's table of d_twisted: names, units, the derived quantities
    and predict, which takes moves as shift_OE / rotate_OE / shift_source / tilt_source do (mm, degrees)."""
    from attosecondraytracing_amd import sensitivity
    sc = scenes["d_twisted"]
    T = np.asarray(sc["ref"]["table"], dtype=float)
    s = sensitivity.Sensitivities(T, (0.0, 0.0, 0.0), 2, None)
    assert len(s.names) == 18 and s.names[0] == ("source", "shift_x") and s.names[5] == ("source", "tilt_z")
    assert s.names[6:12] == [(0, d) for d in sn.ELEMENT_DOFS] and s.names[17] == (1, "yaw")
    assert s.units == (["mm"] * 3 + ["rad"] * 3) * 3 and s.count == int(sc["alive"].sum()) and s.dX is None
    sw = T[0, 1]
    assert np.allclose(s.centroid, T[1:, 0:2] / sw, rtol=1e-15) and np.allclose(s.pointing, T[1:, 9:12] / sw, rtol=1e-15)
    assert np.allclose(s.delay, T[1:, 2] / sw / 299792458000 * 1e15, rtol=1e-14)
    m = T[0, 2:5] / sw
    assert np.allclose(s.spot_variance[:, 0], 2 * (T[1:, 3] / sw - m[0] * T[1:, 0] / sw), rtol=1e-12)
    assert np.allclose(s.path_variance, 2 * (T[1:, 5] / sw - m[2] * T[1:, 2] / sw), rtol=1e-12)
    assert np.allclose(s.spread[:, 2] ** 2, T[1:, 8] / sw - (T[1:, 2] / sw) ** 2, rtol=1e-9)
    assert np.array_equal(s.quantity("delay"), s.delay) and np.array_equal(s.quantity("spread_y"), s.spread[:, 1])
    one = s.predict(shift_OE=(0, "normal", 0.1))
    two = s.predict(rotate_OE=[(1, "pitch", 0.01), (-1, "yaw", -0.02)])
    src = s.predict(shift_source=(np.array([0.0, 3.0, 4.0]), 0.5), tilt_source=(np.array([0.0, 0.0, 2.0]), 0.01))
    assert np.allclose(one["centroid"], 0.1 * s.centroid[s.index(0, "shift_normal")], rtol=1e-14)
    assert np.isclose(two["delay"], np.deg2rad(0.01) * s.delay[s.index(1, "pitch")] - np.deg2rad(0.02) * s.delay[s.index(1, "yaw")], rtol=1e-12)
    assert np.allclose(src["pointing"], 0.5 * (0.6 * s.pointing[1] + 0.8 * s.pointing[2]) + np.deg2rad(0.01) * s.pointing[5], rtol=1e-12)
    both_moves = s.predict(shift_OE=(0, "normal", 0.1), rotate_OE=[(1, "pitch", 0.01), (-1, "yaw", -0.02)])
    twice = s.predict(shift_OE=(0, "normal", 0.2))
    for key in ("centroid", "delay", "pointing"):
        assert np.allclose(both_moves[key], one[key] + two[key], rtol=1e-12, atol=0)
        assert np.allclose(twice[key], 2 * np.asarray(one[key]), rtol=1e-14, atol=0)
    import matplotlib
    matplotlib.use("Agg")
    import ART.ModuleAnalysisAndPlots as mplots
    fig = mplots.SensitivityChart(s, "delay", PerUnit=(0.01, 1e-6))
    bars = [[p.get_height() for p in ax.patches] for ax in fig.axes]
    assert len(fig.axes) == 2 and [len(b) for b in bars] == [9, 9]
    assert np.allclose(bars[0], 0.01 * s.delay[[c for c, u in enumerate(s.units) if u == "mm"]], rtol=1e-12, atol=0)
    assert np.allclose(bars[1], 1e-6 * s.delay[[c for c, u in enumerate(s.units) if u == "rad"]], rtol=1e-12, atol=0)
    matplotlib.pyplot.close(fig)
    with pytest.raises(ValueError, match="quantity"):
        s.quantity("strehl")
    for bad in (dict(shift_OE=(0, "pitch", 1.0)), dict(rotate_OE=(0, "normal", 1.0)), dict(shift_source=("vert", 1.0)),
                dict(tilt_source=(np.zeros(3), 1.0))):
        with pytest.raises(ValueError):
            s.predict(**bad)
    with pytest.raises(IndexError):
        s.predict(shift_OE=(2, "normal", 1.0))

"""CPU: ray tubes (differential ray tracing) -- the long-double restatement of tests/tubes_common.py against its own
finite-difference truth, the header's per-ray functions (csrc/art_tubes.h compiled with g++) against the restatement, the
closed forms (Coddington on a toroid's chief ray and on a convex sphere's, the stigmatic ellipsoid and paraboloid, the
plane mirror, Malus-Dupin), the admission rule of the added scenes, one quadric described in two optic frames, the ABI
mirror, the entry point's host-side refusals and the Python layer's argument errors."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import tubes_common as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = tb.LD


@pytest.fixture(scope="module")
def scenes():
    assert tb.HAVE_LD, "numpy.longdouble has no extended precision on this platform"
    S = {**tb.scenes(), **tb.scenes_more()}
    for sc in S.values():
        sc["hist"], sc["alive"], sc["plan"] = tb.trace_history(sc["els"], *sc["rays"])
        sc["specs"] = [tb.spec_of(oe) for oe in sc["els"]]
        # what the device reads is an fp64 history: both the restatement and the header get the rounded one
        sc["hist64"] = [(np.asarray(P, dtype=float), np.asarray(D, dtype=float)) for P, D in sc["hist"]]
        sc["ref"] = tb.run(sc["specs"], sc["hist64"], sc["source"], sc["det"], sc["w"], sc["alive"])
    return S


LOSSY = {"h_c3": 673, "h_c2": 490}                               # survivors of the golden chains that lose rays


def test_no_ray_is_lost_except_behind_the_mask(scenes):
    for name, sc in scenes.items():
        n = len(sc["rays"][0])
        if name == "e_masked":
            assert n == 1001 and 100 < sc["alive"].sum() < n - 100
        elif name in LOSSY:
            assert n == tb.N_RAYS and sc["alive"].sum() == LOSSY[name], (name, int(sc["alive"].sum()))
        else:
            assert n == tb.N_RAYS and sc["alive"].all(), name
        assert sc["alive"][0], name                              # the chief ray


# ------------------------------------------------------------------------------- restatement against finite differences
MORE = ["h_rotated_quadric", "h_hyperboloid", "h_convex_sphere", "h_convex_cylinder", "h_convex_quadric", "h_mixed8", "h_c3",
        "h_c2"]


@pytest.mark.parametrize("name", ["a_toroid", "b_plane", "b_sphere", "b_parabola", "b_ellipsoid", "b_cylinder", "c_kb",
                                  "d_twisted", "e_masked"] + MORE)
def test_restatement_agrees_with_richardson_extrapolated_central_differences(scenes, name):
    """The Jacobian of the final point (on the detector, or on the last surface) and direction with respect to the two
    source parameters: within 10 x the step-halving estimate of the finite differences, per quantity over the bundle."""
    sc = scenes[name]
    eps = 2e-4 if sc["source"] == "point" else 1e-2
    a = sc["alive"]
    exact = tb.run(sc["specs"], sc["hist"], sc["source"], sc["det"], sc["w"], a)      # (on the long-double history)
    dX, dD, eX, eD = tb.fd_jacobian(sc["els"], *sc["rays"], sc["source"], sc["det"], sc["plan"], eps)
    for what, got, fd, est in (("dX", exact["dX"], dX, eX), ("dD", exact["dD"], dD, eD)):
        err, bound = np.abs(got - fd)[a].max(), 10 * est[a].max()
        print(f"{name} {what}: |restatement - finite differences| {float(err):.2e}, step-halving estimate "
              f"{float(est[a].max()):.2e}, largest entry {float(np.abs(fd[a]).max()):.2e}")
        assert np.isfinite(fd[a]).all() and err <= bound, (name, what, float(err), float(bound))


# -------------------------------------------------------------------------------------------- header against restatement
HARNESS = r'''
#include <cstdio>
#include <vector>
#include "art_tubes.h"
// in: 10 doubles (n, K, seed, has_det, det centre[3], det normal[3]); K x 32 doubles (kind, flags, fwd[9], pos[3],
// centre[3], mp[4], q[6], b[3], c, unused); (K + 1) blocks of n rows (point, direction).  out: n rows of 8 (solid angle,
// area, kappa1, kappa2, axis[3], asymmetry).
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  double h[10];
  if (!f || fread(h, 8, 10, f) != 10) return 2;
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
  std::vector<double> H((size_t)(K + 1) * n * 6), out((size_t)n * 8);
  if (fread(H.data(), 8, H.size(), f) != H.size()) return 4;
  for (long i = 0; i < n; ++i) {
    const double* r = &H[(size_t)i * 6];
    artt::Tube T;
    artt::seed((int)h[2], r + 3, T);
    for (int k = 0; k < K; ++k) {
      const double* nx = &H[((size_t)(k + 1) * n + i) * 6];
      artt::step(S[k], r + 3, r, nx, T);
      r = nx;
    }
    artt::Readout R;
    artt::readout(T, r + 3, r, h[3] != 0.0, h + 4, h + 7, R);
    const double o[8] = {R.solid_angle, R.area, R.kappa1, R.kappa2, R.axis[0], R.axis[1], R.axis[2], R.asymmetry};
    for (int q = 0; q < 8; ++q) out[(size_t)i * 8 + q] = o[q];
  }
  FILE* w = fopen(argv[2], "wb");
  fwrite(out.data(), 8, out.size(), w);
  fclose(w);
  return 0;
}
'''


def element_row(oe, spec=None):
    """The harness' 32 doubles of an element; spec: a tubes_common.reframed description whose frame, centre and
    coefficients replace the element's own."""
    from attosecondraytracing_amd import ModuleGeometry as mgeo, _abi
    M = oe.type
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    quad = hasattr(M, "_quadric_coefficients")
    mp = (list(M._abi_params()) + [0.0] * 4)[:4]
    co = list(M._quadric_coefficients()) if quad else [0.0] * 10
    centre = M.get_centre()
    if spec is not None:
        fwd, centre, co = spec["fwd"], spec["centre"], spec["coeff"]
    return ([float(M._abi_kind), float(_abi.ART_FLAG_QUADRIC if quad else 0)] + list(np.asarray(fwd, dtype=float).reshape(9))
            + list(np.asarray(oe.position, dtype=float)) + list(np.asarray(centre, dtype=float)) + [float(v) for v in mp]
            + [float(v) for v in co] + [0.0])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """(name, scene, rows) -> [n, 8] of the header's functions on the scene's fp64 history, the elements as `rows`."""
    td = tmp_path_factory.mktemp("tubes_harness")
    src, exe = td / "h.cpp", td / "h"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DART_HOST_TWIN", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "attosecondraytracing_amd", "csrc"), "-o", str(exe), str(src)])

    def run(name, sc, rows):
        n, K = len(sc["rays"][0]), len(sc["els"])
        det = sc["det"]
        head = [n, K, 0 if sc["source"] == "point" else 1, 0 if det is None else 1] + \
            (list(det[0]) + list(det[1]) if det is not None else [0.0] * 6)
        fin, fout = str(td / (name + ".in")), str(td / (name + ".out"))
        with open(fin, "wb") as f:
            f.write(np.asarray(head, dtype=np.float64).tobytes())
            for row in rows:
                assert len(row) == 32
                f.write(np.asarray(row, dtype=np.float64).tobytes())
            for P, D in sc["hist64"]:
                f.write(np.ascontiguousarray(np.column_stack([P, D]), dtype=np.float64).tobytes())
        subprocess.check_call([str(exe), fin, fout])
        return np.fromfile(fout, dtype=np.float64).reshape(n, 8)
    return run


@pytest.fixture(scope="module")
def header(scenes, harness):
    """name -> [n, 8] of the header's functions on the scene's fp64 history."""
    return {name: harness(name, sc, [element_row(oe) for oe in sc["els"]]) for name, sc in scenes.items()}


def as_result(out):
    return {"solid_angle": out[:, 0], "area": out[:, 1], "kappa": out[:, 2:4].T, "axis": out[:, 4:7], "asymmetry": out[:, 7]}


def test_header_functions_agree_with_the_restatement(scenes, header):
    for name, sc in scenes.items():
        got = as_result(header[name])
        tb.check_against_restatement(got, sc["ref"], name)
        a = sc["alive"]
        assert np.abs(np.linalg.norm(got["axis"][a], axis=1) - 1).max() <= 1e-14
        assert (got["kappa"][0][a] <= got["kappa"][1][a]).all()
    assert tb.axes_error(as_result(header["a_toroid"])["axis"], scenes["a_toroid"]["ref"]["axis"], scenes["a_toroid"]["alive"]) <= tb.PARITY


@pytest.mark.parametrize("name", MORE)
def test_added_scene_is_admitted_with_a_tenth_of_the_bar_to_spare(scenes, header, name):
    """A scene may judge the device at PARITY only if the fp64 header on the CPU, same formulas and same history, stays a
    factor of ten inside it (and every curvature is well conditioned: check_against_restatement asserts cond < COND_MAX)."""
    sc = scenes[name]
    got, ref, a = as_result(header[name]), sc["ref"], sc["alive"]
    assert (ref["cond"][a] < tb.COND_MAX).all()
    worst = {key: tb.compare(got[key], ref[key], a, f"{name} {key}", bar=tb.PARITY / 10) for key in ("solid_angle", "area", "kappa")}
    k1, k2 = (np.nan_to_num(np.asarray(k, dtype=float)) for k in ref["kappa"])
    apart = a & (k2 - k1 >= tb.AXIS_GAP * (np.abs(k1) + np.abs(k2)))
    worst["axis"] = tb.axes_error(got["axis"], ref["axis"], apart)
    print(f"{name}: header against restatement {worst}; axes compared on {int(apart.sum())} of {int(a.sum())} rays")
    assert worst["axis"] <= tb.PARITY / 10, (name, worst)
    if name == "h_hyperboloid":                                  # (not the stigmatic pose: its axes are compared)
        assert 2 * apart.sum() >= a.sum()
    if name == "h_rotated_quadric":
        q = sc["specs"][0]["coeff"]
        assert all(v != 0 for v in q[:6]) and q[6] == 0 and q[7] == 0


def test_the_same_quadric_in_another_optic_frame(scenes, harness, header):
    """h_rotated_quadric's surface described again with its optic frame turned by 50 degrees about (1, 2, 3) and shifted by
    (3, -2, 5) mm: a quadric with b[0], b[1], c and a centre that no Python class produces.  The history is the same
    rays; both descriptions agree with the restatement of each, and with one another, at the bar."""
    sc = scenes["h_rotated_quadric"]
    spec = sc["specs"][0]
    moved = tb.reframed(spec)
    assert all(v != 0 for v in moved["coeff"]) and moved["centre"].all()
    P = tb.ld(sc["hist64"][1][0][sc["alive"]])                  # the hit points lie on both forms
    for s in (spec, moved):
        x = (P - s["pos"]) @ s["fwd"].T + s["centre"]
        q = s["coeff"]
        Q = np.array([[q[0], q[3], q[4]], [q[3], q[1], q[5]], [q[4], q[5], q[2]]], dtype=LD)
        F = tb._dot(x @ Q, x) + 2 * (x @ np.array(q[6:9], dtype=LD)) + q[9]
        assert np.abs(F).max() <= 1e-12 * np.abs(tb._dot(x @ Q, x)).max()
    ref2 = tb.run([moved], sc["hist64"], sc["source"], sc["det"], sc["w"], sc["alive"])
    got = as_result(header["h_rotated_quadric"])
    got2 = as_result(harness("h_rotated_quadric_moved", sc, [element_row(sc["els"][0], moved)]))
    a = sc["alive"]
    tb.check_against_restatement(got, sc["ref"], "own frame")
    tb.check_against_restatement(got2, ref2, "moved frame")
    tb.check_against_restatement(got2, sc["ref"], "moved frame, header against the restatement in the own frame")
    worst = {key: tb.compare(got2[key], got[key], a, "the two descriptions: " + key) for key in ("solid_angle", "area", "kappa")}
    worst["axis"] = tb.axes_error(got2["axis"], got["axis"], a)
    print(f"the header on the two descriptions of one quadric: {worst}")
    assert worst["axis"] <= tb.PARITY


def both(scenes, header, name):
    ref = scenes[name]["ref"]
    yield "restatement", {k: np.asarray(ref[k], dtype=LD) for k in ("solid_angle", "area", "kappa")}
    yield "header", as_result(header[name])


# ------------------------------------------------------------------------------------------------------- closed forms
def test_coddington_on_the_toroids_chief_ray(scenes, header):
    """1/s + 1/s_t = 2 / (R_t cos i), 1/s + 1/s_s = 2 cos i / r_s with R_t = R + r = 1000, r_s = 100, i = 70 deg, s = 500."""
    s, Rt, rs, ci = LD(500), LD(1000), LD(100), np.cos(np.deg2rad(LD(70)))
    st, ss = 1 / (2 / (Rt * ci) - 1 / s), 1 / (2 * ci / rs - 1 / s)
    assert abs(float(st) - 259.90168229) < 1e-8 and abs(float(ss) - 206.59437398) < 1e-8
    for who, res in both(scenes, header, "a_toroid"):
        f1, f2 = -1 / LD(res["kappa"][0][0]), -1 / LD(res["kappa"][1][0])
        print(f"{who}: chief-ray foci {float(f1):.10f} (sagittal) {float(f2):.10f} (tangential) mm")
        assert abs(f1 - ss) <= 1e-10 * ss and abs(f2 - st) <= 1e-10 * st, who


def test_coddington_on_the_convex_spheres_chief_ray(scenes, header):
    """A sphere that curves away from the light, R = 1000, i = 25 deg, s = 500: 1/s + 1/s_t = -2 / (R cos i),
    1/s + 1/s_s = -2 cos i / R, both images virtual; on the detector 150 mm on the wavefront's radii are 150 - s_t, 150 - s_s."""
    s, R, ci = LD(500), LD(1000), np.cos(np.deg2rad(LD(25)))
    st, ss = 1 / (-2 / (R * ci) - 1 / s), 1 / (-2 * ci / R - 1 / s)
    assert st < 0 and ss < 0
    want = sorted([1 / (150 - st), 1 / (150 - ss)])
    for who, res in both(scenes, header, "h_convex_quadric"):
        k1, k2 = LD(res["kappa"][0][0]), LD(res["kappa"][1][0])
        print(f"{who}: chief-ray curvatures {float(k1):.12e} {float(k2):.12e} 1/mm, Coddington {float(want[0]):.12e} {float(want[1]):.12e}")
        assert abs(k1 - want[0]) <= 1e-10 * want[1] and abs(k2 - want[1]) <= 1e-10 * want[1], who
        assert (tb.ld(res["kappa"][0])[scenes["h_convex_quadric"]["alive"]] > 0).all(), who     # diverging everywhere


def test_ellipsoid_is_stigmatic_for_every_ray(scenes, header):
    sc = scenes["b_ellipsoid"]
    P = sc["hist"][1][0]
    r1, r2 = tb.qc._norm(P - tb.ld(sc["F1"])), tb.qc._norm(tb.ld(sc["F2"]) - P)
    for who, res in both(scenes, header, "b_ellipsoid"):
        for k in res["kappa"]:
            assert np.abs(tb.ld(k) + 1 / r2).max() <= 1e-10 * (1 / r2).max(), who
        assert np.abs(np.abs(tb.ld(res["solid_angle"])) - (r1 / r2) ** 2).max() <= 1e-10 * ((r1 / r2) ** 2).max(), who
    assert float(((r1 / r2) ** 2).max() / ((r1 / r2) ** 2).min()) > 1.1          # the sine condition is violated


def test_plane_mirror_keeps_the_solid_angle_and_spreads_the_area(scenes, header):
    sc = scenes["b_plane"]
    (P0, _), (P1, D1) = sc["hist"]
    C, nd = tb.ld(sc["det"][0]), tb.ld(sc["det"][1])
    L = tb.qc._norm(P1 - P0) + ((C - P1) @ nd) / (D1 @ nd)
    area = L * L / np.abs(D1 @ nd)
    for who, res in both(scenes, header, "b_plane"):
        assert np.abs(np.abs(tb.ld(res["solid_angle"])) - 1).max() <= 1e-10, who
        assert np.abs(np.abs(tb.ld(res["area"])) - area).max() <= 1e-10 * area.max(), who
        for k in res["kappa"]:
            assert np.abs(tb.ld(k) - 1 / L).max() <= 1e-10 * (1 / L).max(), who


def test_paraboloid_brings_a_plane_wave_to_its_focus(scenes, header):
    sc = scenes["b_parabola"]
    dist = tb.qc._norm(tb.ld(sc["focus"]) - sc["hist"][1][0])
    for who, res in both(scenes, header, "b_parabola"):
        for k in res["kappa"]:
            assert np.abs(-1 / tb.ld(k) - dist).max() <= 1e-10 * dist.max(), who


def test_malus_dupin_on_the_twisted_toroids(scenes, header):
    for name in ("d_twisted", "e_masked"):
        ref, out = scenes[name]["ref"], as_result(header[name])
        a = scenes[name]["alive"]
        rel = out["asymmetry"][a] / (np.abs(out["kappa"][0][a]) + np.abs(out["kappa"][1][a]))
        print(f"{name}: asymmetry of the curvature matrix {float(ref['row'][10]):.2e} (restatement) {rel.max():.2e} (header)")
        assert ref["row"][10] <= 1e-10 and rel.max() <= 1e-10


# ------------------------------------------------------------------------------------------------------------ plumbing
def _lib():
    from attosecondraytracing_amd import _abi
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import __graft_entry__ as g
    if g._stale(g.HIP_LIB, g.HIP_DEPS):
        g.build()
    return _abi, C.CDLL(g.HIP_LIB)


def test_tube_job_matches_the_header(tmp_path):
    _abi, lib = _lib()
    fields = [n for n, _ in _abi.ArtTubeJob._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "art_hip.h"\nint main(void) {\n  printf("%zu", sizeof(ArtTubeJob));\n'
           + "".join(f'  printf(" %zu", offsetof(ArtTubeJob, {n}));\n' for n in fields)
           + '  printf(" %d %d %d %d %d %d\\n", ART_TUBE_POINT, ART_TUBE_PLANE, ART_TUBE_MAX_ELEMS, ART_TUBE_MAX_JOBS, '
             'ART_TUBE_DOUBLES, ART_ABI_VERSION);\n  return 0;\n}\n')
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    J = _abi.ArtTubeJob
    assert vals == [C.sizeof(J)] + [getattr(J, n).offset for n in fields] + [
        _abi.ART_TUBE_POINT, _abi.ART_TUBE_PLANE, _abi.ART_TUBE_MAX_ELEMS, _abi.ART_TUBE_MAX_JOBS, _abi.ART_TUBE_DOUBLES,
        _abi.ART_ABI_VERSION]
    assert _abi.ART_ABI_VERSION == 14
    for name in ("art_ray_tubes", "art_ray_tubes_scratch_doubles"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES


def test_entry_point_refuses_on_the_host_what_it_can():
    """Argument validation comes before any device work: these calls return without touching a GPU."""
    _abi, lib = _lib()
    fn = _abi.bind(lib)
    K = 2
    elems = (_abi.ArtElementDesc * K)()
    for e in elems:
        e.kind = _abi.ART_TORUS
    quad = (_abi.ArtQuadricDesc * K)()

    def job(**kw):
        j = _abi.ArtTubeJob()
        j.views, j.elems, j.n_elems, j.seed, j.n, j.weight = 8, C.addressof(elems), K, _abi.ART_TUBE_POINT, 1000, 8
        for k, v in kw.items():
            setattr(j, k, v)
        return (_abi.ArtTubeJob * 1)(j)

    sd, rt = fn["art_ray_tubes_scratch_doubles"], fn["art_ray_tubes"]
    assert sd(job(), 1) == 11 * 4                                # 11 partial sums per tile of 256 slots
    assert sd(job(n=0), 1) == 11
    for bad in (dict(n=-1), dict(n_elems=0), dict(n_elems=65), dict(seed=2), dict(seed=-1), dict(views=None),
                dict(elems=None), dict(weight=None)):
        assert sd(job(**bad), 1) == _abi.ART_ERR_BAD_ARG, bad
        assert rt(8, job(**bad), 1, 8, 8, None) == _abi.ART_ERR_BAD_ARG, bad
    assert sd(job(n=(1 << 28) + 1), 1) == _abi.ART_ERR_UNSUPPORTED
    assert sd(None, 1) == _abi.ART_ERR_BAD_ARG and sd(job(), 0) == _abi.ART_ERR_BAD_ARG
    assert sd(job(), _abi.ART_TUBE_MAX_JOBS + 1) == _abi.ART_ERR_BAD_ARG
    for args in ((None, job(), 1, 8, 8, None), (8, None, 1, 8, 8, None), (8, job(), 1, None, 8, None), (8, job(), 1, 8, None, None)):
        assert rt(*args) == _abi.ART_ERR_BAD_ARG
    d = _abi.ArtDetectorDesc()
    d.normal[:] = [0.0, 0.0, 2.0]
    assert sd(job(has_detector=1, det=d), 1) == _abi.ART_ERR_BAD_ARG
    d.normal[:] = [0.0, 0.6, 0.8]
    assert sd(job(has_detector=1, det=d), 1) == 44
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
    assert sd(job(quadrics=C.addressof(quad)), 1) == 44


def _chain(els, **src):
    return types.SimpleNamespace(optical_elements=els, source_rays=types.SimpleNamespace(**src))


def test_python_layer_argument_errors():
    """Raised before the history is touched: no device needed."""
    import ART.ModuleDefects as md
    import ART.ModuleDetector as mdet
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    from attosecondraytracing_amd import tubes
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    S = ms.SupportRound(10.0)
    plane = tb.qc.identity_pose(mm.MirrorPlane(S))
    with pytest.raises(TypeError, match="Weights"):
        tubes.ray_tubes([(_chain([plane], source_kind="point"), dict(Weights=1))])
    with pytest.raises(ValueError, match="Source="):
        tubes.tubes(_chain([plane]))
    with pytest.raises(ValueError, match="Source must be"):
        tubes.tubes(_chain([plane]), Source="sphere")
    with pytest.raises(ValueError, match="optical elements"):
        tubes.tubes(_chain([], source_kind="point"))
    with pytest.raises(TypeError, match="no centre and normal"):
        tubes.tubes(_chain([plane], source_kind="plane"), Detector=mdet.Detector(np.zeros(3)))
    conic = mm.MirrorConic(S, 100.0, 100.0, 10.0)
    for optic, word in ((mm.DeformedMirror(mm.MirrorPlane(S), [md.Zernike(S, {(2, 0): 1e-5})]), "defects"),
                        (mm.Grating(mm.MirrorPlane(S), 1200.0), "grating"),
                        (mm.MirrorFreeform(conic, [md.Polynomial(S, {(2, 0): 1e-6})]), "freeform")):
        with pytest.raises(NotImplementedError, match="element 1 .*" + word):
            tubes.tubes(_chain([plane, tb.qc.identity_pose(optic)], source_kind="point"))
    assert OpticalChain.get_RayTubes.__defaults__ == (None, None, True)

"""CPU: the coating math of csrc/art_coating.h (compiled by g++ into the CPU twin, the same header as k_polarisation)
against the mpmath truth of tests/coating_truth.py: the scalar helpers exp_cw, sincos_cw, csqrt_up and cdiv; rs, rp
formed from two directions over the coating x angle matrix of tests/coating_cases.py; the whole per-ray pass through
chains with several coatings and a mask; and the NumPy oracle (tests/polarisation_common.py) and
Coating.reflectance against the same truth.  Bars: 1e-14 absolute on rs, rp (|r| <= 1); within 1e-6 rad of a lossless
medium's critical angle 1e-14 + 4 eps cos^2 t |dr / d cos^2 t| (the rounding of cos t from fp64 directions)."""
import ctypes as C
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import coating_cases as cc
import coating_truth as ct
import polarisation_common as pcm
import twin_backend

EPS = 2.0 ** -52
BAR = 1e-14


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(twin_backend.build_twin())
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    from attosecondraytracing_amd import _abi
    cp = C.POINTER(_abi.ArtCoating)
    lib.art_cpu_coating_rs_rp.argtypes = [cp, C.c_double, dp, dp, C.c_int64, dp, dp]
    lib.art_cpu_polarisation_rays.argtypes = [cp, ip, C.c_int32, dp, C.c_int64, C.c_void_p, C.c_double, dp, dp, dp]
    lib.art_cpu_exp_cw.argtypes = [dp, C.c_int64, dp]
    lib.art_cpu_sincos_cw.argtypes = [dp, C.c_int64, dp, dp]
    lib.art_cpu_csqrt_up.argtypes = [dp, C.c_int64, dp]
    lib.art_cpu_cdiv.argtypes = [dp, dp, C.c_int64, dp]
    for f in ("art_cpu_coating_rs_rp", "art_cpu_polarisation_rays", "art_cpu_exp_cw", "art_cpu_sincos_cw",
              "art_cpu_csqrt_up", "art_cpu_cdiv"):
        getattr(lib, f).restype = None
    return lib


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _cplx(a):
    a = np.asarray(a)
    return a[..., 0] + 1j * a[..., 1]


# ------------------------------------------------------------------------------------------- the scalar helpers
def _ulp(x):
    return np.spacing(np.abs(x))


def test_exp_cw(lib):
    rng = np.random.default_rng(1)
    x = np.concatenate([np.linspace(-745.0, 0.0, 20001), rng.uniform(-745.0, 0.0, 5000), -(10.0 ** rng.uniform(-20, 0, 500)),
                        [-744.44007192138121, -708.39641853226408, -708.39641853226431, -1e-300, -0.0, 0.0,
                         -0.34657359027997264, -0.34657359027997270]])
    out = np.empty_like(x)
    lib.art_cpu_exp_cw(_c(x), len(x), out)
    with mp.workdps(40):
        want = [mp.exp(mpf(float(v))) for v in x]
    wf = np.array([float(w) for w in want])
    err = np.array([abs(mpf(float(o)) - w) for o, w in zip(out, want)], dtype=float)
    normal = wf >= 2.0 ** -1022
    assert np.all(err[normal] <= _ulp(wf[normal])), x[normal][np.argmax(err[normal] / _ulp(wf[normal]))]
    assert np.all(err[~normal] <= 2.0 ** -1074)


def test_sincos_cw(lib):
    rng = np.random.default_rng(2)
    k = np.concatenate([np.arange(-64, 65), rng.integers(-2 ** 39, 2 ** 39, 400), [2 ** 39 - 1, -(2 ** 39) + 1]])
    with mp.workdps(60):
        near = np.array([float(int(q) * mp.pi / 2) for q in k])
    x = np.concatenate([near, np.nextafter(near, np.inf), np.nextafter(near, -np.inf), rng.uniform(-10, 10, 5000),
                        np.sign(rng.normal(size=3000)) * 2.0 ** rng.uniform(-30, 40, 3000), [0.0, -0.0, 2.0 ** 40,
                                                                                               -(2.0 ** 40), 1e-300]])
    x = x[np.abs(x) <= 2.0 ** 40]
    sn, cs = np.empty_like(x), np.empty_like(x)
    lib.art_cpu_sincos_cw(_c(x), len(x), sn, cs)
    worst = 0.0
    with mp.workdps(60):
        for v, s, c in zip(x, sn, cs):
            m = mpf(float(v))
            worst = max(worst, float(abs(mpf(float(s)) - mp.sin(m))), float(abs(mpf(float(c)) - mp.cos(m))))
    assert worst <= 2.3e-16, worst


def _csqrt_truth(z):
    with mp.workdps(40):
        w = mp.sqrt(mp.mpc(z.real, z.imag))
        if w.imag < 0:
            w = -w
        return complex(float(w.real), float(w.imag))


def test_csqrt_up(lib):
    rng = np.random.default_rng(3)
    n = 4000
    mag = 10.0 ** rng.uniform(-100, 100, n)
    ph = rng.uniform(-math.pi, math.pi, n)
    z = list(mag * np.exp(1j * ph))
    # Re < 0 with tiny Im (either sign), Re > 0 with tiny Im, the axes, signed zeros
    for r in (1.0, 3e-3, 2.0e-6, 7e50):
        for t in (1e-30, -1e-30, 1e-300, -1e-300, 5e-324, -5e-324):
            z += [complex(-r, t * r), complex(r, t * r)]
    z += [complex(0.0, 2.0), complex(0.0, -2.0), complex(-4.0, 0.0), complex(4.0, 0.0), complex(-4.0, -0.0),
          complex(4.0, -0.0), complex(0.0, 0.0), complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)]
    z = np.array(z)
    out = np.empty((len(z), 2))
    lib.art_cpu_csqrt_up(_c(np.stack([z.real, z.imag], 1)), len(z), out)
    w = out[:, 0] + 1j * out[:, 1]
    assert np.all(out[:, 1] >= 0.0)                  # the branch Im >= 0 (-0.0 counts: it is >= 0)
    want = np.array([_csqrt_truth(v) for v in z])
    for part in (np.real, np.imag):
        err = np.abs(part(w) - part(want))
        assert np.all(err <= 2 * _ulp(part(want))), (z[np.argmax(err / np.maximum(_ulp(part(want)), 1e-320))])
    assert np.all(w[np.abs(z) == 0] == 0)


def test_cdiv(lib):
    rng = np.random.default_rng(4)
    n = 3000
    a = (rng.normal(size=n) + 1j * rng.normal(size=n)) * 10.0 ** rng.uniform(-150, 150, n)
    ang = rng.uniform(0, 2 * math.pi, n)
    b = np.exp(1j * ang) * 10.0 ** rng.uniform(-150, 150, n)
    # |b.re| = |b.im| exactly, in all four quadrants, and lopsided b (component ratios up to 1e150)
    m = 10.0 ** rng.uniform(-150, 150, 400)
    sg = rng.choice([-1.0, 1.0], (400, 2))
    b[:400] = sg[:, 0] * m + 1j * sg[:, 1] * m
    r = 10.0 ** rng.uniform(-150, 150, 400) * rng.choice([-1.0, 1.0], 400)
    b[400:800] = np.where(rng.random(400) < 0.5, r * 1e-2 + 1j * 1e-2, 1e-2 + 1j * r * 1e-2)
    out = np.empty((n, 2))
    lib.art_cpu_cdiv(_c(np.stack([a.real, a.imag], 1)), _c(np.stack([b.real, b.imag], 1)), n, out)
    got = out[:, 0] + 1j * out[:, 1]
    worst = 0.0
    with mp.workdps(40):
        for x, y, g in zip(a, b, got):
            q = mp.mpc(x.real, x.imag) / mp.mpc(y.real, y.imag)
            worst = max(worst, float(abs(mp.mpc(g.real, g.imag) - q) / abs(q)))
    assert worst <= 4 * EPS, worst


# ------------------------------------------------------------------------------------------- rs, rp from directions
def _twin_rs_rp(lib, coat, k, A, B):
    n = len(A)
    rs, rp = np.empty((n, 2)), np.empty((n, 2))
    lib.art_cpu_coating_rs_rp(C.byref(coat._struct()), k, _c(A), _c(B), n, rs, rp)
    return _cplx(rs), _cplx(rp)


def _matrix(name):
    """Directions, bars and truths of one coating's row of the matrix: lists A, B, bar, (rs, rp), labels."""
    make, k, crit = cc.COATINGS[name]
    coat = make()
    A, B, bars, truth, labels = [], [], [], [], []
    for R in cc.rotations(3):
        for lab, s, c, near in cc.angles(crit):
            a, b = cc.pair(s, c, R)
            t = ct.rs_rp(coat, a, b, k)
            bar = BAR
            if near:
                cm = ct.cos_incidence(a, b)
                bar += 4 * EPS * float(cm * cm * ct.drdc2(coat, cm, k))
            A.append(a); B.append(b); bars.append(bar); labels.append(lab)
            truth.append((ct.to_complex(t[0]), ct.to_complex(t[1])))
    return coat, k, np.array(A), np.array(B), np.array(bars), np.array(truth), labels


_MATRIX = {}


def matrix(name):
    if name not in _MATRIX:
        _MATRIX[name] = _matrix(name)
    return _MATRIX[name]


def _check(got, truth, bars, labels, what):
    err = np.maximum(np.abs(got[0] - truth[:, 0]), np.abs(got[1] - truth[:, 1]))
    bad = [(labels[i], float(err[i])) for i in np.nonzero(err > bars)[0]]
    assert not bad, f"{what}: {len(bad)} of {len(err)} beyond the bar, e.g. {bad[:6]}"
    return float(err.max())


@pytest.mark.parametrize("name", list(cc.COATINGS))
def test_rs_rp_from_directions(lib, name):
    coat, k, A, B, bars, truth, labels = matrix(name)
    _check(_twin_rs_rp(lib, coat, k, A, B), truth, bars, labels, f"art_coating.h, {name}")


def test_matrix_covers_the_edges():
    """The matrix does reach what it claims: the fallback frame, six material slots, 256 layers, kappa > n, a layer
    phase X that underflows, and an interface with Re(kz_a kz_b) < 0 whose Nevot-Croce factor exceeds 1."""
    for lab, s, c in cc.ANGLES[:2]:
        a, b = cc.pair(s, c, cc.rotations(2)[1])
        assert np.linalg.norm(np.cross(a, b)) < 1e-12
    assert len(cc.six_materials().materials) == 6 and len(cc.mosi(128).layers) == 256
    ag = cc.COATINGS["metal633"][0]().substrate
    assert ag.imag > ag.real
    with mp.workdps(40):
        mo = cc.COATINGS["absorber_1mm"][0]().layers[0]
        q = ct._kz(ct._mpN(mo[0]), mpf(1))
        assert mp.exp(-2 * q.imag * cc.K_XUV * mo[1]) < mpf(2) ** -1100
        coat = cc.COATINGS["metal_on_metal"][0]()
        for c in (mpf(1), mpf("0.01")):
            qa, qb = ct._kz(ct._mpN(coat.layers[0][0]), c), ct._kz(ct._mpN(coat.substrate), c)
            assert (qa * qb).real < 0
            assert abs(mp.exp(-2 * qa * qb * (cc.K_VIS * coat.roughness) ** 2)) > 1


@pytest.mark.parametrize("name", list(cc.COATINGS))
def test_oracle_against_truth(name):
    """The NumPy oracle that judges the GPU tests (polarisation_common) agrees with the truth to the same bar."""
    coat, k, A, B, bars, truth, labels = matrix(name)
    cos = np.linalg.norm(B - A, axis=1) / 2
    _check(pcm.coating_rs_rp(coat, None, k, cos=cos), truth, bars, labels, f"oracle, {name}")


def test_reflectance_at_grazing_incidence_against_truth():
    g = np.array([30e-3, 3e-3, 1e-3, 0.3e-3, 0.1e-3])
    theta = math.pi / 2 - g
    for name in ("gold", "mosi40", "si", "six"):
        make, k, _ = cc.COATINGS[name]
        coat = make()
        rs, rp = coat.reflectance(theta, 2 * math.pi / k)
        for t, s, p in zip(theta, rs, rp):
            with mp.workdps(40):
                want = ct.rs_rp_at(coat, mp.cos(mpf(float(t))), k)
            assert max(abs(s - ct.to_complex(want[0])), abs(p - ct.to_complex(want[1]))) <= BAR, (name, t)


# ------------------------------------------------------------------------------------------- the per-ray pass
def _chain_dirs(rng, n, grazing):
    """n rays through 4 elements (coating, mask, coating, coating): the direction before each and after the last."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    dirs = [d]
    for e in range(4):
        if e == 1:
            dirs.append(d.copy())
            continue
        g = grazing[(np.arange(n) + e) % len(grazing)]
        u = np.cross(d, rng.normal(size=(n, 3)))
        u /= np.linalg.norm(u, axis=1)[:, None]
        nrm = -np.sin(g)[:, None] * d + np.cos(g)[:, None] * u       # angle of incidence pi / 2 - g
        d = d - 2 * np.sum(d * nrm, axis=1)[:, None] * nrm
        d /= np.linalg.norm(d, axis=1)[:, None]
        dirs.append(d)
    return dirs


@pytest.mark.parametrize("state", ["s", "p", "circular", "unpolarised"])
def test_per_ray_pass_through_chains(lib, state):
    rng = np.random.default_rng(12)
    n = 18
    grazing = np.array([1e-4, 1e-3, 3e-3, 0.03, 0.4, 1.2, math.pi / 2 - 1e-3])
    dirs = _chain_dirs(rng, n, grazing)
    coats = [cc.mosi(128), None, cc.six_materials(), cc.gold()]
    table = (type(coats[0]._struct()) * 3)(*[c._struct() for c in coats if c is not None])
    idx = np.array([0, -1, 1, 2], dtype=np.int32)
    k = cc.K_XUV
    s1 = np.cross(dirs[0], dirs[1])
    s1 /= np.linalg.norm(s1, axis=1)[:, None]
    p1 = np.cross(dirs[0], s1)
    D = np.stack(dirs)
    for i in range(n):
        P = {"s": s1[i], "p": p1[i], "circular": (s1[i] + 1j * p1[i]) / math.sqrt(2), "unpolarised": None}[state]
        Pb = None if P is None else _c(np.stack([np.real(P), np.imag(P)], 1).reshape(-1))
        T, E0, E1 = np.empty(1), np.empty((1, 6)), np.empty((1, 6))
        lib.art_cpu_polarisation_rays(table, idx, 4, _c(D[:, i:i + 1]), 1, None if Pb is None else Pb.ctypes.data, k,
                                      T, E0, E1)
        want = ct.chain([d[i] for d in dirs], coats, k, P)
        for got, Ew in zip((E0[0], E1[0]), want["E"]):
            Ew = np.array([ct.to_complex(z) for z in Ew])
            Eg = got[0::2] + 1j * got[1::2]
            assert np.abs(Eg - Ew).max() <= BAR, (state, i)         # (|E| = 1 at the source, |r| <= 1)
        assert abs(T[0] - float(want["T"])) <= 2 * BAR, (state, i)

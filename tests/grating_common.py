"""Oracle and scenes of the grating tests (tests/test_grating_host.py, tests/test_gpu_grating.py).

`diffract` is a NumPy restatement of the per-ray grating math (csrc/art_device.h, grating_hit / grating_diffract) in the
literal form of the grating equation -- s = 1 - |v_t|^2 --, generic in the float type: float64 is the ORACLE the GPU
results are compared with, numpy.longdouble (64-bit significand) the TRUTH the oracle and the header function are judged
by (as tests/truth_common.py does for mirrors).  Substrates: plane, sphere, torus -- the kinds the tests use; rays
start inside the torus tube, as they do for a mirror.  Scenes are built by hand on the host (no device needed): optic at
`distance` on the x axis, plane of incidence = the lab's xz plane, major axis in it."""
import numpy as np

import ART.ModuleMirror as mmirror
import ART.ModuleOpticalElement as moe
import ART.ModuleSupport as msupp
from attosecondraytracing_amd import ModuleGeometry as mgeo

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 1e-18
N_RAYS = 4099            # not a multiple of 256: the last tile is partial
PARITY = 1e-10           # the project's parity bound: relative for points and paths, absolute for directions


def _norm(v):
    return np.sqrt((v * v).sum(axis=-1))


def kahan(U, V):
    return 2 * np.arctan2(_norm(U - V), _norm(U + V))


def element_spec(oe):
    """Plain numbers of an OpticalElement whose optic is a Grating (or a bare mirror: N = 0)."""
    G = oe.type
    M = getattr(G, "Mirror", G)
    kind = {"Plane Mirror": "plane", "SphericalCC Mirror": "sphere", "Toroidal Mirror": "torus"}[M.type]
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    sup = M.support
    q = G._groove_vector() if hasattr(G, "_groove_vector") else (1.0, 0.0)
    return {"kind": kind, "mp": [float(v) for v in M._abi_params()], "centre": np.asarray(M.get_centre(), dtype=float),
            "pos": np.asarray(oe.position, dtype=float), "fwd": np.array(fwd, dtype=float),
            "support": ("round", float(sup.radius)) if hasattr(sup, "radius") else ("rect", float(sup.dimX), float(sup.dimY)),
            "q": q, "N": float(getattr(G, "lines_per_mm", 0.0)), "m": int(getattr(G, "order", 0))}


def _hit(E, A, u, T):
    """(t, valid) of the undeformed substrate in the optic frame."""
    one = np.ones(len(A), dtype=T)
    if E["kind"] == "plane":
        t = -A[:, 2] / u[:, 2]
        return t, t > 0
    if E["kind"] == "sphere":
        R = T(E["mp"][0])
        b, c = (u * A).sum(1), (A * A).sum(1) - R * R          # |u| = 1: t^2 + 2 b t + c
        disc = b * b - c
        ok = disc >= 0
        t = -b + np.sqrt(np.where(ok, disc, one))              # the far root: the concave side (z < 0), origin inside
        z = A[:, 2] + t * u[:, 2]
        return t, ok & (t > 1e-12) & (z < 0)
    R, r = T(E["mp"][0]), T(E["mp"][1])
    t = (-(R + r) - A[:, 2]) / u[:, 2]                          # start on the tangent plane at the vertex: outside the tube
    for _ in range(14):                                         # monotone Newton on the convex (rho - R)^2 + y^2 - r^2
        P = A + t[:, None] * u
        rho = np.sqrt(P[:, 0] ** 2 + P[:, 2] ** 2)
        F = (rho - R) ** 2 + P[:, 1] ** 2 - r * r
        dF = 2 * ((rho - R) * (P[:, 0] * u[:, 0] + P[:, 2] * u[:, 2]) / rho + P[:, 1] * u[:, 1])
        t = t - F / dF
    z = A[:, 2] + t * u[:, 2]
    return t, np.isfinite(t) & (t > 1e-12) & (z < -R)


def _normal(E, P, T):
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    if E["kind"] == "plane":
        return np.stack([0 * x, 0 * x, 0 * x + 1], axis=1)
    if E["kind"] == "sphere":
        g = -P
    else:
        R, r = T(E["mp"][0]), T(E["mp"][1])
        S = x * x + y * y + z * z
        g = -np.stack([x * (S - R * R - r * r), y * (S + R * R - r * r), z * (S - R * R - r * r)], axis=1)
    return g / _norm(g)[:, None]


def diffract(E, point, vector, path, alive, wavelength, grooves=None, T=np.float64, order=None, N=None):
    """The grating E acting on rays (lab frame).  Returns a dict: alive, point, vector, path, inc, grooves (lab frame,
    entries of lost rays meaningless), and u, v (optic frame), s = 1 - |v_t|^2, hit (the ray met the substrate)."""
    t_ = lambda a: np.asarray(a, dtype=T)
    F, C, pos = t_(E["fwd"]), t_(E["centre"]), t_(E["pos"])
    m = T(E["m"] if order is None else order)
    N = T(E["N"] if N is None else N)
    q0 = np.array([T(E["q"][0]), T(E["q"][1]), T(0)], dtype=T)
    A = (t_(point) - pos) @ F.T + C
    u = t_(vector) @ F.T
    with np.errstate(all="ignore"):
        t, ok = _hit(E, A, u, T)
        P = A + t[:, None] * u
        x, y = P[:, 0], P[:, 1]
        if E["support"][0] == "round":
            ok = ok & (x * x + y * y <= T(E["support"][1]) ** 2)
        else:
            ok = ok & (np.abs(x) <= T(E["support"][1]) / 2) & (np.abs(y) <= T(E["support"][2]) / 2)
        n = _normal(E, P, T)
        g = (m * T(wavelength) * N) * q0
        dn = (u * n).sum(1)
        gt = g[None, :] - (n @ g)[:, None] * n
        vt = (u - dn[:, None] * n) + gt
        s = 1 - (vt * vt).sum(1)
        v = vt - (np.sign(dn) * np.sqrt(np.where(s > 0, s, 1)))[:, None] * n
        inc = kahan(-u, n)
        G = N * ((P - C) @ q0)
        vl = v @ F
        vl = vl / _norm(vl)[:, None]
    hit = ok & (np.asarray(alive) != 0)
    g_in = 0 if grooves is None else t_(grooves)
    return {"alive": hit & (s > 0), "hit": hit, "point": (P - C) @ F + pos, "vector": vl, "path": t_(path) + t, "inc": inc,
            "grooves": g_in + m * G, "u": u, "v": v, "s": s}


# ------------------------------------------------------------------------------------------------------------ scenes
def _vogel(n, radius):
    k = np.arange(n, dtype=float)
    rr, th = np.sqrt(k / n) * radius, np.pi * (3.0 - np.sqrt(5.0)) * k
    return rr * np.cos(th), rr * np.sin(th)


def point_source(half_angle, n=N_RAYS):
    """(point, vector, path, alive): cone about +x from the origin, every 7th slot dead."""
    a, b = _vogel(n, np.tan(half_angle))
    v = np.stack([np.ones(n), a, b], axis=1)
    v /= _norm(v)[:, None]
    alive = (np.arange(n) % 7 != 6).astype(np.uint8)
    return np.zeros((n, 3)), v, np.zeros(n), alive


def plane_wave(radius, n=N_RAYS):
    a, b = _vogel(n, radius)
    alive = (np.arange(n) % 7 != 6).astype(np.uint8)
    return np.stack([np.zeros(n), a, b], axis=1), np.tile([1.0, 0.0, 0.0], (n, 1)), np.zeros(n), alive


def place(optic, distance, incidence_deg):
    """OpticalElement at `distance` on the x axis, incidence angle in the lab's xz plane, major axis in that plane."""
    th = np.deg2rad(incidence_deg)
    normal = np.array([-np.cos(th), 0.0, np.sin(th)])
    major = np.array([np.sin(th), 0.0, np.cos(th)])
    return moe.OpticalElement(optic, np.array([float(distance), 0.0, 0.0]), normal, major)


def plane_grating(N, m, groove_angle, size=400.0):
    return mmirror.Grating(mmirror.MirrorPlane(msupp.SupportRectangle(size, size / 4)), N, m, groove_angle)


def sphere_grating(N=1200.0, m=-1):
    return mmirror.Grating(mmirror.MirrorSpherical(5649.0, msupp.SupportRectangle(60.0, 10.0)), N, m)


def torus_grating(N=1200.0, m=-1):
    return mmirror.Grating(mmirror.MirrorToroidal(5600.0, 50.0, msupp.SupportRectangle(60.0, 10.0)), N, m)


def scenes():
    """name -> (element, rays, wavelength): every single-grating scene of the GPU tests, for the oracle-against-truth check."""
    out = {}
    cone = point_source(5e-3)
    for m in (-1, 0, 1):
        for ang in (0.0, 90.0):
            out[f"eq_m{m}_a{int(ang)}"] = (place(plane_grating(1200.0, m, ang), 500.0, 80.0), cone, 30e-6)
    out["evanescent"] = (place(plane_grating(500.0, 1, 0.0), 500.0, 80.0), cone, 30e-6)
    out["tilt"] = (place(plane_grating(600.0, 1, 0.0, 60.0), 100.0, 30.0), plane_wave(5.0), 800e-6)
    narrow = point_source(2e-3)
    for wl in (10e-6, 40e-6):
        out[f"sphere_{int(wl * 1e6)}"] = (place(sphere_grating(), 237.0, 87.0), narrow, wl)
        out[f"torus_{int(wl * 1e6)}"] = (place(torus_grating(), 237.0, 87.0), narrow, wl)
    out["torus_order0"] = (place(torus_grating(1200.0, 0), 237.0, 87.0), narrow, 30e-6)
    return out


def assert_parity(res, ref, mask, what=""):
    """Points and paths within PARITY of the reference magnitudes, directions within PARITY absolute (grooves and the
    incidence angle like paths and directions)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    for key, rel in (("point", True), ("path", True), ("grooves", True), ("vector", False), ("inc", False)):
        a, b = f(res[key])[mask], f(ref[key])[mask]
        if a.size == 0:
            continue
        scale = max(1.0, float(np.abs(b).max())) if rel else 1.0
        err = float(np.abs(a - b).max())
        assert err <= PARITY * scale, f"{what} {key}: {err:.3e} > {PARITY * scale:.3e}"

"""Oracle and scenes of the grating tests (tests/test_grating_host.py, tests/test_gpu_grating.py).

`diffract` is a NumPy restatement of the per-ray grating math (csrc/art_device.h, grating_hit / grating_diffract) in the
literal form of the grating equation -- s = 1 - |v_t|^2 --, generic in the float type: float64 is the ORACLE the GPU
results are compared with, numpy.longdouble (64-bit significand) the TRUTH the oracle and the header function are judged
by (as tests/truth_common.py does for mirrors).  Substrates of `diffract`: plane, concave sphere, torus; rays start inside
the torus tube, as they do for a mirror.  `truth` is the long-double truth on ANY of the six surfaces: it takes the hit mask
and a seed of the root from the same substrate traced as a bare mirror and refines it with tests/truth_common.py, so that it
is no third candidate rule; `scenes_six` holds its scenes (six surfaces, convex sphere and cylinder, groove angles that mix
both components of q0, clipped supports, bundles that straddle the cut-off) and `own_input` the conditions under which the
alive masks can be compared bit for bit.  Scenes are built by hand on the host (no device needed): optic at `distance` on
the x axis, plane of incidence = the lab's xz plane, major axis in it."""
import types

import numpy as np

import truth_common as tc
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


# the kind names and parameter names of truth_common._surface / _base_normal; a convex sphere or cylinder is the same
# surface (the classes store |R|): which side of it the rays meet is a matter of the pose, see place()
KINDS = {"Plane Mirror": "plane", "SphericalCC Mirror": "sphere", "SphericalCX Mirror": "sphere", "Parabolic Mirror": "parabola",
         "Toroidal Mirror": "torus", "Ellipsoidal Mirror": "ellipsoid", "CylindricalCC Mirror": "cylinder",
         "CylindricalCX Mirror": "cylinder"}
PARAMS = {"plane": (), "sphere": ("R",), "parabola": ("p",), "torus": ("R", "r"), "ellipsoid": ("a", "b"), "cylinder": ("R",)}


def element_spec(oe):
    """Plain numbers of an OpticalElement whose optic is a Grating (or a bare mirror: N = 0)."""
    G = oe.type
    M = getattr(G, "Mirror", G)
    kind = KINDS[M.type]
    mp = [float(v) for v in M._abi_params()]
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    sup = M.support
    q = G._groove_vector() if hasattr(G, "_groove_vector") else (1.0, 0.0)
    return {"kind": kind, "mp": mp, "params": dict(zip(PARAMS[kind], mp)), "centre": np.asarray(M.get_centre(), dtype=float),
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
            "grooves": g_in + m * G, "u": u, "v": v, "s": s, "dn": np.abs(dn)}


def truth(E, point, vector, path, alive, wavelength, t_seed, grooves=None):
    """The grating E on ANY of the six substrates in numpy.longdouble.  Not a third candidate rule: which rays hit, and an
    approximation `t_seed` of each one's segment length, come from the same substrate traced as a bare mirror (NaN: the
    mirror lost the ray).  The truth refines that root (truth_common._surface), takes the normal from
    truth_common._base_normal and applies the grating equation in the literal form of `diffract`.  Returns `diffract`'s
    dict plus `term` = m N q0.(P - c), this grating's own share of `grooves`, `side` = sign(u.n) and `xy`, the hit point's
    support coordinates."""
    O = types.SimpleNamespace(kind=E["kind"], params=E["params"])
    F, C, pos = tc.ld(E["fwd"]), tc.ld(E["centre"]), tc.ld(E["pos"])
    m, N = LD(E["m"]), LD(E["N"])
    q0 = tc.ld([E["q"][0], E["q"][1], 0.0])
    seed = np.asarray(t_seed, dtype=np.float64)
    hit = (np.asarray(alive) != 0) & np.isfinite(seed)
    A = (tc.ld(point) - pos) @ F.T + C
    u = tc.ld(vector) @ F.T
    with np.errstate(all="ignore"):
        t = tc._surface(O, A, u, np.where(hit, seed, 1.0))
        P = A + t[:, None] * u
        n = tc._base_normal(O, P)
        g = (m * LD(wavelength) * N) * q0
        dn = (u * n).sum(1)
        gt = g[None, :] - (n @ g)[:, None] * n
        vt = (u - dn[:, None] * n) + gt
        s = 1 - (vt * vt).sum(1)
        v = vt - (np.sign(dn) * np.sqrt(np.where(s > 0, s, 1)))[:, None] * n
        inc = tc.kahan_angle(-u, n)
        term = m * N * ((P - C) @ q0)
        vl = v @ F
        vl = vl / _norm(vl)[:, None]
    g_in = 0 if grooves is None else tc.ld(grooves)
    return {"alive": hit & (s > 0), "hit": hit, "point": (P - C) @ F + pos, "vector": vl, "path": tc.ld(path) + t, "inc": inc,
            "grooves": g_in + term, "term": term, "u": u, "v": v, "s": s, "dn": np.abs(dn), "side": np.sign(dn),
            "xy": (P - C)[:, :2]}


MARGIN_S = 1e-9          # |s| below this: the order is neither clearly propagating nor clearly evanescent
MARGIN_EDGE = 1e-9       # mm from the support's edge: neither clearly on the optic nor clearly off it


def edge_distance(E, xy):
    """Distance (mm, float64) of support coordinates from the support's edge; for a rectangle the distance from the nearer
    of its two pairs of edge LINES, which is never more than the distance from the edge itself."""
    x, y = np.abs(np.asarray(xy[:, 0], dtype=LD)), np.abs(np.asarray(xy[:, 1], dtype=LD))
    if E["support"][0] == "round":
        d = np.abs(np.sqrt(x * x + y * y) - LD(E["support"][1]))
    else:
        d = np.minimum(np.abs(x - LD(E["support"][1]) / 2), np.abs(y - LD(E["support"][2]) / 2))
    return np.asarray(d, dtype=np.float64)


def inside(E, xy):
    x, y = xy[:, 0], xy[:, 1]
    if E["support"][0] == "round":
        return x * x + y * y <= LD(E["support"][1]) ** 2
    return (np.abs(x) <= LD(E["support"][1]) / 2) & (np.abs(y) <= LD(E["support"][2]) / 2)


def marginal(E, ref, ref_large, alive):
    """Counts (rays with |s| < MARGIN_S among those that hit, rays within MARGIN_EDGE of the support's edge among those alive
    on input) and the two smallest distances.  `ref_large`: the truth of the same scene with the large support, which
    every input-alive ray hits -- it gives the hit points of the rays that E's own support clips."""
    alive = np.asarray(alive) != 0
    assert np.array_equal(ref_large["hit"], alive), "the large support must catch every ray that is alive on input"
    s = np.abs(np.asarray(ref["s"], dtype=np.float64))[ref["hit"]]
    d = edge_distance(E, ref_large["xy"])[alive]
    assert np.array_equal(ref["hit"], alive & np.asarray(inside(E, ref_large["xy"]), dtype=bool)), \
        "the mirror's hit mask is not the truth's hit points inside the support"
    return int((s < MARGIN_S).sum()), int((d < MARGIN_EDGE).sum()), float(s.min()) if s.size else np.inf, float(d.min())


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


def place(optic, distance, incidence_deg, convex=False, outside=False):
    """OpticalElement at `distance` on the x axis, incidence angle in the lab's xz plane, major axis in that plane.
    convex: the element normal is reversed and the major axis kept.  frame_maps then ends in the reference's point inversion
    (RotationPoint at an angle of pi): the optic frame is the MIRROR IMAGE of the usual one, the rays still start inside the
    sphere or cylinder and meet its z < 0 cap with u.n < 0, and q0 is mirrored with the frame.
    outside: normal AND major axis reversed -- the usual pose turned by 180 degrees about the lab's y axis, a proper frame.
    The rays then meet the z < 0 cap of a convex sphere or cylinder from outside, with u.n > 0."""
    th = np.deg2rad(incidence_deg)
    normal = np.array([-np.cos(th), 0.0, np.sin(th)]) * (-1.0 if convex or outside else 1.0)
    major = np.array([np.sin(th), 0.0, np.cos(th)]) * (-1.0 if outside else 1.0)
    return moe.OpticalElement(optic, np.array([float(distance), 0.0, 0.0]), normal, major)


def on_pose(optic, oe):
    """`optic` in the pose of the element `oe` (the bare substrate of a grating, or the same grating on another support)."""
    return moe.OpticalElement(optic, np.asarray(oe.position, dtype=float), np.asarray(oe.normal, dtype=float),
                              np.asarray(oe.majoraxis, dtype=float))


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


# substrate -> (mirror(support), incidence in degrees, half angle of the cone, the paraboloid's round supports)
_ROUND = {"paraboloid"}
SUBSTRATES = {
    "plane": (lambda S: mmirror.MirrorPlane(S), 80.0, 5e-3),
    "sphere": (lambda S: mmirror.MirrorSpherical(5649.0, S), 87.0, 2e-3),
    "torus": (lambda S: mmirror.MirrorToroidal(5600.0, 50.0, S), 87.0, 2e-3),
    "paraboloid": (lambda S: mmirror.MirrorParabolic(200.0, 30.0, S), 50.0, 8e-3),
    "ellipsoid": (lambda S: mmirror.MirrorEllipsoidal(S, SemiMajorAxis=400.0, SemiMinorAxis=60.0), 80.0, 3e-3),
    "cylinder": (lambda S: mmirror.MirrorCylindrical(500.0, S), 75.0, 4e-3),
    "convex_cylinder": (lambda S: mmirror.MirrorCylindrical(-500.0, S), 75.0, 4e-3),
    "convex_sphere": (lambda S: mmirror.MirrorSpherical(-800.0, S), 60.0, 4e-3),
    "convex_cylinder_outside": (lambda S: mmirror.MirrorCylindrical(-500.0, S), 75.0, 4e-3),
    "convex_sphere_outside": (lambda S: mmirror.MirrorSpherical(-800.0, S), 60.0, 4e-3),
}
GENERIC = [(1200.0, -1, 0.0), (900.0, 1, 33.0), (600.0, 2, 118.0), (1200.0, -1, 90.0)]          # (N, m, groove angle)
CUT_OFF = {"plane": (37.0, 631.38, 1), "sphere": (20.0, 48.61, 1), "torus": (20.0, 48.62, 1), "paraboloid": (33.0, 16097.49, 1),
           "ellipsoid": (33.0, 601.95, 1), "cylinder": (33.0, 1344.72, 1), "convex_cylinder": (33.0, 1344.71, 1),
           "convex_sphere": (33.0, 5182.11, 1),
           # met from outside the rays run along -x of the optic frame: the order that grows |v_t| is -1
           "convex_cylinder_outside": (33.0, 1344.71, -1), "convex_sphere_outside": (33.0, 5182.07, -1)}   # groove angle, N, m
# generic scenes in which the whole bundle is evanescent (asserted from the truth)
EVANESCENT = {f"{sub}_N900_m1_a33" for sub in ("plane", "sphere", "torus", "ellipsoid")} | {"convex_cylinder_outside_N1200_m-1_a0"}
CLIPPED_HITS = {"plane": 995, "sphere": 1875, "torus": 1876, "paraboloid": 1864, "ellipsoid": 1833, "cylinder": 1394,
                "convex_cylinder": 1394, "convex_sphere": 1393, "convex_cylinder_outside": 1393,
                "convex_sphere_outside": 1393}           # of 3514 rays alive on input
SIX_DISTANCE, SIX_WAVELENGTH = 237.0, 30e-6


def substrate(name, clipped=False):
    """The bare mirror of a substrate on its large support, or on the small one that clips 47 to 72 % of the bundle."""
    if name in _ROUND:
        S = msupp.SupportRound(1.5 if clipped else 12.0)
    else:
        S = msupp.SupportRectangle(12.0, 0.6) if clipped else msupp.SupportRectangle(60.0, 10.0)
    return SUBSTRATES[name][0](S)


def six_element(name, N, m, angle, clipped=False):
    return place(mmirror.Grating(substrate(name, clipped), N, m, angle), SIX_DISTANCE, SUBSTRATES[name][1],
                 convex=name.startswith("convex"), outside=name.endswith("_outside"))


def scenes_six():
    """name -> scene: a grating on each of the six surfaces (and on the convex sphere and cylinder) in three families --
    `generic` (four groove angles and orders, every ray hits), `clipped` (a small support) and `cutoff` (m = +1 with N such
    that about half of the bundle is evanescent).  A scene: dict of `oe`, `rays`, `wl`, `family`, `substrate` and `large`,
    the same grating on the large support (`oe` itself unless clipped)."""
    out = {}
    for sub, (_, _, half) in SUBSTRATES.items():
        rays = point_source(half)

        def add(name, family, N, m, ang, clipped=False):
            oe = six_element(sub, N, m, ang, clipped)
            out[f"{sub}_{name}"] = {"oe": oe, "rays": rays, "wl": SIX_WAVELENGTH, "family": family, "substrate": sub,
                                    "large": six_element(sub, N, m, ang) if clipped else oe}
        for N, m, ang in GENERIC:
            add(f"N{int(N)}_m{m}_a{int(ang)}", "generic", N, m, ang)
        add("clipped", "clipped", 600.0, 2, 118.0, clipped=True)
        add("cutoff", "cutoff", CUT_OFF[sub][1], CUT_OFF[sub][2], CUT_OFF[sub][0])
    return out


def own_input(sc, E, ref, ref_large, what, alive=None):
    """What every test of these scenes asserts about its own input first: no marginal ray, and the family's split."""
    alive = sc["rays"][3] if alive is None else alive
    n_s, n_edge, s_min, d_min = marginal(E, ref, ref_large, alive)
    n_in, n_hit, n_alive = int((alive != 0).sum()), int(ref["hit"].sum()), int(ref["alive"].sum())
    print(f"{what}: {n_alive} alive of {n_hit} hit of {n_in}; smallest |s| {s_min:.2e}, nearest to the edge {d_min:.2e} mm, "
          f"|u.n| {float(ref['dn'][ref['hit']].min()):.2e} to {float(ref['dn'][ref['hit']].max()):.2e}")
    assert n_s == 0 and n_edge == 0, \
        f"{what}: {n_s} rays within {MARGIN_S} of the cut-off, {n_edge} within {MARGIN_EDGE} mm of the edge"
    side = np.asarray(ref["side"][ref["hit"]], dtype=float)
    want = 1.0 if sc["substrate"].endswith("_outside") else -1.0
    assert (side == want).all(), what + ": the rays meet the other side of the surface"
    if sc["family"] == "clipped":
        assert 0 < n_hit < n_in
    else:
        assert n_hit == n_in
    if sc["family"] == "cutoff":
        assert 0 < n_alive < n_hit
    else:
        assert n_alive in (0, n_hit)                    # a whole bundle propagates, or a whole bundle is evanescent (EVANESCENT)
    return n_hit, n_alive


def worst_deviation(res, ref, mask):
    """key -> largest deviation on `mask`, relative to the reference magnitudes for points, paths and grooves, absolute for
    directions and the incidence angle (the quantities assert_parity bounds)."""
    f = lambda a: np.asarray(a, dtype=LD)
    out = {}
    for key, rel in (("point", True), ("path", True), ("grooves", True), ("vector", False), ("inc", False)):
        a, b = f(np.asarray(res[key])[mask]), f(np.asarray(ref[key])[mask])
        scale = max(1.0, float(np.abs(b).max())) if rel and a.size else 1.0
        out[key] = float(np.abs(a - b).max()) / scale if a.size else 0.0
    return out


def assert_parity(res, ref, mask, what=""):
    """Points and paths within PARITY of the reference magnitudes, directions within PARITY absolute (grooves and the
    incidence angle like paths and directions)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    for key, rel in (("point", True), ("path", True), ("grooves", True), ("vector", False), ("inc", False)):
        a, b = f(np.asarray(res[key])[mask]), f(np.asarray(ref[key])[mask])     # (masked first: a lost ray's entry may be anything)
        if a.size == 0:
            continue
        scale = max(1.0, float(np.abs(b).max())) if rel else 1.0
        err = float(np.abs(a - b).max())
        assert err <= PARITY * scale, f"{what} {key}: {err:.3e} > {PARITY * scale:.3e}"

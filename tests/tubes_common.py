"""Ray tubes (differential ray tracing) restated in NumPy long double, the scenes of the ray-tube tests, and a
finite-difference truth.  TEST INFRASTRUCTURE, written from the formulas, not from csrc/art_tubes.h: the
transverse bases, the eigen-decomposition and the quadric's scaling are deliberately formed another way.

State per ray: dP[j], dD[j] (j = a, b), lab frame.  Seed from the source direction D0 with (u, v) = perp_pair(D0):
point source dP = 0, dD = (u, v); plane wave dP = (u, v), dD = 0.  Step at an element, D incoming, P_prev, P the hit:
  t = (P - P_prev).D;  g, H: gradient and Hessian of the implicit form at P_optic = fwd (P - pos) + centre;  n = -g/|g|
  a_j = dP_j + t dD_j;  dt_j = -(n.a_j)/(n.D);  dQ_j = a_j + D dt_j;  dn_j = -(H dQ_j - n (n.H dQ_j))/|g|
  dD'_j = dD_j - 2 [(dD_j.n + D.dn_j) n + (D.n) dn_j]        (mask: the plane rule, dD unchanged)
Read-out: the same transport onto the detector plane (dX_j), or dX_j = dQ_j without one."""
import numpy as np

import quadric_common as qc
import truth_common as tc

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 1e-18
PARITY = 1e-10
COND_MAX = 1e6
N_RAYS = 1000


def ld(a):
    return np.asarray(a, dtype=LD)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def perp_pair(D):
    """(u, v), orthonormal and perpendicular to the unit rows of D: Gram-Schmidt of the lab axis of D's smallest
    component, v = D x u."""
    D = ld(D)
    e = np.zeros_like(D)
    e[np.arange(len(D)), np.argmin(np.abs(D), axis=1)] = 1
    u = _unit(e - _dot(e, D)[:, None] * D)
    return u, np.cross(D, u)


# ------------------------------------------------------------------------------------------------------ surfaces
def spec_of(oe):
    """Plain numbers of an OpticalElement: kind, parameters, pose."""
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    M = oe.type
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    s = {"fwd": ld(fwd), "pos": ld(oe.position), "centre": ld(M.get_centre())}
    name = type(M).__name__
    if hasattr(M, "_quadric_coefficients"):
        s["kind"], s["coeff"] = "quadric", [LD(v) for v in M._quadric_coefficients()]
    elif name == "Mask":
        s["kind"] = "mask"
    elif name == "MirrorPlane":
        s["kind"] = "plane"
    elif name == "MirrorSpherical":
        s["kind"] = "sphere"
    elif name == "MirrorParabolic":
        s["kind"], s["p"] = "parabola", LD(M.p)
    elif name == "MirrorEllipsoidal":
        s["kind"], s["a"], s["b"] = "ellipsoid", LD(M.a), LD(M.b)
    elif name == "MirrorCylindrical":
        s["kind"] = "cylinder"
    elif name == "MirrorToroidal":
        s["kind"], s["R"], s["r"] = "torus", LD(M.majorradius), LD(M.minorradius)
    else:
        raise ValueError(name)
    return s


def grad_hess(s, P):
    """g [n, 3] and H [n, 3, 3] of the element's implicit form at the optic-frame points P."""
    n = len(P)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    H = np.zeros((n, 3, 3), dtype=LD)
    o = np.zeros(n, dtype=LD)
    k = s["kind"]
    if k in ("plane", "mask"):
        g = np.stack([o, o, o + 1], 1)
    elif k == "sphere":
        g = P.copy()
        H[:] = np.eye(3, dtype=LD)
    elif k == "parabola":
        g = np.stack([x, y, o - s["p"]], 1)
        H[:, 0, 0] = H[:, 1, 1] = 1
    elif k == "ellipsoid":
        a2, b2 = s["a"] ** 2, s["b"] ** 2
        g = np.stack([x * b2, y * a2, z * a2], 1)
        H[:, 0, 0], H[:, 1, 1], H[:, 2, 2] = b2, a2, a2
    elif k == "cylinder":
        g = np.stack([o, y, z], 1)
        H[:, 1, 1] = H[:, 2, 2] = 1
    elif k == "torus":
        S = _dot(P, P)
        kxz, ky = S - s["R"] ** 2 - s["r"] ** 2, S + s["R"] ** 2 - s["r"] ** 2
        g = np.stack([x * kxz, y * ky, z * kxz], 1)
        H[:, 0, 0], H[:, 1, 1], H[:, 2, 2] = kxz, ky, kxz
        H += 2 * P[:, :, None] * P[:, None, :]
    elif k == "quadric":
        q = s["coeff"]
        Q = np.array([[q[0], q[3], q[4]], [q[3], q[1], q[5]], [q[4], q[5], q[2]]], dtype=LD)
        g = 2 * (P @ Q + np.array(q[6:9], dtype=LD))
        H[:] = 2 * Q
    else:
        raise ValueError(k)
    return g, H


# ------------------------------------------------------------------------------------------------- the restatement
def seed(D0, source):
    u, v = perp_pair(D0)
    z = np.zeros_like(u)
    uv, zz = np.stack([u, v], 1), np.stack([z, z], 1)
    return (zz, uv) if source == "point" else (uv, zz)          # dP, dD: [n, 2, 3]


def transport(dP, dD, t, D, n):
    """The tangents carried over t along D onto the plane with normal n: dQ [n, 2, 3]."""
    a = dP + t[:, None, None] * dD
    dt = -_dot(a, n[:, None, :]) / _dot(n, D)[:, None]
    return a + D[:, None, :] * dt[:, :, None]


def step(s, D, Pprev, P, dP, dD):
    F = s["fwd"]
    Po = (P - s["pos"]) @ F.T + s["centre"]
    g, H = grad_hess(s, Po)
    gn = np.sqrt(_dot(g, g))
    n = (-g / gn[:, None]) @ F                                  # back to the lab frame
    dQ = transport(dP, dD, _dot(P - Pprev, D), D, n)
    if s["kind"] == "mask":
        return dQ, dD
    Hl = F.T @ H @ F                                            # the Hessian in the lab frame
    HdQ = np.einsum("nab,njb->nja", Hl, dQ)
    dn = -(HdQ - n[:, None, :] * _dot(HdQ, n[:, None, :])[:, :, None]) / gn[:, None, None]
    c = _dot(dD, n[:, None, :]) + _dot(dn, D[:, None, :])
    return dQ, dD - 2 * (c[:, :, None] * n[:, None, :] + _dot(D, n)[:, None, None] * dn)


def readout(D, P, dP, dD, det=None):
    if det is None:
        dX = dP
        area = _dot(D, np.cross(dX[:, 0], dX[:, 1]))
    else:
        C, nd = ld(det[0]), np.broadcast_to(ld(det[1]), D.shape)
        dX = transport(dP, dD, _dot(C - P, nd) / _dot(D, nd), D, nd)
        area = _dot(nd, np.cross(dX[:, 0], dX[:, 1]))
    sa = _dot(D, np.cross(dD[:, 0], dD[:, 1]))
    v = np.stack(perp_pair(D), 1)                               # [n, 2, 3]
    aperp = dX - D[:, None, :] * _dot(dX, D[:, None, :])[:, :, None]
    A = np.einsum("nic,njc->nij", v, aperp)
    B = np.einsum("nic,njc->nij", v, dD)
    det_A = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    with np.errstate(all="ignore"):
        Ainv = np.stack([np.stack([A[:, 1, 1], -A[:, 0, 1]], 1), np.stack([-A[:, 1, 0], A[:, 0, 0]], 1)], 1) / det_A[:, None, None]
        Cm = B @ Ainv
        m, d, o = (Cm[:, 0, 0] + Cm[:, 1, 1]) / 2, (Cm[:, 0, 0] - Cm[:, 1, 1]) / 2, (Cm[:, 0, 1] + Cm[:, 1, 0]) / 2
        r = np.sqrt(d * d + o * o)
        phi = np.arctan2(o, d) / 2                              # the direction of kappa2; kappa1's is a quarter turn on
        axis = -np.sin(phi)[:, None] * v[:, 0] + np.cos(phi)[:, None] * v[:, 1]
        fro = (A * A).sum(axis=(1, 2))
        smin2 = (fro - np.sqrt(np.maximum(fro * fro - 4 * det_A ** 2, 0))) / 2
        cond = np.sqrt((fro - smin2) / smin2)
    return {"solid_angle": sa, "area": area, "kappa": np.stack([m - r, m + r]), "axis": axis,
            "asymmetry": np.abs(Cm[:, 0, 1] - Cm[:, 1, 0]), "cond": cond, "dX": dX, "dD": dD}


def run(specs, hist, source, det=None, w=None, alive=None):
    """hist: [(P, D)] of the source and after each element ([n, 3] each); alive: [n] bool, the rays alive in every view.
    Per-ray arrays (long double; NaN for the rays that do not count), `weight`, and `row`, the sums of art_ray_tubes."""
    hist = [(ld(P), ld(D)) for P, D in hist]
    n = len(hist[0][0])
    alive = np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
    w = np.ones(n, dtype=LD) if w is None else ld(w)
    hist = [(np.where(alive[:, None], P, 1), np.where(alive[:, None], D, LD(1) / np.sqrt(LD(3)))) for P, D in hist]
    dP, dD = seed(hist[0][1], source)
    with np.errstate(all="ignore"):
        for k, s in enumerate(specs):
            dP, dD = step(s, hist[k][1], hist[k][0], hist[k + 1][0], dP, dD)
        out = readout(hist[-1][1], hist[-1][0], dP, dD, det)
    nan = LD(np.nan)
    for key in ("solid_angle", "area", "asymmetry", "cond"):
        out[key] = np.where(alive, out[key], nan)
    out["kappa"] = np.where(alive[None, :], out["kappa"], nan)
    out["axis"] = np.where(alive[:, None], out["axis"], nan)
    out["weight"] = np.where(alive, w * np.abs(out["solid_angle"]), 0)
    k1, k2 = out["kappa"]
    fin = alive & np.isfinite(k1) & np.isfinite(k2)
    sa = np.abs(out["solid_angle"][alive])
    row = np.zeros(16, dtype=LD)
    row[0], row[1], row[2] = alive.sum(), w[alive].sum(), out["weight"].sum()
    if alive.any():
        row[3], row[4] = sa.min(), sa.max()
    row[5] = (w * np.abs(out["area"]))[alive].sum()
    row[8], row[9] = w[fin].sum(), fin.sum()
    if fin.any() and row[8] != 0:
        row[6], row[7] = (w * k1)[fin].sum() / row[8], (w * k2)[fin].sum() / row[8]
    if fin.any():
        den = (np.abs(k1) + np.abs(k2))[fin]
        row[10] = np.where(den > 0, out["asymmetry"][fin] / np.where(den > 0, den, 1), 0).max()
    out["row"], out["alive"], out["finite"] = row, alive, fin
    return out


# ---------------------------------------------------------------------------------------------- the truth's tracers
def oracle_element(oe):
    """The oracle's description of a mirror or mask of the package (kinds, parameters, support, pose)."""
    from oracle import art_oracle as orc
    kinds = {0: "plane", 1: "sphere", 2: "parabola", 3: "torus", 4: "ellipsoid", 5: "cylinder", 6: "mask"}
    sups = {0: "round", 1: "roundhole", 2: "rect", 3: "recthole", 4: "rectrecthole"}
    o = oe.type
    kind = kinds[o._abi_kind]
    params = {}
    if kind in ("sphere", "cylinder"):
        params = {"R": o.radius}
    elif kind == "parabola":
        params = {"feff": o.feff, "offaxis_rad": o.offaxisangle, "p": o.p}
    elif kind == "torus":
        params = {"R": o.majorradius, "r": o.minorradius}
    elif kind == "ellipsoid":
        params = {"a": o.a, "b": o.b, "offaxis_rad": o._offaxisangle}
    return orc.Element(orc.Optic(kind, orc.Support(sups[o.support._abi_kind], o.support._abi_params()), params, [], o.type),
                       np.asarray(oe.position, float), np.asarray(oe.normal, float), np.asarray(oe.majoraxis, float))


def trace_history(els, P0, D0, plan=None):
    """The chain in long double: [(P, D)] of the source and after every element, the rays alive at the end, and the `plan`
    (survivors and segment lengths per element, from the fp64 oracle) that a perturbed re-trace reuses.  Quadrics:
    quadric_common.trace; every other kind: truth_common.element_truth on the oracle's survivors."""
    from oracle import art_oracle as orc
    n = len(P0)
    P, D = ld(P0).copy(), _unit(ld(D0))
    alive = np.ones(n, dtype=bool)
    hist, made = [(P, D)], []
    for k, oe in enumerate(els):
        s = spec_of(oe)
        Pn, Dn = P.copy(), D.copy()
        if s["kind"] == "quadric":
            res = qc.trace(qc.element_spec(oe), P, D, np.zeros(n), alive.astype(np.uint8))
            ok = res["alive"]
            Pn[ok], Dn[ok] = res["point"][ok], res["vector"][ok]
            made.append(None)
        else:
            E = oracle_element(oe)
            if plan is None:
                idx = np.flatnonzero(alive)
                B = orc.make_bundle(np.asarray(P[idx], dtype=float), np.asarray(D[idx], dtype=float), idx)
                hit = orc.ray_tracing_calculation(B, [E])[0]
                keep = np.asarray(hit.number)
                seeds = np.linalg.norm(hit.point - np.asarray(P[keep], dtype=float), axis=1)
            else:
                keep, seeds = plan[k]
            made.append((keep, seeds))
            ok = np.zeros(n, dtype=bool)
            ok[keep] = True
            Pk, Dk, _, _ = tc.element_truth(E, P[keep], D[keep], seeds, fwd=s["fwd"])
            Pn[keep], Dn[keep] = Pk, Dk
        alive = alive & ok
        P, D = Pn, Dn
        hist.append((P, D))
    return hist, alive, made


def source_rays(kind, size, n=N_RAYS, origin=(0.0, 0.0, 0.0), axis=(1.0, 0.0, 0.0)):
    """A Vogel spiral whose ray 0 is the axis itself: point source of half-angle `size` or plane wave of radius `size`."""
    k = np.arange(n, dtype=float)
    rr, th = np.sqrt(k / n), np.pi * (3.0 - np.sqrt(5.0)) * k
    a, b = rr * np.cos(th), rr * np.sin(th)
    d = np.asarray(axis, dtype=float)
    d = d / np.linalg.norm(d)
    t1, t2 = (np.asarray(v, dtype=float) for v in perp_pair(d[None, :]))
    o = np.asarray(origin, dtype=float)
    if kind == "point":
        v = d[None, :] + np.tan(size) * (a[:, None] * t1 + b[:, None] * t2)
        return np.tile(o, (n, 1)), v / np.linalg.norm(v, axis=1)[:, None]
    return o[None, :] + size * (a[:, None] * t1 + b[:, None] * t2), np.tile(d, (n, 1))


def perturbed(P0, D0, source, j, eps):
    """The source moved by eps along seed direction j (0: u, 1: v) of every ray."""
    u, v = perp_pair(_unit(ld(D0)))
    e = (u, v)[j] * LD(eps)
    if source == "point":
        return ld(P0), _unit(_unit(ld(D0)) + e)
    return ld(P0) + e, ld(D0)


def fd_jacobian(els, P0, D0, source, det, plan, eps):
    """Central differences of the final point (on the detector plane, or on the last surface) and direction with respect
    to the two source parameters, at steps eps and eps / 2, Richardson-extrapolated.  Returns (dX, dD) [n, 2, 3] and the
    step-halving estimates: |extrapolated - value at eps / 2|, the error of the better of the two differences."""
    def final(P, D):
        hist, _, _ = trace_history(els, P, D, plan)
        X, V = hist[-1]
        if det is not None:
            C, nd = ld(det[0]), ld(det[1])
            X = X + (((C - X) @ nd) / (V @ nd))[:, None] * V
        return X, V

    out = []
    for j in range(2):
        per = []
        for h in (eps, eps / 2):
            Xp, Vp = final(*perturbed(P0, D0, source, j, +h))
            Xm, Vm = final(*perturbed(P0, D0, source, j, -h))
            per.append(((Xp - Xm) / (2 * LD(h)), (Vp - Vm) / (2 * LD(h))))
        (X1, V1), (X2, V2) = per
        out.append(((4 * X2 - X1) / 3, (4 * V2 - V1) / 3, np.abs(X2 - X1) / 3, np.abs(V2 - V1) / 3))
    dX, dD = np.stack([out[0][0], out[1][0]], 1), np.stack([out[0][1], out[1][1]], 1)
    eX, eD = np.stack([out[0][2], out[1][2]], 1), np.stack([out[0][3], out[1][3]], 1)
    return dX, dD, eX, eD


# ----------------------------------------------------------------------------------------------------------- scenes
def place_chain(optics, distances, incidences, rolls):
    """OpticalElements along a chief ray that starts at the origin along +x: element k lies distances[k] behind the
    previous one, its normal at incidences[k] degrees to the incoming ray in the plane turned by rolls[k] degrees about
    it.  Returns (elements, the chief ray's last point, its final direction)."""
    import ART.ModuleOpticalElement as moe
    p, d = np.zeros(3), np.array([1.0, 0.0, 0.0])
    ref = np.array([0.0, 0.0, 1.0])
    els = []
    for O, dist, inc, roll in zip(optics, distances, incidences, rolls):
        p = p + dist * d
        t = ref - (ref @ d) * d
        t = t / np.linalg.norm(t)
        s = np.cross(d, t)
        r = np.deg2rad(roll)
        t = np.cos(r) * t + np.sin(r) * s
        th = np.deg2rad(inc)
        normal = -np.cos(th) * d + np.sin(th) * t
        major = np.sin(th) * d + np.cos(th) * t
        els.append(moe.OpticalElement(O, p.copy(), normal, major))
        if type(O).__name__ != "Mask":
            ref = t
            d = d + 2 * np.cos(th) * normal
            d = d / np.linalg.norm(d)
    return els, p, d


def ellipsoid_scene(p, q, included_deg, half_angle, n=N_RAYS, support=60.0):
    """MirrorEllipsoidal from focus to focus in the identity pose (lab = optic frame - centre): the source at the focus
    `p` from the support's centre, aimed at it.  Returns (elements, (P0, D0), F1, F2) in the lab frame."""
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    M = mm.MirrorEllipsoidal(ms.SupportRound(support), OffAxisAngle=included_deg, f_object=p, f_image=q)
    C = np.asarray(M.get_centre(), dtype=float)
    c = np.sqrt(M.a ** 2 - M.b ** 2)
    foci = [np.array([c, 0.0, 0.0]) - C, np.array([-c, 0.0, 0.0]) - C]
    foci.sort(key=lambda F: abs(np.linalg.norm(F) - p))
    F1, F2 = foci
    assert abs(np.linalg.norm(F1) - p) <= 1e-9 * p and abs(np.linalg.norm(F2) - q) <= 1e-9 * q
    return [qc.identity_pose(M)], source_rays("point", half_angle, n, F1, -F1), F1, F2


TORUS_D = {"R": 6702.146766572041, "r": 208.3778132003165}      # the twisted two-toroid configuration's mirrors (f = 600)


def twisted(n=N_RAYS, mask=False):
    """The two toroids of the twisted configuration: 80 degrees incidence, 600 mm apart, the second plane of incidence
    turned by 10 degrees, a point source 600 mm before the first; the detector is tilted by 5 degrees and stands at 0.8 of
    the 600 mm to the best focus.  mask: a round hole midway between the toroids that clips the outer rays."""
    import ART.ModuleMask as mmask
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    tor = lambda: mm.MirrorToroidal(TORUS_D["R"], TORUS_D["r"], ms.SupportRectangle(300.0, 40.0))
    optics, dist, inc, roll = [tor(), tor()], [600.0, 600.0], [80.0, -80.0], [0.0, -10.0]
    if mask:
        optics.insert(1, mmask.Mask(ms.SupportRoundHole(60.0, 9.0, 0.0, 0.0)))
        dist, inc, roll = [600.0, 300.0, 300.0], [80.0, 0.0, -80.0], [0.0, 0.0, -10.0]
    els, p, d = place_chain(optics, dist, inc, roll)
    t = np.cross(d, [0.0, 1.0, 0.0])
    t = t / np.linalg.norm(t)
    a = np.deg2rad(5.0)
    normal = -(np.cos(a) * d + np.sin(a) * t)
    return els, source_rays("point", 0.02, n), (p + 0.8 * 600.0 * d, normal)


def scenes():
    """name -> dict(els, rays=(P0, D0), source, det, w): the scenes (a) - (e) of the ray-tube tests.  Supports are large
    enough that no ray is lost, except behind the mask of (e)."""
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    big = ms.SupportRectangle(300.0, 100.0)
    w = lambda n: 0.5 + ((np.arange(n) * 0.6180339887498949) % 1.0)
    S = {}
    mk = lambda els, rays, source, det=None, wt=None, **kw: dict(els=els, rays=rays, source=source, det=det, w=wt, **kw)
    els, _, _ = place_chain([mm.MirrorToroidal(900.0, 100.0, big)], [500.0], [70.0], [0.0])
    S["a_toroid"] = mk(els, source_rays("point", 0.01), "point", wt=w(N_RAYS))
    els, p, d = place_chain([mm.MirrorPlane(big)], [300.0], [45.0], [20.0])
    S["b_plane"] = mk(els, source_rays("point", 0.02), "point", det=tilted_detector(p, d))
    els, _, _ = place_chain([mm.MirrorSpherical(1000.0, big)], [500.0], [10.0], [35.0])
    S["b_sphere"] = mk(els, source_rays("point", 0.02), "point", wt=w(N_RAYS))
    els, p, d = place_chain([mm.MirrorParabolic(100.0, 0.0, ms.SupportRound(30.0))], [200.0], [0.0], [0.0])
    S["b_parabola"] = mk(els, source_rays("plane", 10.0), "plane", focus=p + 100.0 * d)
    els, rays, F1, F2 = ellipsoid_scene(400.0, 250.0, 60.0, 0.02)
    S["b_ellipsoid"] = mk(els, rays, "point", F1=F1, F2=F2, wt=w(N_RAYS))
    els, _, _ = place_chain([mm.MirrorCylindrical(500.0, big)], [400.0], [30.0], [-15.0])
    S["b_cylinder"] = mk(els, source_rays("point", 0.02), "point")
    kb = [mm.MirrorEllipticalCylinder(ms.SupportRectangle(120.0, 20.0), 1000.0, 600.0, 2.0),
          mm.MirrorEllipticalCylinder(ms.SupportRectangle(120.0, 20.0), 1100.0, 500.0, 2.0)]
    els, _, _ = place_chain(kb, [1000.0, 100.0], [88.0, 88.0], [0.0, 90.0])
    S["c_kb"] = mk(els, source_rays("point", 1e-3), "point")
    els, rays, det = twisted()
    S["d_twisted"] = mk(els, rays, "point", det=det, wt=w(N_RAYS))
    els, rays, det = twisted(1001, mask=True)
    S["e_masked"] = mk(els, rays, "point", det=det, wt=w(1001))
    return S


def tilted_detector(p, d, distance=150.0):
    """The detector of b_plane: `distance` along the chief ray (p, d), its normal 0.2 off the ray."""
    t = np.cross(d, [0.3, 0.5, 0.8])
    nd = -(d + 0.2 * t / np.linalg.norm(t))
    return p + distance * d, nd / np.linalg.norm(nd)


def rotated_conic():
    """The elliptical conic (400, 250, 30 degrees) with its pole frame turned by 35 degrees about z, Q' = Rz Q Rz^T: a
    MirrorQuadric all six entries of whose q are non-zero (b = (0, 0, -0.5) is Rz's axis and stays)."""
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    q = [LD(v) for v in mm.MirrorConic(ms.SupportRound(80.0), 400.0, 250.0, 30.0)._quadric_coefficients()]
    Q = np.array([[q[0], q[3], q[4]], [q[3], q[1], q[5]], [q[4], q[5], q[2]]], dtype=LD)
    a = np.deg2rad(LD(35))
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=LD)
    Q = Rz @ Q @ Rz.T
    M = mm.MirrorQuadric(ms.SupportRound(80.0), (Q + Q.T) / 2, np.array([0, 0, LD(-0.5)]))
    assert all(abs(v) > 1e-6 * max(np.abs(M._quadric_coefficients()[:6])) for v in M._quadric_coefficients()[:6])
    return M


def scenes_more():
    """name -> scene, as scenes(): a quadric with every coefficient of q set, a hyperboloid, two convex mirrors, and three
    golden chains (eight elements of four kinds; two twisted chains that lose rays at a mask and at the toroids' edges)."""
    import ART.ModuleMirror as mm
    import ART.ModuleSupport as ms
    import parity_common as pc
    from conftest import load_golden
    big = ms.SupportRectangle(300.0, 100.0)
    w = lambda n: 0.5 + ((np.arange(n) * 0.6180339887498949) % 1.0)
    S = {}
    mk = lambda els, rays, source, det=None, wt=None, **kw: dict(els=els, rays=rays, source=source, det=det, w=wt, **kw)
    els, p, d = place_chain([rotated_conic()], [400.0], [60.0], [20.0])
    S["h_rotated_quadric"] = mk(els, source_rays("point", 0.02), "point", det=tilted_detector(p, d), wt=w(N_RAYS))
    # the hyperboloid 5 degrees off its design incidence of 70: from its focus at 70 degrees it is stigmatic, every ray an
    # umbilic, and no principal direction could be compared
    els, p, d = place_chain([mm.MirrorConic(ms.SupportRound(80.0), 400.0, -250.0, 20.0)], [400.0], [65.0], [-25.0])
    S["h_hyperboloid"] = mk(els, source_rays("point", 0.01), "point", det=tilted_detector(p, d))
    els, _, _ = place_chain([mm.MirrorSpherical(-1000.0, big)], [500.0], [25.0], [35.0])
    S["h_convex_sphere"] = mk(els, source_rays("point", 0.02), "point", wt=w(N_RAYS))
    els, _, _ = place_chain([mm.MirrorCylindrical(-500.0, big)], [400.0], [30.0], [-15.0])
    S["h_convex_cylinder"] = mk(els, source_rays("point", 0.02), "point")
    # the two classes above are traced on the sheet of their concave twins (convexity enters the incidence angle alone): a
    # surface that curves away from the light is this quadric, the sphere of radius 1000 about (0, 0, -1000)
    ball = mm.MirrorQuadric(ms.SupportRound(80.0), -np.eye(3) / 2000.0, np.array([0.0, 0.0, -0.5]))
    els, p, d = place_chain([ball], [500.0], [25.0], [35.0])
    S["h_convex_quadric"] = mk(els, source_rays("point", 0.02), "point", det=tilted_detector(p, d), chief=(p, d))
    for name, golden in (("h_mixed8", "c4_mixed8"), ("h_c3", "c3_twisted_chain04"), ("h_c2", "c2_fxf_chain05")):
        scene, a = load_golden(golden)
        D0 = np.asarray(a["src_vector"], dtype=float)
        rays = (np.asarray(a["src_point"], dtype=float), D0 / np.linalg.norm(D0, axis=1)[:, None])
        assert len(D0) == N_RAYS
        S[name] = mk(pc.build_elements(scene, a), rays, "point", wt=w(N_RAYS) if name == "h_c3" else None)
    return S


def reframed(spec, axis=(1.0, 2.0, 3.0), degrees=50.0, shift=(3.0, -2.0, 5.0)):
    """The same physical quadric described in another optic frame, x' = R x + c0 (R: `degrees` about `axis`, c0 = `shift`):
    fwd' = R fwd, centre' = c0 (the spec's own centre is 0), Q' = R Q R^T, b' = R b - Q' c0, and c' from
    F(x) = F'(R x + c0).  The numbers are rounded to fp64, as a descriptor holds them, and then taken as exact."""
    assert spec["kind"] == "quadric" and not np.asarray(spec["centre"]).any()
    k = ld(axis) / np.sqrt(_dot(ld(axis), ld(axis)))
    a = np.deg2rad(LD(degrees))
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=LD)
    R = np.eye(3, dtype=LD) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    q, c0 = spec["coeff"], ld(shift)
    Q = np.array([[q[0], q[3], q[4]], [q[3], q[1], q[5]], [q[4], q[5], q[2]]], dtype=LD)
    b = np.array(q[6:9], dtype=LD)
    Q2 = R @ Q @ R.T
    Q2 = (Q2 + Q2.T) / 2
    b2 = R @ b - Q2 @ c0
    c2 = q[9] + c0 @ Q2 @ c0 - 2 * (R @ b) @ c0
    fp64 = lambda v: ld(np.asarray(v, dtype=float))
    coeff = [Q2[0, 0], Q2[1, 1], Q2[2, 2], Q2[0, 1], Q2[0, 2], Q2[1, 2], b2[0], b2[1], b2[2], c2]
    return dict(spec, fwd=fp64(R @ spec["fwd"]), centre=fp64(c0), coeff=[LD(float(v)) for v in coeff])


def compare(got, ref, alive, what, bar=PARITY):
    """|got - ref| <= bar * max |ref| over the rays `alive`; returns the error over that scale."""
    got, ref = ld(got), ld(ref)
    sel = alive if got.ndim == 1 else (alive[:, None] if got.shape[0] == len(alive) else alive[None, :])
    sel = np.broadcast_to(sel, got.shape)
    if not sel.any():
        return 0.0
    scale = np.abs(ref[sel]).max()
    err = np.abs(got[sel] - ref[sel]).max()
    assert err <= bar * scale or err == 0, f"{what}: {float(err):.3e} against {bar:g} of {float(scale):.3e}"
    return float(err / scale) if scale > 0 else 0.0


def axes_error(got, ref, sel):
    """Largest |got -+ ref| over the rays sel: a principal direction has no sign."""
    got, ref = ld(got)[sel], ld(ref)[sel]
    if len(got) == 0:
        return 0.0
    return float(np.minimum(np.abs(got - ref).max(axis=1), np.abs(got + ref).max(axis=1)).max())


# A principal direction is compared where the two curvatures are apart by at least this fraction of their size: an
# eigenvector moves by (error of the matrix) / (gap), so fp64 rounding of a few 1e-16 |kappa| stays below 1e-12 there.
AXIS_GAP = 1e-3


def check_against_restatement(got, ref, name):
    """got: dict of solid_angle, area, kappa [2, n], axis [n, 3]; ref: tubes_common.run's.  The project's parity bar."""
    a = ref["alive"]
    assert (ref["cond"][a] < COND_MAX).all(), name            # every curvature of these scenes is well conditioned
    worst = {}
    for key in ("solid_angle", "area", "kappa"):
        worst[key] = compare(got[key], ref[key], a, f"{name} {key}")
    k1, k2 = ref["kappa"]
    apart = a & (np.nan_to_num(np.asarray(k2 - k1, dtype=float)) >= AXIS_GAP * np.nan_to_num(np.asarray(np.abs(k1) + np.abs(k2), dtype=float)))
    worst["axis"] = axes_error(got["axis"], ref["axis"], apart)
    assert worst["axis"] <= PARITY, (name, worst)
    print(f"{name}: worst deviation from the restatement {worst}; axes compared on {int(apart.sum())} rays")
    return max(worst.values())

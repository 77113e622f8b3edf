"""Alignment sensitivities restated in NumPy long double, and their finite-difference truth.  TEST INFRASTRUCTURE, written
from the formulas, not from csrc/art_tubes.h: all six columns of a group travel as one array, the Hessian is
taken to the lab frame, and the motion fields are formed from the element's own axes.

Group 0 is the source, group g >= 1 element g - 1; column c = 6 g + i.  Element columns: with r_0, r_1, r_2 = major axis,
normal x major, normal, i = 0..2 shift along r_i (s = r_i, theta = 0), i = 3..5 rotation about r_i through the position
(s = r_i x (X - pos), theta = r_i).  Source columns: i = 0..2 dP = e_i, i = 3..5 dD = e_i x D0.
At the element that moves:  t = (P - P_prev).D, a = dP + t dD, dt = -n.(a - s(P)) / (n.D), dQ = a + D dt,
  dn = dn_surf(dQ - s(P)) + theta x n, dD' = dD - 2 [(dD.n + D.dn) n + (D.n) dn], dP' = dQ, dL += dt;
everywhere else the same with s = theta = 0 (a mask keeps dD).  Detector: the plane rule, dL += dt, (dX, dY) = (rot dX_lab)[0:2]."""
import copy

import numpy as np

import tubes_common as tb

LD = tb.LD
ld = tb.ld
_dot = tb._dot
COLS = 6
SOURCE_DOFS = ("shift_x", "shift_y", "shift_z", "tilt_x", "tilt_y", "tilt_z")
ELEMENT_DOFS = ("shift_major", "shift_cross", "shift_normal", "roll", "pitch", "yaw")
SCENES = ("a_toroid", "b_sphere", "c_kb", "d_twisted", "h_mixed8")


def detector_rot(normal):
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    return mgeo.rotation_matrix(np.asarray(normal, dtype=float), np.array([0.0, 0.0, 1.0]))


def axes_of(oe):
    """r_0, r_1, r_2 of an element from its own vectors: major axis, normal x major, normal."""
    m, n = ld(oe.majoraxis), ld(oe.normal)
    return np.stack([m, np.cross(n, m), n])


def _element_step(s, D, Pprev, P, dP, dD, dL, sv, th):
    """dP, dD [n, c, 3], dL [n, c]; sv, th [n, c, 3] (zeros at an element that stays)."""
    F = s["fwd"]
    Po = (P - s["pos"]) @ F.T + s["centre"]
    g, H = tb.grad_hess(s, Po)
    gn = np.sqrt(_dot(g, g))
    n = (-g / gn[:, None]) @ F
    nD = _dot(n, D)
    a = dP + _dot(P - Pprev, D)[:, None, None] * dD
    dt = -_dot(a - sv, n[:, None, :]) / nD[:, None]
    dQ = a + D[:, None, :] * dt[:, :, None]
    if s["kind"] == "mask":
        return dQ, dD, dL + dt
    Hl = F.T @ H @ F
    Hv = np.einsum("nab,ncb->nca", Hl, dQ - sv)
    dn = -(Hv - n[:, None, :] * _dot(Hv, n[:, None, :])[:, :, None]) / gn[:, None, None] + np.cross(th, n[:, None, :])
    k = _dot(dD, n[:, None, :]) + _dot(dn, D[:, None, :])
    return dQ, dD - 2 * (k[:, :, None] * n[:, None, :] + nD[:, None, None] * dn), dL + dt


def run(specs, axes, hist, det, rot, w=None, alive=None, origin=(0.0, 0.0, 0.0), path=None):
    """specs: tubes_common.spec_of per element; axes: axes_of per element; hist: [(P, D)] of the source and after each
    element; det = (centre, normal), rot its 3x3; path: the path at the last view (None: the sum of the legs).
    Returns per-ray dX, dY, dL [M, n], dD [M, n, 3], dXlab [M, n, 3] (NaN where the ray does not count), the nominal
    X, Y, L about `origin`, and `table`, the [1 + M, 16] sums of art_sensitivities."""
    hist = [(ld(P), ld(D)) for P, D in hist]
    n, K = len(hist[0][0]), len(specs)
    alive = np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
    w = np.ones(n, dtype=LD) if w is None else ld(w)
    hist = [(np.where(alive[:, None], P, 1), np.where(alive[:, None], D, LD(1) / np.sqrt(LD(3)))) for P, D in hist]
    if path is None:
        path = sum(np.sqrt(_dot(hist[k + 1][0] - hist[k][0], hist[k + 1][0] - hist[k][0])) for k in range(K))
    path = np.where(alive, ld(path), 0)
    C, nd, R = ld(det[0]), ld(det[1]), ld(rot)
    Pl, Dl = hist[-1]
    tdet = ((C - Pl) @ nd) / (Dl @ nd)
    XY = (Pl + tdet[:, None] * Dl - C) @ R.T
    X, Y, L = XY[:, 0] - LD(origin[0]), XY[:, 1] - LD(origin[1]), path + tdet - LD(origin[2])
    M = COLS * (K + 1)
    out = {k: np.zeros((M, n), dtype=LD) for k in ("dX", "dY", "dL")}
    out["dD"], out["dXlab"] = np.zeros((M, n, 3), dtype=LD), np.zeros((M, n, 3), dtype=LD)
    eye = np.eye(3, dtype=LD)
    zero = np.zeros((n, COLS, 3), dtype=LD)
    with np.errstate(all="ignore"):
        for g in range(K + 1):
            dP, dD, dL = zero.copy(), zero.copy(), np.zeros((n, COLS), dtype=LD)
            if g == 0:
                dP[:, 0:3] = eye[None]
                dD[:, 3:6] = np.cross(eye[None], hist[0][1][:, None, :])
            for e in range(max(g - 1, 0), K):
                sv, th = zero, zero
                if e == g - 1:
                    r, rel = axes[e], hist[e + 1][0] - specs[e]["pos"]
                    sv = np.concatenate([np.broadcast_to(r[None], (n, 3, 3)), np.cross(r[None], rel[:, None, :])], 1)
                    th = np.concatenate([zero[:, 0:3], np.broadcast_to(r[None], (n, 3, 3))], 1)
                dP, dD, dL = _element_step(specs[e], hist[e][1], hist[e][0], hist[e + 1][0], dP, dD, dL, sv, th)
            a = dP + tdet[:, None, None] * dD
            dt = -(a @ nd) / (Dl @ nd)[:, None]
            dXl = a + Dl[:, None, :] * dt[:, :, None]
            dxy = dXl @ R.T
            sl = slice(COLS * g, COLS * (g + 1))
            out["dX"][sl], out["dY"][sl], out["dL"][sl] = dxy[:, :, 0].T, dxy[:, :, 1].T, (dL + dt).T
            out["dD"][sl], out["dXlab"][sl] = dD.transpose(1, 0, 2), dXl.transpose(1, 0, 2)
    table = np.zeros((1 + M, 16), dtype=LD)
    wa = np.where(alive, w, 0)
    z = lambda v: np.where(alive, v, 0)
    table[0, :8] = [alive.sum(), wa.sum(), (wa * z(X)).sum(), (wa * z(Y)).sum(), (wa * z(L)).sum(), (wa * z(X) ** 2).sum(),
                    (wa * z(Y) ** 2).sum(), (wa * z(L) ** 2).sum()]
    for c in range(M):
        dX, dY, dL = z(out["dX"][c]), z(out["dY"][c]), z(out["dL"][c])
        table[1 + c, :9] = [(wa * dX).sum(), (wa * dY).sum(), (wa * dL).sum(), (wa * z(X) * dX).sum(), (wa * z(Y) * dY).sum(),
                            (wa * z(L) * dL).sum(), (wa * dX * dX).sum(), (wa * dY * dY).sum(), (wa * dL * dL).sum()]
        table[1 + c, 9:12] = (wa[:, None] * np.where(alive[:, None], out["dD"][c], 0)).sum(axis=0)
    nan = LD(np.nan)
    for k in ("dX", "dY", "dL"):
        out[k] = np.where(alive[None, :], out[k], nan)
    for k in ("dD", "dXlab"):
        out[k] = np.where(alive[None, :, None], out[k], nan)
    far = lambda v: float(np.abs(v[alive]).max()) if alive.any() else 0.0
    out.update(X=X, Y=Y, L=L, table=table, alive=alive, span=(far(np.sqrt(_dot(C - Pl, C - Pl))), far(path + tdet)))
    return out


# ------------------------------------------------------------------------------------------- the finite-difference truth
def moved_elements(els, k, i, h):
    """A copy of the elements with element k moved by h (mm or rad) in its degree of freedom i, by the package's methods."""
    els = copy.deepcopy(els)
    name = ("shift_along_major", "shift_along_cross", "shift_along_normal", "rotate_roll_by", "rotate_pitch_by", "rotate_yaw_by")[i]
    getattr(els[k], name)(float(h) if i < 3 else float(np.rad2deg(h)))
    return els


def moved_source(P0, D0, i, h):
    """The source moved by h in its degree of freedom i by what shift_source / tilt_source apply to a ray list:
    ModuleGeometry.TranslationRayList by distance * axis, RotationAroundAxisRayList about axis by the angle."""
    from attosecondraytracing_amd import ModuleGeometry as mgeo, ModuleOpticalRay as mray
    rays = [mray.Ray(np.array(p, dtype=float), np.array(d, dtype=float), Number=k) for k, (p, d) in enumerate(zip(P0, D0))]
    axis = np.eye(3)[i % 3]
    if i < 3:
        rays = mgeo.TranslationRayList(rays, float(h) * mgeo.Normalize(axis))
    else:
        rays = mgeo.RotationAroundAxisRayList(rays, axis, np.deg2rad(float(np.rad2deg(h))))
    return np.array([r.point for r in rays]), np.array([r.vector for r in rays])


def final(els, P0, D0, det, plan):
    """Hit point on the detector, final direction and path (the sum of the legs) of a re-trace with the nominal plan."""
    hist, _, _ = tb.trace_history(els, P0, D0, plan)
    X, V = hist[-1]
    C, nd = ld(det[0]), ld(det[1])
    t = ((C - X) @ nd) / (V @ nd)
    legs = sum(np.sqrt(_dot(hist[k + 1][0] - hist[k][0], hist[k + 1][0] - hist[k][0])) for k in range(len(els)))
    return X + t[:, None] * V, V, legs + t


def fd_column(els, P0, D0, det, plan, g, i, h):
    """Richardson-extrapolated central differences (steps h, h / 2) of (detector hit point, direction, path) with respect
    to column i of group g, and the step-halving estimates |extrapolated - value at h / 2|."""
    per = []
    for step in (h, h / 2):
        pm = []
        for sgn in (+1, -1):
            if g == 0:
                pm.append(final(els, *moved_source(P0, D0, i, sgn * step), det, plan))
            else:
                pm.append(final(moved_elements(els, g - 1, i, sgn * step), P0, D0, det, plan))
        per.append([(a - b) / (2 * LD(step)) for a, b in zip(*pm)])
    one, two = per
    return [(4 * b - a) / 3 for a, b in zip(one, two)], [np.abs(b - a) / 3 for a, b in zip(one, two)]


def with_detector(sc):
    """The scene's detector, or tubes_common.tilted_detector on its chief ray's last point and direction."""
    if sc["det"] is not None:
        return sc["det"]
    P, D = sc["hist"][-1]
    return tb.tilted_detector(np.asarray(P[0], dtype=float), np.asarray(D[0], dtype=float))


def prepare(sc, every=1):
    """Traces a scene of tubes_common (every `every`-th ray, the chief ray first) and adds hist, alive, plan, specs, axes,
    det, rot, hist64 and `ref`, the restatement on the fp64 history."""
    sc = dict(sc)
    P0, D0 = sc["rays"]
    sc["rays"] = (P0[::every], D0[::every])
    sc["w"] = None if sc["w"] is None else sc["w"][::every]
    sc["hist"], sc["alive"], sc["plan"] = tb.trace_history(sc["els"], *sc["rays"])
    sc["specs"] = [tb.spec_of(oe) for oe in sc["els"]]
    sc["axes"] = [axes_of(oe) for oe in sc["els"]]
    sc["det"] = with_detector(sc)
    sc["rot"] = detector_rot(sc["det"][1])
    sc["hist64"] = [(np.asarray(P, dtype=float), np.asarray(D, dtype=float)) for P, D in sc["hist"]]
    sc["ref"] = run(sc["specs"], sc["axes"], sc["hist64"], sc["det"], sc["rot"], sc["w"], sc["alive"])
    return sc


def all_scenes():
    return {**tb.scenes(), **tb.scenes_more()}


def units_of(K):
    return np.array(([0] * 3 + [1] * 3) * (K + 1))           # 0: per mm, 1: per rad


def compare_columns(got, ref, alive, what, K, bar=tb.PARITY):
    """got, ref [M, n(, 3)]: |got - ref| <= bar * the largest |ref| among the job's columns of the same unit."""
    got, ref = ld(got), ld(ref)
    u = units_of(K)
    worst = 0.0
    for unit in (0, 1):
        r, v = ref[u == unit][:, alive], got[u == unit][:, alive]
        if r.size == 0:
            continue
        scale, err = np.abs(r).max(), np.abs(v - r).max()
        assert np.isfinite(v).all() and (err <= bar * scale or err == 0), \
            f"{what} per {('mm', 'rad')[unit]}: {float(err):.3e} against {bar:g} of {float(scale):.3e}"
        worst = max(worst, float(err / scale) if scale > 0 else 0.0)
    return worst


def compare_table(got, ref, K, what, span, bar=tb.PARITY):
    """The [1 + M, 16] table.  Every entry q of the column rows: against the largest |reference| of entry q among the
    columns of the same unit (the three components of sum w dD' share one scale).  Row 0 has no columns: sum w and the
    second moments against themselves; the first moments are taken about the origin and cancel by design, so they are
    judged by the size of their terms, sum w |X| <= sqrt(sum w . sum w X^2).
    span = run()'s: X, Y and L are differences of fp64 numbers of the sizes span = (distance to the detector, path) and no
    fp64 code knows them better than a few eps of those, however small they themselves are (one ray about its own
    mean: zero).  Every sum that holds X, Y or L is therefore allowed FLOOR = 16 eps(fp64) x span per unit of the other
    factors, beside the bar: sum w for the first moments, 2 sum w |X| + sum w FLOOR for the second, sum w |dX| <=
    sqrt(sum w . sum w dX^2) for the products with a column."""
    got, ref = ld(got), ld(ref)
    assert got.shape == ref.shape == (1 + COLS * (K + 1), 16), what
    assert got[0, 0] == ref[0, 0] and not got[0, 8:].any() and not got[1:, 12:].any(), what
    floor = [16 * LD(np.finfo(np.float64).eps) * LD(v) for v in (span[0], span[0], span[1])]
    sw = ref[0, 1]
    worst = 0.0
    for q in range(1, 8):
        if q == 1:
            scale, extra = np.abs(ref[0, q]), 0
        elif q < 5:
            scale, extra = np.sqrt(sw * ref[0, q + 3]), sw * floor[q - 2]
        else:
            scale, extra = np.abs(ref[0, q]), floor[q - 5] * (2 * np.sqrt(sw * ref[0, q]) + sw * floor[q - 5])
        err = np.abs(got[0, q] - ref[0, q])
        assert err <= bar * scale + extra, f"{what} row 0 [{q}]: {float(err):.3e} against {bar:g} of {float(scale):.3e} + {float(extra):.3e}"
        worst = max(worst, float(err / scale) if scale > 0 and err > extra else 0.0)
    u = units_of(K)
    for unit in (0, 1):
        rows = 1 + np.flatnonzero(u == unit)
        for q in range(12):
            if q < 9:
                scale, err = np.abs(ref[rows, q]).max(), np.abs(got[rows, q] - ref[rows, q]).max()
            else:                                                  # the three components of one vector share a scale
                scale, err = np.abs(ref[rows, 9:12]).max(), np.abs(got[rows, q] - ref[rows, q]).max()
            extra = floor[q - 3] * np.sqrt(sw * np.abs(ref[rows, q + 3]).max()) if q in (3, 4, 5) else 0
            assert err <= bar * scale + extra, \
                f"{what} entry {q} per {('mm', 'rad')[unit]}: {float(err):.3e} against {bar:g} of {float(scale):.3e} + {float(extra):.3e}"
            worst = max(worst, float(err / scale) if scale > 0 and err > extra else 0.0)
    return worst

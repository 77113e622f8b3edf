"""Wavefront aberrations as Zernike fits, summed on the device (art_hip.h, art_wavefront): Detector.get_Wavefront.

For a bundle on a detector with centre C and frame e1, e2, n (the rows e1, e2 of its rotation and its normal, the frame
of get_FocalField):

* reference point  R = C + X e1 + Y e2 - s n: pixel (X, Y) of get_FocalField in the plane of Shifts=[s]
  (Detector.shiftByDistance's sign); the default is the detector centre, X = Y = s = 0;
* wavefront error  W_r = (path_r - RefPath) + d_r . (R - p_r) in mm for every alive ray (positive: the ray arrives
  late), RefPath by default the mean optical path of the alive rays, as in get_FocalField.  k W_r is the phase that
  get_FocalField gives ray r at R, to rounding;
* pupil            x_r = (d_r . e1 - a1) / rho, y_r = (d_r . e2 - a2) / rho, the direction cosines in the detector
  frame about the pupil centre (a1, a2) (default (0, 0): the detector axis, the mean ray after autoplace), scaled by
  the pupil radius rho (default: the largest distance of an alive ray from (a1, a2), found on the device).  With an
  explicit radius, rays with x^2 + y^2 > 1 get weight 0 and are counted as `outside`;
* basis            all Z_nm(x, y), n <= Order, in the unnormalised Andersen convention of ModuleDefects.Zernike and
  zernike_monomials (Z_10 = y, Z_11 = x; keys (n, m), 0 <= m <= n), J = (Order + 1)(Order + 2) / 2 of them, plus the
  column d_r . n;
* weights          the bundle's intensities, or 1, with the equal-solid-angle caveat of focal.py.

The device returns, per bundle, the Gram matrix G = sum_r w_r v_r v_r^T of v_r = [Z_0 .. Z_{J-1}, d.n, W_r], the
number of rays used and outside, sum w, the radius and the range of W -- one pass over the bundle and a fixed-order
sum, so the host never reads the rays.  The rest is fp64 algebra on G here: the Zernike coefficients (the weighted
least-squares fit of W), the rms about the mean, the rms left after the fit, and the best reference point R*, the
solution of the sub-problem {Z_00, Z_11, Z_10, d.n} against W: W at R' is exactly W + d . (R' - R), so R* minimises
the weighted rms of W (rms_best) over all reference points.

Limits: the fit describes the wavefront on the rays' directions; no binned residual maps are formed on the device
(`map` evaluates the fitted polynomial); all rays are taken as mutually coherent (no partial coherence); a collimated
beam, whose pupil coordinates would be positions rather than directions, is not covered."""
import math

import numpy as np

from . import _abi
from .bundle import RayBundle

MAX_JOBS_PER_CALL = 64
DEFAULT_ORDER = 8
_REMOVABLE = {"piston": ((0, 0),), "tilt": ((1, 0), (1, 1)), "defocus": ((2, 1),)}


def zernike_keys(order):
    """The (n, m) keys of the basis in column order: column n (n + 1) / 2 + m."""
    return [(n, m) for n in range(order + 1) for m in range(n + 1)]


def unpack_gram(row):
    """The symmetric K x K matrix G of an output row of art_wavefront (K in row[6])."""
    K = int(row[6])
    iu = np.triu_indices(K)
    G = np.zeros((K, K))
    G[iu] = row[8:8 + K * (K + 1) // 2]
    return G + np.triu(G, 1).T


def _lstsq(M, b):
    """Solve M x = b for a symmetric positive semi-definite M, Jacobi-scaled (minimum-norm where M is singular)."""
    d = np.sqrt(np.diag(M))
    d = np.where(d > 0, d, 1.0)
    x = np.linalg.lstsq(M / np.outer(d, d), b / d, rcond=None)[0]
    return x / d


def solve(G, sum_w):
    """(coefficients [J], rms, rms_residual, beta [4], rms_best) from the Gram matrix G of rows [Z_0 .. Z_{J-1}, d.n, W]
    and sum w: the weighted least-squares fit of W, the rms about the mean, the rms after the fit, and the solution
    beta of min || W + beta_0 Z_00 + beta_1 Z_11 + beta_2 Z_10 + beta_3 d.n ||_w with its rms."""
    K = G.shape[0]
    J = K - 2
    gww = G[K - 1, K - 1]
    c = _lstsq(G[:J, :J], G[:J, K - 1])
    mean = G[0, K - 1] / sum_w
    rms = math.sqrt(max(gww / sum_w - mean * mean, 0.0))
    rms_residual = math.sqrt(max(gww - float(c @ G[:J, K - 1]), 0.0) / sum_w)
    sub = [0, 2, 1, J] if J > 2 else [0, J]
    b = G[sub, K - 1]
    beta = -_lstsq(G[np.ix_(sub, sub)], b)
    rms_best = math.sqrt(max(gww + float(beta @ b), 0.0) / sum_w)
    if J <= 2:                     # order 0: the point can move along the axis only
        beta = np.array([beta[0], 0.0, 0.0, beta[1]])
    return c, rms, rms_residual, beta, rms_best


def disk_moments(order):
    """{(n, m): (mean, mean square)} of Z_nm over the unit disk, exact from the monomial tables."""
    from .ModuleDefects import zernike_monomials
    from math import gamma
    tables = zernike_monomials(max(order, 2))

    def integral(C):            # int over the unit disk of sum_pq C[p, q] x^p y^q
        s = 0.0
        for p, q in zip(*np.nonzero(C)):
            if p % 2 == 0 and q % 2 == 0:
                s += C[p, q] * 2 * gamma((p + 1) / 2) * gamma((q + 1) / 2) / ((p + q + 2) * gamma((p + q + 2) / 2))
        return s

    out = {}
    for key in zernike_keys(order):
        C = tables[key].astype(float)
        D = C.shape[0]
        sq = np.zeros((2 * D, 2 * D))
        for p, q in zip(*np.nonzero(C)):
            sq[p:p + D, q:q + D] += C[p, q] * C
        out[key] = (integral(C) / math.pi, integral(sq) / math.pi)
    return out


class Wavefront:
    """The Zernike fit of one bundle's wavefront (see the module's docstring).  Lengths in mm.

    coefficients {(n, m): c} with W ~ sum c Z_nm(x, y); waves: the same over the wavelength (NaN without one);
    term_rms {(n, m)}: the rms of c Z_nm over the unit disk (0 for piston); rms: the weighted rms of W about its mean;
    rms_residual: what the fit leaves; rms_best: the rms about the mean at the best reference point; best_focus:
    (X, Y, Shift) of that point in get_FocalField's conventions; strehl_marechal: exp(-(2 pi rms_best / wavelength)^2);
    count / outside: rays used / rays outside an explicit pupil radius; pupil_radius, pupil_centre, centre, shift,
    ref_path, order, wavelength, sum_w, w_range (min, max of W); gram: the K x K matrix the device formed; opd [n] and
    pupil [2, n] (x, y): device tensors over the slots with PerRay=True (NaN for slots not used), else None.  Without a
    used ray every result is NaN and count is 0."""

    def __init__(self, row, order, centre, shift, ref_path, pupil_centre, wavelength, opd=None, pupil=None):
        self.order = int(order)
        self.centre, self.shift = (float(centre[0]), float(centre[1])), float(shift)
        self.ref_path, self.pupil_centre = float(ref_path), (float(pupil_centre[0]), float(pupil_centre[1]))
        self.wavelength = math.nan if wavelength is None else float(wavelength)
        self.opd, self.pupil = opd, pupil
        self.count, self.outside = int(row[0]), int(row[1])
        self.sum_w = float(row[2])
        keys = zernike_keys(self.order)
        self.gram = unpack_gram(row)
        nan = math.nan
        if self.count > 0 and self.sum_w > 0:
            c, self.rms, self.rms_residual, beta, self.rms_best = solve(self.gram, self.sum_w)
            self.pupil_radius = float(row[3])
            self.w_range = (float(row[4]), float(row[5]))
            self.best_focus = (self.centre[0] + beta[1] / self.pupil_radius,
                               self.centre[1] + beta[2] / self.pupil_radius, self.shift - beta[3])
        else:
            c = np.full(len(keys), nan)
            self.rms = self.rms_residual = self.rms_best = self.pupil_radius = nan
            self.w_range, self.best_focus = (nan, nan), (nan, nan, nan)
        self.coefficients = {k: float(v) for k, v in zip(keys, c)}
        self.waves = {k: v / self.wavelength for k, v in self.coefficients.items()}
        self.strehl_marechal = math.exp(-(2 * math.pi * self.rms_best / self.wavelength) ** 2)
        mom = disk_moments(self.order)
        self.term_rms = {k: abs(v) * math.sqrt(max(mom[k][1] - mom[k][0] ** 2, 0.0)) for k, v in self.coefficients.items()}

    def map(self, pixels=128, remove=()):
        """The fitted surface sum c_nm Z_nm (mm) on a pixels x pixels grid over [-1, 1]^2 of pupil coordinates (row = y),
        NaN outside the unit disk, evaluated from the monomial tables; `remove`: any of "piston", "tilt", "defocus"."""
        from .ModuleDefects import zernike_monomials
        pixels = int(pixels)
        if pixels < 2:
            raise ValueError("pixels must be an integer >= 2")
        drop = set()
        for name in remove:
            if name not in _REMOVABLE:
                raise ValueError(f"remove: unknown term {name!r} (one of {sorted(_REMOVABLE)})")
            drop.update(_REMOVABLE[name])
        tables = zernike_monomials(max(self.order, 2))
        A = sum(c * tables[k].astype(float) for k, c in self.coefficients.items() if k not in drop)
        u = np.linspace(-1.0, 1.0, pixels)
        x, y = np.meshgrid(u, u)
        surf = np.polynomial.polynomial.polyval2d(x, y, A) if np.ndim(A) else np.full_like(x, float(A))
        return np.where(x * x + y * y <= 1.0, surf, np.nan)

    @property
    def pv(self):
        """Peak to valley (mm) of map(128)."""
        m = self.map(128)
        return float(np.nanmax(m) - np.nanmin(m)) if np.isfinite(m).any() else math.nan


def _finite(v, name, count=None):
    vals = np.atleast_1d(np.asarray(v, dtype=float)) if count else np.asarray([float(v)])
    if (count and vals.shape != (count,)) or not np.isfinite(vals).all():
        raise ValueError(f"{name} must be {count} finite numbers" if count else f"{name} must be finite")
    return [float(a) for a in vals]


def resolve(Order=DEFAULT_ORDER, Centre=None, Shift=0.0, RefPath=None, PupilCentre=None, PupilRadius=None,
            Wavelength=None, PerRay=False):
    """get_Wavefront's arguments validated: a dict (ValueError naming the argument otherwise)."""
    if isinstance(Order, bool) or not (np.isscalar(Order) and float(Order) == int(Order)) \
            or not 0 <= int(Order) <= _abi.ART_WAVEFRONT_MAX_ORDER:
        raise ValueError(f"Order must be an integer in [0, {_abi.ART_WAVEFRONT_MAX_ORDER}]")
    p = {"order": int(Order), "per_ray": bool(PerRay)}
    p["centre"] = (0.0, 0.0) if Centre is None else tuple(_finite(Centre, "Centre", 2))
    p["shift"] = _finite(Shift, "Shift")[0]
    p["ref_path"] = None if RefPath is None else _finite(RefPath, "RefPath")[0]
    p["pupil_centre"] = (0.0, 0.0) if PupilCentre is None else tuple(_finite(PupilCentre, "PupilCentre", 2))
    if PupilRadius is None:
        p["pupil_radius"] = 0.0
    else:
        r = _finite(PupilRadius, "PupilRadius")[0]
        if not r > 0:
            raise ValueError("PupilRadius must be finite and positive")
        p["pupil_radius"] = r
    if Wavelength is not None:
        wl = _finite(Wavelength, "Wavelength")[0]
        if not wl > 0:
            raise ValueError("Wavelength must be finite and positive")
        p["wavelength"] = wl
    else:
        p["wavelength"] = None
    return p


def wavefronts(requests):
    """requests: [(bundle, detector, kwargs)], kwargs those of Detector.get_Wavefront.  Returns one Wavefront per request,
    in order.  The default reference paths come from one batch of lite read-outs, read back together; then all bundles
    of one backend go to the device in ONE call of art_wavefront (blocks of MAX_JOBS_PER_CALL)."""
    import torch
    items = []
    for B, det, kw in requests:
        p = resolve(**(kw or {}))
        B = RayBundle.of(B)
        det._iscomplete()
        if p["wavelength"] is None:
            p["wavelength"] = B.wavelength
        items.append([B, det, p, None])
    pending = []                      # (item, statistics on the device) for the default reference paths
    for it in items:
        if it[2]["ref_path"] is None:
            r = it[1].readout(it[0], store=False, lite=True, sync=False)
            pending.append((it, r["stats"] if "stats" in r else r["stats_dev"]))
    if pending:
        dev = [s for _, s in pending if not isinstance(s, np.ndarray)]
        host = iter(torch.stack([torch.as_tensor(s)[:2] for s in dev]).cpu().numpy() if dev else ())
        for it, s in pending:
            st = s if isinstance(s, np.ndarray) else next(host)
            it[2]["ref_path"] = (float(st[1] / st[0]) + it[0].phase_ref_offset(it[2]["wavelength"])) if st[0] > 0 else 0.0
    groups = {}
    for pos, it in enumerate(items):
        groups.setdefault(id(it[0].backend), []).append(pos)
    results = [None] * len(items)
    for positions in groups.values():
        be = items[positions[0]][0].backend
        for lo in range(0, len(positions), MAX_JOBS_PER_CALL):
            part = positions[lo:lo + MAX_JOBS_PER_CALL]
            jobs = [_job(items[pos]) for pos in part]
            out = be.wavefront(jobs).cpu().numpy()          # the one copy back to the host
            for k, pos in enumerate(part):
                B, det, p, per = items[pos]
                results[pos] = Wavefront(out[k], p["order"], p["centre"], p["shift"], p["ref_path"], p["pupil_centre"],
                                         p["wavelength"], *(per or (None, None)))
    return results


def _job(item):
    B, det, p, _ = item
    be, n = B.backend, B.n_slots
    j = _abi.ArtWavefrontJob()
    j.det = det._desc()
    j.b, j._keep = B.phase_path_view(p["wavelength"])       # (behind a grating: path + wavelength * grooves)
    j.w = None if B.intensity is None else B.intensity.data_ptr()
    j.n = n
    j.ref[:] = [p["centre"][0], p["centre"][1], p["shift"]]
    j.L_ref = p["ref_path"]
    j.pupil[:] = [p["pupil_centre"][0], p["pupil_centre"][1], p["pupil_radius"]]
    j.order = p["order"]
    if p["per_ray"]:
        opd = be.empty(n)
        pupil = be.empty(2 * n).reshape(2, n) if n else be.empty(0).reshape(2, 0)
        j.opd, j.pupil_x, j.pupil_y = (opd.data_ptr(), pupil[0].data_ptr(), pupil[1].data_ptr()) if n else (None, None, None)
        item[3] = (opd, pupil)
    return j


def wavefront(det, RayList, Order=DEFAULT_ORDER, Centre=None, Shift=0.0, RefPath=None, PupilCentre=None,
              PupilRadius=None, Wavelength=None, PerRay=False):
    """Detector.get_Wavefront (see the module's docstring)."""
    kw = dict(Order=Order, Centre=Centre, Shift=Shift, RefPath=RefPath, PupilCentre=PupilCentre, PupilRadius=PupilRadius,
              Wavelength=Wavelength, PerRay=PerRay)
    return wavefronts([(RayList, det, kw)])[0]

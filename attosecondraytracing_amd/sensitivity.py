"""Alignment sensitivities on the device (art_hip.h, art_sensitivities): OpticalChain.get_Sensitivities.

"How far does the spot move, and how much later does the pulse arrive, per microradian of pitch on mirror 3" used to cost
one re-trace per degree of freedom and step (get_OE_loop_list) and a finite difference on the host.  The transport that
carries ray tubes through every surface (csrc/art_tubes.h) also differentiates a ray with respect to a rigid
motion of any element or of the source: one streaming pass over the history a traced chain already holds gives the whole
alignment Jacobian -- 6 degrees of freedom per element plus 6 of the source, their effect on the detector centroid, the
arrival time, the pointing, the spot size and the path spread -- exact to first order and without a re-trace.

Degrees of freedom, in the order of the table (M = 6 (K + 1) columns):
  ("source", "shift_x" | "shift_y" | "shift_z")   mm   shift_source along the lab axes
  ("source", "tilt_x" | "tilt_y" | "tilt_z")      rad  tilt_source about the lab axes (the points held)
  (k, "shift_major" | "shift_cross" | "shift_normal")  mm   OpticalElement.shift_along_major / _cross / _normal of element k
  (k, "roll" | "pitch" | "yaw")                   rad  rotate_roll_by / _pitch_by / _yaw_by: rigid rotations of the optic
                                                       about its position (the package's methods take degrees)

Limits: a placed Detector is required; first order only; the set of counted rays is the nominal trace's (alive in every
bundle of the history): vignetting that changes with the motion is not differentiated; DeformedMirror, Grating and
MirrorFreeform elements raise NotImplementedError, as for get_RayTubes."""
import ctypes as C

import numpy as np

from . import _abi
from .analysis import LightSpeed
from .polarisation import history
from .tubes import _refuse

MAX_JOBS_PER_CALL = _abi.ART_TUBE_MAX_JOBS
COLS = _abi.ART_SENS_COLS
SOURCE_DOFS = ("shift_x", "shift_y", "shift_z", "tilt_x", "tilt_y", "tilt_z")
ELEMENT_DOFS = ("shift_major", "shift_cross", "shift_normal", "roll", "pitch", "yaw")
QUANTITIES = ("centroid_x", "centroid_y", "delay", "spot_variance_x", "spot_variance_y", "path_variance", "spread_x",
              "spread_y", "spread_path")
_FS_PER_MM = 1e15 / LightSpeed


def dof_names(K):
    return [("source", d) for d in SOURCE_DOFS] + [(k, d) for k in range(K) for d in ELEMENT_DOFS]


class Sensitivities:
    """What get_Sensitivities returns, per degree of freedom c of `names` (units[c]: "mm" or "rad"):
    centroid [M, 2]: d(mean X, mean Y) on the detector in mm per unit; delay [M]: d(mean path) in fs per unit;
    pointing [M, 3]: the mean change of the final direction (lab frame) per unit; spot_variance [M, 2]: d sigma_X^2,
    d sigma_Y^2 in mm^2 per unit; path_variance [M]: d sigma_L^2 in mm^2 per unit; spread [M, 3]: the rms of dX, dY, dL
    about their means (mm per unit) -- spot and path spread grow by spread^2 u^2 in quadrature where the first-order term
    vanishes (at a focus).  count, sum_w: the rays alive in every bundle of the history; mean = (X, Y, path) and
    variance of the nominal bundle; table: the [1 + M, 16] sums of art_sensitivities (host), origin: what X, Y and the
    path were taken about.  With PerRay: DEVICE dX, dY, dL [M, n] (NaN for the rays that do not count); without: None."""

    def __init__(self, table, origin, K, per_ray):
        self.table, self.origin = table, np.asarray(origin, dtype=float)
        self.names = dof_names(K)
        self.units = ["mm" if n[1].startswith("shift") else "rad" for n in self.names]
        r0, T = table[0], table[1:]
        self.count, self.sum_w = int(r0[0]), float(r0[1])
        sw = self.sum_w if self.sum_w > 0 else np.nan
        m = r0[2:5] / sw                                     # means about the origin
        self.mean = m + self.origin
        self.variance = r0[5:8] / sw - m * m
        d = T[:, 0:3] / sw                                   # mean dX, dY, dL
        self.centroid = d[:, 0:2].copy()
        self.delay = d[:, 2] * _FS_PER_MM
        self.pointing = T[:, 9:12] / sw
        var = 2.0 * (T[:, 3:6] / sw - m[None, :] * d)
        self.spot_variance, self.path_variance = var[:, 0:2].copy(), var[:, 2].copy()
        self.spread = np.sqrt(np.maximum(T[:, 6:9] / sw - d * d, 0.0))
        self.dX = self.dY = self.dL = None
        if per_ray is not None:
            self.dX, self.dY, self.dL = per_ray

    def index(self, who, dof):
        return self.names.index((who, dof))

    def quantity(self, name):
        """One of QUANTITIES as an [M] array."""
        if name not in QUANTITIES:
            raise ValueError(f"quantity must be one of {QUANTITIES}")
        k = "xy".find(name[-1]) if name[-2:] in ("_x", "_y") else 2
        if name.startswith("centroid"):
            return self.centroid[:, k]
        if name.startswith("spot_variance"):
            return self.spot_variance[:, k]
        if name.startswith("spread"):
            return self.spread[:, k]
        return self.delay if name == "delay" else self.path_variance

    def moves(self, shift_OE=(), rotate_OE=(), shift_source=(), tilt_source=()):
        """The [M] vector of a set of moves in the table's units.  shift_OE: (index, "major" | "cross" | "normal", mm) or a
        list of them; rotate_OE: (index, "roll" | "pitch" | "yaw", degrees); shift_source: (lab vector, mm) along the
        normalised vector; tilt_source: (lab vector, degrees) about it -- as the chain's methods of these names take them."""
        u = np.zeros(len(self.names))
        K = len(self.names) // COLS - 1
        many = lambda v: [v] if (isinstance(v, tuple) and len(v) and not isinstance(v[0], tuple)) else list(v)
        for idx, axis, dist in many(shift_OE):
            if axis not in ("major", "cross", "normal"):
                raise ValueError('a shift axis must be one of ["major", "cross", "normal"]')
            u[self.index(range(K)[idx], "shift_" + axis)] += float(dist)
        for idx, axis, deg in many(rotate_OE):
            if axis not in ("roll", "pitch", "yaw"):
                raise ValueError('a rotation axis must be one of ["roll", "pitch", "yaw"]')
            u[self.index(range(K)[idx], axis)] += np.deg2rad(float(deg))
        for first, moved in ((0, shift_source), (3, tilt_source)):
            for axis, amount in many(moved):
                a = np.asarray(axis, dtype=float) if not isinstance(axis, str) else None
                if a is None or a.shape != (3,) or not np.linalg.norm(a) > 0:
                    raise ValueError("a source move needs its axis as a lab vector of length 3")
                u[first:first + 3] += a / np.linalg.norm(a) * (float(amount) if first == 0 else np.deg2rad(float(amount)))
        return u

    def predict(self, **moves):
        """First-order effect of a set of moves (see `moves`): dict of centroid [2] in mm, delay in fs, pointing [3]."""
        u = self.moves(**moves)
        return {"centroid": u @ self.centroid, "delay": float(u @ self.delay), "pointing": u @ self.pointing}


def sensitivities(requests):
    """requests: [(chain, kwargs)], kwargs those of OpticalChain.get_Sensitivities.  One Sensitivities per request, in
    order; all chains of one backend go to the device in ONE call of art_sensitivities (blocks of MAX_JOBS_PER_CALL), and
    the one copy back to the host per call is the table.  The origins (the weighted means of X, Y and the path) come from
    the detector's read-out statistics of the final bundle, all enqueued before the first is read."""
    items = []
    for chain, kw in requests:
        kw = dict(kw or {})
        unknown = set(kw) - {"Detector", "PerRay"}
        if unknown:
            raise TypeError(f"unknown arguments {sorted(unknown)}")
        det = kw.get("Detector")
        if det is None:
            raise TypeError("sensitivities need a Detector")
        det._iscomplete()
        els = list(chain.optical_elements)
        if not 1 <= len(els) <= _abi.ART_TUBE_MAX_ELEMS:
            raise ValueError(f"a chain needs 1..{_abi.ART_TUBE_MAX_ELEMS} optical elements")
        for k, oe in enumerate(els):
            _refuse(k, oe)
        items.append((history(chain), els, det, bool(kw.get("PerRay", False))))
    stats = [det.readout(bundles[-1], sync=False, store=False) for bundles, _, det, _ in items]
    origins = []
    for st in stats:
        s = st["stats"] if "stats" in st else st["stats_dev"].cpu().numpy()
        origins.append(tuple(float(v) / float(s[8]) for v in s[9:12]) if s[8] > 0 and np.isfinite(s[8:12]).all()
                       else (0.0, 0.0, 0.0))
    groups = {}
    for pos, it in enumerate(items):
        groups.setdefault(id(it[0][-1].backend), []).append(pos)
    results = [None] * len(items)
    for positions in groups.values():
        be = items[positions[0]][0][-1].backend
        for lo in range(0, len(positions), MAX_JOBS_PER_CALL):
            part = positions[lo:lo + MAX_JOBS_PER_CALL]
            made = [_job(items[pos], origins[pos]) for pos in part]
            rows = be.sensitivities(*[[m[q] for m in made] for q in range(4)]).cpu().numpy()
            at = 0
            for k, pos in enumerate(part):
                K = len(items[pos][1])
                size = 1 + COLS * (K + 1)
                results[pos] = Sensitivities(rows[at:at + size].copy(), origins[pos], K, made[k][4])
                at += size
    return results


def _job(item, origin):
    from . import ModuleProcessing as mp
    bundles, els, det, per_ray = item
    last = bundles[-1]
    be, n = last.backend, last.n_slots
    K = len(els)
    descs = [mp.element_descriptor(oe, True, be)[0] for oe in els]
    elems = (_abi.ArtElementDesc * K)()
    for k, d in enumerate(descs):
        C.memmove(C.addressof(elems[k]), C.addressof(d), C.sizeof(_abi.ArtElementDesc))
    quadrics = None
    if any(d.flags & _abi.ART_FLAG_QUADRIC for d in descs):
        quadrics = (_abi.ArtQuadricDesc * K)()
        for k, d in enumerate(descs):
            if d.flags & _abi.ART_FLAG_QUADRIC:
                quadrics[k] = be._quadric_desc(d.quadric._quadric_coefficients())
    j = _abi.ArtSensitivityJob()
    j.n_elems, j.n = K, n
    j.det = det._desc()
    j.origin[:] = origin
    j.w = None if last.intensity is None else last.intensity.data_ptr()
    arrays = None
    if per_ray:
        M = COLS * (K + 1)
        buf = be.empty(3 * M * max(n, 1))
        arrays = tuple(buf[q * M * n:(q + 1) * M * n].reshape(M, n) for q in range(3))
        j.dX, j.dY, j.dL = (a.data_ptr() for a in arrays)
    views = (_abi.ArtBundleView * (K + 1))(*[b.view() for b in bundles])
    return j, views, elems, quadrics, arrays


def sensitivity(chain, Detector, PerRay=False):
    """OpticalChain.get_Sensitivities (see the module's docstring)."""
    return sensitivities([(chain, dict(Detector=Detector, PerRay=PerRay))])[0]

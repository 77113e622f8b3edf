"""Exact weighted quantiles and encircled energy on the device (art_hip.h, art_quantiles): Detector.get_EncircledEnergy,
OpticalChain.get_EncircledEnergy, weighted_quantiles.

A second moment (the rms spot, the rms duration) mostly measures the tails of a focus with a sharp core, which is what
grazing-incidence optics make; such optics are specified by the radius that holds a given share of the power instead: the
half-energy width HEW = twice the 50 % radius, W90, the encircled-energy curve.  Both directions are rank statistics of
ALL rays and run next to the bundle:

  quantile   the smallest key v whose slots up to it hold at least the share f of the weight: a most-significant-digit
             radix select in six passes over the keys, nothing read back in between.  The answer is the key of an actual
             ray, not a bin edge, and needs no range chosen in advance.
  rank sum   the weight within each of a sorted list of radii, in one pass: the encircled-energy curve.

Weights are art_histogram's fixed-point integers q = rint(ldexp(w, shift)) (histogram.shift_for picks the shift), every
sum is an integer sum, so a result is the same bytes on every run.  The definition, with W = sum q over the valid slots:

    T = min(W, max(1, ceil(f * float(W))))     value = the smallest key v with sum_{key <= v} q >= T

A NaN key makes a slot invalid (counted, otherwise ignored); dead slots contribute nothing; +-inf are ordinary keys.

Limits: geometric rays only -- the encircled energy of a diffraction image (get_FocalField) is not this; the "Delay" metric
is the window SYMMETRIC about the centre, not the shortest window that holds the share; weights must be finite and >= 0;
at most 16 fractions, 256 radii and 64 planes per call, 2^28 rays."""
import math

import numpy as np

from . import _abi
from . import histogram as hist

MAX_FRACTIONS = _abi.ART_QUANTILE_MAX_FRACTIONS
MAX_THRESHOLDS = _abi.ART_QUANTILE_MAX_THRESHOLDS
_METRICS = {"radius": _abi.ART_QKEY_RADIUS, "X": _abi.ART_QKEY_X, "Y": _abi.ART_QKEY_Y, "Delay": _abi.ART_QKEY_DELAY}


def target(W, f):
    """T of the definition above for the integer weight sum W and the fraction f (0 when W is 0)."""
    W = int(W)
    return min(W, max(1, int(math.ceil(float(f) * float(W)))))


def key_bits(values):
    """The order-preserving uint64 image of float64 keys that the device sorts by: -0 becomes +0, a non-negative value
    gets its sign bit set, a negative value is complemented.  (NaN has no place in the order: such slots are invalid.)"""
    v = np.array(values, dtype=np.float64, copy=True)
    v[v == 0.0] = 0.0
    b = v.view(np.uint64)
    neg = (b >> np.uint64(63)).astype(bool)
    return np.where(neg, ~b, b | np.uint64(1 << 63))


def _fractions(Fractions):
    f = [float(v) for v in np.atleast_1d(np.asarray(Fractions, dtype=float))]
    if not f:
        raise ValueError("Fractions must not be empty")
    if len(f) > MAX_FRACTIONS:
        raise ValueError(f"at most {MAX_FRACTIONS} fractions per call")
    if not all(0.0 <= v <= 1.0 for v in f):
        raise ValueError("every fraction must lie in [0, 1]")
    return f


def _thresholds(T, planes, name="Thresholds", non_negative=False):
    """None, or the float64 array [planes, R] of `T` ([R]: the same for every plane), sorted along R."""
    if T is None:
        return None
    t = np.asarray(T, dtype=np.float64)
    if t.ndim == 1:
        t = np.tile(t, (planes, 1))
    if t.ndim != 2 or t.shape[0] != planes:
        raise ValueError(f"{name} must be a list, or one list per plane")
    if t.shape[1] > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} {name} per call")
    if np.isnan(t).any() or (np.diff(t, axis=1) < 0).any():
        raise ValueError(f"{name} must be sorted in ascending order")
    if non_negative and (t < 0).any():
        raise ValueError(f"{name} must not be negative")
    return None if t.shape[1] == 0 else np.ascontiguousarray(t)


def _weight_range(w):
    """(min, max) of a weight tensor as ONE small device tensor (read back by the caller), None without weights."""
    import torch
    if w is None or w.numel() == 0:
        return None
    return torch.stack(torch.aminmax(w))


def _shift_from(n, rng):
    """The fixed-point shift for n slots whose weights span rng = (min, max) (None: no weights)."""
    if rng is None:
        return 0
    lo, hi = float(rng[0]), float(rng[1])
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError("the rays' intensities must be finite to be ranked")
    if lo < 0:
        raise ValueError("the rays' intensities must not be negative to be ranked")
    return hist.shift_for(n, hi)


class Quantiles:
    """What weighted_quantiles returns, numpy arrays.  values [P, K]: the quantiles (NaN where a plane has no weight);
    below, upto [P, K]: the integer weight sums over the keys < and <= the value; total [P]: W; count, invalid [P]: the
    valid slots and the alive slots with a NaN key; shift: the fixed-point shift S, weight = ldexp(q, -S); fractions [K];
    targets [P, K]: T.  With Thresholds: thresholds [P, R], rank_sums, rank_counts [P, R]: the weight and the number of
    valid slots with key <= threshold."""

    def __init__(self, values, below, upto, totals, shift, fractions, thresholds=None, rank_sums=None, rank_counts=None):
        self.values = np.asarray(values, dtype=np.float64)
        self.below, self.upto = np.asarray(below, dtype=np.int64), np.asarray(upto, dtype=np.int64)
        totals = np.asarray(totals, dtype=np.int64).reshape(-1, 3)
        self.total, self.count, self.invalid = totals[:, 0].copy(), totals[:, 1].copy(), totals[:, 2].copy()
        self.shift = int(shift)
        self.fractions = np.asarray(fractions, dtype=np.float64)
        self.targets = np.array([[target(W, f) for f in self.fractions] for W in self.total], dtype=np.int64).reshape(
            len(self.total), len(self.fractions))
        self.thresholds = thresholds
        self.rank_sums = None if rank_sums is None else np.asarray(rank_sums, dtype=np.int64)
        self.rank_counts = None if rank_counts is None else np.asarray(rank_counts, dtype=np.int64)

    @property
    def weight(self):
        """The total weight per plane, ldexp(W, -shift)."""
        return np.ldexp(self.total.astype(np.float64), -self.shift)


class EncircledEnergy:
    """What get_EncircledEnergy returns, numpy arrays.  radii [P, K]: the radius (mm; "X", "Y": the half width; "Delay":
    the half window in fs) about the centre that holds each of `fractions` of the power in each plane, the coordinate of
    an actual ray (NaN without power); enclosed [P, R]: the share of the power within each of `Radii` (the exact integer
    sums divided by W), None without Radii; centre [P, 2]: (cx, cy) on the detector; delay_centre [P]: the window's centre
    (fs, "Delay" only) measured from path_centre [P], the mean optical path (mm); power [P]: ldexp(W, -shift); count [P]:
    the rays that count; shifts [P]: the planes (Detector.shiftByDistance's sign); hew [P]: twice the 0.5 radius, None
    when 0.5 is not among the fractions; best_focus: the shift with the smallest first radius (None without any);
    quantiles: the integers behind it all (Quantiles)."""

    def __init__(self, quantiles, centres, shifts, metric, radii=None):
        q = self.quantiles = quantiles
        self.metric = metric
        self.radii, self.fractions = q.values, q.fractions
        self.Radii = None if radii is None else np.asarray(radii, dtype=np.float64)
        W = q.total.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            self.enclosed = None if q.rank_sums is None else q.rank_sums / W
        centres = np.asarray(centres, dtype=np.float64).reshape(-1, 4)
        self.centre = centres[:, 0:2].copy()
        self.delay_centre, self.path_centre = centres[:, 2].copy(), centres[:, 3].copy()
        self.power, self.count = q.weight, q.count
        self.shifts = np.asarray(shifts, dtype=np.float64)
        half = [k for k, f in enumerate(self.fractions) if f == 0.5]
        self.hew = 2.0 * self.radii[:, half[0]] if half else None
        first = self.radii[:, 0]
        self.best_focus = None if np.isnan(first).all() else float(self.shifts[int(np.nanargmin(first))])


def _desc(key, planes, fractions, shift, scratch_bound):
    d = _abi.ArtQuantileDesc()
    d.key, d.planes, d.n_fractions, d.wshift = key, planes, len(fractions), int(shift)
    d.scratch_bound = int(scratch_bound or 0)
    for k, f in enumerate(fractions):
        d.fraction[k] = f
    return d


def _host(out):
    """The device results of HipBackend.quantiles as host arrays: (values, below, upto, totals, rank_sums, rank_counts,
    centres)."""
    g = lambda k: None if out[k] is None else out[k].cpu().numpy()
    return g("values"), g("below"), g("upto"), g("totals"), g("rank_sums"), g("rank_counts"), g("centres")


def weighted_quantiles(values, Fractions, rays=None, Weights=None, Thresholds=None, ScratchBound=None):
    """Quantiles (Quantiles) of any per-ray device tensor `values`, [n] or [P, n] (P planes with keys of their own), at
    `Fractions`.  `rays` (a RayBundle or ray list) supplies which slots are alive and, unless Weights ([n], device) is
    given, the intensities as weights; without either every slot counts with weight 1.  Thresholds ([R] or [P, R], sorted)
    asks for the rank sums as well.  ScratchBound (doubles) bounds the device scratch: planes are then processed in
    blocks, which never changes a result."""
    import torch
    from .bundle import RayBundle
    f = _fractions(Fractions)
    if values.dim() not in (1, 2):
        raise ValueError("values must be a tensor [n] or [P, n]")
    keys = values.reshape(1, -1) if values.dim() == 1 else values
    P, n = int(keys.shape[0]), int(keys.shape[1])
    if not 1 <= P <= _abi.ART_FOCAL_MAX_PLANES:
        raise ValueError(f"1 to {_abi.ART_FOCAL_MAX_PLANES} planes of keys per call")
    if keys.dtype != torch.float64:
        raise ValueError("values must be float64")
    th = _thresholds(Thresholds, P)
    B = None if rays is None else RayBundle.of(rays)
    w = Weights if Weights is not None else (None if B is None else B.intensity)
    if B is not None and B.n_slots != n:
        raise ValueError("values and rays differ in their number of slots")
    if w is not None and int(w.numel()) < n:
        raise ValueError("Weights must hold one weight per slot")
    shift = _shift_from(n, _weight_range(None if w is None else w[:n]))
    from . import _lib
    be = B.backend if B is not None else _lib.get_backend()
    keys = keys.contiguous()
    d = _desc(_abi.ART_QKEY_GIVEN, P, f, shift, ScratchBound)
    d.keys = keys.data_ptr() if n else None
    d.alive = B.alive.data_ptr() if (B is not None and n) else None
    v, below, upto, totals, rs, rc, _ = _host(be.quantiles(d, None, w, n, th))
    return Quantiles(v, below, upto, totals, shift, f, th, rs, rc)


def _resolve(det, RayList, Fractions, Radii, Metric, Centre, Shifts):
    """The arguments of get_EncircledEnergy, checked before the device is touched."""
    from .bundle import RayBundle
    if Metric not in _METRICS:
        raise ValueError('Metric: one of "radius", "X", "Y", "Delay"')
    f = _fractions(Fractions)
    shifts = [0.0] if Shifts is None else [float(s) for s in np.atleast_1d(np.asarray(Shifts, dtype=float))]
    if not 1 <= len(shifts) <= _abi.ART_FOCAL_MAX_PLANES or not all(math.isfinite(s) for s in shifts):
        raise ValueError(f"Shifts must be 1 to {_abi.ART_FOCAL_MAX_PLANES} finite distances")
    P = len(shifts)
    th = _thresholds(Radii, P, "Radii", non_negative=True)
    centre = None
    if Centre is not None:
        c = np.asarray(Centre, dtype=np.float64)
        centre = np.zeros((P, 3))
        if Metric == "Delay":
            if c.ndim > 1 or (c.ndim == 1 and c.shape[0] != P):
                raise ValueError('Centre of the "Delay" metric: one delay (fs), or one per plane')
            centre[:, 2] = c
        else:
            if c.shape not in ((2,), (P, 2)):
                raise ValueError("Centre must be two detector coordinates (X, Y), or one pair per plane")
            centre[:, 0:2] = c
        if not np.isfinite(centre).all():
            raise ValueError("Centre must be finite")
    det._iscomplete()
    return RayBundle.of(RayList), f, shifts, th, centre


def encircled_energies(jobs):
    """jobs: [(rays, detector, kwargs)], rays a bundle, a ray list or an OpticalChain (its last bundle), kwargs those of
    Detector.get_EncircledEnergy.  One EncircledEnergy per job, in order: the weights' ranges are read back together, then
    every job is enqueued, then the results are read back."""
    import torch
    items = []
    for rays, det, kw in jobs:
        kw = dict(kw or {})
        unknown = set(kw) - {"Fractions", "Radii", "Metric", "Centre", "Shifts"}
        if unknown:
            raise TypeError(f"unknown arguments {sorted(unknown)}")
        if hasattr(rays, "get_output_rays"):
            rays = rays.get_output_rays()[-1]
        metric = kw.get("Metric", "radius")
        B, f, shifts, th, centre = _resolve(det, rays, kw.get("Fractions", (0.5, 0.8, 0.9)), kw.get("Radii"), metric,
                                            kw.get("Centre"), kw.get("Shifts"))
        items.append((B, det, f, shifts, th, centre, metric))
    ranges = [_weight_range(None if it[0].intensity is None else it[0].intensity[:it[0].n_slots]) for it in items]
    some = [r for r in ranges if r is not None]
    host = iter(torch.stack(some).cpu().numpy() if some else ())
    shifts_w = [_shift_from(it[0].n_slots, None if r is None else next(host)) for it, r in zip(items, ranges)]
    pending = []
    for (B, det, f, shifts, th, centre, metric), S in zip(items, shifts_w):
        d = _desc(_METRICS[metric], len(shifts), f, S, None)
        d.det = det._desc()
        for p, v in enumerate(shifts):
            d.shift[p] = -v                  # shiftByDistance(v) moves the plane to centre - v * normal
        if centre is not None:
            d.centre_given = 1
            for p in range(len(shifts)):
                d.centre[p][:] = [float(c) for c in centre[p]]
        pending.append(B.backend.quantiles(d, B.view(), B.intensity, B.n_slots, th))
    results = []
    for (B, det, f, shifts, th, centre, metric), S, out in zip(items, shifts_w, pending):
        v, below, upto, totals, rs, rc, centres = _host(out)
        q = Quantiles(v, below, upto, totals, S, f, th, rs, rc)
        results.append(EncircledEnergy(q, centres, shifts, metric, None if th is None else th[0]))
    return results


def encircled_energy(det, RayList, Fractions=(0.5, 0.8, 0.9), Radii=None, Metric="radius", Centre=None, Shifts=None):
    """Detector.get_EncircledEnergy (see the module's docstring and EncircledEnergy)."""
    return encircled_energies([(RayList, det, dict(Fractions=Fractions, Radii=Radii, Metric=Metric, Centre=Centre,
                                                   Shifts=Shifts))])[0]

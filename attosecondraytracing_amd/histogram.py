"""Histograms of ALL rays of a bundle, binned on the device (art_hip.h, art_histogram): spot images and delay profiles
on a detector (Detector.get_Histogram), footprints on an optic (OpticalChain.get_Footprint).

Bins follow numpy.histogramdd with edges numpy.linspace(lo, hi, bins + 1).  Counts are exact integers.  Intensities are
summed in fixed point, q = rint(ldexp(w, S)) as int64, so the sums are the same bytes on every run and add exactly
across calls; S is chosen so that no sum can overflow, and each ray's weight is off by at most 2^-(S+1), a bin of n rays
by at most n * 2^-(S+1)."""
import math

import numpy as np

from . import _abi
from .bundle import RayBundle

_DETECTOR_AXES = {"X": _abi.ART_HAXIS_X, "Y": _abi.ART_HAXIS_Y, "Delay": _abi.ART_HAXIS_DELAY}


class Histogram:
    """counts: int64 array of shape `bins` (axis 0 slowest); intensity: float64 ldexp(wsums, -shift), or None when the
    rays carry no intensity; edges: one numpy.linspace array per axis; outside: (alive rays outside the range, their
    intensity or None); shift: S of the fixed-point weights; wsums / totals: the integers the device summed (wsums None
    without intensity; totals = [binned rays, outside rays, sum q binned, sum q outside])."""

    def __init__(self, counts, wsums, totals, edges, shift):
        self.counts = counts
        self.wsums = wsums
        self.totals = totals
        self.edges = edges
        self.shift = shift
        self.intensity = None if wsums is None else np.ldexp(wsums.astype(np.float64), -shift)
        self.outside = (int(totals[1]), None if wsums is None else float(np.ldexp(float(totals[3]), -shift)))


def shift_for(n_total, wmax):
    """S = 62 - ceil(log2(n_total + 1)) - E with wmax < 2^E: n_total weights of magnitude <= wmax sum to less than
    2^62 in units of 2^-S (clamped to the ABI's [-1074, 1074])."""
    E = math.frexp(wmax)[1] if wmax > 0 else -1074
    return max(-1074, min(1074, 62 - int(n_total).bit_length() - E))


def weight_shift(n_total, w):
    """The shift for binning n_total rays with weights `w` (a tensor, or None): one torch.amax, read back."""
    if w is None:
        return 0
    import torch
    wmax = float(torch.amax(torch.abs(w))) if w.numel() else 0.0
    if not math.isfinite(wmax):
        raise ValueError("the rays' intensities must be finite to be binned")
    return shift_for(n_total, wmax)


def per_axis_bins(Bins, ndim):
    b = [int(Bins)] * ndim if np.isscalar(Bins) else [int(v) for v in Bins]
    if len(b) != ndim or min(b) < 1:
        raise ValueError("Bins must be a positive int or one positive int per axis")
    return b


def resolve_range(lo, hi):
    """numpy's rule for a range: lo == hi is widened by 0.5 on either side."""
    lo, hi = float(lo), float(hi)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError("a range must be finite with lo <= hi")
    return (lo - 0.5, hi + 0.5) if lo == hi else (lo, hi)


def per_axis_ranges(Range, ndim, default):
    if Range is None:
        return [resolve_range(*default(k)) for k in range(ndim)]
    Range = list(Range)
    if len(Range) != ndim:
        raise ValueError("Range must be None or one (lo, hi) per axis")
    return [resolve_range(*r) for r in Range]


def bin_bundle(B, desc, axes, bins, ranges):
    """Fill desc's axes, bins and ranges, bin the bundle on its backend, read the result back."""
    desc.ndim = len(axes)
    for k, (ax, nb, (lo, hi)) in enumerate(zip(axes, bins, ranges)):
        desc.axis[k], desc.bins[k], desc.lo[k], desc.hi[k] = ax, nb, lo, hi
    counts, wsums, totals, shift = B.backend.histogram(desc, B.view(), B.intensity, B.n_slots)
    return Histogram(counts.cpu().numpy().reshape(bins), None if wsums is None else wsums.cpu().numpy().reshape(bins),
                     totals.cpu().numpy(), [np.linspace(lo, hi, nb + 1) for nb, (lo, hi) in zip(bins, ranges)], shift)


def detector_histogram(det, RayList, Axes=("X", "Y"), Bins=100, Range=None):
    """Detector.get_Histogram: the alive rays binned on `det` by the axes "X", "Y" (detector-plane coordinates, as
    get_PointList2D) and "Delay" (fs, as get_Delays: centred on the mean path).  The default range of an axis is its
    min..max over the alive rays."""
    from .ModuleDetector import LightSpeed
    Axes = (Axes,) if isinstance(Axes, str) else tuple(Axes)
    if not 1 <= len(Axes) <= 3 or any(a not in _DETECTOR_AXES for a in Axes):
        raise ValueError('Axes: one to three of "X", "Y", "Delay"')
    B = RayBundle.of(RayList)
    s = det.readout(B, store=False, lite=True)["stats"]
    centre = s[1] / s[0] if s[0] > 0 else 0.0
    lims = {"X": (s[2], s[3]), "Y": (s[4], s[5]),
            "Delay": ((s[12] - centre) / LightSpeed * 1e15, (s[13] - centre) / LightSpeed * 1e15)}
    default = lambda k: lims[Axes[k]] if s[0] > 0 else (0.0, 1.0)       # (numpy's range of no values)
    ranges = per_axis_ranges(Range, len(Axes), default)
    desc = _abi.ArtHistogramDesc()
    desc.source = _abi.ART_HIST_DETECTOR
    desc.map = det._desc()
    desc.delay_centre = float(centre)
    return bin_bundle(B, desc, [_DETECTOR_AXES[a] for a in Axes], per_axis_bins(Bins, len(Axes)), ranges)


def spectrometer_histogram(det, bundles, Bins=200, Range=None):
    """ModuleAnalysisAndPlots.SpectrometerImage: the X-Y spot histograms of several bundles (one per wavelength,
    OpticalChain.get_SpectralRays) on one detector, SUMMED on the device -- art_histogram with accumulate = 1 into the
    first bundle's bins, one fixed-point shift for all of them, so the sum is exact.  Range defaults to the joint
    bounding box of the alive rays."""
    import torch
    Bs = [RayBundle.of(b) for b in bundles]
    if not Bs:
        raise ValueError("no bundle to bin")
    stats = [det.readout(B, store=False, lite=True)["stats"] for B in Bs]
    live = [s for s in stats if s[0] > 0]
    lims = [(min(s[2 + 2 * k] for s in live), max(s[3 + 2 * k] for s in live)) for k in range(2)] if live else [(0.0, 1.0)] * 2
    ranges = per_axis_ranges(Range, 2, lambda k: lims[k])
    bins = per_axis_bins(Bins, 2)
    desc = _abi.ArtHistogramDesc()
    desc.source = _abi.ART_HIST_DETECTOR
    desc.map = det._desc()
    desc.ndim = 2
    for k, (nb, (lo, hi)) in enumerate(zip(bins, ranges)):
        desc.axis[k], desc.bins[k], desc.lo[k], desc.hi[k] = k, nb, lo, hi
    weighted = all(B.intensity is not None for B in Bs)
    shift = 0
    if weighted:
        wmax = max((float(torch.amax(torch.abs(B.intensity))) if B.intensity.numel() else 0.0) for B in Bs)
        if not math.isfinite(wmax):
            raise ValueError("the rays' intensities must be finite to be binned")
        shift = shift_for(sum(B.n_slots for B in Bs), wmax)
    out = None
    for B in Bs:
        counts, wsums, totals, _ = B.backend.histogram(desc, B.view(), B.intensity if weighted else None, B.n_slots,
                                                       out=out, shift=shift)
        out = (counts, wsums, totals)
    return Histogram(counts.cpu().numpy().reshape(bins), None if wsums is None else wsums.cpu().numpy().reshape(bins),
                     totals.cpu().numpy(), [np.linspace(lo, hi, nb + 1) for nb, (lo, hi) in zip(bins, ranges)], shift)


def footprint(oe, RayList, Bins=100, Range=None):
    """OpticalChain.get_Footprint: the hit points on optical element `oe` in its support frame, fwd (P - position)
    (MirrorProjection's coordinates), binned over +-_CircumRect()/2 by default."""
    from . import ModuleGeometry as mgeo
    B = RayBundle.of(RayList)
    half = np.asarray(oe.type.support._CircumRect(), dtype=float) / 2
    ranges = per_axis_ranges(Range, 2, lambda k: (-half[k], half[k]))
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    desc = _abi.ArtHistogramDesc()
    desc.source = _abi.ART_HIST_FRAME
    desc.map.rot[:] = [float(v) for v in np.asarray(fwd, dtype=float).reshape(9)]
    desc.map.centre[:] = [float(v) for v in np.asarray(oe.position, dtype=float)]
    return bin_bundle(B, desc, [0, 1], per_axis_bins(Bins, 2), ranges)

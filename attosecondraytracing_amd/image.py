"""Partially coherent focal images of extended sources, summed on the device (art_hip.h, art_focal_image):
Detector.get_FocalImage, OpticalChain.get_FocalImage.

The rays of an ExtendedSource bundle come from mutually incoherent point sources.  Rays of one point source interfere,
rays of different point sources do not, so the image is the sum over the point sources of the intensities of their
coherent focal fields (focal.py's model inside a group):

    I_q(X, Y) = sum_g | sum_{r in g} sqrt(w_r) exp(i k [(path_r - RefPath) + d_r . (x - p_r)]) |^2

Slot i of every bundle of a chain is source ray i and ExtendedSource numbers its rays as point source index * rays per
point source + index in the cone, so the groups are contiguous ranges of slots: the device gets their offsets (`seg`,
built on the device, never read back) and sums every group's field and the groups' intensities in one call.

Limits of the model: focal.py's inside a group; the point sources are fully incoherent with each other and
monochromatic (no partially coherent pulses, no coatings)."""
import numpy as np

from . import focal
from .bundle import RayBundle


class FocalImage:
    """intensity: device float64 [P, ny, nx] (plane, row = Y, column = X); x, y, shifts, wavelength, ref_path: as in
    focal.FocalField; groups: the number of mutually incoherent groups; power: sum of w over the alive rays;
    ideal_peak: sum over the groups of (sum of sqrt(w) over the group's alive rays)^2, the peak if every group focused
    perfectly at one pixel; strehl [P]: peak intensity / ideal_peak (at most 1; NaN without alive rays); peak [P, 2]:
    (x, y) of each plane's brightest pixel; rms [P, 2]: the intensity-weighted standard deviations of x and y over the
    grid (NaN for a plane without intensity)."""

    def __init__(self, intensity, x, y, shifts, wavelength, ref_path, groups, power, ideal_peak):
        self.intensity = intensity
        self.x, self.y = x, y
        self.shifts = np.asarray(shifts, dtype=float)
        self.wavelength = float(wavelength)
        self.ref_path = float(ref_path)
        self.groups = int(groups)
        self.power = float(power)
        self.ideal_peak = float(ideal_peak)
        self.strehl, self.peak, self.rms = image_metrics(intensity.cpu().numpy(), x, y, self.ideal_peak)


def image_metrics(intensity, x, y, ideal_peak):
    """(strehl [P], peak [P, 2], rms [P, 2]) of intensity [P, ny, nx] (see FocalImage)."""
    P = intensity.shape[0]
    peak_value, peak = focal.strehl_and_peak(intensity, x, y, 1.0 if ideal_peak > 0 else 0.0)
    strehl = peak_value / ideal_peak if ideal_peak > 0 else np.full(P, np.nan)
    x, y = np.asarray(x, float), np.asarray(y, float)
    rms = np.full((P, 2), np.nan)
    for q in range(P):
        total = intensity[q].sum()
        if not total > 0:
            continue
        for c, (axis, marginal) in enumerate(((x, intensity[q].sum(axis=0)), (y, intensity[q].sum(axis=1)))):
            mean = (marginal * axis).sum() / total
            rms[q, c] = np.sqrt(max((marginal * (axis - mean) ** 2).sum() / total, 0.0))
    return strehl, peak, rms


def segments(B, RaysPerSource=None, Groups=None):
    """(seg, groups): the device int64 tensor of groups + 1 slot offsets of bundle B's mutually incoherent groups, group
    g = slots [seg[g], seg[g + 1]), and their number.  Exactly one of RaysPerSource (the group of a slot is its ray
    number // RaysPerSource; the number is the slot index when B.number is None) and Groups (one integer id per slot).
    The ids must not decrease over the slots -- groups are contiguous ranges; ids that occur in no slot are skipped."""
    import torch
    if (RaysPerSource is None) == (Groups is None):
        raise ValueError("give exactly one of RaysPerSource and Groups")
    n, dev = B.n_slots, B.alive.device
    if RaysPerSource is not None:
        per = int(RaysPerSource)
        if per != RaysPerSource or per < 1:
            raise ValueError("RaysPerSource must be a positive integer")
        if B.number is None:
            groups = (n + per - 1) // per
            return torch.clamp(torch.arange(groups + 1, dtype=torch.int64, device=dev) * per, max=n), groups
        ids = torch.div(B.number[:n], per, rounding_mode="floor")
    else:
        ids = torch.as_tensor(np.asarray(Groups) if not isinstance(Groups, torch.Tensor) else Groups)
        if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.shape != (n,):
            raise ValueError("Groups must be one integer id per slot")
        ids = ids.to(device=dev, dtype=torch.int64)
    if n == 0:
        return torch.zeros(1, dtype=torch.int64, device=dev), 0
    if bool((ids[1:] < ids[:-1]).any()):
        raise ValueError("the group ids must be non-decreasing over the slots: the groups must be contiguous slot ranges")
    _, counts = torch.unique_consecutive(ids, return_counts=True)
    seg = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=seg[1:])
    return seg, int(counts.numel())


def group_sums(B, seg):
    """(power, ideal_peak): sum of w over the alive slots, and sum over the groups of (sum of sqrt(w) over the group's
    alive slots)^2 (w = 1 without intensities)."""
    import torch
    n = B.n_slots
    alive = B.alive[:n] != 0
    if B.intensity is None:
        w = amp = alive.to(torch.float64)
    else:
        w = torch.where(alive, B.intensity[:n], 0.0)
        amp = torch.sqrt(w)
    run = torch.zeros(n + 1, dtype=torch.float64, device=alive.device)
    torch.cumsum(amp, 0, out=run[1:])
    lo, hi = seg[:-1], torch.maximum(seg[1:], seg[:-1])
    A = run[hi] - run[lo]
    return float(w.sum()), float((A * A).sum())


def focal_image(det, RayList, RaysPerSource=None, Groups=None, Size=None, Pixels=128, Centre=None, Shifts=None,
                Wavelength=None, RefPath=None):
    """Detector.get_FocalImage (see the module's docstring).  The grid, Centre, Size, Shifts, Wavelength and RefPath
    resolve as in focal.focal_field; the groups as in segments.  All groups and planes are summed in one device call."""
    import torch
    B = RayBundle.of(RayList)
    seg, groups = segments(B, RaysPerSource, Groups)
    fd, x, y, shifts, wavelength, ref, _ = focal.focal_desc(det, B, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
    if groups == 0:                 # no slot: one empty group for the device
        seg = torch.zeros(2, dtype=torch.int64, device=B.alive.device)
    view, _keep = B.phase_path_view(wavelength)          # (behind a grating: path + wavelength * grooves)
    intensity = B.backend.focal_image(fd, seg, max(groups, 1), view, B.intensity, B.n_slots)
    power, ideal = group_sums(B, seg)
    return FocalImage(intensity, x, y, shifts, wavelength, ref, groups, power, ideal)

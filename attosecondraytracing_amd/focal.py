"""Coherent focal fields, summed on the device (art_hip.h, art_focal_field): Detector.get_FocalField.

Every alive ray is taken as a local plane wave of amplitude sqrt(w) (w = the bundle's intensity, or 1) and phase k times
its optical path, and the waves are summed on a pixel grid in the detector plane and in planes shifted along the
detector's axis (the Debye / angular-spectrum picture):

    E_q(X, Y) = sum_r sqrt(w_r) exp(i k [(path_r - RefPath) + d_r . (x - p_r)]),   x = the pixel's point in space

At a ray's own hit point the phase is k (opl_r - RefPath), opl_r the value behind Detector.get_Delays.

Limits of the model: each ray stands for an equal share of the beam's solid angle, scaled by w (true to O(NA^2) for the
Vogel-spiral sources at the numerical apertures of the shipped configurations, not for arbitrary ray sets); all rays
are summed as mutually coherent, which is wrong for ExtendedSource bundles (partial coherence: image.py,
Detector.get_FocalImage)."""
import math

import numpy as np

from . import _abi
from . import ModuleProcessing as mp
from .bundle import RayBundle


class FocalField:
    """field: device complex128 [P, ny, nx] (plane, row = Y, column = X); intensity: numpy |field|^2; x, y: the pixel
    centres (mm, detector coordinates, as get_PointList2D); shifts: the planes' distances along the detector axis
    (Detector.shiftByDistance's sign: positive = away from the optic); strehl [P]: peak intensity / amplitude_sum^2
    (NaN without alive rays); peak [P, 2]: (x, y) of each plane's brightest pixel (NaN without alive rays);
    wavelength (mm); ref_path: the optical path of phase 0; amplitude_sum: sum of sqrt(w) over the alive rays."""

    def __init__(self, field, x, y, shifts, wavelength, ref_path, amplitude_sum):
        self.field = field
        self.intensity = np.abs(field.cpu().numpy()) ** 2
        self.x, self.y = x, y
        self.shifts = np.asarray(shifts, dtype=float)
        self.wavelength = float(wavelength)
        self.ref_path = float(ref_path)
        self.amplitude_sum = float(amplitude_sum)
        self.strehl, self.peak = strehl_and_peak(self.intensity, x, y, self.amplitude_sum)


def strehl_and_peak(intensity, x, y, amplitude_sum):
    """Per plane of intensity [P, ny, nx]: max / amplitude_sum^2 and the (x, y) of the first brightest pixel; NaN for
    both when amplitude_sum is 0 (no alive ray)."""
    P = intensity.shape[0]
    flat = intensity.reshape(P, -1)
    if not amplitude_sum > 0:
        return np.full(P, np.nan), np.full((P, 2), np.nan)
    idx = np.argmax(flat, axis=1)
    strehl = flat[np.arange(P), idx] / amplitude_sum ** 2
    l, j = np.unravel_index(idx, intensity.shape[1:])
    return strehl, np.stack([np.asarray(x)[j], np.asarray(y)[l]], axis=1)


def _per_axis(v, name, cast):
    vals = [v, v] if np.isscalar(v) else list(v)
    if len(vals) != 2:
        raise ValueError(f"{name} must be a scalar or one value per axis")
    return [cast(a) for a in vals]


def pixel_axis(centre, size, pixels):
    """(x0, dx, centres): Centre + linspace(-Size/2, Size/2, Pixels), formed as x0 + j * dx as the device does."""
    x0 = float(centre) - 0.5 * size
    dx = size / (pixels - 1) if pixels > 1 else 0.0
    return x0, dx, x0 + np.arange(pixels) * dx


def resolve_grid(Size, Pixels, Centre, Shifts, wavelength, NA, bbox_centre):
    """The arguments of get_FocalField, resolved: (pixels (nx, ny), sizes (sx, sy), centre (cx, cy), shifts).  NA is a
    callable (evaluated only when Size is None); bbox_centre: the alive rays' bounding-box centre or None."""
    if wavelength is None or not (math.isfinite(wavelength) and wavelength > 0):
        raise ValueError("a focal field needs a finite positive wavelength: the bundle has none, pass Wavelength=")
    pix = _per_axis(Pixels, "Pixels", lambda p: int(p) if float(p) == int(p) else -1)
    if min(pix) < 1 or max(pix) > _abi.ART_FOCAL_MAX_PIXELS:
        raise ValueError(f"Pixels must be integers in [1, {_abi.ART_FOCAL_MAX_PIXELS}]")
    if Size is None:
        airy = mp.ReturnAiryRadius(wavelength, NA())
        if not airy > 0:
            raise ValueError("the numerical aperture is too small for a default Size (16 Airy radii): pass Size=")
        Size = 16 * airy
    sizes = _per_axis(Size, "Size", float)
    if not all(math.isfinite(s) and s > 0 for s in sizes):
        raise ValueError("Size must be finite and positive")
    if Centre is None:
        if bbox_centre is None:
            raise ValueError("no alive ray to centre the grid on: pass Centre=")
        Centre = bbox_centre
    centre = [float(c) for c in Centre]
    if len(centre) != 2 or not all(math.isfinite(c) for c in centre):
        raise ValueError("Centre must be two finite detector coordinates (X, Y)")
    shifts = [0.0] if Shifts is None else [float(s) for s in np.atleast_1d(np.asarray(Shifts, dtype=float))]
    if not 1 <= len(shifts) <= _abi.ART_FOCAL_MAX_PLANES or not all(math.isfinite(s) for s in shifts):
        raise ValueError(f"Shifts must be 1 to {_abi.ART_FOCAL_MAX_PLANES} finite distances")
    return pix, sizes, centre, shifts


def amplitude_sum(B):
    """sum of sqrt(w) over the alive slots (w = 1 without intensities)."""
    import torch
    alive = B.alive[:B.n_slots] != 0
    if B.intensity is None:
        return float(alive.sum())
    return float(torch.where(alive, torch.sqrt(torch.where(alive, B.intensity, 0.0)), 0.0).sum())


def focal_desc(det, B, Size, Pixels, Centre, Shifts, Wavelength, RefPath):
    """get_FocalField's arguments resolved for bundle B on det (see focal_field): (ArtFocalDesc, x, y, shifts, wavelength,
    ref_path, stats), stats the lite read-out's statistics."""
    wavelength = B.wavelength if Wavelength is None else float(Wavelength)
    s = det.readout(B, store=False, lite=True)["stats"]
    alive = s[0] > 0
    bbox = (0.5 * (s[2] + s[3]), 0.5 * (s[4] + s[5])) if alive else None
    pix, sizes, centre, shifts = resolve_grid(Size, Pixels, Centre, Shifts, wavelength,
                                              lambda: mp.ReturnNumericalAperture(B, 1) if alive else 0.0, bbox)
    # (behind a grating the phase path is path + wavelength * grooves: bundle.RayBundle.phase_path_view)
    ref = ((s[1] / s[0] if alive else 0.0) + B.phase_ref_offset(wavelength)) if RefPath is None else float(RefPath)
    x0, dx, x = pixel_axis(centre[0], sizes[0], pix[0])
    y0, dy, y = pixel_axis(centre[1], sizes[1], pix[1])
    fd = _abi.ArtFocalDesc()
    fd.det = det._desc()
    fd.k = 2 * math.pi / wavelength
    fd.L_ref = ref
    fd.x0, fd.dx, fd.nx = x0, dx, pix[0]
    fd.y0, fd.dy, fd.ny = y0, dy, pix[1]
    fd.planes = len(shifts)
    for q, v in enumerate(shifts):
        fd.shift[q] = -v          # shiftByDistance(v) moves the plane to centre - v * normal
    return fd, x, y, shifts, wavelength, ref, s


def focal_field(det, RayList, Size=None, Pixels=128, Centre=None, Shifts=None, Wavelength=None, RefPath=None):
    """Detector.get_FocalField (see the module's docstring).  Pixel centres: Centre + linspace(-Size/2, Size/2, Pixels)
    per axis (Size, Pixels scalars or one per axis); Centre defaults to the alive rays' bounding-box centre
    (get_PointList2DCentre's), Size to 16 Airy radii (ReturnAiryRadius(wavelength, ReturnNumericalAperture)), Shifts to
    (0,), Wavelength to the bundle's, RefPath to the mean optical path of the alive rays (what get_Delays subtracts).
    All planes are summed in one device call."""
    B = RayBundle.of(RayList)
    fd, x, y, shifts, wavelength, ref, _ = focal_desc(det, B, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
    view, _keep = B.phase_path_view(wavelength)
    field = B.backend.focal_field(fd, view, B.intensity, B.n_slots)
    return FocalField(field, x, y, shifts, wavelength, ref, amplitude_sum(B))

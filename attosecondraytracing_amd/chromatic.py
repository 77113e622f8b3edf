"""Pulses at focus from chromatic sources, summed on the device (art_hip.h, art_focal_chromatic):
Detector.get_ChromaticFocalPulse, OpticalChain.get_ChromaticFocalPulse.

pulse.py takes the source as achromatic: one traced bundle serves every frequency and only k (optical path) changes.  A
high-harmonic source is not: every harmonic leaves the medium with its own divergence and its own apparent source
position along the axis.  Here every frequency omega_j of the pulse gets, per ray r,

    an amplitude factor  exp(-u_r c_j),   c_j = 2 / Theta_j^2     (a Gaussian beam, intensity 1/e^2 at half-angle Theta_j)
    a phase              k_j z_j u_r                             (a spherical wave centred at S + z_j a, not at S)

with u_r = 1 - cos(angle between the ray's SOURCE direction and the axis a), Theta_j = Divergence(omega_j) and
z_j = Position(omega_j) (mm, positive downstream).  All frequencies and planes are summed in one device call; the
frequency grid, the weights g_j and the Fourier sum are pulse.py's.

Limits of the model: the rays are not re-traced, so it is first order in z_j over the distance to the first optic;
there is one axis for all frequencies; the apodisation is Gaussian only; chains with gratings are refused.
Detector.get_ChromaticFocalPulse sums the scalar field; OpticalChain.get_ChromaticFocalPulse(..., Coatings=, Polarisation=)
sums the vector field behind the chain's coatings (art_focal_vector_chromatic, vector_chromatic_focal_pulse below): per
ray and frequency the amplitude above times the field vector_pulse.py carries through the mirrors, so the pulse train
at focus has both what the source and what the coatings do to every harmonic."""
import math

import numpy as np

from . import _abi
from . import focal
from . import pulse
from . import vector_pulse
from .bundle import RayBundle

C_MM_PER_FS = pulse.C_MM_PER_FS
COMB_HALF_WIDTHS = 3.0       # harmonic_comb: a line is exactly 0 beyond this many line widths (FWHM) from its centre
SUM_BLOCK_ELEMENTS = 1 << 24   # amplitude_sum: slots x frequencies held on the device at once


def line_width(LineDeltaFT):
    """The spectral intensity FWHM (rad/fs) of a transform-limited Gaussian line of duration LineDeltaFT (fs)."""
    return 4 * math.log(2) / LineDeltaFT


def harmonic_comb(FundamentalWavelength, Orders, LineDeltaFT, Amplitudes=None, Phases=None):
    """A Spectrum= callable omega (rad/fs, array) -> complex amplitude for a comb of harmonics: line q of Orders sits at
    q * omega_1 (omega_1 = 2 pi c / FundamentalWavelength, mm), a Gaussian of Fourier-limited duration LineDeltaFT (fs,
    intensity FWHM) with amplitude Amplitudes[q] (default 1) and phase Phases[q] (rad, default 0).  A line is exactly 0
    further than 3 line widths (line_width(LineDeltaFT)) from its centre, so the frequencies between the lines carry
    no weight and cost nothing in get_ChromaticFocalPulse."""
    w1 = 2 * math.pi * C_MM_PER_FS / pulse._positive(FundamentalWavelength, "FundamentalWavelength")
    tau = pulse._positive(LineDeltaFT, "LineDeltaFT")
    orders = np.atleast_1d(np.asarray(Orders, dtype=float))
    if orders.ndim != 1 or len(orders) < 1 or not (np.isfinite(orders).all() and (orders > 0).all()):
        raise ValueError("Orders must be one or more finite positive harmonic orders")
    amps = np.ones(len(orders)) if Amplitudes is None else np.atleast_1d(np.asarray(Amplitudes, dtype=float))
    phases = np.zeros(len(orders)) if Phases is None else np.atleast_1d(np.asarray(Phases, dtype=float))
    if amps.shape != orders.shape or phases.shape != orders.shape or not (np.isfinite(amps).all() and np.isfinite(phases).all()):
        raise ValueError("Amplitudes and Phases must hold one finite value per order")
    coef = amps * np.exp(1j * phases)
    cut = COMB_HALF_WIDTHS * line_width(tau)

    def spectrum(omega):
        omega = np.asarray(omega, dtype=float)
        out = np.zeros(omega.shape, dtype=complex)
        for q, a in zip(orders, coef):
            near = np.abs(omega - q * w1) <= cut
            out[near] += a * pulse.gaussian_spectrum(omega[near], q * w1, tau)
        return out

    return spectrum


def gaussian_divergence(Waist):
    """A Divergence= callable omega -> Theta (rad): the far-field 1/e^2 half-angle lambda / (pi w0) = 2 c / (omega w0)
    of a Gaussian beam whose waist radius w0 (mm) is Waist, a scalar or a callable omega -> w0."""
    if not callable(Waist):
        w0 = pulse._positive(Waist, "Waist")

    def divergence(omega):
        omega = np.asarray(omega, dtype=float)
        return 2 * C_MM_PER_FS / (omega * (np.asarray(Waist(omega), dtype=float) if callable(Waist) else w0))

    return divergence


class _ChromaticSource:
    """What a chromatic source adds to a pulse: divergence, position, axis, best_focus (see ChromaticFocalPulse)."""

    def __init__(self, divergence, position, axis, best_focus, *args):
        super().__init__(*args)
        self.divergence, self.position = np.asarray(divergence, dtype=float), np.asarray(position, dtype=float)
        self.axis, self.best_focus = np.asarray(axis, dtype=float), np.asarray(best_focus, dtype=float)


class ChromaticFocalPulse(_ChromaticSource, pulse.FocalPulse):
    """pulse.FocalPulse of a chromatic source, and: divergence [J] (Theta_j, rad; inf without apodisation), position [J]
    (z_j, mm), axis (the unit axis a), best_focus [J] (the value of Shifts with the largest |E_j| at the pixel nearest
    the grid's centre; NaN for a frequency of weight 0 and without alive rays).  amplitude_sum is the ideal peak of the
    same apodised source, sum_j |g_j| S_j / sum_j |g_j| with S_j = sum over the alive rays of sqrt(w_r) exp(-u_r c_j), so
    `strehl` stays "against a perfect focus of this source".  The slices of `spectrum` at frequencies of weight 0 are 0."""


def _per_frequency(f, omega, name, positive):
    """f(omega) validated as one finite (positive) value per frequency."""
    v = np.asarray(f(omega.copy()), dtype=float)
    if v.shape != omega.shape or not np.isfinite(v).all() or (positive and not (v > 0).all()):
        raise ValueError(f"{name} must return {len(omega)} finite{' positive' if positive else ''} values for the "
                         f"{len(omega)} frequencies")
    return v


def source_u(S, axis, alive):
    """u_r = 1 - cos(angle between slot r's direction in the source bundle S and the unit axis), formed as the device
    forms it; 0 in slots that are not `alive`.  Device tensor [n_slots]."""
    import torch
    n = S.n_slots
    d = S.data[3:6, :n]
    sx, sy, sz = d[0] - axis[0], d[1] - axis[1], d[2] - axis[2]
    return torch.where(alive, 0.5 * ((sx * sx + sy * sy) + sz * sz), 0.0)


def apodised_amplitude_sums(B, u, c):
    """S_j = sum over the alive slots of sqrt(w_r) exp(-u_r c_j) for every c_j of c: numpy [len(c)].  Summed on the
    device in blocks of frequencies, so that no slots x frequencies array is ever held at once."""
    import torch
    n = B.n_slots
    alive = B.alive[:n] != 0
    amp = alive.to(torch.float64) if B.intensity is None else \
        torch.where(alive, torch.sqrt(torch.where(alive, B.intensity[:n], 0.0)), 0.0)
    out = np.zeros(len(c))
    block = max(1, SUM_BLOCK_ELEMENTS // max(n, 1))
    for j0 in range(0, len(c), block):
        cj = torch.as_tensor(c[j0:j0 + block], dtype=torch.float64, device=u.device)
        out[j0:j0 + block] = (torch.exp(-(u[None, :] * cj[:, None])) * amp[None, :]).sum(dim=1).cpu().numpy()
    return out


def _axis(Axis, S):
    if Axis is None:
        from . import ModuleProcessing as mp
        Axis = mp.FindCentralRay(S).vector
    a = np.asarray(Axis, dtype=float).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0:
        raise ValueError("Axis must be three finite numbers, not all 0")
    return a / np.linalg.norm(a)


def _check_source_args(Divergence, Position):
    if Divergence is not None and not callable(Divergence):
        raise TypeError("Divergence must be None or a callable omega -> half-angle (rad)")
    if Position is not None and not callable(Position) and (
            isinstance(Position, bool) or not isinstance(Position, (int, float, np.integer, np.floating))):
        raise TypeError("Position must be None, a distance (mm) or a callable omega -> distance")


def _source_model(Divergence, Position, Axis, S, omega, dw):
    """Per frequency of omega (spacing dw): Theta_j, z_j, the unit axis, c_j = 2 / Theta_j^2 and the wavenumbers k_j."""
    J = len(omega)
    theta = np.full(J, np.inf) if Divergence is None else _per_frequency(Divergence, omega, "Divergence", True)
    if Position is None or not callable(Position):
        z = np.full(J, 0.0 if Position is None else float(Position))
        if not np.isfinite(z).all():
            raise ValueError("Position must be finite")
    else:
        z = _per_frequency(Position, omega, "Position", False)
    axis = _axis(Axis, S)
    with np.errstate(over="ignore", divide="ignore"):
        c = 2.0 / theta ** 2
    if not np.isfinite(c).all():
        raise ValueError("Divergence is too small: 2 / Theta^2 overflows")
    kj = omega[0] / C_MM_PER_FS + np.arange(J) * (dw / C_MM_PER_FS)     # art_focal_spectrum's k_j, formed as it forms them
    return theta, z, axis, c, kj


def chromatic_focal_pulse(det, RayList, SourceRays, DeltaFT, Divergence=None, Position=None, Axis=None, Size=None,
                          Pixels=64, Centre=None, Shifts=None, Wavelength=None, RefPath=None, Spectrum=None,
                          TimeWindow=None, Times=256):
    """Detector.get_ChromaticFocalPulse (see the module's docstring).  RayList: the bundle at focus; SourceRays: the
    source bundle it was traced from, slot for slot.  Divergence: a callable omega (rad/fs, array) -> Theta (rad, finite
    and > 0) or None (no apodisation); Position: a callable omega -> z (mm), a scalar, or None (0); Axis: the source's
    axis (default: the mean direction of SourceRays).  Every other argument as in get_FocalPulse.  Frequencies whose
    weight g_j is 0 are left out of the device call."""
    import torch
    DeltaFT, TimeWindow, Nt = pulse.check_pulse_args(DeltaFT, TimeWindow, Times, Spectrum)
    _check_source_args(Divergence, Position)
    if SourceRays is None:
        raise TypeError("SourceRays is required: the source bundle the rays were traced from")
    B, S = RayBundle.of(RayList), RayBundle.of(SourceRays)
    if getattr(B, "grooves", None) is not None or getattr(S, "grooves", None) is not None:
        raise NotImplementedError("get_ChromaticFocalPulse: these rays crossed a grating, so one bundle no longer serves "
                                  "all frequencies; trace one bundle per wavelength with OpticalChain.get_SpectralRays")
    if S.n_slots != B.n_slots:
        raise ValueError(f"SourceRays has {S.n_slots} slots and the rays at focus {B.n_slots}: the two bundles must be "
                         "slot-aligned (the chain's history is)")
    setup = pulse.PulseSetup(det, B, DeltaFT, TimeWindow, Nt, Spectrum, Size, Pixels, Centre, Shifts, Wavelength, RefPath)

    def call(axis, table, kj):
        d = _abi.ArtFocalChromaticDesc()
        d.f = setup.fd
        d.axis[:] = [float(a) for a in axis]
        return B.backend.focal_chromatic(d, B.view(), S.view(), B.intensity, B.n_slots, table)     # [P, kept, ny, nx]

    return _chromatic_pulse(ChromaticFocalPulse, setup, B, S, Divergence, Position, Axis, call, torch.abs)


def _chromatic_pulse(cls, setup, B, S, Divergence, Position, Axis, call, on_axis):
    """What the two chromatic drivers share once their own checks have passed and the PulseSetup stands: the source
    model, the mask `keep` of the frequencies whose weight is not 0, the table of rows (k_j, c_j, z_j, 0) for those, the
    driver's device call(axis, table, kept k_j) -> field [P, kept, *rest], the Fourier sum, amplitude_sum and best_focus.
    on_axis maps the field at the centre pixel, [P, kept] or [P, kept, 3], to the measure [P, kept] whose argmax over the
    planes is best_focus."""
    g = setup.g
    theta, z, axis, c, kj = _source_model(Divergence, Position, Axis, S, setup.omega, setup.dw)
    keep = np.abs(g) > 0
    table = np.stack([kj[keep], c[keep], z[keep], np.zeros(int(keep.sum()))], axis=1)
    field = call(axis, table, kj[keep])
    spectrum, envelope = setup.fourier_sum(field, keep)
    if Divergence is None:
        amplitude_sum = focal.amplitude_sum(B)          # every S_j is the plain sum
    else:
        alive = B.alive[:B.n_slots] != 0
        Sj = apodised_amplitude_sums(B, source_u(S, axis, alive), c[keep])
        amplitude_sum = float((np.abs(g[keep]) * Sj).sum() / setup.gsum)
    best = np.full(len(g), np.nan)
    if amplitude_sum > 0:
        ny, nx = field.shape[-2:]
        measure = on_axis(field[..., (ny - 1) // 2, (nx - 1) // 2]).cpu().numpy()
        best[keep] = np.asarray(setup.shifts, dtype=float)[np.argmax(measure, axis=0)]
    return cls(theta, z, axis, best, setup, spectrum, envelope, amplitude_sum)


class ChromaticVectorFocalPulse(_ChromaticSource, vector_pulse.VectorFocalPulse):
    """vector_pulse.VectorFocalPulse of a chromatic source, and: divergence [J], position [J], axis as in
    ChromaticFocalPulse; best_focus [J]: the value of Shifts with the largest sum_c |F_c|^2 at the pixel nearest the
    grid's centre (NaN for a frequency of weight 0 and without alive rays).  amplitude_sum is ChromaticFocalPulse's, the
    ideal peak of the same apodised source, so `strehl` reads "against a perfect focus of this apodised source behind
    lossless mirrors".  The slices of `spectrum` at frequencies of weight 0 are 0."""


def vector_chromatic_focal_pulse(chain, Coatings, Detector, DeltaFT, Polarisation, Divergence=None, Position=None, Axis=None,
                                 Size=None, Pixels=64, Centre=None, Shifts=None, Wavelength=None, RefPath=None,
                                 Spectrum=None, TimeWindow=None, Times=256, ScratchBytes=None):
    """OpticalChain.get_ChromaticFocalPulse with Coatings (see the module's docstring): chromatic_focal_pulse's source
    model, frequency grid and weights with vector_pulse.vector_focal_pulse's coatings, input state and history, in one
    device call.  Frequencies whose weight g_j is 0 are left out of it, and the materials' tables are evaluated at the
    others only."""
    import torch
    DeltaFT, TimeWindow, Nt = pulse.check_pulse_args(DeltaFT, TimeWindow, Times, Spectrum)
    _check_source_args(Divergence, Position)
    coats, P, bundles = vector_pulse._setup(chain, Coatings, Detector, Polarisation)
    S, B = bundles[0], bundles[-1]
    setup = pulse.PulseSetup(Detector, B, DeltaFT, TimeWindow, Nt, Spectrum, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
    vector_pulse._check_state(bundles, P)

    def call(axis, table, kj):
        sd = setup.spectrum_desc(len(table))     # (k_0 and dk are checked by the library, not used: the table holds the k_j)
        return vector_pulse._vector_spectrum(bundles, coats, P, sd, 2 * math.pi / kj, ScratchBytes,
                                             chromatic=(axis, table))                 # [P, kept, 3, ny, nx]

    return _chromatic_pulse(ChromaticVectorFocalPulse, setup, B, S, Divergence, Position, Axis, call,
                            lambda f: (torch.abs(f) ** 2).sum(dim=2))

"""Space-time focal fields of broadband pulses, summed on the device (art_hip.h, art_focal_spectrum):
Detector.get_FocalPulse.

All optics are mirrors, so one traced bundle serves every frequency of the pulse; here they are also taken as achromatic
(only the phase k (optical path) changes with k) -- coatings whose reflection depends on the frequency, and the vector
field they act on, are OpticalChain.get_FocalPulse (vector_pulse.py); sources whose divergence and position depend on the
frequency are Detector.get_ChromaticFocalPulse (chromatic.py).  The focal field of focal.py (see its docstring for the model and its limits) is summed at J
wavenumbers k_j = omega_j / c in one device call, and a Fourier sum over them gives the envelope in time:

    A(x, y, t) = sum_j g_j E_j(x, y) exp(-i (omega_j - omega_0) t) / sum_j |g_j|,     g_j = s(omega_j) omega_j / omega_0

s is the spectral amplitude (by default the Gaussian whose intensity FWHM in time is DeltaFT) and omega_j / omega_0 the
k-dependence of the Debye integral; its constant factor -i is dropped, which only fixes the carrier-envelope phase.
omega is in rad/fs, t in fs, and t = 0 is RefPath / c: a ray whose optical path exceeds RefPath by L arrives at
t = L / c.  The omega_j are spaced 2 pi / T, so A is periodic in T, the time window; it is sampled at Times points of
[-T/2, T/2).  With this normalisation an ideal focus of a transform-limited pulse peaks at amplitude_sum at t = 0,
so `strehl` is the peak intensity over that of an ideal, transform-limited focus."""
import math

import numpy as np

from . import _abi
from . import focal
from .bundle import RayBundle

LightSpeed = 299792458000  # mm/s
C_MM_PER_FS = LightSpeed * 1e-15
SPAN_FLOOR = 1e-6        # the grid spans the frequencies where the default spectrum s is at least this


def half_span(DeltaFT):
    """|omega - omega_0| (rad/fs) at which the default spectrum falls to SPAN_FLOOR."""
    return math.sqrt(8 * math.log(2) * math.log(1 / SPAN_FLOOR)) / DeltaFT


def gaussian_spectrum(omega, omega0, DeltaFT):
    """exp(-(omega - omega0)^2 DeltaFT^2 / (8 ln 2)): a transform-limited pulse whose intensity FWHM is DeltaFT (fs)."""
    return np.exp(-(np.asarray(omega, float) - omega0) ** 2 * DeltaFT ** 2 / (8 * math.log(2)))


def spectral_grid(wavelength, DeltaFT, T):
    """(omega0, offsets): omega0 = 2 pi c / wavelength (rad/fs) and the integer offsets m of the grid
    omega = omega0 + m * 2 pi / T, symmetric about omega0 and spanning |omega - omega0| <= half_span(DeltaFT).  Raises
    ValueError when that needs more than ART_FOCAL_MAX_WAVENUMBERS wavenumbers or reaches omega <= 0."""
    omega0 = 2 * math.pi * C_MM_PER_FS / wavelength
    half = half_span(DeltaFT)
    if not omega0 - half > 0:
        raise ValueError(f"the spectrum of a {DeltaFT} fs pulse reaches omega <= 0 at {wavelength} mm: the pulse is too "
                         "short for its carrier")
    m = int(math.floor(half / (2 * math.pi / T)))
    if 2 * m + 1 > _abi.ART_FOCAL_MAX_WAVENUMBERS:
        raise ValueError(f"a time window of {T} fs needs {2 * m + 1} wavenumbers for a {DeltaFT} fs pulse, more than "
                         f"{_abi.ART_FOCAL_MAX_WAVENUMBERS}: pass a smaller TimeWindow or a longer DeltaFT")
    return omega0, np.arange(-m, m + 1)


def fwhm(y, dt):
    """Full width at half maximum of the periodic samples y (spacing dt) about their first maximum: the half-maximum
    crossings on either side, linearly interpolated between samples.  NaN when the maximum is not > 0 or y does not
    fall to half of it within half a period on either side."""
    y = np.asarray(y, float)
    N = len(y)
    i = int(np.argmax(y))
    h = 0.5 * y[i]
    if not h > 0:
        return math.nan

    def side(step):
        for k in range(1, N // 2 + 1):
            a, b = y[(i + step * (k - 1)) % N], y[(i + step * k) % N]
            if b <= h:
                return (k - 1) + (a - h) / (a - b)
        return math.nan

    return (side(1) + side(-1)) * dt


class FocalPulse:
    """spectrum: device complex128 [P, J, ny, nx], the focal fields at omega [J] (rad/fs) with the weights g applied;
    envelope: device complex128 [P, Nt, ny, nx], A at the times t [Nt] (fs); intensity: numpy |A|^2; x, y (mm) and
    shifts as in focal.FocalField.  Per plane: strehl [P] = space-time peak of |A|^2 / amplitude_sum^2; peak [P, 3] =
    (x, y, t) of that peak; duration [P] = FWHM (fs) of |A|^2 against t at the peak pixel; profile [P, Nt] = |A|^2
    summed over the pixels and duration_integrated [P] its FWHM; fluence [P, ny, nx] = sum over t of |A|^2 dt;
    arrival [P, ny, nx] = the fluence-weighted mean t (the pulse front; NaN where the fluence is 0).  Without alive
    rays every metric is NaN and the fields are 0.  Also: omega0, weights (g [J]), time_window (T), delta_ft,
    wavelength, ref_path, amplitude_sum."""

    def __init__(self, setup, spectrum, envelope, amplitude_sum):
        fill_pulse(self, setup, spectrum, envelope, amplitude_sum, lambda parts: parts)


def fill_pulse(p, setup, spectrum, envelope, amplitude_sum, intensity_of):
    """The constructor FocalPulse and vector_pulse.VectorFocalPulse share: sets every attribute of FocalPulse's docstring
    on p from the PulseSetup, the device tensors and amplitude_sum; intensity_of maps |envelope|^2 (numpy, the envelope's
    shape) to the intensity [P, Nt, ny, nx].  Returns (|envelope|^2, dt)."""
    p.spectrum, p.envelope = spectrum, envelope
    p.omega, p.omega0, p.weights = setup.omega, float(setup.omega0), setup.g
    p.t, p.time_window = setup.t, float(setup.T)
    p.x, p.y = setup.x, setup.y
    p.shifts = np.asarray(setup.shifts, dtype=float)
    p.delta_ft, p.wavelength = float(setup.DeltaFT), float(setup.wavelength)
    p.ref_path, p.amplitude_sum = float(setup.ref), float(amplitude_sum)
    parts = np.abs(envelope.cpu().numpy()) ** 2
    p.intensity = intensity_of(parts)
    dt = p.time_window / len(p.t)
    (p.strehl, p.peak, p.duration, p.profile, p.duration_integrated, p.fluence,
     p.arrival) = pulse_metrics(p.intensity, p.t, p.x, p.y, dt, p.amplitude_sum)
    return parts, dt


def pulse_metrics(I, t, x, y, dt, amplitude_sum):
    """(strehl, peak, duration, profile, duration_integrated, fluence, arrival) of the intensity I [P, Nt, ny, nx]
    sampled at t with spacing dt (see FocalPulse)."""
    P = I.shape[0]
    profile = I.sum(axis=(2, 3))
    fluence = I.sum(axis=1) * dt
    with np.errstate(invalid="ignore", divide="ignore"):
        arrival = np.where(fluence > 0, (I * np.asarray(t)[None, :, None, None]).sum(axis=1) * dt / fluence, np.nan)
    if not amplitude_sum > 0:
        nan = np.full(P, np.nan)
        return nan, np.full((P, 3), np.nan), nan.copy(), profile, nan.copy(), fluence, np.full_like(fluence, np.nan)
    flat = I.reshape(P, -1)
    idx = np.argmax(flat, axis=1)
    strehl = flat[np.arange(P), idx] / amplitude_sum ** 2
    n, l, j = np.unravel_index(idx, I.shape[1:])
    peak = np.stack([np.asarray(x)[j], np.asarray(y)[l], np.asarray(t)[n]], axis=1)
    duration = np.array([fwhm(I[p, :, l[p], j[p]], dt) for p in range(P)])
    duration_integrated = np.array([fwhm(profile[p], dt) for p in range(P)])
    return strehl, peak, duration, profile, duration_integrated, fluence, arrival


def _positive(v, name):
    v = float(v)
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be finite and positive")
    return v


def check_pulse_args(DeltaFT, TimeWindow, Times, Spectrum):
    """(DeltaFT, TimeWindow or None, Nt) validated as get_FocalPulse's arguments."""
    DeltaFT = _positive(DeltaFT, "DeltaFT")
    if TimeWindow is not None:
        TimeWindow = _positive(TimeWindow, "TimeWindow")
    if not (np.isscalar(Times) and float(Times) == int(Times) and int(Times) >= 1):
        raise ValueError("Times must be a positive integer")
    if Spectrum is not None and not callable(Spectrum):
        raise ValueError("Spectrum must be a callable omega -> complex amplitude")
    return DeltaFT, TimeWindow, int(Times)


def spectral_setup(wavelength, DeltaFT, TimeWindow, Spectrum, stats):
    """The frequency grid and weights of a pulse: (T, omega0, m, dw, omega, g, gsum), T defaulting to 16 DeltaFT +
    4 (max opl - min opl) / c over the alive rays of the lite read-out `stats`."""
    T = TimeWindow
    if T is None:
        spread = stats[13] - stats[12] if stats[0] > 0 else 0.0
        T = 16 * DeltaFT + 4 * spread / C_MM_PER_FS
    omega0, m = spectral_grid(wavelength, DeltaFT, T)
    dw = 2 * math.pi / T
    omega = omega0 + m * dw
    if Spectrum is None:
        amp = gaussian_spectrum(omega, omega0, DeltaFT).astype(complex)
    else:
        amp = np.asarray(Spectrum(omega.copy()), dtype=complex)
        if amp.shape != omega.shape or not np.isfinite(amp).all():
            raise ValueError(f"Spectrum must return {len(omega)} finite amplitudes for the {len(omega)} frequencies")
    g = amp * omega / omega0
    gsum = np.abs(g).sum()
    if not gsum > 0:
        raise ValueError("Spectrum is zero on the whole frequency grid")
    return T, omega0, m, dw, omega, g, gsum


class PulseSetup:
    """What the four pulse-at-focus drivers (focal_pulse here, vector_pulse.vector_focal_pulse and the two of
    chromatic.py) share: get_FocalField's arguments resolved by focal.focal_desc for the bundle B on det (fd, x, y,
    shifts, wavelength, ref), the frequency grid and weights of spectral_setup (T, omega0, m, dw, omega, g, gsum), the
    samples t [Nt] of [-T/2, T/2) and Nt, DeltaFT as check_pulse_args returned them.  A driver builds one after its own
    argument checks, hands spectrum_desc() or a table of its own to its backend call and gives the field to fourier_sum."""

    def __init__(self, det, B, DeltaFT, TimeWindow, Nt, Spectrum, Size, Pixels, Centre, Shifts, Wavelength, RefPath):
        self.fd, self.x, self.y, self.shifts, self.wavelength, self.ref, s = \
            focal.focal_desc(det, B, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
        self.T, self.omega0, self.m, self.dw, self.omega, self.g, self.gsum = \
            spectral_setup(self.wavelength, DeltaFT, TimeWindow, Spectrum, s)
        self.Nt, self.DeltaFT = Nt, DeltaFT
        self.t = -0.5 * self.T + np.arange(Nt) * (self.T / Nt)

    def spectrum_desc(self, nk=None):
        """The ArtFocalSpectrumDesc of the grid: k_0 = omega_0 / c, dk = dw / c and nk wavenumbers (default: all J)."""
        sd = _abi.ArtFocalSpectrumDesc()
        sd.f = self.fd
        sd.f.k = self.omega[0] / C_MM_PER_FS
        sd.dk = self.dw / C_MM_PER_FS
        sd.nk = len(self.omega) if nk is None else nk
        return sd

    def fourier_sum(self, field, keep=None):
        """(spectrum [P, J, *rest], envelope [P, Nt, *rest]) of the device field [P, Jk, *rest] the backend returned, rest
        = (ny, nx) or (3, ny, nx): the field times the weights g, and the Fourier sum of that over the frequencies.
        keep=None means that EVERY frequency went to the device, those of weight 0 included (Jk = J); the achromatic
        drivers (focal_pulse, vector_focal_pulse) pass that.  Only the chromatic drivers drop the frequencies of weight
        0: they pass keep, the boolean mask [J] of the Jk frequencies in the call, and the slices of spectrum at the
        others are 0."""
        import torch
        g = self.g if keep is None else self.g[keep]
        P, Jk, rest = field.shape[0], field.shape[1], tuple(field.shape[2:])
        dev = field.device
        kept = field * torch.as_tensor(g, device=dev)[(None, slice(None)) + (None,) * len(rest)]
        if Jk == len(self.omega):
            spectrum = kept
        else:
            spectrum = torch.zeros((P, len(self.omega)) + rest, dtype=kept.dtype, device=dev)
            spectrum[:, torch.as_tensor(np.flatnonzero(keep), device=dev)] = kept
        # (the matrix of the Fourier sum, [Nt, J], is formed here, on the host, while the device works on the field)
        M = np.exp(-1j * (self.m * self.dw)[None, :] * self.t[:, None]) / self.gsum
        if keep is not None:
            M = np.ascontiguousarray(M[:, keep])
        envelope = torch.matmul(torch.as_tensor(M, device=dev), kept.reshape(P, Jk, -1))
        return spectrum, envelope.reshape((P, self.Nt) + rest)


def focal_pulse(det, RayList, DeltaFT, Size=None, Pixels=64, Centre=None, Shifts=None, Wavelength=None, RefPath=None,
                Spectrum=None, TimeWindow=None, Times=256):
    """Detector.get_FocalPulse (see the module's docstring).  Size, Pixels, Centre, Shifts, Wavelength and RefPath as
    in get_FocalField.  DeltaFT: the Fourier-limited duration (intensity FWHM, fs) that sets the frequency grid and the
    default spectrum; Spectrum: a callable omega (rad/fs, array) -> complex amplitude that replaces the default
    Gaussian (a chirp is a quadratic phase); TimeWindow: T (fs), default 16 DeltaFT + 4 (max opl - min opl) / c over
    the alive rays; Times: samples of [-T/2, T/2).  All wavenumbers and planes are summed in one device call."""
    DeltaFT, TimeWindow, Nt = check_pulse_args(DeltaFT, TimeWindow, Times, Spectrum)
    B = RayBundle.of(RayList)
    setup = PulseSetup(det, B, DeltaFT, TimeWindow, Nt, Spectrum, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
    field = B.backend.focal_spectrum(setup.spectrum_desc(), B.view(), B.intensity, B.n_slots)
    return FocalPulse(setup, *setup.fourier_sum(field), focal.amplitude_sum(B))

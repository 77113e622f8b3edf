"""Pulses at focus behind dispersive coatings, summed on the device (art_hip.h, art_focal_vector_spectrum):
OpticalChain.get_FocalPulse and OpticalChain.get_VectorFocalField.

polarisation.py carries a complex field vector through the chain's mirrors at one wavelength; pulse.py sums scalar
plane waves at the frequencies of a pulse.  Here the two meet: per ray r and frequency omega_j the field
E_r(omega_j) of the polarisation pass -- every coating's rs, rp at k_j = omega_j / c and at the optical constants its
materials have there (coating.Material) -- is the ray's amplitude in the focal sum,

    F_c(x, y; omega_j) = sum_r sqrt(w_r) (E_r(omega_j) . u_c) exp(i k_j Phi_r(x, y)),     u = e1, e2, n of the detector

and the envelope A_c(x, y, t) is pulse.py's Fourier sum of each component; the intensity is sum_c |A_c|^2.  So the
pulse at focus has the mirrors' bandwidth, their group delay and chirp, and the s / p mixing of an out-of-plane chain.

The input state P is normalised per ray as in get_Polarisation (E_0 = P - (P.d) d over its norm), so |E_r| <= 1 and the
metrics are those of pulse.FocalPulse with the same reference: `strehl` is the peak of sum_c |A_c|^2 over
amplitude_sum^2, what an ideal focus of a transform-limited pulse behind lossless mirrors gives -- it now includes what
the mirrors lose."""
import ctypes as C
import math

import numpy as np

from . import _abi
from . import focal
from . import polarisation as _pol
from . import pulse

DEFAULT_SCRATCH_BYTES = 8 * _abi.ART_FOCAL_VECTOR_SCRATCH_DEFAULT


class VectorFocalPulse:
    """spectrum: device complex128 [P, J, 3, ny, nx], the focal fields at omega [J] (rad/fs) with the weights g applied,
    components c = 0, 1, 2 along e1, e2 and the normal of the detector; envelope: device complex128 [P, Nt, 3, ny, nx] at
    the times t [Nt] (fs); intensity: numpy [P, Nt, ny, nx] = sum_c |A_c|^2.  strehl, peak, duration, profile,
    duration_integrated, fluence and arrival: pulse.FocalPulse's metrics of that intensity; longitudinal [P]: the
    share of the fluence in c = 2 (NaN without fluence).  Also omega0, weights, time_window, x, y, shifts, delta_ft,
    wavelength, ref_path, amplitude_sum, as in pulse.FocalPulse."""

    def __init__(self, setup, spectrum, envelope, amplitude_sum):
        parts, dt = pulse.fill_pulse(self, setup, spectrum, envelope, amplitude_sum, lambda parts: parts.sum(axis=2))
        total = self.fluence.sum(axis=(1, 2))                           # (parts: [P, Nt, 3, ny, nx])
        with np.errstate(invalid="ignore", divide="ignore"):
            self.longitudinal = np.where(total > 0, parts[:, :, 2].sum(axis=(1, 2, 3)) * dt / total, np.nan)


class VectorFocalField:
    """field: device complex128 [P, 3, ny, nx] (plane, component along e1, e2, normal of the detector, row = Y,
    column = X); intensity: numpy [P, ny, nx] = sum_c |field_c|^2; strehl [P] and peak [P, 2] of that intensity as in
    focal.FocalField; x, y, shifts, wavelength, ref_path, amplitude_sum as there."""

    def __init__(self, field, x, y, shifts, wavelength, ref_path, amplitude_sum):
        self.field = field
        self.intensity = (np.abs(field.cpu().numpy()) ** 2).sum(axis=1)
        self.x, self.y = x, y
        self.shifts = np.asarray(shifts, dtype=float)
        self.wavelength = float(wavelength)
        self.ref_path = float(ref_path)
        self.amplitude_sum = float(amplitude_sum)
        self.strehl, self.peak = focal.strehl_and_peak(self.intensity, x, y, self.amplitude_sum)


def _setup(chain, Coatings, Detector, Polarisation):
    els = list(chain.optical_elements)
    if not 1 <= len(els) <= _abi.ART_POLARISATION_MAX_ELEMS:
        raise ValueError(f"a chain needs 1..{_abi.ART_POLARISATION_MAX_ELEMS} optical elements")
    coats = _pol.resolve_coatings(els, Coatings)
    P = _pol._state(Polarisation)
    if P is None:
        raise ValueError("a vector focal field needs a polarised input (Polarisation=...)")
    Detector._iscomplete()
    return coats, P, _pol.history(chain)


def _vector_spectrum(bundles, coats, P, sd, wavelengths, scratch_bytes, chromatic=None):
    """art_focal_vector_spectrum for the history `bundles`, one Coating or None per element, the ArtFocalSpectrumDesc
    sd and the wavelengths (mm) of its wavenumbers: device complex128 [planes, nk, 3, ny, nx].  chromatic = (axis,
    table): art_focal_vector_chromatic with that unit axis and that table of sd.nk rows (k_j, c_j, z_j, 0) instead,
    `wavelengths` those of the table's k_j."""
    last = bundles[-1]
    n = last.n_slots
    if scratch_bytes is None:
        scratch_bytes = DEFAULT_SCRATCH_BYTES
    if not (float(scratch_bytes) == int(scratch_bytes) and int(scratch_bytes) >= 8):
        raise ValueError("ScratchBytes must be an integer number of bytes >= 8")
    if 3 * sd.f.planes * sd.nk > 65535:
        raise ValueError(f"{sd.f.planes} planes x {sd.nk} frequencies x 3 components exceed one call (65535): pass fewer "
                         "Shifts or a smaller TimeWindow")
    d = _abi.ArtFocalVectorSpectrumDesc()
    d.s = sd
    coat_list, coat_pos = [], {}
    for e, c in enumerate(coats):
        if c is None:
            d.coating[e] = -1
        else:
            if id(c) not in coat_pos:
                coat_pos[id(c)] = len(coat_list)
                coat_list.append(c)
            d.coating[e] = coat_pos[id(c)]
    d.n_elems = len(coats)
    d.n = n
    d.pol[:] = [P[0].real, P[0].imag, P[1].real, P[1].imag, P[2].real, P[2].imag]
    d.w = None if (last.intensity is None or n == 0) else last.intensity.data_ptr()
    d.scratch_bound = int(scratch_bytes) // 8
    centre = float(wavelengths[len(wavelengths) // 2])
    structs = [c._struct(centre) for c in coat_list]
    mats = np.stack([c.material_table(wavelengths) for c in coat_list], axis=1) if coat_list else \
        np.zeros((len(wavelengths), 0, _abi.ART_COATING_MAX_MATERIALS, 2))
    views = (_abi.ArtBundleView * (len(coats) + 1))(*[b.view() for b in bundles])
    if chromatic is None:
        return last.backend.focal_vector_spectrum(d, views, structs, mats)
    vc = _abi.ArtFocalVectorChromaticDesc()
    vc.v = d
    vc.axis[:] = [float(a) for a in chromatic[0]]
    return last.backend.focal_vector_chromatic(vc, views, structs, mats, chromatic[1])


def _check_state(bundles, P):
    """ValueError when P is (nearly) parallel to a source ray that reaches the end (its transverse part is not defined)."""
    import torch
    src, last = bundles[0], bundles[-1]
    n = last.n_slots
    if n == 0:
        return
    alive = last.alive[:n] != 0
    dirs = torch.stack([src.data[3][:n], src.data[4][:n], src.data[5][:n]]).to(torch.complex128)
    Pt = torch.as_tensor(P, device=dirs.device)
    perp = Pt[:, None] - (Pt[:, None] * dirs).sum(dim=0)[None, :] * dirs
    norm = torch.sqrt((perp.abs() ** 2).sum(dim=0))
    norm = torch.where(alive, norm, torch.full_like(norm, math.inf))
    if float(norm.min()) < 1e-9:
        raise ValueError("Polarisation is (nearly) parallel to the direction of a source ray")


def vector_focal_pulse(chain, Coatings, Detector, DeltaFT, Polarisation, Size=None, Pixels=64, Centre=None, Shifts=None,
                       Wavelength=None, RefPath=None, Spectrum=None, TimeWindow=None, Times=256, ScratchBytes=None):
    """OpticalChain.get_FocalPulse (see the module's docstring and pulse.focal_pulse for the shared arguments)."""
    DeltaFT, TimeWindow, Nt = pulse.check_pulse_args(DeltaFT, TimeWindow, Times, Spectrum)
    coats, P, bundles = _setup(chain, Coatings, Detector, Polarisation)
    B = bundles[-1]
    setup = pulse.PulseSetup(Detector, B, DeltaFT, TimeWindow, Nt, Spectrum, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
    _check_state(bundles, P)
    sd = setup.spectrum_desc()
    k = sd.f.k + np.arange(sd.nk) * sd.dk                  # (the device's k_j)
    field = _vector_spectrum(bundles, coats, P, sd, 2 * math.pi / k, ScratchBytes)
    return VectorFocalPulse(setup, *setup.fourier_sum(field), focal.amplitude_sum(B))


def vector_focal_field(chain, Coatings, Detector, Polarisation, Size=None, Pixels=128, Centre=None, Shifts=None,
                       Wavelength=None, RefPath=None):
    """OpticalChain.get_VectorFocalField: the one-frequency case of art_focal_vector_spectrum (nk = 1)."""
    coats, P, bundles = _setup(chain, Coatings, Detector, Polarisation)
    B = bundles[-1]
    fd, x, y, shifts, wavelength, ref, _ = focal.focal_desc(Detector, B, Size, Pixels, Centre, Shifts, Wavelength, RefPath)
    _check_state(bundles, P)
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.dk = 0.0
    sd.nk = 1
    field = _vector_spectrum(bundles, coats, P, sd, np.array([wavelength]), None)
    return VectorFocalField(field[:, 0], x, y, shifts, wavelength, ref, focal.amplitude_sum(B))

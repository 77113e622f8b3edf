"""Mirror coatings and polarisation on the device (art_hip.h, art_polarisation): OpticalChain.get_Polarisation.

One streaming pass over a traced chain's history.  Per ray and mirror, the directions before and after the reflection
give the normal, the angle of incidence and the s / p frame; the coating gives rs, rp (coating.Coating); the field
follows the 3x3 polarisation ray-tracing step E' = rs (E.s) s + rp (E.p_in) p_out.  A mask leaves the
field as it is.  The result is a reflectance-weighted alias of the final bundle, so every analysis that reads
Ray.intensity (histograms, focal fields and pulses, wavefronts, getETransmission, intensity-coloured spot diagrams)
takes the coatings into account.

The chain's history comes from get_output_rays(); a lazy history (history="lazy") is materialised by its own mechanism,
which costs one re-trace of the chain.  Tabulated materials (coating.Material) are evaluated at the one wavelength of
the call; a pulse behind dispersive coatings, and the reflection phase in the focal field, are vector_pulse.py
(OpticalChain.get_FocalPulse, get_VectorFocalField).  Out of scope: transmissive optics, and fusing this pass into the
trace."""
import ctypes as C
import math

import numpy as np

from . import _abi
from .coating import Coating

MAX_JOBS_PER_CALL = 64


class Polarisation:
    """What get_Polarisation returns.  transmission: percent, 100 sum w_out / sum w over the source's alive rays
    (getETransmission's definition); throughput: DEVICE [n] w_out = w T; rays: an alias of the final bundle with
    intensity = throughput; count: rays alive at the end; t_min, t_max: the range of T over them; with a Detector:
    stokes (S0, S1, S2, S3) in its frame (e1, e2 = rows 0, 1 of its rotation), stokes_normalised = stokes / S0,
    degree = sqrt(S1^2 + S2^2 + S3^2) / S0, longitudinal = sum w |E.n|^2 / (S0 + sum w |E.n|^2), the part of the field
    not transverse to the detector; field: DEVICE complex128 [3, n] (PerRay=True, polarised input only), else None."""

    def __init__(self, row, throughput, rays, field, has_det):
        self.count = int(row[0])
        self.sum_w_source = float(row[1])
        self.sum_w_out = float(row[2])
        self.transmission = 100.0 * self.sum_w_out / self.sum_w_source if self.sum_w_source > 0 else math.nan
        self.t_min, self.t_max = float(row[3]), float(row[4])
        self.throughput, self.rays, self.field = throughput, rays, field
        nan = math.nan
        if has_det:
            self.stokes = tuple(float(v) for v in row[5:9])
            self.longitudinal_sum = float(row[9])
            S0 = self.stokes[0]
            self.stokes_normalised = tuple(v / S0 for v in self.stokes) if S0 > 0 else (nan,) * 4
            self.degree = math.sqrt(sum(v * v for v in self.stokes[1:])) / S0 if S0 > 0 else nan
            tot = S0 + self.longitudinal_sum
            self.longitudinal = self.longitudinal_sum / tot if tot > 0 else nan
        else:
            self.stokes = self.stokes_normalised = None
            self.degree = self.longitudinal = self.longitudinal_sum = None


def _is_mask(oe):
    return getattr(oe.type, "type", None) == "Mask"


def resolve_coatings(elements, Coatings):
    """One Coating or None per element: a single Coating applies to every mirror; a list has one entry per element,
    None for masks (a mask given a coating, or a mirror given none, is a ValueError)."""
    if isinstance(Coatings, Coating):
        return [None if _is_mask(oe) else Coatings for oe in elements]
    lst = list(Coatings)
    if len(lst) != len(elements):
        raise ValueError(f"Coatings: {len(lst)} entries for {len(elements)} optical elements")
    for k, (oe, c) in enumerate(zip(elements, lst)):
        if _is_mask(oe):
            if c is not None:
                raise ValueError(f"element {k} is a mask: its coating must be None")
        elif not isinstance(c, Coating):
            raise ValueError(f"element {k} is a mirror: it needs a Coating")
    return lst


def _state(P):
    if P is None:
        return None
    v = np.asarray(P, dtype=complex).reshape(-1)
    if v.shape != (3,) or not np.all(np.isfinite(v.real)) or not np.all(np.isfinite(v.imag)):
        raise ValueError("Polarisation must be None or three finite (complex) numbers")
    return v


def history(chain):
    """[source bundle, the bundle after each element]: the K + 1 views of a chain's polarisation pass."""
    out = chain.get_output_rays()
    bundles = [chain.source_rays] + [out[k] for k in range(len(chain.optical_elements))]   # (a lazy history materialises here)
    n = bundles[-1].n_slots
    if any(b.n_slots != n for b in bundles):
        raise ValueError("the bundles of the chain's history do not have the same slots")
    return bundles


def polarisations(requests):
    """requests: [(chain, Coatings, kwargs)], kwargs those of OpticalChain.get_Polarisation.  One Polarisation per
    request, in order; all chains of one backend go to the device in ONE call of art_polarisation (blocks of
    MAX_JOBS_PER_CALL), and the one copy back to the host is the table of sums."""
    items = []
    for chain, Coatings, kw in requests:
        kw = dict(kw or {})
        unknown = set(kw) - {"Polarisation", "Detector", "Wavelength", "PerRay"}
        if unknown:
            raise TypeError(f"unknown arguments {sorted(unknown)}")
        els = list(chain.optical_elements)
        if not 1 <= len(els) <= _abi.ART_POLARISATION_MAX_ELEMS:
            raise ValueError(f"a chain needs 1..{_abi.ART_POLARISATION_MAX_ELEMS} optical elements")
        coats = resolve_coatings(els, Coatings)
        P = _state(kw.get("Polarisation"))
        per_ray = bool(kw.get("PerRay", False))
        if per_ray and P is None:
            raise ValueError("PerRay=True needs a polarised input (Polarisation=...)")
        det = kw.get("Detector")
        if det is not None:
            det._iscomplete()
        bundles = history(chain)
        wl = kw.get("Wavelength")
        wl = bundles[-1].wavelength if wl is None else wl
        if wl is None or not math.isfinite(float(wl)) or float(wl) <= 0:
            raise ValueError("Wavelength must be finite and positive (the bundle carries none)")
        items.append((bundles, coats, P, det, float(wl), per_ray))
    groups = {}
    for pos, it in enumerate(items):
        groups.setdefault(id(it[0][-1].backend), []).append(pos)
    results = [None] * len(items)
    for positions in groups.values():
        be = items[positions[0]][0][-1].backend
        for lo in range(0, len(positions), MAX_JOBS_PER_CALL):
            part = positions[lo:lo + MAX_JOBS_PER_CALL]
            coat_list, coat_pos = [], {}
            jobs, views, outs = [], [], []
            for pos in part:
                j, v, keep = _job(items[pos], coat_list, coat_pos)
                jobs.append(j)
                views.append(v)
                outs.append(keep)
            rows = be.polarisation(jobs, views, [c._struct() for c in coat_list]).cpu().numpy()
            for k, pos in enumerate(part):
                bundles, _, P, det, _, _ = items[pos]
                w_out, field = outs[k]
                if P is not None and rows[k][0] > 0 and rows[k][10] < 1e-9:
                    raise ValueError("Polarisation is (nearly) parallel to the direction of a source ray")
                rays = bundles[-1].alias()
                rays.intensity = w_out
                rays.touch()                       # (new weights: drop what was cached for the original ones)
                results[pos] = Polarisation(rows[k], w_out, rays, field, det is not None)
    return results


def _job(item, coat_list, coat_pos):
    bundles, coats, P, det, wl, per_ray = item
    last = bundles[-1]
    be, n = last.backend, last.n_slots
    j = _abi.ArtPolarisationJob()
    K = len(coats)
    for e, c in enumerate(coats):
        if c is None:
            j.coating[e] = -1
        else:
            key = (id(c), wl) if c.dispersive else id(c)   # (tabulated materials are evaluated at the job's wavelength)
            if key not in coat_pos:
                coat_pos[key] = len(coat_list)
                coat_list.append(c.at(wl) if c.dispersive else c)
            j.coating[e] = coat_pos[key]
    j.n_elems = K
    j.n = n
    if P is not None:
        j.polarised = 1
        j.pol[:] = [P[0].real, P[0].imag, P[1].real, P[1].imag, P[2].real, P[2].imag]
    j.k = 2 * math.pi / wl
    if det is not None:
        j.has_det = 1
        j.det = det._desc()
    src = bundles[0]
    j.w0 = None if src.intensity is None else src.intensity.data_ptr()
    j.w = None if last.intensity is None else last.intensity.data_ptr()
    w_out = be.empty(max(n, 1))[:n]
    j.w_out = w_out.data_ptr()
    field = None
    if per_ray:
        import torch
        buf = be.empty(6 * max(n, 1))
        j.field = buf.data_ptr()
        field = torch.view_as_complex(buf[:6 * n].reshape(3, n, 2))
    views = (_abi.ArtBundleView * (K + 1))(*[b.view() for b in bundles])
    return j, views, (w_out, field)


def polarisation(chain, Coatings, Polarisation=None, Detector=None, Wavelength=None, PerRay=False):
    """OpticalChain.get_Polarisation (see the module's docstring)."""
    kw = dict(Polarisation=Polarisation, Detector=Detector, Wavelength=Wavelength, PerRay=PerRay)
    return polarisations([(chain, Coatings, kw)])[0]

"""Mirror coatings: the reflection coefficients rs, rp of a substrate under a stack of layers (art_hip.h,
art_polarisation; DESIGN.md 3 has the model).

Time dependence exp(-i w t); a refractive index is N = n + i kappa with kappa >= 0, given as a number or in the XUV form
(delta, beta) for N = 1 - delta + i beta.  Layers run from the top down; each layer's roughness is that of the interface
at its top (Nevot-Croce), `Roughness` that of the substrate's top interface.  Lengths in mm, like the wavelength.

A material whose optical constants vary with the wavelength is a Material: a table, interpolated linearly in photon
energy.  Wherever one wavelength is asked for (Coating.reflectance, get_Polarisation) it is evaluated there; a pulse
(OpticalChain.get_FocalPulse) evaluates it at every frequency of its grid."""
import math

import numpy as np

from . import _abi


class Material:
    """Material(Wavelengths, N) or Material(Wavelengths, delta=..., beta=...): tabulated optical constants N = n + i kappa
    (= 1 - delta + i beta) at the distinct wavelengths of the table (mm, any order, at least one).  at(wavelength) is
    linear in photon energy (1 / wavelength) between the nodes and exact at them; outside the table it raises ValueError
    (no extrapolation).  ValueError for a non-finite entry or kappa < 0."""

    def __init__(self, Wavelengths, N=None, delta=None, beta=None):
        wl = np.atleast_1d(np.asarray(Wavelengths, dtype=float))
        if N is None:
            if delta is None or beta is None:
                raise ValueError("a Material needs N, or delta and beta")
            N = (1.0 - np.asarray(delta, dtype=float)) + 1j * np.asarray(beta, dtype=float)
        elif delta is not None or beta is not None:
            raise ValueError("a Material takes N or (delta, beta), not both")
        N = np.atleast_1d(np.asarray(N, dtype=complex))
        if wl.ndim != 1 or wl.shape != N.shape or len(wl) < 1:
            raise ValueError("Wavelengths and the optical constants must be 1-D and of equal length")
        if not (np.isfinite(wl).all() and (wl > 0).all()):
            raise ValueError("Wavelengths must be finite and positive")
        if not (np.isfinite(N.real).all() and np.isfinite(N.imag).all()) or (N.imag < 0).any():
            raise ValueError("optical constants must be finite with kappa >= 0")
        order = np.argsort(1.0 / wl)
        self.energy = (1.0 / wl)[order]              # 1 / wavelength (1/mm), ascending: proportional to photon energy
        if (np.diff(self.energy) <= 0).any():
            raise ValueError("Wavelengths must be distinct")
        self.wavelengths, self.N = wl[order], N[order]

    def at(self, wavelength):
        """N at `wavelength` (mm; a scalar or an array), complex."""
        w = np.asarray(wavelength, dtype=float)
        e = 1.0 / w
        lo, hi = self.energy[0], self.energy[-1]
        inside = (w > 0) & (e >= lo) & (e <= hi)
        if (e.ndim == 0 and not inside) or (e.ndim > 0 and not inside.all()):
            raise ValueError(f"wavelength outside the material's table [{self.wavelengths.min()}, "
                             f"{self.wavelengths.max()}] mm (no extrapolation)")
        i = np.clip(np.searchsorted(self.energy, e, side="right") - 1, 0, max(len(self.energy) - 2, 0))
        if len(self.energy) == 1:
            out = np.broadcast_to(self.N[0], e.shape).copy()
        else:
            f = (e - self.energy[i]) / (self.energy[i + 1] - self.energy[i])
            out = np.where(f == 0, self.N[i], np.where(f == 1, self.N[i + 1], (1 - f) * self.N[i] + f * self.N[i + 1]))
        return complex(out) if out.ndim == 0 else out

    def __repr__(self):
        return f"Material({len(self.energy)} wavelengths in [{self.wavelengths.min()}, {self.wavelengths.max()}] mm)"


def refractive_index(v):
    """N from a number or a (delta, beta) pair: 1 - delta + i beta.  ValueError unless finite with kappa >= 0.  A
    Material is returned as it is."""
    if isinstance(v, Material):
        return v
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("an optical constant is N or a (delta, beta) pair")
        N = complex(1.0 - float(v[0]), float(v[1]))
    else:
        try:
            N = complex(v)
        except TypeError:
            raise ValueError("an optical constant is N or a (delta, beta) pair") from None
    if not (math.isfinite(N.real) and math.isfinite(N.imag)) or N.imag < 0:
        raise ValueError(f"refractive index {N} must be finite with kappa >= 0")
    return N


def _length(v, name):
    x = float(v)
    if not math.isfinite(x) or x < 0:
        raise ValueError(f"{name} must be finite and >= 0")
    return x


class Coating:
    """Coating(Substrate, Layers=(), Roughness=0.0): Substrate N, (delta, beta) or a Material; Layers [(N, (delta, beta)
    or Material, thickness_mm, roughness_mm)], top first, at most ART_COATING_MAX_LAYERS; at most
    ART_COATING_MAX_MATERIALS distinct indices in all (a Material counts once per object).  Coating.ideal() is the
    perfect conductor (rs = -1, rp = +1).  dispersive: some material is tabulated."""

    def __init__(self, Substrate, Layers=(), Roughness=0.0):
        self.is_ideal = False
        self.substrate = refractive_index(Substrate)
        layers = list(Layers)
        if len(layers) > _abi.ART_COATING_MAX_LAYERS:
            raise ValueError(f"a coating has at most {_abi.ART_COATING_MAX_LAYERS} layers")
        self.layers = []
        for ly in layers:
            if len(ly) != 3:
                raise ValueError("a layer is (N or (delta, beta), thickness_mm, roughness_mm)")
            self.layers.append((refractive_index(ly[0]), _length(ly[1], "layer thickness"),
                                _length(ly[2], "layer roughness")))
        self.roughness = _length(Roughness, "Roughness")
        mats = []
        for N in [self.substrate] + [ly[0] for ly in self.layers]:
            if not any(N is M or (not isinstance(N, Material) and not isinstance(M, Material) and N == M) for M in mats):
                mats.append(N)
        if len(mats) > _abi.ART_COATING_MAX_MATERIALS:
            raise ValueError(f"a coating names at most {_abi.ART_COATING_MAX_MATERIALS} distinct refractive indices")
        self.materials = mats
        self.dispersive = any(isinstance(N, Material) for N in mats)

    def _index(self, N):
        return next(m for m, M in enumerate(self.materials) if M is N or (not isinstance(M, Material) and M == N))

    def indices(self, wavelength=None):
        """The materials' N at `wavelength` (mm), in the order of the device's table; constants need no wavelength."""
        if self.dispersive and wavelength is None:
            raise ValueError("a coating with tabulated materials needs a wavelength")
        return [N.at(wavelength) if isinstance(N, Material) else N for N in self.materials]

    def at(self, wavelength):
        """This coating with every tabulated material replaced by its N at `wavelength` (mm): a Coating of numbers."""
        if not self.dispersive:
            return self
        N = lambda v: v.at(wavelength) if isinstance(v, Material) else v
        return Coating(N(self.substrate), [(N(v), t, s) for v, t, s in self.layers], Roughness=self.roughness)

    def material_table(self, wavelengths):
        """float64 [len(wavelengths), ART_COATING_MAX_MATERIALS, 2]: (n, kappa) of every material at every wavelength,
        the per-frequency table of art_focal_vector_spectrum (unused entries 1, 0)."""
        wl = np.asarray(wavelengths, dtype=float)
        tab = np.zeros((len(wl), _abi.ART_COATING_MAX_MATERIALS, 2))
        tab[:, :, 0] = 1.0
        if self.is_ideal:
            return tab
        for m, N in enumerate(self.materials):
            v = N.at(wl) if isinstance(N, Material) else np.full(len(wl), N)
            tab[:, m, 0], tab[:, m, 1] = v.real, v.imag
        return tab

    @classmethod
    def ideal(cls):
        c = cls(1.0)
        c.is_ideal = True
        return c

    def reflectance(self, theta, wavelength):
        """(rs, rp), complex NumPy arrays shaped like theta (angle of incidence from the normal, rad), at `wavelength`
        (mm): Fresnel interfaces with Nevot-Croce roughness and Parratt's recursion from the substrate up."""
        wl = float(wavelength)
        if not math.isfinite(wl) or wl <= 0:
            raise ValueError("wavelength must be finite and positive")
        th = np.asarray(theta, dtype=float)
        if self.is_ideal:
            return np.full(th.shape, -1.0 + 0j), np.full(th.shape, 1.0 + 0j)
        k = 2 * math.pi / wl
        c2 = np.cos(th) ** 2           # kz / k = sqrt(N^2 - 1 + cos^2 theta): 1 - sin^2 would lose digits at grazing
        at = (lambda N: N.at(wl) if isinstance(N, Material) else N)
        media = [1.0 + 0j] + [at(ly[0]) for ly in self.layers] + [at(self.substrate)]
        sig = [ly[2] for ly in self.layers] + [self.roughness]     # interface j, j + 1 has sig[j]
        kz = []
        for N in media:
            q = np.sqrt((N - 1) * (N + 1) + c2 + 0j)
            kz.append(k * np.where(q.imag < 0, -q, q))
        rs = np.zeros(th.shape, complex)
        rp = np.zeros(th.shape, complex)
        L = len(self.layers)
        for j in range(L, -1, -1):
            a, b = kz[j], kz[j + 1]
            ea, eb = media[j] ** 2, media[j + 1] ** 2
            r_s = (a - b) / (a + b)
            r_p = (eb * a - ea * b) / (eb * a + ea * b)
            if sig[j] > 0:
                f = np.exp(-2 * a * b * sig[j] ** 2)
                r_s, r_p = r_s * f, r_p * f
            if j == L:
                rs, rp = r_s, r_p
            else:
                X = np.exp(2j * b * self.layers[j][1])
                rs = (r_s + rs * X) / (1 + r_s * rs * X)
                rp = (r_p + rp * X) / (1 + r_p * rp * X)
        return rs, rp

    def _struct(self, wavelength=None):
        """The ArtCoating of this coating; tabulated materials are evaluated at `wavelength` (mm)."""
        c = _abi.ArtCoating()
        if self.is_ideal:
            c.ideal = 1
            c.n_materials = 1
            c.materials[0].n, c.materials[0].kappa = 1.0, 0.0
            return c
        c.n_materials = len(self.materials)
        for m, N in enumerate(self.indices(wavelength)):
            c.materials[m].n, c.materials[m].kappa = N.real, N.imag
        c.substrate = self._index(self.substrate)
        c.n_layers = len(self.layers)
        c.roughness = self.roughness
        for l, (N, t, s) in enumerate(self.layers):
            c.layers[l].thickness, c.layers[l].roughness, c.layers[l].material = t, s, self._index(N)
        return c

    def __repr__(self):
        if self.is_ideal:
            return "Coating.ideal()"
        return f"Coating({self.substrate}, {len(self.layers)} layers, Roughness={self.roughness})"

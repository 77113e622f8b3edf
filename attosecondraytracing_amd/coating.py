"""Mirror coatings: the reflection coefficients rs, rp of a substrate under a stack of layers (art_hip.h,
art_polarisation; DESIGN.md 3 has the model).

Time dependence exp(-i w t); a refractive index is N = n + i kappa with kappa >= 0, given as a number or in the XUV form
(delta, beta) for N = 1 - delta + i beta.  Layers run from the top down; each layer's roughness is that of the interface
at its top (Nevot-Croce), `Roughness` that of the substrate's top interface.  Lengths in mm, like the wavelength."""
import math

import numpy as np

from . import _abi


def refractive_index(v):
    """N from a number or a (delta, beta) pair: 1 - delta + i beta.  ValueError unless finite with kappa >= 0."""
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
    """Coating(Substrate, Layers=(), Roughness=0.0): Substrate N or (delta, beta); Layers [(N or (delta, beta),
    thickness_mm, roughness_mm)], top first, at most ART_COATING_MAX_LAYERS; at most ART_COATING_MAX_MATERIALS distinct
    indices in all.  Coating.ideal() is the perfect conductor (rs = -1, rp = +1)."""

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
            if N not in mats:
                mats.append(N)
        if len(mats) > _abi.ART_COATING_MAX_MATERIALS:
            raise ValueError(f"a coating names at most {_abi.ART_COATING_MAX_MATERIALS} distinct refractive indices")
        self.materials = mats

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
        media = [1.0 + 0j] + [ly[0] for ly in self.layers] + [self.substrate]
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

    def _struct(self):
        c = _abi.ArtCoating()
        if self.is_ideal:
            c.ideal = 1
            c.n_materials = 1
            c.materials[0].n, c.materials[0].kappa = 1.0, 0.0
            return c
        c.n_materials = len(self.materials)
        for m, N in enumerate(self.materials):
            c.materials[m].n, c.materials[m].kappa = N.real, N.imag
        c.substrate = self.materials.index(self.substrate)
        c.n_layers = len(self.layers)
        c.roughness = self.roughness
        for l, (N, t, s) in enumerate(self.layers):
            c.layers[l].thickness, c.layers[l].roughness, c.layers[l].material = t, s, self.materials.index(N)
        return c

    def __repr__(self):
        if self.is_ideal:
            return "Coating.ideal()"
        return f"Coating({self.substrate}, {len(self.layers)} layers, Roughness={self.roughness})"

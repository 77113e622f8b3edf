"""The coating x angle matrix of the truth tests (tests/test_coating_truth.py on the CPU twin, tests/
test_gpu_coating_truth.py on the device): coatings built through the public API, wave numbers, and the incidence
angles -- normal, a 1e-14 tilt (the fallback frame), 0.3 / 0.7 / 1.2 rad, grazing 30 .. 0.1 mrad and both sides of the
coating's critical angle -- as pairs of fp64 unit directions in assorted orientations."""
import math

import numpy as np

from attosecondraytracing_amd.coating import Coating

K_XUV = 2 * math.pi / 13.5e-6
K_VIS = 2 * math.pi / 633e-6

# illustrative optical constants: (delta, beta) at 13.5 nm, N = n + i kappa at 633 nm
MO, SI, RU, B4C, C_, SIO2 = (0.0769, 0.0064), (0.0010, 0.0018), (0.1135, 0.0165), (0.0364, 0.0044), (0.0381, 0.0069), \
    (0.0217, 0.0107)
AG, AU = complex(0.13, 4.0), complex(0.18, 3.4)


def mosi(periods):
    layers = []
    for _ in range(periods):
        layers += [(SI, 4.1e-6, 0.3e-6), (MO, 2.8e-6, 0.3e-6)]
    return Coating(SI, layers, Roughness=0.3e-6)


def six_materials():
    """Six distinct materials (every slot of ART_COATING_MAX_MATERIALS), 24 layers with and without roughness."""
    seq = [(RU, 2.0e-6, 0.2e-6), (B4C, 0.6e-6, 0.0), (MO, 2.7e-6, 0.3e-6), (C_, 0.5e-6, 0.1e-6), (SIO2, 3.9e-6, 0.0),
           (MO, 2.6e-6, 0.25e-6)]
    return Coating(SI, seq * 4, Roughness=0.3e-6)


def gold():
    return Coating((0.02, 0.01), [((0.1, 0.06), 40e-6, 0.5e-6)], Roughness=0.3e-6)


# name -> (coating factory, wave number, grazing critical angle or None)
COATINGS = {
    "gold": (gold, K_XUV, None),
    "mosi40": (lambda: mosi(40), K_XUV, None),
    "mosi128": (lambda: mosi(128), K_XUV, None),
    "six": (six_materials, K_XUV, None),
    "si": (lambda: Coating(SI), K_XUV, None),
    "lossless": (lambda: Coating((1e-3, 0.0)), K_XUV, math.asin(math.sqrt(1 - (1 - 1e-3) ** 2))),
    "metal633": (lambda: Coating(AG), K_VIS, None),
    "metal633_rough": (lambda: Coating(AG, Roughness=3e-6), K_VIS, None),
    "metal_on_metal": (lambda: Coating(AG, [(AU, 20e-6, 3e-6)], Roughness=3e-6), K_VIS, None),
    "absorber_1mm": (lambda: Coating(SI, [(MO, 1.0, 0.3e-6)], Roughness=0.3e-6), K_XUV, None),
    "zero_thickness": (lambda: Coating((0.05, 0.02), [(MO, 0.0, 0.0), (RU, 0.0, 0.4e-6), (B4C, 0.0, 0.0)],
                                       Roughness=0.2e-6), K_XUV, None),
}

# (label, sin t, cos t): t the angle of incidence from the normal; grazing angles g give sin t = cos g, cos t = sin g
ANGLES = [("normal", 0.0, 1.0), ("tilt 1e-14", math.sin(1e-14), math.cos(1e-14))] + \
    [("%.1f rad" % t, math.sin(t), math.cos(t)) for t in (0.3, 0.7, 1.2)] + \
    [("%g mrad" % (g * 1e3), math.cos(g), math.sin(g)) for g in (30e-3, 10e-3, 3e-3, 1e-3, 0.3e-3, 0.1e-3)]

# offsets from a critical grazing angle: relative ones are held to the plain bar, absolute ones (rad, within 1e-6 of
# the critical angle) to the bar widened by the conditioning of r in cos^2 t
CRIT_REL = (-0.05, 0.05)
CRIT_ABS = (-1e-7, -1e-10, 1e-10, 1e-7)


def angles(crit):
    """ANGLES plus both sides of the critical grazing angle `crit` (None: none): (label, sin t, cos t, near)."""
    out = [(lab, s, c, False) for lab, s, c in ANGLES]
    if crit is not None:
        for r in CRIT_REL:
            g = crit * (1 + r)
            out.append(("crit %+g" % r, math.cos(g), math.sin(g), False))
        for d in CRIT_ABS:
            g = crit + d
            out.append(("crit %+g rad" % d, math.cos(g), math.sin(g), True))
    return out


def rotations(count, seed=7):
    """The identity and count - 1 random rotations (fp64)."""
    rng = np.random.default_rng(seed)
    out = [np.eye(3)]
    while len(out) < count:
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) > 0:
            out.append(q)
    return out


def pair(sin_t, cos_t, R):
    """Unit directions before and after a reflection at incidence t off the plane with normal R ez, plane of incidence
    R (ex, ez): a = R (sin t, 0, -cos t), b = R (sin t, 0, cos t)."""
    a = R @ np.array([sin_t, 0.0, -cos_t])
    b = R @ np.array([sin_t, 0.0, cos_t])
    return a, b

"""NumPy statement of the focal-field model of art_focal_field (include/art_hip.h), summed directly over rays and pixels:
the oracle of tests/test_focal_host.py and tests/test_gpu_focal.py.

    E_q[l, j] = sum_r sqrt(w_r) exp(i (base_r + shift_q kc_r + Y_l kb_r + X_j ka_r))

with base_r = k ((path_r - L_ref) + d_r . (C - p_r)), ka = k d.e1, kb = k d.e2, kc = k d.n.  base_r is formed in the
header's operation order: d . (C - p) and path - L_ref are each hundreds of mm on a relay while their sum is a
fraction of a wavelength, so a different rounding there alone moves a phase by ~1e-8 rad."""
import numpy as np


def ray_terms(P, D, path, alive, w, k, L_ref, C, normal, rot):
    """(amp, base, ka, kb, kc) of the alive rays.  P, D: (n, 3); rot: the detector's 3x3 map (rows e1, e2, normal)."""
    alive = np.asarray(alive).astype(bool)
    p, d, L = np.asarray(P, float)[alive], np.asarray(D, float)[alive], np.asarray(path, float)[alive]
    amp = np.ones(len(p)) if w is None else np.sqrt(np.asarray(w, float)[alive])
    R = np.asarray(rot, float).reshape(3, 3)
    dot = lambda v: (d[:, 0] * v[0] + d[:, 1] * v[1]) + d[:, 2] * v[2]
    base = k * ((L - L_ref) + ((d[:, 0] * (C[0] - p[:, 0]) + d[:, 1] * (C[1] - p[:, 1])) + d[:, 2] * (C[2] - p[:, 2])))
    return amp, base, k * dot(R[0]), k * dot(R[1]), k * dot(np.asarray(normal, float))


def field(P, D, path, alive, w, k, L_ref, C, normal, rot, x, y, shifts, chunk=512):
    """complex128 [len(shifts), len(y), len(x)]; shifts along +normal (the ABI's convention)."""
    amp, base, ka, kb, kc = ray_terms(P, D, path, alive, w, k, L_ref, C, normal, rot)
    x, y = np.asarray(x, float), np.asarray(y, float)
    E = np.zeros((len(shifts), len(y), len(x)), dtype=np.complex128)
    for q, s in enumerate(shifts):
        for a in range(0, len(amp), chunk):
            sl = slice(a, a + chunk)
            ph = (base[sl] + s * kc[sl])[:, None, None] + kb[sl][:, None, None] * y[None, :, None] \
                + ka[sl][:, None, None] * x[None, None, :]
            E[q] += np.einsum("r,rlj->lj", amp[sl], np.exp(1j * ph))
    return E


def bundle_arrays(B):
    """Host copies of a RayBundle's slots: P (n, 3), D (n, 3), path, alive, w (None without intensities)."""
    n = B.n_slots
    data = B.data[:, :n].cpu().numpy()
    return (data[0:3].T.copy(), data[3:6].T.copy(), data[6].copy(), B.alive[:n].cpu().numpy().astype(bool),
            None if B.intensity is None else B.intensity[:n].cpu().numpy())


def field_of(B, det, f):
    """The oracle's field for bundle B on detector det with the grid and shifts of FocalField f (Python shifts, i.e.
    shiftByDistance's sign: the ABI gets their negatives)."""
    d = det._desc()
    P, D, L, alive, w = bundle_arrays(B)
    return field(P, D, L, alive, w, 2 * np.pi / f.wavelength, f.ref_path, np.array(d.centre[:]), np.array(d.normal[:]),
                 np.array(d.rot[:]), f.x, f.y, [-s for s in f.shifts])


def converging_bundle(n, NA, R, focus=(0.0, 0.0, 0.0), wavelength=1e-3, backend=None, weights=None):
    """An ideal focus: directions equal-area (Vogel spiral) on the disk of radius NA about +z, points on the sphere of
    radius R about `focus`, every ray with optical path 0 there -- so all reach the focus with path R."""
    from attosecondraytracing_amd.bundle import RayBundle
    i = np.arange(n)
    rho = NA * np.sqrt((i + 0.5) / n)
    th = i * np.pi * (3 - np.sqrt(5))
    u = np.stack([rho * np.cos(th), rho * np.sin(th), np.sqrt(1 - rho ** 2)], axis=1)
    P = np.asarray(focus, float) - R * u
    return RayBundle.from_arrays(P, u, intensity=weights, wavelength=wavelength, backend=backend)


def bessel_j1(x, m=4001):
    """J1 by quadrature: (1/pi) int_0^pi cos(t - x sin t) dt."""
    t = np.linspace(0, np.pi, m)
    x = np.atleast_1d(np.asarray(x, float))
    return np.trapezoid(np.cos(t[None, :] - x[:, None] * np.sin(t[None, :])), t, axis=1) / np.pi \
        if hasattr(np, "trapezoid") else np.trapz(np.cos(t[None, :] - x[:, None] * np.sin(t[None, :])), t, axis=1) / np.pi


def airy(v):
    """(2 J1(v) / v)^2, 1 at v = 0."""
    v = np.asarray(v, float)
    out = np.ones_like(v)
    nz = v != 0
    out[nz] = (2 * bessel_j1(v[nz]) / v[nz]) ** 2
    return out

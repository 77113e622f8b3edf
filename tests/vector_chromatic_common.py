"""Statement of art_focal_vector_chromatic's contract (include/art_hip.h) on top of the helpers the two calls it joins
already have.  TEST INFRASTRUCTURE (the judge of tests/test_vector_chromatic_host.py and
tests/test_gpu_vector_chromatic.py).

Per table row (k_j, c_j, z_j, 0): tests/vector_pulse_truth.py's amplitudes at k_j (mpmath per ray: the field through the
coatings with the materials' constants at k_j) times exp(-u c_j), then its direct sum with ks = [k_j] and the optical
paths L + z_j u; u comes from tests/chromatic_common.py's source_u (1 - cos of the angle between the ray's SOURCE
direction and the axis)."""
import numpy as np

import chromatic_common as cc
import focal_common as fc
import vector_pulse_truth as vt


def field(P, V, L, alive, w, dirs, axis, table, coats, pol, L_ref, C, normal, rot, x, y, shifts, workers=None):
    """complex128 [len(shifts), len(table), 3, len(y), len(x)]; shifts along +normal (the ABI's convention).  dirs: the
    K + 1 direction arrays (n, 3) of the history, dirs[0] the source's; coats: K coating.Coating or None; pol: the input
    state.  Only the alive slots enter (every one of them goes through mpmath: keep them few)."""
    table = np.asarray(table, dtype=float).reshape(-1, 4)
    alive = np.asarray(alive, dtype=bool)
    idx = np.nonzero(alive)[0]
    with np.errstate(invalid="ignore"):
        u = cc.source_u(dirs[0], axis)
    L = np.asarray(L, dtype=float)
    E = vt.amplitudes([[d[i] for d in dirs] for i in idx], coats, table[:, 0], pol, workers=workers)    # [alive, J, 3]
    out = []
    for j, (k, c, z, _) in enumerate(table):
        amp = E[:, j:j + 1, :] * np.exp(-(u[idx] * c))[:, None, None]
        with np.errstate(invalid="ignore"):
            path = L + z * u
        out.append(vt.field(P, V, path, alive, w, amp, [k], L_ref, C, normal, rot, x, y, shifts)[:, 0])
    return np.stack(out, axis=1)


def field_of(bundles, det, fdesc, axis, table, coats, pol, workers=None):
    """The truth for the history `bundles` (RayBundle objects, bundles[0] the source) on detector det, with the grid,
    planes and L_ref of the ArtFocalDesc fdesc."""
    d = det._desc()
    P, V, L, alive, w = fc.bundle_arrays(bundles[-1])
    dirs = [b.data[3:6, :b.n_slots].cpu().numpy().T for b in bundles]
    x = fdesc.x0 + np.arange(fdesc.nx) * fdesc.dx
    y = fdesc.y0 + np.arange(fdesc.ny) * fdesc.dy
    return field(P, V, L, alive, w, dirs, axis, table, coats, pol, fdesc.L_ref, np.array(d.centre[:]),
                 np.array(d.normal[:]), np.array(d.rot[:]), x, y, [fdesc.shift[q] for q in range(fdesc.planes)],
                 workers=workers)

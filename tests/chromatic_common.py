"""NumPy statement of the chromatic focal-field model of art_focal_chromatic (include/art_hip.h): per table row
(k_j, c_j, z_j, 0) the direct sum of tests/focal_common.py at k_j, with the optical path L + z_j u and the intensities
w exp(-2 u c_j), u = 1 - cos(angle between the ray's SOURCE direction and the axis).  The oracle of
tests/test_chromatic_host.py and tests/test_gpu_chromatic.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import focal_common as fc


def source_u(Dsrc, axis):
    """u_r = 0.5 ((s_x - a_x)^2 + (s_y - a_y)^2 + (s_z - a_z)^2), summed left to right: Dsrc (n, 3), axis a unit vector."""
    s = np.asarray(Dsrc, float) - np.asarray(axis, float)[None, :]
    return 0.5 * ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])


def field(P, D, path, alive, w, Dsrc, axis, table, L_ref, C, normal, rot, x, y, shifts):
    """complex128 [len(shifts), len(table), len(y), len(x)]; shifts along +normal (the ABI's convention).  Values in
    slots that are not alive (NaN included) never enter: focal_common selects the alive slots first.  The rows are
    independent sums, so a few threads take them side by side (NumPy releases the interpreter inside them)."""
    u = source_u(Dsrc, axis)
    w = np.ones(len(u)) if w is None else np.asarray(w, float)
    path = np.asarray(path, float)

    def one(row):
        k, c, z, _ = row
        with np.errstate(invalid="ignore"):
            return fc.field(P, D, path + z * u, alive, w * np.exp(-2 * u * c), k, L_ref, C, normal, rot, x, y, shifts)

    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack(list(pool.map(one, np.asarray(table, float))), axis=1)


def field_of(B, S, det, fdesc, axis, table):
    """The oracle's field for the bundle B at focus and its source bundle S on detector det, with the grid, planes and
    L_ref of the ArtFocalDesc fdesc."""
    d = det._desc()
    P, D, L, alive, w = fc.bundle_arrays(B)
    Dsrc = S.data[3:6, :S.n_slots].cpu().numpy().T
    x = fdesc.x0 + np.arange(fdesc.nx) * fdesc.dx
    y = fdesc.y0 + np.arange(fdesc.ny) * fdesc.dy
    return field(P, D, L, alive, w, Dsrc, axis, table, fdesc.L_ref, np.array(d.centre[:]), np.array(d.normal[:]),
                 np.array(d.rot[:]), x, y, [fdesc.shift[q] for q in range(fdesc.planes)])

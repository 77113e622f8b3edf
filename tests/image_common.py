"""NumPy statement of art_focal_image (include/art_hip.h): the partially coherent image is the sum over the groups of
|focal_common.field|^2 of each group's rays.  The oracle of tests/test_image_host.py and tests/test_gpu_image.py, with
the segment logic (ids -> offsets, the device's clamping) in plain NumPy."""
import numpy as np

import focal_common as fc


def seg_of_ids(ids):
    """Offsets (groups + 1) of the runs of equal values in the non-decreasing ids; ids absent from every slot (gaps) make
    no group.  [0] for no slot."""
    ids = np.asarray(ids)
    if len(ids) == 0:
        return np.zeros(1, dtype=np.int64)
    assert np.all(np.diff(ids) >= 0)
    starts = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]]))
    return np.concatenate([starts, [len(ids)]]).astype(np.int64)


def seg_of_sizes(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def ids_of_sizes(sizes, first=0, gap_after=None, gap=5):
    """One id per slot for groups of the given sizes: consecutive integers from `first`, with `gap` ids skipped after
    group gap_after."""
    ids, cur = [], first
    for g, s in enumerate(sizes):
        ids.append(np.full(s, cur, dtype=np.int64))
        cur += 1 + (gap if g == gap_after else 0)
    return np.concatenate(ids)


def clamped_ranges(seg, n):
    """The device's reading of any seg: every offset clamped to [0, n], seg[g + 1] <= seg[g] an empty group."""
    s = np.clip(np.asarray(seg, dtype=np.int64), 0, n)
    return [(int(a), int(b)) for a, b in zip(s[:-1], s[1:]) if b > a]


def image(P, D, path, alive, w, seg, k, L_ref, C, normal, rot, x, y, shifts):
    """float64 [len(shifts), len(y), len(x)]: sum over the groups [seg[g], seg[g+1]) (clamped) of |field|^2."""
    n = len(path)
    I = np.zeros((len(shifts), len(y), len(x)))
    for a, b in clamped_ranges(seg, n):
        sl = slice(a, b)
        E = fc.field(P[sl], D[sl], path[sl], alive[sl], None if w is None else w[sl], k, L_ref, C, normal, rot, x, y, shifts)
        I += np.abs(E) ** 2
    return I


def ideal_peak(alive, w, seg):
    """sum over the groups of (sum of sqrt(w) over the group's alive slots)^2."""
    amp = np.where(alive, 1.0 if w is None else np.sqrt(np.where(alive, w, 0.0)), 0.0) * np.ones(len(alive))
    return float(sum(amp[a:b].sum() ** 2 for a, b in clamped_ranges(seg, len(alive))))


def image_of(B, det, f, seg):
    """The oracle's image for bundle B on detector det with the grid and shifts of FocalImage f (Python shifts:
    shiftByDistance's sign, the ABI gets their negatives) and the offsets seg."""
    d = det._desc()
    P, D, L, alive, w = fc.bundle_arrays(B)
    return image(P, D, L, alive, w, seg, 2 * np.pi / f.wavelength, f.ref_path, np.array(d.centre[:]), np.array(d.normal[:]),
                 np.array(d.rot[:]), f.x, f.y, [-s for s in f.shifts])

"""Compensator sums restated in NumPy long double.  TEST INFRASTRUCTURE, written from the formulas (include/art_hip.h,
art_alignment_sums), on top of sensitivity_common.run: the chosen columns are rows of its per-ray arrays, the detector's
own column is the closed form dX_lab = nd - D / (nd.D), dL = -1 / (nd.D), and the table is summed directly about given
centres."""
import numpy as np

import sensitivity_common as sn
import tubes_common as tb

LD = tb.LD
ld = tb.ld
DOUBLES, MAX_DOFS, PILOT = 192, 8, 1024
CENTRES, MEANS, CROSS, PAIRS = 8, 32, 56, 80
DETECTOR = ("detector", "shift_normal")


def id_of(dof, K):
    """art_sensitivities' column id of (who, name); -1 for the detector."""
    who, name = dof
    if who == "detector":
        return -1
    if who == "source":
        return sn.SOURCE_DOFS.index(name)
    return sn.COLS * (who % K + 1) + sn.ELEMENT_DOFS.index(name)


def pair_index(a, b):
    return a * (2 * MAX_DOFS + 1 - a) // 2 + (b - a)


def detector_column(D, det, rot):
    """dX, dY, dL [n] of the detector shifted by Detector.shiftByDistance: centre' = centre - u normal."""
    nd, R = ld(det[1]), ld(rot)
    inD = 1 / (ld(D) @ nd)
    dxy = (nd[None, :] - ld(D) * inD[:, None]) @ R.T
    return dxy[:, 0], dxy[:, 1], -inD


def columns(ref, ids, D_last, det, rot):
    """[3, C, n] long double: dX, dY, dL of the chosen columns from sensitivity_common.run's result (NaN -> 0 where the ray
    does not count)."""
    out = np.zeros((3, len(ids), len(ref["alive"])), dtype=LD)
    for a, c in enumerate(ids):
        per = detector_column(D_last, det, rot) if c < 0 else (ref["dX"][c], ref["dY"][c], ref["dL"][c])
        for q in range(3):
            out[q, a] = np.where(ref["alive"], per[q], 0)
    return out


def pilot_centres(ref, cols, w):
    """The weighted means of the columns over the first min(n, PILOT) slots; zeros when no ray counts there."""
    a = ref["alive"].copy()
    a[PILOT:] = False
    wa = np.where(a, ld(w), 0)
    sw = wa.sum()
    return (cols * wa).sum(axis=2) / sw if sw > 0 else np.zeros(cols.shape[:2], dtype=LD)


def truth_table(ref, cols, w, centres):
    """The [192] block of art_alignment_sums in long double about `centres` [3, C]."""
    alive = ref["alive"]
    wa = np.where(alive, ld(w), 0)
    Q = [np.where(alive, ref[k], 0) for k in ("X", "Y", "L")]
    Cn = cols.shape[1]
    t = np.zeros(DOUBLES, dtype=LD)
    t[0], t[1] = alive.sum(), wa.sum()
    for q in range(3):
        t[2 + q], t[5 + q] = (wa * Q[q]).sum(), (wa * Q[q] * Q[q]).sum()
        d = np.where(alive[None, :], cols[q] - ld(centres)[q][:, None], 0)
        for a in range(Cn):
            t[CENTRES + 8 * q + a] = ld(centres)[q, a]
            t[MEANS + 8 * q + a] = (wa * d[a]).sum()
            t[CROSS + 8 * q + a] = (wa * Q[q] * d[a]).sum()
            for b in range(a, Cn):
                t[PAIRS + 36 * q + pair_index(a, b)] = (wa * d[a] * d[b]).sum()
    return t


def column_floor(cols, names, alive, span):
    """f [C]: what fp64 cannot know of a column per ray, 16 eps(fp64) x the size of the terms it is formed from: the
    components of unit vectors for a shift (1 mm per mm), a lever arm for a rotation (span[0], the distance to the detector,
    mm per rad), or the largest |dX|, |dY| or |dL| among the job's columns of the same unit where that is larger
    (sensitivity_common.compare_columns judges the per-ray values by that scale).  A column that vanishes by symmetry, a
    cylinder shifted along its axis, is rounding of that size in any arithmetic, the long-double restatement's included."""
    units = [n[1].startswith("shift") for n in names]
    eps = 16 * LD(np.finfo(np.float64).eps)
    big = lambda u: max([np.abs(cols[:, b][:, alive]).max() for b in range(len(names)) if units[b] == u and alive.any()] or [0])
    return [eps * max(big(u), LD(1) if u else LD(span[0])) for u in units]


def compare_table(got, ref_table, Cn, what, span, f=None, bar=tb.PARITY):
    """Every entry of the block against the long-double sums.  Scales by Cauchy-Schwarz: a pair entry against
    sqrt(S_aa S_bb), sum w Q d'Q_a against sqrt(sum w Q^2 . S_aa), sum w d'Q_a against sqrt(sum w . S_aa).  Row 0 and the
    floor of everything that holds X, Y or L are sensitivity_common.compare_table's: span = run()'s (distance to the
    detector, path), and no fp64 code knows X, Y, L better than FLOOR = 16 eps(fp64) x span.  f = column_floor(): the same
    for the columns.  A sum of products is allowed, beside the bar, each factor's floor times the rms of the other:
    sum w d'Q_a: sw f_a;  sum w Q d'Q_a: FLOOR sqrt(sw S_aa) + f_a sqrt(sw sum w Q^2) + sw FLOOR f_a;
    sum w d'Q_a d'Q_b: f_a sqrt(sw S_bb) + f_b sqrt(sw S_aa) + sw f_a f_b.  Returns the worst ratio to the bar's scale."""
    got, ref = ld(got), ld(ref_table)
    assert got.shape == ref.shape == (DOUBLES,), what
    assert got[0] == ref[0], what
    assert not got[PAIRS + 108:].any(), what
    worst = 0.0
    sw = ref[1]
    f = [0] * Cn if f is None else f
    floor = [16 * LD(np.finfo(np.float64).eps) * LD(v) for v in (span[0], span[0], span[1])]
    for q in range(1, 8):                                        # row 0, as sensitivity_common.compare_table
        if q == 1:
            scale, extra = np.abs(ref[q]), 0
        elif q < 5:
            scale, extra = np.sqrt(sw * ref[q + 3]), sw * floor[q - 2]
        else:
            scale, extra = np.abs(ref[q]), floor[q - 5] * (2 * np.sqrt(sw * ref[q]) + sw * floor[q - 5])
        err = np.abs(got[q] - ref[q])
        assert err <= bar * scale + extra, f"{what} row 0 [{q}]: {float(err):.3e} against {bar:g} of {float(scale):.3e} + {float(extra):.3e}"
        worst = max(worst, float(err / scale) if scale > 0 and err > extra else 0.0)
    for q in range(3):
        S = lambda a: ref[PAIRS + 36 * q + pair_index(a, a)]
        for a in range(MAX_DOFS):
            if a >= Cn:
                for base in (CENTRES, MEANS, CROSS):
                    assert got[base + 8 * q + a] == 0, (what, q, a)
                continue
            assert got[CENTRES + 8 * q + a] == ref[CENTRES + 8 * q + a], (what, "centre", q, a)
            cross = floor[q] * np.sqrt(sw * S(a)) + f[a] * np.sqrt(sw * ref[5 + q]) + sw * floor[q] * f[a]
            for base, other, extra in ((MEANS, sw, sw * f[a]), (CROSS, ref[5 + q], cross)):
                scale = np.sqrt(other * S(a))
                err = abs(got[base + 8 * q + a] - ref[base + 8 * q + a])
                assert err <= bar * scale + extra, \
                    f"{what} q {q} place {a} entry {base}: {float(err):.3e} against {bar:g} of {float(scale):.3e} + {float(extra):.3e}"
                worst = max(worst, float(err / scale) if scale > 0 and err > extra else 0.0)
        for a in range(MAX_DOFS):
            for b in range(a, MAX_DOFS):
                at = PAIRS + 36 * q + pair_index(a, b)
                if b >= Cn:
                    assert got[at] == 0, (what, q, a, b)
                    continue
                scale = np.sqrt(S(a) * S(b))
                extra = f[a] * np.sqrt(sw * S(b)) + f[b] * np.sqrt(sw * S(a)) + sw * f[a] * f[b]
                err = abs(got[at] - ref[at])
                assert err <= bar * scale + extra, \
                    f"{what} q {q} pair {a},{b}: {float(err):.3e} against {bar:g} of {float(scale):.3e} + {float(extra):.3e}"
                worst = max(worst, float(err / scale) if scale > 0 and err > extra else 0.0)
    return worst

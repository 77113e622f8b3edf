"""The definition of art_quantiles (include/art_hip.h) restated in NumPy: TEST INFRASTRUCTURE for tests/test_quantile_host.py
and tests/test_gpu_quantile.py, written from the header's comment and not from csrc/art_quantile.h.  No radix, no digits: a
stable sort, an integer cumsum, and the rule for T.

    q_i   = (int64) rint(ldexp(w_i, shift))        1 without weights; a negative q counts as 0
    W     = sum q_i over the valid slots           valid: alive and the key not NaN
    T     = min(W, max(1, ceil(f * float(W))))
    value = the smallest key v with sum_{key <= v} q >= T,  below = sum_{key < v} q,  upto = sum_{key <= v} q"""
import math

import numpy as np


def fixed_weights(w, shift, n):
    if w is None:
        return np.ones(n, dtype=np.int64)
    q = np.rint(np.ldexp(np.asarray(w, dtype=np.float64), int(shift))).astype(np.int64)
    return np.maximum(q, 0)


def target(W, f):
    W = int(W)
    return min(W, max(1, int(math.ceil(float(f) * float(W)))))


def select(keys, q, alive, fractions):
    """One plane: (values [K], below [K], upto [K], (W, valid, invalid)) of keys [n] with integer weights q [n]."""
    keys = np.asarray(keys, dtype=np.float64)
    alive = np.ones(len(keys), dtype=bool) if alive is None else np.asarray(alive).astype(bool)
    nan = np.isnan(keys)
    ok = alive & ~nan
    k = keys[ok] + 0.0                                  # (-0 + 0 = +0: the two zeros are one key)
    qq = np.asarray(q, dtype=np.int64)[ok]
    order = np.argsort(k, kind="stable")
    k, qq = k[order], qq[order]
    cum = np.cumsum(qq, dtype=np.int64)
    W = int(cum[-1]) if len(cum) else 0
    values, below, upto = [], [], []
    for f in fractions:
        T = target(W, f)
        if W == 0:
            values.append(np.nan); below.append(0); upto.append(0)
            continue
        j = int(np.searchsorted(cum, T, side="left"))   # the first slot at which the running sum reaches T
        v = k[j]
        lo, hi = np.searchsorted(k, v, side="left"), np.searchsorted(k, v, side="right")
        values.append(v)
        below.append(int(cum[lo - 1]) if lo > 0 else 0)
        upto.append(int(cum[hi - 1]))
    return (np.array(values, dtype=np.float64), np.array(below, dtype=np.int64), np.array(upto, dtype=np.int64),
            (W, int(ok.sum()), int((alive & nan).sum())))


def rank_sums(keys, q, alive, thresholds):
    """One plane: (sum q [key <= t], count [key <= t]) for every threshold t, over the valid slots."""
    keys = np.asarray(keys, dtype=np.float64)
    alive = np.ones(len(keys), dtype=bool) if alive is None else np.asarray(alive).astype(bool)
    ok = alive & ~np.isnan(keys)
    k, qq = keys[ok], np.asarray(q, dtype=np.int64)[ok]
    sums = np.array([int(qq[k <= t].sum()) for t in thresholds], dtype=np.int64)
    counts = np.array([int((k <= t).sum()) for t in thresholds], dtype=np.int64)
    return sums, counts


def restate(keys, w, alive, fractions, shift, thresholds=None):
    """All planes of keys [P, n]: a dict with the fields of quantile.Quantiles."""
    keys = np.atleast_2d(np.asarray(keys, dtype=np.float64))
    P, n = keys.shape
    q = fixed_weights(w, shift, n)
    per = [select(keys[p], q, alive, fractions) for p in range(P)]
    out = {"values": np.stack([r[0] for r in per]), "below": np.stack([r[1] for r in per]),
           "upto": np.stack([r[2] for r in per]), "totals": np.array([r[3] for r in per], dtype=np.int64).reshape(P, 3)}
    if thresholds is not None:
        th = np.asarray(thresholds, dtype=np.float64)
        th = np.tile(th, (P, 1)) if th.ndim == 1 else th
        rs = [rank_sums(keys[p], q, alive, th[p]) for p in range(P)]
        out["rank_sums"], out["rank_counts"] = np.stack([r[0] for r in rs]), np.stack([r[1] for r in rs])
    return out


def same_values(a, b):
    """Equal by bit pattern, except that the two zeros are equal and NaN equals NaN."""
    a, b = np.asarray(a, dtype=np.float64) + 0.0, np.asarray(b, dtype=np.float64) + 0.0
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def self_check():
    """Unit weights: the quantile is numpy's sorted array at index T - 1, the rank count numpy.searchsorted's."""
    rng = np.random.default_rng(5)
    k = np.round(rng.normal(size=1000), 2)               # with ties
    s = np.sort(k)
    fr = [0.0, 0.1, 0.5, 0.9, 1.0]
    v, below, upto, (W, valid, invalid) = select(k, np.ones(1000, dtype=np.int64), None, fr)
    assert (W, valid, invalid) == (1000, 1000, 0)
    for j, f in enumerate(fr):
        T = target(1000, f)
        assert v[j] == s[T - 1]
        assert below[j] == np.searchsorted(s, v[j], side="left") and upto[j] == np.searchsorted(s, v[j], side="right")
        assert below[j] < T <= upto[j]
    th = [-10.0, -0.5, 0.0, s[17], 10.0]
    sums, counts = rank_sums(k, np.ones(1000, dtype=np.int64), None, th)
    assert list(counts) == [int(np.searchsorted(s, t, side="right")) for t in th] and list(sums) == list(counts)


self_check()

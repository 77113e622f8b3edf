"""CPU (no GPU needed): the host side of art_quantiles -- argument errors raised before the device is touched, the result
classes built from the NumPy restatement's numbers, the rule for T at its edges, the order-preserving key map, the
descriptor's layout against the header and what the entry points refuse on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quantile_common as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import __graft_entry__ as g
    from attosecondraytracing_amd import _abi
    g.ensure_built()
    return _abi, C.CDLL(g.HIP_LIB)


def _detector():
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.zeros(3), np.array([0.0, 0.0, 10.0]), np.array([0.0, 0.0, -1.0]))


def test_argument_errors_come_before_the_device():
    import torch
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd import quantile
    det, rays = _detector(), object()          # (never looked at: every error below is raised first)
    for bad in ((-0.1,), (1.5,), (0.5, float("nan")), ()):
        with pytest.raises(ValueError, match="[Ff]raction"):
            det.get_EncircledEnergy(rays, Fractions=bad)
    with pytest.raises(ValueError, match="at most 16"):
        det.get_EncircledEnergy(rays, Fractions=np.linspace(0, 1, 17))
    for bad in ((2.0, 1.0), (-1.0, 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="Radii"):
            det.get_EncircledEnergy(rays, Radii=bad)
    with pytest.raises(ValueError, match="Metric"):
        det.get_EncircledEnergy(rays, Metric="R")
    with pytest.raises(ValueError, match="Shifts"):
        det.get_EncircledEnergy(rays, Shifts=[0.0, float("inf")])
    with pytest.raises(ValueError, match="Centre"):
        det.get_EncircledEnergy(rays, Centre=(0.0, 1.0, 2.0))
    with pytest.raises(TypeError, match="no centre and normal"):
        mdet.Detector(np.zeros(3)).get_EncircledEnergy(rays)
    keys = torch.arange(8, dtype=torch.float64)
    for w in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            quantile.weighted_quantiles(keys, [0.5], Weights=torch.tensor([1.0] * 7 + [w], dtype=torch.float64))
    with pytest.raises(ValueError, match="negative"):
        quantile.weighted_quantiles(keys, [0.5], Weights=torch.tensor([1.0] * 7 + [-1.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="sorted"):
        quantile.weighted_quantiles(keys, [0.5], Thresholds=[1.0, 0.0])
    with pytest.raises(ValueError, match="[Ff]raction"):
        quantile.weighted_quantiles(keys, [])
    with pytest.raises(ValueError, match="float64"):
        quantile.weighted_quantiles(keys.float(), [0.5])


def test_target_rule_at_its_edges():
    from attosecondraytracing_amd import quantile
    for W in (0, 1, 2, 7, 1000, 2 ** 53 + 1, 2 ** 61):
        for f in (0.0, 1.0, 0.5, 1e-30, 0.1, 1.0 - 2.0 ** -53):
            assert quantile.target(W, f) == qc.target(W, f)
    assert qc.target(0, 0.0) == 0 and qc.target(0, 1.0) == 0                # no weight: no target, the value is NaN
    assert qc.target(1000, 0.0) == 1 and qc.target(1000, 1.0) == 1000      # f = 0: the smallest key with weight; f = 1: the largest
    assert qc.target(7, 0.5) == 4 and qc.target(2, 0.5) == 1
    # W = 2^53 + 1 is not a double: float(W) rounds to 2^53 (half to even), and T must not exceed W
    W = 2 ** 53 + 1
    assert qc.target(W, 1.0) == 2 ** 53 and qc.target(W, 0.0) == 1 and qc.target(W, 0.5) == 2 ** 52


def test_key_map_preserves_the_order():
    from attosecondraytracing_amd import quantile
    tiny = np.finfo(np.float64).tiny
    v = np.array([-np.inf, -1e308, -2.0, -1.0 - 2.0 ** -52, -1.0, -tiny, -5e-324, -0.0, 0.0, 5e-324, tiny, 1.0,
                  1.0 + 2.0 ** -52, 2.0, 1e308, np.inf])
    b = quantile.key_bits(v)
    assert b.dtype == np.uint64
    d = np.diff(b.astype(object))
    assert all(x > 0 for i, x in enumerate(d) if not (v[i] == 0 and v[i + 1] == 0)), d
    assert b[7] == b[8] == 1 << 63                                          # the two zeros are one key
    assert b[0] == (1 << 52) - 1 and b[-1] == (0xFFF << 52)                 # the infinities are ordinary keys at the ends
    rng = np.random.default_rng(1)
    r = rng.normal(size=4000) * 10.0 ** rng.integers(-300, 300, size=4000)
    assert np.array_equal(np.argsort(quantile.key_bits(r), kind="stable"), np.argsort(r, kind="stable"))


def test_result_classes_from_the_restatement():
    from attosecondraytracing_amd import quantile
    rng = np.random.default_rng(2)
    n, shift = 500, 40
    x, y = rng.normal(size=n) * 1e-3, rng.normal(size=n) * 2e-3
    w = rng.uniform(0.5, 1.5, size=n)
    fr = [0.5, 0.8, 0.9]
    planes = np.stack([np.hypot(x, y), np.hypot(2 * x, y)])                 # "radii" in two planes
    radii = np.linspace(0.0, 8e-3, 17)
    r = qc.restate(planes, w, None, fr, shift, radii)
    q = quantile.Quantiles(r["values"], r["below"], r["upto"], r["totals"], shift, fr, np.tile(radii, (2, 1)),
                           r["rank_sums"], r["rank_counts"])
    assert q.values.shape == (2, 3) and q.total.shape == (2,) and list(q.count) == [n, n] and list(q.invalid) == [0, 0]
    assert np.all(q.below < q.targets) and np.all(q.targets <= q.upto)
    assert np.allclose(q.weight, w.sum(), rtol=1e-9)
    centres = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 0.0, 0.0]])
    e = quantile.EncircledEnergy(q, centres, [0.0, 0.5], "radius", radii)
    assert e.radii is q.values and np.array_equal(e.centre, [[0.0, 0.0], [1.0, 2.0]])
    assert np.array_equal(e.hew, 2 * q.values[:, 0]) and e.best_focus == 0.0
    assert e.enclosed.shape == (2, 17) and np.all(np.diff(e.enclosed, axis=1) >= 0) and e.enclosed[0, -1] <= 1.0
    assert np.array_equal(e.enclosed, r["rank_sums"] / r["totals"][:, :1])
    for p in range(2):                                                      # the curve reaches f at the f-radius
        for k, f in enumerate(fr):
            inside = int(qc.fixed_weights(w, shift, n)[planes[p] <= q.values[p, k]].sum())
            assert inside == q.upto[p, k] and inside >= f * q.total[p] - 1
    assert quantile.EncircledEnergy(quantile.Quantiles(r["values"], r["below"], r["upto"], r["totals"], shift, [0.4, 0.8, 0.9]),
                                    centres, [0.0, 0.5], "X").hew is None
    empty = qc.restate(np.full((1, 4), np.nan), None, None, [0.5], 0)
    assert np.isnan(empty["values"]).all() and list(empty["totals"][0]) == [0, 0, 4]
    e0 = quantile.EncircledEnergy(quantile.Quantiles(empty["values"], empty["below"], empty["upto"], empty["totals"], 0, [0.5]),
                                  np.full((1, 4), np.nan), [0.0], "radius")
    assert e0.best_focus is None and np.isnan(e0.hew).all() and e0.count[0] == 0


def test_descriptor_matches_the_header(tmp_path):
    _abi, lib = _lib()
    fields = [n for n, _ in _abi.ArtQuantileDesc._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "art_hip.h"\nint main(void) {\n  printf("%zu", sizeof(struct ArtQuantileDesc));\n'
           + "".join(f'  printf(" %zu", offsetof(struct ArtQuantileDesc, {n}));\n' for n in fields)
           + '  printf(" %d %d %d %d %d %d %d %d %lld %d\\n", ART_QKEY_GIVEN, ART_QKEY_RADIUS, ART_QKEY_X, ART_QKEY_Y, '
             'ART_QKEY_DELAY, ART_QUANTILE_MAX_FRACTIONS, ART_QUANTILE_MAX_THRESHOLDS, ART_FOCAL_MAX_PLANES, '
             '(long long)ART_QUANTILE_SCRATCH_DEFAULT, ART_ABI_VERSION);\n  return 0;\n}\n')
    c, exe = tmp_path / "t.c", tmp_path / "t"
    c.write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _abi.ArtQuantileDesc
    assert vals == [C.sizeof(D)] + [getattr(D, n).offset for n in fields] + [
        _abi.ART_QKEY_GIVEN, _abi.ART_QKEY_RADIUS, _abi.ART_QKEY_X, _abi.ART_QKEY_Y, _abi.ART_QKEY_DELAY,
        _abi.ART_QUANTILE_MAX_FRACTIONS, _abi.ART_QUANTILE_MAX_THRESHOLDS, _abi.ART_FOCAL_MAX_PLANES,
        _abi.ART_QUANTILE_SCRATCH_DEFAULT, _abi.ART_ABI_VERSION]
    assert _abi.ART_ABI_VERSION == 14
    for name in ("art_quantiles", "art_quantile_scratch_doubles"):
        assert hasattr(lib, name) and name in _abi.PROTOTYPES


def test_entry_points_refuse_on_the_host_what_they_can():
    """Argument validation comes before any device work: these calls return without touching a GPU."""
    _abi, lib = _lib()
    fn = _abi.bind(lib)
    sd, run = fn["art_quantile_scratch_doubles"], fn["art_quantiles"]
    th = (C.c_double * 4)(0.0, 1.0, 1.0, float("inf"))

    def desc(**kw):
        d = _abi.ArtQuantileDesc()
        d.key, d.planes, d.n_fractions, d.keys = _abi.ART_QKEY_GIVEN, 2, 3, 8
        d.fraction[0], d.fraction[1], d.fraction[2] = 0.5, 0.0, 1.0
        d.values = d.below = d.upto = d.totals = 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    n = 1000
    state = 2 * 3 * 5 + 2 * 2 + 4 * 2                                       # 5 words per (plane, fraction), counts, centres
    assert sd(desc(), n) == state + 2 * 3 * 2048 + 2 * 2                    # given keys: bins only, both planes in one block
    assert sd(desc(n_thresholds=2), n) == state + 2 * 3 * 2048 + 2 * 2 * 3
    assert sd(desc(scratch_bound=1), n) == state + 3 * 2048 + 2             # one plane per block whatever the bound
    metric = dict(key=_abi.ART_QKEY_RADIUS)
    det = _abi.ArtDetectorDesc()
    det.normal[:] = [0.0, 0.6, 0.8]
    assert sd(desc(det=det, **metric), n) == state + 2 * 1024 * 5 + 2 * (3 * 2048 + 2 + n)     # + partial sums + staged keys
    for bad in (dict(key=5), dict(key=-1), dict(planes=0), dict(planes=65), dict(n_fractions=0), dict(n_fractions=17),
                dict(n_thresholds=-1), dict(n_thresholds=257), dict(wshift=1075), dict(wshift=-1075), dict(scratch_bound=-1)):
        assert sd(desc(**bad), n) == _abi.ART_ERR_BAD_ARG, bad
        assert run(desc(**bad), None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG, bad
    assert sd(None, n) == _abi.ART_ERR_BAD_ARG and sd(desc(), -1) == _abi.ART_ERR_BAD_ARG
    assert sd(desc(), (1 << 28) + 1) == _abi.ART_ERR_UNSUPPORTED
    assert run(desc(), None, None, n, None, None) == _abi.ART_ERR_BAD_ARG                     # no scratch
    for out in ("values", "below", "upto", "totals", "keys"):
        assert run(desc(**{out: None}), None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG, out
    d = desc()
    d.fraction[1] = 1.5
    assert run(d, None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG and b"fraction" in fn["art_last_error"]()
    d.fraction[1] = float("nan")
    assert run(d, None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG
    ranks = dict(n_thresholds=2, thresholds_dev=8, thresholds_host=C.addressof(th), rank_sums=8, rank_counts=8)
    for missing in ("thresholds_dev", "thresholds_host", "rank_sums", "rank_counts"):
        assert run(desc(**dict(ranks, **{missing: None})), None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG, missing
    unsorted = (C.c_double * 4)(0.0, 1.0, 1.0, 0.5)
    assert run(desc(**dict(ranks, thresholds_host=C.addressof(unsorted))), None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG
    assert b"sorted" in fn["art_last_error"]()
    nan = (C.c_double * 4)(0.0, float("nan"), 1.0, 2.0)
    assert run(desc(**dict(ranks, thresholds_host=C.addressof(nan))), None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG
    # detector metrics: a bundle view, a unit normal, finite shifts and centres
    assert run(desc(det=det, **metric), None, None, n, 8, None) == _abi.ART_ERR_BAD_ARG      # no view
    view = _abi.ArtBundleView(*([8] * 9))
    bad_det = _abi.ArtDetectorDesc()
    bad_det.normal[:] = [0.0, 0.0, 2.0]
    assert run(desc(det=bad_det, **metric), C.byref(view), None, n, 8, None) == _abi.ART_ERR_BAD_ARG
    d = desc(det=det, **metric)
    d.shift[1] = float("inf")
    assert run(d, C.byref(view), None, n, 8, None) == _abi.ART_ERR_BAD_ARG
    d = desc(det=det, centre_given=1, **metric)
    d.centre[1][0] = float("nan")
    assert run(d, C.byref(view), None, n, 8, None) == _abi.ART_ERR_BAD_ARG

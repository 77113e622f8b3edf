"""CPU: the Python layer of the device histogram (attosecondraytracing_amd/histogram.py, Detector.get_Histogram,
OpticalChain.get_Footprint) against a NumPy stand-in for art_histogram on top of the CPU twin backend, and the
ArtHistogramDesc layout against include/art_hip.h."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from attosecondraytracing_amd import _abi
from twin_backend import TwinBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(ptr, n, ty=C.c_double):
    return np.ctypeslib.as_array((ty * n).from_address(ptr)) if n else np.zeros(0)


class NumpyHistBackend(TwinBackend):
    """art_histogram's contract in NumPy: coordinates from the twin's detector read-out or the frame map, bins by
    numpy.histogramdd, weights quantised with rint(ldexp(w, S))."""

    def histogram(self, hdesc, view, w, n, out=None, shift=None):
        from attosecondraytracing_amd import histogram as hist
        if shift is None:
            shift = hist.weight_shift(n, None if w is None else w[:n])
        hdesc.wshift = shift
        ndim = hdesc.ndim
        bins = [hdesc.bins[k] for k in range(ndim)]
        alive = _host(view.alive, n, C.c_uint8).astype(bool) if n else np.zeros(0, dtype=bool)
        if hdesc.source == _abi.ART_HIST_DETECTOR:
            X, Y, O = self.empty(n), self.empty(n), self.empty(n)
            if n:
                self.detector(hdesc.map, view, n, XY=(X, Y), opl=O)
            v = {0: X.numpy(), 1: Y.numpy(), 3: (O.numpy() - hdesc.delay_centre) / 299792458000.0 * 1e15}
        else:
            P = np.stack([_host(p, n) for p in (view.ox, view.oy, view.oz)], axis=1) if n else np.zeros((0, 3))
            R = (P - np.array(hdesc.map.centre[:])) @ np.array(hdesc.map.rot[:]).reshape(3, 3).T
            v = {k: R[:, k] for k in range(3)}
        sample = np.stack([v[hdesc.axis[k]] for k in range(ndim)], axis=1)[alive]
        edges = [np.linspace(hdesc.lo[k], hdesc.hi[k], bins[k] + 1) for k in range(ndim)]
        counts = np.histogramdd(sample, bins=edges)[0].astype(np.int64)
        inside = np.ones(len(sample), dtype=bool)
        for k in range(ndim):
            inside &= (sample[:, k] >= edges[k][0]) & (sample[:, k] <= edges[k][-1])
        wsums = None
        q = np.zeros(len(sample), dtype=np.int64)
        if w is not None:
            q = np.rint(np.ldexp(w[:n].numpy()[alive], shift)).astype(np.int64)
            wsums = np.zeros(bins, dtype=np.int64)
            idx = [np.clip(np.searchsorted(edges[k], sample[inside, k], side="right") - 1, 0, bins[k] - 1)
                   for k in range(ndim)]
            np.add.at(wsums, tuple(idx), q[inside])
            wsums = torch.from_numpy(wsums.reshape(-1))
        totals = torch.tensor([inside.sum(), (~inside).sum(), q[inside].sum(), q[~inside].sum()], dtype=torch.int64)
        return torch.from_numpy(counts.reshape(-1)), wsums, totals, shift


@pytest.fixture(scope="module")
def twin():
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = NumpyHistBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def _bundle(points, intensity=None, backend=None, vectors=None):
    from attosecondraytracing_amd.bundle import RayBundle
    P = np.asarray(points, dtype=float)
    V = np.tile([0.0, 0.0, 1.0], (len(P), 1)) if vectors is None else vectors
    return RayBundle.from_arrays(P, V, intensity=intensity, backend=backend)


def _detector():
    import ART.ModuleDetector as mdet
    return mdet.Detector(np.zeros(3), np.array([0.0, 0.0, 10.0]), np.array([0.0, 0.0, 1.0]))


def test_default_ranges_are_the_alive_min_max(twin):
    rng = np.random.default_rng(0)
    P = np.column_stack([rng.normal(0, 1, 500), rng.normal(2, 0.5, 500), np.zeros(500)])
    D = _detector()
    V = np.column_stack([rng.normal(0, 0.05, 500), rng.normal(0, 0.05, 500), np.ones(500)])
    B = _bundle(P, rng.uniform(0.5, 1.5, 500), twin, V)
    XY = D.get_PointList2D(B)
    h = D.get_Histogram(B, ("X", "Y"), 20)
    assert h.edges[0][0] == XY[:, 0].min() and h.edges[0][-1] == XY[:, 0].max()
    assert h.edges[1][0] == XY[:, 1].min() and h.edges[1][-1] == XY[:, 1].max()
    assert np.array_equal(h.counts, np.histogramdd(XY, bins=h.edges)[0])
    assert h.outside[0] == 0 and h.counts.sum() == 500
    d = D.get_Delays(B)
    hd = D.get_Histogram(B, "Delay", 7)
    assert hd.edges[0][0] == d.min() and hd.edges[0][-1] == d.max()


def test_a_degenerate_axis_is_widened_like_numpys(twin):
    P = np.column_stack([np.linspace(-1, 1, 50), np.full(50, 0.25), np.zeros(50)])
    D = _detector()
    h = D.get_Histogram(_bundle(P, backend=twin), ("X", "Y"), 5)
    y = D.get_PointList2D(_bundle(P, backend=twin))[0, 1]
    assert h.edges[1][0] == y - 0.5 and h.edges[1][-1] == y + 0.5
    assert np.array_equal(h.edges[1], np.histogram_bin_edges(np.full(3, y), bins=5))


def test_per_axis_bins_and_ranges(twin):
    rng = np.random.default_rng(1)
    P = np.column_stack([rng.uniform(-1, 1, 300), rng.uniform(-2, 2, 300), np.zeros(300)])
    D = _detector()
    B = _bundle(P, backend=twin)
    h = D.get_Histogram(B, ("X", "Y"), Bins=(8, 3), Range=[(-0.5, 0.5), (-1.0, 3.0)])
    assert h.counts.shape == (8, 3)
    assert np.array_equal(h.edges[0], np.linspace(-0.5, 0.5, 9)) and np.array_equal(h.edges[1], np.linspace(-1, 3, 4))
    XY = D.get_PointList2D(B)
    assert np.array_equal(h.counts, np.histogramdd(XY, bins=h.edges)[0])
    assert h.outside[0] == 300 - h.counts.sum() and h.outside[1] is None
    with pytest.raises(ValueError):
        D.get_Histogram(B, ("X", "Y"), Bins=(8, 3, 2))
    with pytest.raises(ValueError):
        D.get_Histogram(B, ("X",), Bins=0)
    with pytest.raises(ValueError):
        D.get_Histogram(B, ("X",), Range=[(1.0, 0.0)])
    with pytest.raises(ValueError):
        D.get_Histogram(B, ("X", "Z"))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000, 10 ** 7, 2 ** 40])
@pytest.mark.parametrize("wmax", [1e-300, 0.3, 1.0, 1.5, 2.0, 1e6])
def test_shift_choice_and_its_overflow_bound(n, wmax):
    from attosecondraytracing_amd.histogram import shift_for
    S = shift_for(n, wmax)
    E = math.frexp(wmax)[1]
    assert wmax < 2.0 ** E
    assert S == 62 - math.ceil(math.log2(n + 1)) - E
    # n weights of at most wmax: each |q| <= 2^(S+E), the sum stays below 2^62
    assert n * 2 ** (S + E) < 2 ** 62
    assert shift_for(n, 0.0) == 1074


def test_weighted_sums_and_shift(twin):
    from attosecondraytracing_amd.histogram import shift_for
    rng = np.random.default_rng(2)
    P = np.column_stack([rng.normal(0, 1, 400), rng.normal(0, 1, 400), np.zeros(400)])
    w = rng.uniform(0.0, 3.0, 400)
    D = _detector()
    h = D.get_Histogram(_bundle(P, w, twin), ("X",), 16)
    assert h.shift == shift_for(400, w.max())
    XY = D.get_PointList2D(_bundle(P, w, twin))
    ref = np.histogram(XY[:, 0], bins=h.edges[0], weights=w)[0]
    assert np.all(np.abs(h.intensity - ref) <= h.counts * 2.0 ** -(h.shift + 1) + 1e-12 * ref)


def test_non_finite_intensities_are_refused(twin):
    P = np.zeros((10, 3))
    w = np.ones(10)
    w[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        _detector().get_Histogram(_bundle(P, w, twin), ("X",), 4)
    w[3] = np.inf
    with pytest.raises(ValueError, match="finite"):
        _detector().get_Histogram(_bundle(P, w, twin), ("X",), 4)


def test_without_intensities_there_is_no_intensity(twin):
    h = _detector().get_Histogram(_bundle(np.zeros((10, 3)), None, twin), ("X", "Y"), 4)
    assert h.intensity is None and h.wsums is None and h.outside == (0, None)
    assert h.counts.sum() == 10


def test_footprint_bins_the_support_frame(twin):
    import ART.ModuleGeometry as mgeo
    import test_plots as tp
    sc = tp.build_plot_scene()
    chain = sc["chain"]
    oe = chain.optical_elements[2]
    h = chain.get_Footprint(2, Bins=(10, 6))
    half = np.asarray(oe.type.support._CircumRect(), dtype=float) / 2
    assert np.array_equal(h.edges[0], np.linspace(-half[0], half[0], 11))
    P = chain.get_output_rays()[2].points()
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    xy = (P - np.asarray(oe.position, dtype=float)) @ fwd.T
    assert np.abs(h.counts - np.histogramdd(xy[:, :2], bins=h.edges)[0]).sum() <= 2


def test_histogram_desc_layout_matches_header():
    import subprocess
    import tempfile
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "art_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\n", sizeof(ArtHistogramDesc),
         offsetof(ArtHistogramDesc, ndim), offsetof(ArtHistogramDesc, axis), offsetof(ArtHistogramDesc, bins),
         offsetof(ArtHistogramDesc, wshift), offsetof(ArtHistogramDesc, lo), offsetof(ArtHistogramDesc, hi),
         offsetof(ArtHistogramDesc, delay_centre), offsetof(ArtHistogramDesc, map), ART_HIST_DETECTOR,
         ART_HIST_FRAME, ART_HAXIS_X, ART_HAXIS_Y, ART_HAXIS_DELAY, ART_HIST_MAX_BINS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, c])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    H = _abi.ArtHistogramDesc
    assert vals == [C.sizeof(H), H.ndim.offset, H.axis.offset, H.bins.offset, H.wshift.offset, H.lo.offset,
                    H.hi.offset, H.delay_centre.offset, H.map.offset, _abi.ART_HIST_DETECTOR, _abi.ART_HIST_FRAME,
                    _abi.ART_HAXIS_X, _abi.ART_HAXIS_Y, _abi.ART_HAXIS_DELAY, _abi.ART_HIST_MAX_BINS]
    hdr = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    assert "#define ART_ABI_VERSION %d" % _abi.ART_ABI_VERSION in hdr

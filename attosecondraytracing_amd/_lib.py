"""Loader of libart_hip.so -- the only compute backend of this package.

There is NO CPU fallback: if the shared library was not built (`python -c "import __graft_entry__ as g;
g.build()"`), or no gfx950 device is visible, the first attempt to trace rays raises RuntimeError.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library, in-tree.  No environment variable redirects the loader: a diagnostic BUILD is loaded by handing its
# path to HipBackend(path=...) explicitly (tools/ab_kernel.py does), never by the process-wide get_backend().
LIB_PATH = os.path.join(_HERE, "libart_hip.so")

_BACKEND = None


class ArtError(RuntimeError):
    pass


class HipBackend:
    """Thin typed wrapper: torch tensors in, C-ABI calls out.  All calls are asynchronous on torch's
    current HIP stream of the bundle's device.  Stream-safe like the C ABI underneath: every piece of scratch memory and
    every staging pair the wrapper reuses between calls is kept PER STREAM (keyed by the current stream's handle), so two
    torch streams may issue read-outs, compactions, scene launches and analyses concurrently."""

    name = "hip"

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} not found: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no CPU fallback.")
        self.lib = C.CDLL(path)
        self.fn = _abi.bind(self.lib)
        v = self.fn["art_abi_version"]()
        if v != _abi.ART_ABI_VERSION:
            raise RuntimeError(f"libart_hip.so ABI version {v} != expected {_abi.ART_ABI_VERSION}: rebuild it")
        if not torch.cuda.is_available():
            raise RuntimeError("No HIP device visible to PyTorch: ray tracing needs an MI355X (gfx950). "
                               "There is no CPU fallback.")
        n = self.fn["art_device_count"]()
        if n <= 0:
            raise RuntimeError("libart_hip.so found no gfx950 device (art_device_count() = %d: %s)"
                               % (n, self.last_error()))
        self.device = torch.device("cuda", torch.cuda.current_device())
        self._scratch = {}
        self._side_streams = {}
        self._scene_pool, self._scene_uploads = {}, {}
        self._job_pool = {}
        # bookkeeping for measurements: launches of the fused kernels over at least `count_from` slots, in issue order
        # (bench.py reports which of them lie inside its timed region, so that a kernel trace can be cut to it)
        self.count_from, self.counted_launches = None, 0
        self.trace_events = None   # set to a list to collect (start, end) HIP events around each trace launch
        self.readout_events = None  # likewise around each fused read-out (kernel + final fold)

    # ------------------------------------------------------------------ helpers
    def last_error(self):
        return self.fn["art_last_error"]().decode("utf-8", "replace")

    def check(self, rc, what):
        if rc != 0:
            raise ArtError(f"{what} failed with code {rc}: {self.last_error()}")

    def stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        torch.cuda.current_stream(self.device).synchronize()

    def empty(self, n, dtype=torch.float64):
        return torch.empty(int(n), dtype=dtype, device=self.device)

    def zeros(self, n, dtype=torch.float64):
        return torch.zeros(int(n), dtype=dtype, device=self.device)

    def from_numpy(self, a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device)

    def stream_key(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def side_stream_context(self, name):
        """`with be.side_stream_context(name):` -- torch's current stream becomes a stream of this backend's own (one per
        name) that has NOT waited for the caller's stream: for small latency-critical work (the alignment rays of a
        placement) whose read-backs must not queue behind bulk kernels.  Tensors created inside belong to that stream."""
        st = self._side_streams.get(name)
        if st is None:
            st = self._side_streams[name] = torch.cuda.Stream(device=self.device)
        return torch.cuda.stream(st)

    def scratch(self, key, n, dtype):
        """Reused scratch memory `key` of the CURRENT stream (work of one stream is ordered, so one area per stream and
        purpose is enough; two streams never share one)."""
        key = (key, self.stream_key())
        t = self._scratch.get(key)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = torch.empty(int(max(n, 1)), dtype=dtype, device=self.device)
            self._scratch[key] = t
        return t

    def _scratch_for(self, key, fn_name, *args):
        """The scratch area `key` of the current stream, sized by the library's `fn_name`(*args)."""
        ns = self.fn[fn_name](*args)
        if ns < 0:
            raise ArtError(f"{fn_name} failed with code {ns}: {self.last_error()}")
        return self.scratch(key, ns, torch.float64)

    @staticmethod
    def _ptr(t, n):
        """The device pointer of the optional per-slot tensor t (mostly the weights): NULL without it or without slots."""
        return None if (t is None or n == 0) else t.data_ptr()

    @staticmethod
    def _chromatic_table(table):
        """`table` as the contiguous float64 host array [nk, 4] of rows (k_j, c_j, z_j, 0) that the chromatic calls take."""
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 4:
            raise ValueError("the chromatic table must have rows (k_j, c_j, z_j, 0)")
        return table

    @staticmethod
    def _quadric_desc(coefficients):
        """The ArtQuadricDesc of ten coefficients (q[6], b[3], c: include/art_hip.h)."""
        q = _abi.ArtQuadricDesc()
        co = [float(v) for v in coefficients]
        q.q[:], q.b[:], q.c = co[0:6], co[6:9], co[9]
        return q

    # ------------------------------------------------------------------ entry points
    def _timed(self, call, sink="trace_events"):
        """Run one launch; when the sink list is set, bracket it with HIP events recorded on the launch stream."""
        events = getattr(self, sink)
        if events is None:
            return call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call()
        e1.record()
        events.append((e0, e1))
        return rc

    def trace_element(self, desc, view_in, view_out, n):
        sp = self.stream_ptr()
        self.check(self._timed(lambda: self.fn["art_trace_element"](C.byref(desc), C.byref(view_in),
                                                                    C.byref(view_out), n, sp)), "art_trace_element")

    def trace_grating(self, desc, q, lines_per_mm, order, wavelengths, view_in, views_out, n, grooves_in=None,
                      grooves_out=None):
        """art_trace_grating: `desc` (an ArtElementDesc with ART_FLAG_GRATING) diffracts the bundle `view_in` into one
        bundle per wavelength (mm) in ONE launch.  grooves_in: device tensor [n] or None; grooves_out: device tensor
        [len(wavelengths), n] (contiguous) or None."""
        nw = len(wavelengths)
        wl_host = (C.c_double * nw)(*[float(w) for w in wavelengths])
        varr = (_abi.ArtBundleView * nw)(*views_out)
        wl_dev = self.from_numpy(np.array([float(w) for w in wavelengths], dtype=np.float64))
        v_dev = self.from_numpy(np.frombuffer(bytes(varr), dtype=np.uint8).copy())
        g = _abi.ArtGratingDesc()
        g.q[0], g.q[1] = float(q[0]), float(q[1])
        g.lines_per_mm, g.order, g.nw = float(lines_per_mm), int(order), nw
        g.wavelengths, g.outs = wl_dev.data_ptr(), v_dev.data_ptr()
        g.grooves_in = None if grooves_in is None else grooves_in.data_ptr()
        g.grooves_out = None if grooves_out is None else grooves_out.data_ptr()
        sp = self.stream_ptr()
        self.check(self._timed(lambda: self.fn["art_trace_grating"](C.byref(desc), C.byref(g), wl_host, varr,
                                                                    C.byref(view_in), n, sp)), "art_trace_grating")
        return wl_dev, v_dev          # (read by the launch: the caller keeps them alive with the outputs)

    def trace_quadric(self, desc, coefficients, view_in, view_out, n):
        """art_trace_quadric: `desc` (an ArtElementDesc with ART_FLAG_QUADRIC) reflects the bundle `view_in` off the quadric
        whose ten coefficients (q[6], b[3], c: include/art_hip.h) are `coefficients`."""
        q = self._quadric_desc(coefficients)
        sp = self.stream_ptr()
        self.check(self._timed(lambda: self.fn["art_trace_quadric"](C.byref(desc), C.byref(q), C.byref(view_in),
                                                                    C.byref(view_out), n, sp)), "art_trace_quadric")

    def trace_freeform(self, desc, coefficients, figure, view_in, view_out, n):
        """art_trace_freeform: `desc` (an ArtElementDesc with ART_FLAG_FREEFORM) reflects the bundle `view_in` off the base
        quadric `coefficients` (q[6], b[3], c) carrying the figure `figure` = (device tensor of ART_ZERN_STRIDE doubles in
        the dense layout, radius, order): include/art_hip.h."""
        q = self._quadric_desc(coefficients)
        table, radius, order = figure
        if table.numel() < _abi.ART_ZERN_STRIDE:
            raise ValueError("trace_freeform: the figure table must hold ART_ZERN_STRIDE doubles")
        f = _abi.ArtFigureDesc(table.data_ptr(), float(radius), int(order), 0)
        sp = self.stream_ptr()
        self.check(self._timed(lambda: self.fn["art_trace_freeform"](C.byref(desc), C.byref(q), C.byref(f), C.byref(view_in),
                                                                     C.byref(view_out), n, sp)), "art_trace_freeform")

    def trace_chain(self, descs, view_in, views_out, n, readout=None):
        """art_trace_chain, or art_trace_chain_readout when `readout` (from new_chain_readout) is given."""
        m = len(descs)
        if m > 1 or readout is not None:       # (a one-element chain without read-out is the per-element kernel's)
            self.note_launches(n, -(-m // 8))
        darr = (_abi.ArtElementDesc * m)(*descs)
        varr = (_abi.ArtBundleView * m)(*views_out)
        sp = self.stream_ptr()
        if readout is None:
            self.check(self._timed(lambda: self.fn["art_trace_chain"](darr, m, C.byref(view_in), varr, n, sp)),
                       "art_trace_chain")
        else:
            ro = readout["struct"]
            self.check(self._timed(lambda: self.fn["art_trace_chain_readout"](darr, m, C.byref(view_in), varr,
                                                                              C.byref(ro), n, sp)),
                       "art_trace_chain_readout")

    MAX_FUSED_READOUT_RAYS = 1 << 28     # one launch (art_trace_chain_readout)

    def new_chain_readout(self, ddesc, w, n, centres=(0.0, 0.0, 0.0), store=True, scratch=None, lite=False, targets=None):
        """Outputs + descriptor of a read-out fused behind a chain launch (ArtChainReadout): returns a dict with the
        result tensors 'X', 'Y', 'opl' (None with store=False), 'stats_dev' and the ctypes 'struct'.  lite=True: only
        count, sum of paths, bounding box and path range are reduced (ArtChainReadout.lite).  targets=(X, Y, opl): the
        read-out writes into these caller-owned tensors (e.g. the sections of a survivor send buffer: zero-copy gather)."""
        X = Y = opl = None
        if targets is not None:
            X, Y, opl = targets
            assert all(t.numel() >= n and t.dtype == torch.float64 and t.is_contiguous() for t in (X, Y, opl))
            store = True
        elif store:
            X, Y, opl = self.empty(n), self.empty(n), self.empty(n)
        out = self.empty(24)
        if scratch is None:
            scratch = self.scratch("chain_ro", self.fn["art_chain_readout_scratch_doubles"](n), torch.float64)
        ro = _abi.ArtChainReadout()
        ro.det = ddesc
        ro.w = None if w is None else w.data_ptr()
        ro.cx, ro.cy, ro.co = (float(v) for v in centres)
        ro.X, ro.Y, ro.opl = (None, None, None) if not store else (X.data_ptr(), Y.data_ptr(), opl.data_ptr())
        ro.scratch, ro.out24 = scratch.data_ptr(), out.data_ptr()
        ro.lite = 1 if lite else 0
        ro.sums = 0
        return {"struct": ro, "X": X, "Y": Y, "opl": opl, "P3": None, "stats_dev": out, "_keep": (w, scratch), "lite": bool(lite)}

    def new_chain_sums(self, w, n, scratch=None):
        """Descriptor of the SUMS tail (ArtChainReadout.sums): the tracing launch forms pass (1) of the analysis for the
        chain's last bundle -- count, sum point, sum vector, sum w, sum path in 'sums_dev'[0..8] -- while the ray is still
        in registers.  Hand 'sums_dev' to the analysis of that bundle (analysis.analyse does, through the bundle)."""
        out = self.empty(24)
        if scratch is None:
            scratch = self.scratch("chain_ro", self.fn["art_chain_readout_scratch_doubles"](n), torch.float64)
        ro = _abi.ArtChainReadout()
        ro.w = None if w is None else w.data_ptr()
        ro.X = ro.Y = ro.opl = None
        ro.scratch, ro.out24 = scratch.data_ptr(), out.data_ptr()
        ro.lite, ro.sums = 0, 1
        return {"struct": ro, "sums_dev": out, "_keep": (w, scratch), "sums": True}

    def chain_readout_scratch(self, n, count):
        """`count` scratch areas for fused read-outs of `count` chains in one scene launch."""
        per = int(self.fn["art_chain_readout_scratch_doubles"](n))
        t = torch.empty(per * count, dtype=torch.float64, device=self.device)
        return [t[k * per:(k + 1) * per] for k in range(count)]

    # scene table (include/art_hip.h: art_scene_bytes / art_scene_pack / art_trace_scene): many chains, one launch
    def scene_alloc(self, n_chains, n_elems, transient=False):
        """(pinned host image, device image) uint8 tensors of art_scene_bytes(n_chains, n_elems).
        transient=True (one-shot launches, RayTracingCalculationMany): the pair comes from a per-size pool instead of
        being allocated -- pinning host memory costs milliseconds.  A pooled pair is reused by the next call of the
        same size: the device image is only read by launches that were enqueued before the next upload on the same
        stream, and the pinned image is re-packed only after its last upload has completed (scene_pack waits)."""
        nb = int(self.fn["art_scene_bytes"](n_chains, n_elems))
        if nb <= 0:
            raise ArtError("art_scene_bytes: bad chain or element count")
        if transient:
            pkey = (nb, self.stream_key())          # per stream: another stream's launch may still read its device image
            pair = self._scene_pool.get(pkey)
            if pair is None:
                pair = self._scene_pool[pkey] = (torch.empty(nb, dtype=torch.uint8, pin_memory=True),
                                                 torch.empty(nb, dtype=torch.uint8, device=self.device))
            ev = self._scene_uploads.pop(pair[0].data_ptr(), None)
            if ev is not None:
                ev.synchronize()
            return pair
        return (torch.empty(nb, dtype=torch.uint8, pin_memory=True),
                torch.empty(nb, dtype=torch.uint8, device=self.device))

    def scene_pack(self, descs, views_in, views_out, n_chains, n_elems, host_image, readouts=None):
        """Pack descriptors (flat, chain-major), views and optional per-chain fused read-outs (new_chain_readout
        dicts) into the host image; returns the scene flags."""
        darr = (_abi.ArtElementDesc * (n_chains * n_elems))(*descs)
        iarr = (_abi.ArtBundleView * n_chains)(*views_in)
        oarr = (_abi.ArtBundleView * (n_chains * n_elems))(*views_out)
        rarr = None if readouts is None else (_abi.ArtChainReadout * n_chains)(*[r["struct"] for r in readouts])
        rc = self.fn["art_scene_pack"](darr, n_chains, n_elems, iarr, oarr, rarr, host_image.data_ptr())
        if rc < 0:
            self.check(rc, "art_scene_pack")
        return rc

    def scene_upload(self, host_image, dev_image):
        """Host image -> device image on the current stream; returns an event the host waits for before it re-packs."""
        dev_image.copy_(host_image, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._scene_uploads[host_image.data_ptr()] = ev
        return ev

    # row summaries (include/art_hip.h): which rows of a chain's input hold one value in every slot
    def row_summary_bytes(self):
        return int(self.fn["art_row_summary_bytes"]())

    def bundle_row_summary(self, view, w, n, out):
        """art_bundle_row_summary of the bundle `view` and the weights `w` (tensor or None) into `out` (device uint8
        tensor of row_summary_bytes()), on the current stream."""
        self.check(self.fn["art_bundle_row_summary"](C.byref(view), self._ptr(w, n), n, out.data_ptr(), self.stream_ptr()),
                   "art_bundle_row_summary")

    def scene_set_row_summaries(self, host_image, summaries):
        """Attach the device array of per-chain summaries (uint8 tensor, n_chains x row_summary_bytes(); None detaches)
        to a packed host image; scene_pack clears it."""
        self.check(self.fn["art_scene_set_row_summaries"](host_image.data_ptr(),
                                                          None if summaries is None else summaries.data_ptr()),
                   "art_scene_set_row_summaries")

    def note_launches(self, n, k=1):
        if self.count_from is not None and n >= self.count_from:
            self.counted_launches += k

    def trace_scene(self, dev_image, host_image, n, segments=1):
        """ONE launch (per 8 elements) for every chain of a packed scene; counts and flags come from the host image's
        header (art_scene_pack), of which dev_image is the uploaded copy."""
        self.note_launches(n, segments)
        sp = self.stream_ptr()
        self.check(self._timed(lambda: self.fn["art_trace_scene"](dev_image.data_ptr(), host_image.data_ptr(), n, sp)),
                   "art_trace_scene")

    def pack_rays(self, points, vectors, path0, n, view):
        self.check(self.fn["art_pack_rays"](points.data_ptr(), vectors.data_ptr(),
                                            None if path0 is None else path0.data_ptr(), n, C.byref(view),
                                            self.stream_ptr()), "art_pack_rays")

    def transform_bundle(self, M, T, rotate_points, view_in, view_out, n):
        m = (C.c_double * 9)(*[float(v) for v in np.asarray(M).reshape(9)])
        t = (C.c_double * 3)(*[float(v) for v in np.asarray(T).reshape(3)])
        self.check(self.fn["art_transform_bundle"](m, t, int(bool(rotate_points)), C.byref(view_in), C.byref(view_out),
                                                   n, self.stream_ptr()), "art_transform_bundle")

    def detector(self, ddesc, view, n, p3=None, XY=None, opl=None):
        p = [t.data_ptr() for t in p3] if p3 is not None else [None, None, None]
        xy = [t.data_ptr() for t in XY] if XY is not None else [None, None]
        o = opl.data_ptr() if opl is not None else None
        self.check(self.fn["art_detector"](C.byref(ddesc), C.byref(view), n, p[0], p[1], p[2], xy[0], xy[1], o,
                                           self.stream_ptr()), "art_detector")

    def detector_readout(self, ddesc, view, w, n, centres=(0.0, 0.0, 0.0), p3=None, XY=None, opl=None, to_host=True):
        """Fused read-out + statistics (art_detector_readout); returns the 24 statistics."""
        out = self.empty(24)      # n == 0: the library writes the reduction identities (0, +inf, -inf)
        p = [t.data_ptr() for t in p3] if (p3 is not None and n > 0) else [None, None, None]
        xy = [t.data_ptr() for t in XY] if (XY is not None and n > 0) else [None, None]
        sp, scratch = self.stream_ptr(), self._red_scratch()
        self.check(self._timed(lambda: self.fn["art_detector_readout"](
            C.byref(ddesc), C.byref(view), self._ptr(w, n), n, float(centres[0]),
            float(centres[1]), float(centres[2]), p[0], p[1], p[2], xy[0], xy[1],
            self._ptr(opl, n), scratch.data_ptr(), out.data_ptr(), sp),
            "readout_events"), "art_detector_readout")
        return out.cpu().numpy() if to_host else out

    def detector_scan_moments(self, ddesc, view, w, n, co, span=0.0):
        """32 moment sums for a detector scan along its normal + [32] the number of rays whose path is not linear
        over shifts in [0, span] (art_detector_scan_moments); host array."""
        if n == 0:
            return np.zeros(33)
        out = self.empty(33)
        self.check(self.fn["art_detector_scan_moments"](C.byref(ddesc), C.byref(view),
                                                        None if w is None else w.data_ptr(), n, float(co), float(span),
                                                        self._red_scratch().data_ptr(), out.data_ptr(),
                                                        self.stream_ptr()), "art_detector_scan_moments")
        return out.cpu().numpy()

    def histogram(self, hdesc, view, w, n, out=None, shift=None):
        """art_histogram on the current stream.  hdesc: ArtHistogramDesc; its wshift is set here, to `shift` or to
        histogram.weight_shift(n, w) (one torch.amax, read back; ValueError for non-finite weights, before the launch).
        out = (counts, wsums, totals) from an earlier call: ADD to them (accumulate), else new tensors are zeroed.
        Returns (counts, wsums or None, totals, shift), device int64 tensors."""
        from . import histogram as hist
        if shift is None:
            shift = hist.weight_shift(n, None if w is None else w[:n])
        hdesc.wshift = int(shift)
        if out is None:
            nbins = int(np.prod([hdesc.bins[k] for k in range(max(1, min(3, hdesc.ndim)))]))
            out = (self.empty(nbins, torch.int64), None if w is None else self.empty(nbins, torch.int64),
                   self.empty(4, torch.int64))
            accumulate = 0
        else:
            accumulate = 1
        counts, wsums, totals = out
        self.check(self.fn["art_histogram"](C.byref(hdesc), C.byref(view), self._ptr(w, n), n, accumulate,
                                            counts.data_ptr(), None if wsums is None else wsums.data_ptr(),
                                            totals.data_ptr(), self.stream_ptr()), "art_histogram")
        return counts, wsums, totals, shift

    def quantiles(self, qdesc, view, w, n, thresholds=None):
        """art_quantiles on the current stream.  qdesc: ArtQuantileDesc with key, planes, fractions, wshift, keys / alive or
        det / shift / centre and scratch_bound filled in; thresholds: None or a HOST float64 array [planes, R].  The output
        tensors are made here.  Returns a dict of DEVICE tensors: values [P, K], below, upto [P, K] (int64), totals [P, 3],
        rank_sums, rank_counts [P, R] (None without thresholds), centres [P, 4] (metrics; None for given keys).  Nothing is
        read back."""
        P, K = qdesc.planes, qdesc.n_fractions
        R = 0 if thresholds is None else int(thresholds.shape[1])
        qdesc.n_thresholds = R
        keep = []
        if R > 0:
            th = np.ascontiguousarray(thresholds, dtype=np.float64)
            th_dev = self.from_numpy(th)
            qdesc.thresholds_host, qdesc.thresholds_dev = th.ctypes.data, th_dev.data_ptr()
            keep += [th, th_dev]
        ints = torch.empty(P * (2 * K + 3 + 2 * R), dtype=torch.int64, device=self.device)
        below, upto = ints[:P * K].view(P, K), ints[P * K:2 * P * K].view(P, K)
        totals = ints[2 * P * K:2 * P * K + 3 * P].view(P, 3)
        o = 2 * P * K + 3 * P
        rank_sums = ints[o:o + P * R].view(P, R) if R else None
        rank_counts = ints[o + P * R:o + 2 * P * R].view(P, R) if R else None
        values = torch.empty((P, K), dtype=torch.float64, device=self.device)
        metric = qdesc.key != _abi.ART_QKEY_GIVEN
        centres = torch.empty((P, 4), dtype=torch.float64, device=self.device) if metric else None
        qdesc.values, qdesc.below, qdesc.upto, qdesc.totals = values.data_ptr(), below.data_ptr(), upto.data_ptr(), totals.data_ptr()
        qdesc.rank_sums = rank_sums.data_ptr() if R else None
        qdesc.rank_counts = rank_counts.data_ptr() if R else None
        qdesc.centres_out = centres.data_ptr() if metric else None
        scratch = self._scratch_for("quantile", "art_quantile_scratch_doubles", C.byref(qdesc), n)
        self.check(self.fn["art_quantiles"](C.byref(qdesc), None if view is None else C.byref(view), self._ptr(w, n), n,
                                            scratch.data_ptr(), self.stream_ptr()), "art_quantiles")
        return {"values": values, "below": below, "upto": upto, "totals": totals, "rank_sums": rank_sums,
                "rank_counts": rank_counts, "centres": centres, "_keep": keep}

    def focal_field(self, fdesc, view, w, n):
        """art_focal_field on the current stream: a new device complex128 tensor [planes, ny, nx] (scratch reused per
        stream)."""
        field = torch.empty((fdesc.planes, fdesc.ny, fdesc.nx), dtype=torch.complex128, device=self.device)
        scratch = self._scratch_for("focal", "art_focal_scratch_doubles", fdesc.nx, fdesc.ny, fdesc.planes, n)
        self.check(self.fn["art_focal_field"](C.byref(fdesc), C.byref(view), self._ptr(w, n), n, scratch.data_ptr(),
                                              field.data_ptr(), self.stream_ptr()), "art_focal_field")
        return field

    def focal_spectrum(self, sdesc, view, w, n):
        """art_focal_spectrum on the current stream: a new device complex128 tensor [planes, nk, ny, nx] (scratch
        reused per stream)."""
        f = sdesc.f
        field = torch.empty((f.planes, sdesc.nk, f.ny, f.nx), dtype=torch.complex128, device=self.device)
        scratch = self._scratch_for("focal", "art_focal_spectrum_scratch_doubles", f.nx, f.ny, f.planes, sdesc.nk, n)
        self.check(self.fn["art_focal_spectrum"](C.byref(sdesc), C.byref(view), self._ptr(w, n), n, scratch.data_ptr(),
                                                 field.data_ptr(), self.stream_ptr()), "art_focal_spectrum")
        return field

    def focal_chromatic(self, desc, final_view, source_view, w, n, table):
        """art_focal_chromatic on the current stream: a new device complex128 tensor [planes, nk, ny, nx].  desc: an
        ArtFocalChromaticDesc (its nk is set here); table: host array [nk, 4] of rows (k_j, c_j, z_j, 0), uploaded here
        and validated by the library on this host copy; scratch reused per stream."""
        table = self._chromatic_table(table)
        f = desc.f
        desc.nk = nk = int(table.shape[0])
        scratch = self._scratch_for("focal", "art_focal_chromatic_scratch_doubles", f.nx, f.ny, f.planes, nk, n)
        field = torch.empty((f.planes, nk, f.ny, f.nx), dtype=torch.complex128, device=self.device)
        table_dev = self.from_numpy(table)
        self.check(self.fn["art_focal_chromatic"](C.byref(desc), C.byref(final_view), C.byref(source_view),
                                                  self._ptr(w, n), n, table_dev.data_ptr(), table.ctypes.data_as(_abi.c_double_p),
                                                  scratch.data_ptr(), field.data_ptr(), self.stream_ptr()),
                   "art_focal_chromatic")
        return field

    def focal_image(self, fdesc, seg, groups, view, w, n):
        """art_focal_image on the current stream: a new device float64 tensor [planes, ny, nx].  seg: device int64
        tensor of groups + 1 slot offsets (never read back); scratch reused per stream."""
        d = _abi.ArtFocalImageDesc()
        d.f = fdesc
        d.groups = int(groups)
        d.seg = seg.data_ptr()
        image = torch.empty((fdesc.planes, fdesc.ny, fdesc.nx), dtype=torch.float64, device=self.device)
        scratch = self._scratch_for("focal", "art_focal_image_scratch_doubles", fdesc.nx, fdesc.ny, fdesc.planes, d.groups, n)
        self.check(self.fn["art_focal_image"](C.byref(d), C.byref(view), self._ptr(w, n), n, scratch.data_ptr(),
                                              image.data_ptr(), self.stream_ptr()), "art_focal_image")
        return image

    def _red_scratch(self):
        return self.scratch("red", self.fn["art_reduce_scratch_doubles"](), torch.float64)

    def detector_stats(self, alive, X, Y, opl, w, n, to_host=True):
        out = self.empty(16)      # n == 0: one workgroup with nothing to add leaves the reduction identities
        ptr = lambda t: self._ptr(t, n)
        if n == 0:
            alive = self.zeros(1, torch.uint8)
        self.check(self.fn["art_detector_stats"](alive.data_ptr(), ptr(X), ptr(Y), ptr(opl), ptr(w), n,
                                                 self._red_scratch().data_ptr(), out.data_ptr(), self.stream_ptr()),
                   "art_detector_stats")
        return out.cpu().numpy() if to_host else out

    def detector_moments(self, alive, X, Y, opl, w, n, cx, cy, co):
        if n == 0:
            return np.zeros(8)
        out = self.empty(8)
        ptr = lambda t: None if t is None else t.data_ptr()
        self.check(self.fn["art_detector_moments"](alive.data_ptr(), ptr(X), ptr(Y), ptr(opl), ptr(w), n,
                                                   float(cx), float(cy), float(co), self._red_scratch().data_ptr(),
                                                   out.data_ptr(), self.stream_ptr()), "art_detector_moments")
        return out.cpu().numpy()

    def bundle_sums(self, view, w, n):
        if n == 0:
            return np.zeros(8)
        out = self.empty(8)
        self.check(self.fn["art_bundle_sums"](C.byref(view), None if w is None else w.data_ptr(), n,
                                              self._red_scratch().data_ptr(), out.data_ptr(), self.stream_ptr()),
                   "art_bundle_sums")
        return out.cpu().numpy()

    def gaussian_intensity(self, view, axis, fraction, n):
        w = self.empty(n)
        a = (C.c_double * 3)(*[float(v) for v in axis])
        self.check(self.fn["art_gaussian_intensity"](C.byref(view), a, float(fraction), n,
                                                     self._red_scratch().data_ptr(), w.data_ptr(), self.stream_ptr()),
                   "art_gaussian_intensity")
        return w

    def gaussian_intensity_central(self, view, fraction, n):
        """Gaussian weights about the bundle's own central ray, axis formed on the device (art_gaussian_intensity_central);
        nothing returns to the host."""
        w = self.empty(n)
        sums8 = self.empty(8)
        self.check(self.fn["art_gaussian_intensity_central"](C.byref(view), float(fraction), n, self._red_scratch().data_ptr(),
                                                             sums8.data_ptr(), w.data_ptr(), self.stream_ptr()),
                   "art_gaussian_intensity_central")
        return w

    def bundle_max_angle(self, view, axis, n):
        """(largest angle to `axis`, largest |point|) over the alive rays; host floats."""
        if n == 0:
            return 0.0, 0.0
        out = self.empty(2)
        a = (C.c_double * 3)(*[float(v) for v in axis])
        self.check(self.fn["art_bundle_max_angle"](C.byref(view), a, n, self._red_scratch().data_ptr(),
                                                   out.data_ptr(), self.stream_ptr()), "art_bundle_max_angle")
        o = out.cpu().numpy()
        return float(o[0]), float(o[1])

    def compact(self, alive, n):
        """Returns (idx tensor int64 [count], count)."""
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device), 0
        ints = self.fn["art_compact_scratch_ints"](n)
        sc = self.scratch("compact", ints, torch.int32)
        idx = torch.empty(int(max(n, 1)), dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.check(self.fn["art_compact"](alive.data_ptr(), n, sc.data_ptr(), idx.data_ptr(), cnt.data_ptr(),
                                          self.stream_ptr()), "art_compact")
        c = int(cnt.cpu().item())
        return idx[:c], c

    def make_source(self, kind, size, rot, S, first, n, n_total, view, step=1):
        """Slots 0..n-1 = global rays first, first + step, ... of an n_total-ray source (art_make_source_strided)."""
        r = (C.c_double * 9)(*[float(v) for v in np.asarray(rot).reshape(9)])
        s = (C.c_double * 3)(*[float(v) for v in np.asarray(S).reshape(3)])
        self.check(self.fn["art_make_source_strided"](kind, float(size), r, s, first, int(step), n, n_total, C.byref(view),
                                                      self.stream_ptr()), "art_make_source_strided")

    def exchange_pack(self, stats, X, Y, opl, alive, slots, send):
        """stats[24] + (X, Y, opl, alive) of the sampled slots -> send[24 + 4k] (art_exchange_pack)."""
        k = int(slots.numel())
        self.check(self.fn["art_exchange_pack"](stats.data_ptr(), X.data_ptr(), Y.data_ptr(), opl.data_ptr(),
                                                alive.data_ptr(), slots.data_ptr(), k, send.data_ptr(),
                                                self.stream_ptr()), "art_exchange_pack")

    def exchange_fold(self, recv, world, stride, out):
        """Fold `world` gathered statistics vectors into the global 24 (art_exchange_fold)."""
        self.check(self.fn["art_exchange_fold"](recv.data_ptr(), int(world), int(stride), out.data_ptr(),
                                                self.stream_ptr()), "art_exchange_fold")

    def survivor_bytes(self, count, dense=False):
        return int(self.fn["art_survivor_bytes"](int(count), 1 if dense else 0))

    def pack_survivors(self, alive, X, Y, opl, number, first, step, send):
        """Records (X, Y, path, number:int32) of the alive slots, in slot order, behind a (count, flags) header in
        the uint8 tensor `send` (art_pack_survivors); nothing returns to the host."""
        n = int(alive.numel())
        sc = self.scratch("compact", self.fn["art_compact_scratch_ints"](n), torch.int32)
        ptr = lambda t: self._ptr(t, n)
        self.check(self.fn["art_pack_survivors"](ptr(alive), n, ptr(X), ptr(Y), ptr(opl), ptr(number), int(first),
                                                 int(step), sc.data_ptr(), send.data_ptr(), int(send.numel()),
                                                 self.stream_ptr()), "art_pack_survivors")

    def survivor_finish(self, stats_dev, n, send, xhdr=None):
        """Header of a ZERO-COPY send buffer whose sections the read-out wrote directly (art_survivor_finish): (n, dense) if
        every slot is alive, else (count, unpacked); `xhdr` (26 doubles): the rank's block of the header exchange."""
        self.check(self.fn["art_survivor_finish"](stats_dev.data_ptr(), int(n), send.data_ptr(),
                                                  None if xhdr is None else xhdr.data_ptr(), self.stream_ptr()),
                   "art_survivor_finish")

    def survivor_xheader(self, send, stats_dev, xhdr):
        """The rank's block of the header exchange behind art_pack_survivors (art_survivor_xheader)."""
        self.check(self.fn["art_survivor_xheader"](send.data_ptr(), None if stats_dev is None else stats_dev.data_ptr(),
                                                   xhdr.data_ptr(), self.stream_ptr()), "art_survivor_xheader")

    def trace_guides(self, descs, rays, alive):
        """Advance guide ray j (row j of the DEVICE tensor rays[count, 8], in place) through descs[j]; alive[count] uint8
        (art_trace_guides, 8 rays per launch)."""
        count = len(descs)
        sp = self.stream_ptr()
        for k0 in range(0, count, _abi.ART_GUIDES_MAX):
            m = min(_abi.ART_GUIDES_MAX, count - k0)
            darr = (_abi.ArtElementDesc * m)(*descs[k0:k0 + m])
            self.check(self.fn["art_trace_guides"](darr, m, rays.data_ptr() + 64 * k0, alive.data_ptr() + k0, sp),
                       "art_trace_guides")

    def _upload_table(self, arr, purpose=None):
        """A DEVICE copy of the ctypes job table `arr`, enqueued on the current stream.  `purpose`: a second table that
        the same launches read (its own pool entry, so that two tables of one size never share a device copy)."""
        nb = C.sizeof(arr)
        # pinned staging + device table from a per-size pool (pinning host memory costs milliseconds): the pinned image is
        # rewritten only after its previous upload has completed, the device table is read by launches enqueued before
        # the next upload on the same stream
        pkey = (nb, self.stream_key()) if purpose is None else (purpose, nb, self.stream_key())
        pair = self._job_pool.get(pkey)
        if pair is None:
            pair = self._job_pool[pkey] = [torch.empty(nb, dtype=torch.uint8, pin_memory=True),
                                           torch.empty(nb, dtype=torch.uint8, device=self.device), None]
        host, dev, ev = pair
        if ev is not None:
            ev.synchronize()
        C.memmove(host.data_ptr(), C.addressof(arr), nb)
        dev.copy_(host, non_blocking=True)
        pair[2] = torch.cuda.Event()
        pair[2].record()
        return dev

    def wavefront(self, jobs):
        """art_wavefront for a list of ArtWavefrontJob (host structs; their `out` is set here): uploads the job table,
        enqueues the three launches and returns the DEVICE tensor out[len(jobs), ART_WAVEFRONT_DOUBLES]."""
        c = len(jobs)
        out = torch.empty((c, _abi.ART_WAVEFRONT_DOUBLES), dtype=torch.float64, device=self.device)
        for k, j in enumerate(jobs):
            j.out = out.data_ptr() + 8 * _abi.ART_WAVEFRONT_DOUBLES * k
        arr = (_abi.ArtWavefrontJob * c)(*jobs)
        scratch = self._scratch_for("wavefront", "art_wavefront_scratch_doubles", arr, c)
        dev = self._upload_table(arr)
        self.check(self.fn["art_wavefront"](dev.data_ptr(), arr, c, scratch.data_ptr(), self.stream_ptr()), "art_wavefront")
        return out

    def polarisation(self, jobs, views, coatings):
        """art_polarisation for a list of ArtPolarisationJob (host structs; their `views` and `out` are set here), the
        HOST ctypes arrays of every job's K + 1 views and a list of ArtCoating: uploads views, coatings and job table,
        enqueues the two launches and returns the DEVICE tensor out[len(jobs), ART_POLARISATION_DOUBLES]."""
        c = len(jobs)
        out = torch.empty((c, _abi.ART_POLARISATION_DOUBLES), dtype=torch.float64, device=self.device)
        blob = b"".join(bytes(v) for v in views) + b"".join(bytes(k) for k in coatings)
        dev = self._upload_table((C.c_char * len(blob)).from_buffer_copy(blob), "polarisation views")
        off = 0
        jarr = (_abi.ArtPolarisationJob * c)()
        for k, (j, v) in enumerate(zip(jobs, views)):
            jarr[k] = j
            jarr[k].views = dev.data_ptr() + off
            jarr[k].out = out.data_ptr() + 8 * _abi.ART_POLARISATION_DOUBLES * k
            off += C.sizeof(v)
        carr = (_abi.ArtCoating * max(len(coatings), 1))(*coatings)
        cdev = dev.data_ptr() + off if coatings else None
        scratch = self._scratch_for("polarisation", "art_polarisation_scratch_doubles", jarr, c)
        jdev = self._upload_table(jarr)
        self.check(self.fn["art_polarisation"](jdev.data_ptr(), jarr, c, cdev, carr, len(coatings), scratch.data_ptr(),
                                               self.stream_ptr()), "art_polarisation")
        return out

    def ray_tubes(self, jobs, views, elems, quadrics):
        """art_ray_tubes for a list of ArtTubeJob (host structs; their `views`, `elems` and `quadrics` are set here) and,
        per job, the HOST ctypes arrays of its K + 1 views, its K element descriptors and its K quadrics (or None):
        uploads the tables, enqueues the two launches and returns the DEVICE tensor out[len(jobs), ART_TUBE_DOUBLES].
        An element the pass does not cover raises NotImplementedError with the library's message."""
        c = len(jobs)
        out = torch.empty((c, _abi.ART_TUBE_DOUBLES), dtype=torch.float64, device=self.device)
        parts = []
        for v, e, q in zip(views, elems, quadrics):
            parts += [bytes(v), bytes(e), b"" if q is None else bytes(q)]
        blob = b"".join(parts)
        dev = self._upload_table((C.c_char * len(blob)).from_buffer_copy(blob), "ray tube tables")
        off = 0
        jhost, jdev = (_abi.ArtTubeJob * c)(), (_abi.ArtTubeJob * c)()
        for k, (j, v, e, q) in enumerate(zip(jobs, views, elems, quadrics)):
            jhost[k] = j
            jdev[k] = j
            jhost[k].views = jdev[k].views = dev.data_ptr() + off
            off += C.sizeof(v)
            jhost[k].elems, jdev[k].elems = C.addressof(e), dev.data_ptr() + off
            off += C.sizeof(e)
            if q is not None:
                jhost[k].quadrics, jdev[k].quadrics = C.addressof(q), dev.data_ptr() + off
                off += C.sizeof(q)
        ns = self.fn["art_ray_tubes_scratch_doubles"](jhost, c)
        if ns == _abi.ART_ERR_UNSUPPORTED:
            raise NotImplementedError(self.last_error())
        if ns < 0:
            raise ArtError(f"art_ray_tubes_scratch_doubles failed with code {ns}: {self.last_error()}")
        scratch = self.scratch("ray tubes", ns, torch.float64)
        table = self._upload_table(jdev)
        self.check(self.fn["art_ray_tubes"](table.data_ptr(), jhost, c, scratch.data_ptr(), out.data_ptr(),
                                            self.stream_ptr()), "art_ray_tubes")
        return out

    def sensitivities(self, jobs, views, elems, quadrics):
        """art_sensitivities for a list of ArtSensitivityJob, with the tables as ray_tubes takes and uploads them.  Returns
        the DEVICE tensor of the jobs' tables one after another, [sum of 1 + 6 (K_j + 1), ART_SENS_DOUBLES].  An element
        the pass does not cover raises NotImplementedError with the library's message."""
        c = len(jobs)
        rows = sum(1 + _abi.ART_SENS_COLS * (j.n_elems + 1) for j in jobs)
        out = torch.empty((rows, _abi.ART_SENS_DOUBLES), dtype=torch.float64, device=self.device)
        parts = []
        for v, e, q in zip(views, elems, quadrics):
            parts += [bytes(v), bytes(e), b"" if q is None else bytes(q)]
        blob = b"".join(parts)
        dev = self._upload_table((C.c_char * len(blob)).from_buffer_copy(blob), "sensitivity tables")
        off = 0
        jhost, jdev = (_abi.ArtSensitivityJob * c)(), (_abi.ArtSensitivityJob * c)()
        for k, (j, v, e, q) in enumerate(zip(jobs, views, elems, quadrics)):
            jhost[k] = j
            jdev[k] = j
            jhost[k].views = jdev[k].views = dev.data_ptr() + off
            off += C.sizeof(v)
            jhost[k].elems, jdev[k].elems = C.addressof(e), dev.data_ptr() + off
            off += C.sizeof(e)
            if q is not None:
                jhost[k].quadrics, jdev[k].quadrics = C.addressof(q), dev.data_ptr() + off
                off += C.sizeof(q)
        ns = self.fn["art_sensitivities_scratch_doubles"](jhost, c)
        if ns == _abi.ART_ERR_UNSUPPORTED:
            raise NotImplementedError(self.last_error())
        if ns < 0:
            raise ArtError(f"art_sensitivities_scratch_doubles failed with code {ns}: {self.last_error()}")
        scratch = self.scratch("sensitivities", ns, torch.float64)
        table = self._upload_table(jdev)
        self.check(self.fn["art_sensitivities"](table.data_ptr(), jhost, c, scratch.data_ptr(), out.data_ptr(),
                                                self.stream_ptr()), "art_sensitivities")
        return out

    def alignment_sums(self, jobs, views, elems, quadrics, out=None):
        """art_alignment_sums for a list of ArtAlignmentJob, with the tables as sensitivities takes and uploads them.
        Returns the DEVICE tensor [len(jobs), ART_ALIGN_DOUBLES] (`out`, when the caller brings one).  An element the pass
        does not cover raises NotImplementedError with the library's message."""
        c = len(jobs)
        if out is None:
            out = torch.empty((c, _abi.ART_ALIGN_DOUBLES), dtype=torch.float64, device=self.device)
        if out.shape != (c, _abi.ART_ALIGN_DOUBLES) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 tensor [jobs, ART_ALIGN_DOUBLES]")
        parts = []
        for v, e, q in zip(views, elems, quadrics):
            parts += [bytes(v), bytes(e), b"" if q is None else bytes(q)]
        blob = b"".join(parts)
        dev = self._upload_table((C.c_char * len(blob)).from_buffer_copy(blob), "alignment tables")
        off = 0
        jhost, jdev = (_abi.ArtAlignmentJob * c)(), (_abi.ArtAlignmentJob * c)()
        for k, (j, v, e, q) in enumerate(zip(jobs, views, elems, quadrics)):
            jhost[k] = j
            jdev[k] = j
            jhost[k].views = jdev[k].views = dev.data_ptr() + off
            off += C.sizeof(v)
            jhost[k].elems, jdev[k].elems = C.addressof(e), dev.data_ptr() + off
            off += C.sizeof(e)
            if q is not None:
                jhost[k].quadrics, jdev[k].quadrics = C.addressof(q), dev.data_ptr() + off
                off += C.sizeof(q)
        ns = self.fn["art_alignment_sums_scratch_doubles"](jhost, c)
        if ns == _abi.ART_ERR_UNSUPPORTED:
            raise NotImplementedError(self.last_error())
        if ns < 0:
            raise ArtError(f"art_alignment_sums_scratch_doubles failed with code {ns}: {self.last_error()}")
        scratch = self.scratch("alignment_sums", ns, torch.float64)
        table = self._upload_table(jdev)
        self.check(self.fn["art_alignment_sums"](table.data_ptr(), jhost, c, scratch.data_ptr(), out.data_ptr(),
                                                 self.stream_ptr()), "art_alignment_sums")
        return out

    def focal_vector_tables(self, vdesc, views, coatings, materials):
        """Uploads the tables of art_focal_vector_spectrum and points vdesc at them (`views`, `materials`, `n_coatings`).
        views: the HOST ctypes array of the chain's K + 1 views; coatings: a list of ArtCoating; materials: float64
        NumPy [nk, len(coatings), ART_COATING_MAX_MATERIALS, 2] (n, kappa).  Returns the call's other table arguments
        (coatings_dev, coatings_host, materials_host); the caller keeps them alive until the call has been made."""
        nk, nc = vdesc.s.nk, len(coatings)
        mats = np.ascontiguousarray(materials, dtype=np.float64)
        if mats.shape != (nk, nc, _abi.ART_COATING_MAX_MATERIALS, 2):
            raise ValueError(f"materials must be [nk, coatings, {_abi.ART_COATING_MAX_MATERIALS}, 2]")
        blob = bytes(views) + b"".join(bytes(k) for k in coatings) + mats.tobytes()
        dev = self._upload_table((C.c_char * len(blob)).from_buffer_copy(blob), "focal vector spectrum")
        vdesc.views = dev.data_ptr()
        vdesc.n_coatings = nc
        cdev = dev.data_ptr() + C.sizeof(views) if nc else None
        vdesc.materials = dev.data_ptr() + C.sizeof(views) + nc * C.sizeof(_abi.ArtCoating) if nc else None
        carr = (_abi.ArtCoating * max(nc, 1))(*coatings)
        marr = (_abi.ArtCoatingMaterial * max(mats.size // 2, 1)).from_buffer_copy(mats.tobytes() or bytes(16))
        return cdev, carr, marr

    def focal_vector_spectrum(self, vdesc, views, coatings, materials):
        """art_focal_vector_spectrum on the current stream (arguments as focal_vector_tables): a new device complex128
        tensor [planes, nk, 3, ny, nx] (scratch reused per stream)."""
        f = vdesc.s.f
        field = torch.empty((f.planes, vdesc.s.nk, 3, f.ny, f.nx), dtype=torch.complex128, device=self.device)
        cdev, carr, marr = self.focal_vector_tables(vdesc, views, coatings, materials)
        scratch = self._scratch_for("focal vector", "art_focal_vector_spectrum_scratch_doubles", C.byref(vdesc))
        self.check(self.fn["art_focal_vector_spectrum"](C.byref(vdesc), C.byref(views[vdesc.n_elems]), cdev, carr, marr,
                                                        scratch.data_ptr(), field.data_ptr(), self.stream_ptr()),
                   "art_focal_vector_spectrum")
        return field

    def focal_vector_chromatic(self, vcdesc, views, coatings, materials, table):
        """art_focal_vector_chromatic on the current stream: a new device complex128 tensor [planes, nk, 3, ny, nx].
        vcdesc: an ArtFocalVectorChromaticDesc (its v.s.nk is set here); views, coatings, materials as
        focal_vector_tables, one row of materials per row of the table; table: host array [nk, 4] of rows
        (k_j, c_j, z_j, 0), uploaded here and validated by the library on this host copy; scratch reused per stream."""
        table = self._chromatic_table(table)
        v = vcdesc.v
        v.s.nk = nk = int(table.shape[0])
        f = v.s.f
        cdev, carr, marr = self.focal_vector_tables(v, views, coatings, materials)
        scratch = self._scratch_for("focal vector", "art_focal_vector_chromatic_scratch_doubles", C.byref(vcdesc))
        field = torch.empty((f.planes, nk, 3, f.ny, f.nx), dtype=torch.complex128, device=self.device)
        table_dev = self.from_numpy(table)
        self.check(self.fn["art_focal_vector_chromatic"](C.byref(vcdesc), C.byref(views[v.n_elems]), C.byref(views[0]),
                                                         cdev, carr, marr, table_dev.data_ptr(),
                                                         table.ctypes.data_as(_abi.c_double_p), scratch.data_ptr(),
                                                         field.data_ptr(), self.stream_ptr()),
                   "art_focal_vector_chromatic")
        return field

    def analyse_bundles(self, jobs, n):
        """art_analyse_bundles for a list of ArtAnalysisJob (host structs): uploads the job table, enqueues the four
        launches and returns the DEVICE tensor out[len(jobs), 64] -- nothing is read back here."""
        c = len(jobs)
        arr = (_abi.ArtAnalysisJob * c)(*jobs)
        dev = self._upload_table(arr)
        out = torch.empty((c, _abi.ART_ANALYSIS_DOUBLES), dtype=torch.float64, device=self.device)
        # (jobs that bring their sums along need no per-tile partials, but the area is sized for the general case)
        scratch = self.scratch("analysis", self.fn["art_analysis_scratch_doubles"](c, int(n)), torch.float64)
        self.check(self.fn["art_analyse_bundles"](dev.data_ptr(), arr, c, int(n), scratch.data_ptr(), out.data_ptr(),
                                                  self.stream_ptr()), "art_analyse_bundles")
        return out

    def bundle_sums9(self, bundle):
        """DEVICE tensor [64] whose first nine doubles are the analysis sums of `bundle` (count, sum point, sum vector, sum
        intensity, sum path: art_analyse_bundles with ONE job of mode ART_JOB_SUMS -- the canonical fold order, the same
        bits as the analysis' own pass or the tail of a tracing launch); nothing is read back."""
        j = _abi.ArtAnalysisJob()
        j.b = bundle.view()
        j.w = None if bundle.intensity is None else bundle.intensity.data_ptr()
        j.mode = _abi.ART_JOB_SUMS
        return self.analyse_bundles([j], bundle.n_slots)[0]

    def make_extended_source(self, radius, divergence, n_points, per, rot, S, first, n, view):
        r = (C.c_double * 9)(*[float(v) for v in np.asarray(rot).reshape(9)])
        s = (C.c_double * 3)(*[float(v) for v in np.asarray(S).reshape(3)])
        self.check(self.fn["art_make_extended_source"](float(radius), float(divergence), int(n_points), int(per), r, s,
                                                       first, n, C.byref(view), self.stream_ptr()),
                   "art_make_extended_source")


def get_backend():
    """The process-wide backend; created on first use, raises loudly if the HIP path is unavailable."""
    global _BACKEND
    if _BACKEND is None:
        _BACKEND = HipBackend()
    return _BACKEND

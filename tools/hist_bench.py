#!/usr/bin/env python3
"""Time art_histogram on relay4's final bundle (1e7 rays by default, Gaussian weights) for the shapes of DESIGN.md 5,
each bracketed by HIP events over `reps` back-to-back calls, beside art_detector_scan_moments on the same bundle (the
read-out pass that reads the same 65 B per ray).  Kernel times come from a rocprofv3 --kernel-trace --stats run of this
script:

    python tools/hist_bench.py [rays] [--reps 20]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rays", nargs="?", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _abi, _lib
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    be = _lib.get_backend()
    chain, _ = workloads.build_scene(4, small_n=int(args.rays))
    last = chain.get_output_rays()[-1]
    n = last.n_slots
    g = torch.Generator(device="cpu").manual_seed(1)
    last.intensity = torch.exp(-0.5 * torch.randn(n, generator=g, dtype=torch.float64) ** 2).to(be.device)
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    masked = last.copy()
    masked.intensity = last.intensity
    k = torch.arange(n, device=be.device)
    masked.alive[((k // 2) % 3) == 0] = 0           # a third of the slots dead, evenly spread pairs
    masked.touch()

    def desc(axes, bins):
        h = D.get_Histogram(last, axes, bins)          # default ranges: the alive rays' min..max
        d = _abi.ArtHistogramDesc()
        d.source, d.ndim, d.map = _abi.ART_HIST_DETECTOR, len(axes), D._desc()
        d.delay_centre = float(D.readout(last, store=False, lite=True)["stats"][1] / len(last))
        for i, a in enumerate(axes):
            d.axis[i], d.bins[i] = {"X": _abi.ART_HAXIS_X, "Y": _abi.ART_HAXIS_Y, "Delay": _abi.ART_HAXIS_DELAY}[a], h.counts.shape[i]
            d.lo[i], d.hi[i] = h.edges[i][0], h.edges[i][-1]
        return d, h.shift

    shapes = [("(a) 256x256 X-Y", last, ("X", "Y"), 256), ("(b) 1024 Delay", last, ("Delay",), 1024),
              ("(c) 64^3 X-Y-Delay", last, ("X", "Y", "Delay"), 64), ("(d) 2048x2048 X-Y", last, ("X", "Y"), 2048),
              ("(e) (a), a third dead", masked, ("X", "Y"), 256)]

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3     # us

    rows = []
    for name, B, axes, bins in shapes:
        d, S = desc(axes, bins)
        view = B.view()
        rows.append((name, lambda d=d, S=S, B=B, view=view: be.histogram(d, view, B.intensity, n, shift=S)))
    scan_out = be.empty(33)
    rows.append(("art_detector_scan_moments (w)", lambda: be.fn["art_detector_scan_moments"](
        D._desc(), last.view(), last.intensity.data_ptr(), n, 700.0, 0.0, be._red_scratch().data_ptr(),
        scan_out.data_ptr(), be.stream_ptr())))
    print(f"# relay4 final bundle: {n} slots, {len(last)} alive, {args.reps} calls each (HIP events, whole call)")
    for name, fn in rows:
        print(f"{name:40s} {timed(fn):9.1f} us/call", flush=True)


if __name__ == "__main__":
    main()

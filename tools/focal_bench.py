#!/usr/bin/env python3
"""Time art_focal_field on relay4's final bundle for the two shapes of DESIGN.md 5 -- 1e6 rays x 256^2 x 1 plane and
1e7 rays x 128^2 x 8 planes -- each bracketed by HIP events over `reps` back-to-back calls, and print the rate by the
8-flop count (one complex multiply-add per ray, pixel and plane).  Kernel times come from a rocprofv3 --kernel-trace
--stats run of this script:

    python tools/focal_bench.py [--reps 5] [--shapes 0,1]"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10 ** 6, 256, 1), (10 ** 7, 128, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="0,1")
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _abi, _lib
    import ART.ModuleDetector as mdet
    import ART.ModuleProcessing as mp
    from tools.bench import workloads
    be = _lib.get_backend()
    for s in (int(v) for v in args.shapes.split(",")):
        rays, pix, planes = SHAPES[s]
        chain, _ = workloads.build_scene(4, small_n=rays)
        last = chain.get_output_rays()[-1]
        n = last.n_slots
        D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
        D.autoplace(last, 600.0)
        st = D.readout(last, store=False, lite=True)["stats"]
        size = 16 * mp.ReturnAiryRadius(last.wavelength, mp.ReturnNumericalAperture(last, 1))
        fd = _abi.ArtFocalDesc()
        fd.det = D._desc()
        fd.k, fd.L_ref = 2 * math.pi / last.wavelength, st[1] / st[0]
        fd.x0 = fd.y0 = -0.5 * size
        fd.dx = fd.dy = size / (pix - 1)
        fd.nx = fd.ny = pix
        fd.planes = planes
        for q in range(planes):
            fd.shift[q] = 0.05 * q
        view = last.view()
        call = lambda: be.focal_field(fd, view, None, n)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            call()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        flops = 8.0 * n * pix * pix * planes
        print(f"{rays:.0e} rays ({n} slots, {len(last)} alive) x {pix}^2 x {planes} planes: {ms:9.3f} ms/call "
              f"{flops / ms * 1e-9:8.2f} TFLOP/s (8-flop count over all slots)", flush=True)


if __name__ == "__main__":
    main()

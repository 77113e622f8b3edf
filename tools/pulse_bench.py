#!/usr/bin/env python3
"""Time art_focal_spectrum on relay4's final bundle for the shapes of DESIGN.md 5 -- (a) 1e6 rays x 128^2 x 64
wavenumbers x 1 plane, (b) 1e7 rays x 64^2 x 32 wavenumbers x 2 planes, and (c) 1e6 rays x 256^2 x 1 wavenumber, shape
(a) of tools/focal_bench.py, beside art_focal_field on the same descriptor -- each bracketed by HIP events over `reps`
back-to-back calls, and print the rate by the 8-flop count (one complex multiply-add per ray, pixel, wavenumber and
plane).  Kernel times come from a rocprofv3 --kernel-trace --stats run of this script:

    python tools/pulse_bench.py [--reps 5] [--shapes 0,1,2]"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(10 ** 6, 128, 64, 1), (10 ** 7, 64, 32, 2), (10 ** 6, 256, 1, 1)]


def _time(call, reps):
    import torch
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="0,1,2")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _abi, _lib
    import ART.ModuleDetector as mdet
    import ART.ModuleProcessing as mp
    from tools.bench import workloads
    be = _lib.get_backend()
    for s in (int(v) for v in args.shapes.split(",")):
        rays, pix, nk, planes = SHAPES[s]
        chain, _ = workloads.build_scene(4, small_n=rays)
        last = chain.get_output_rays()[-1]
        n = last.n_slots
        D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
        D.autoplace(last, 600.0)
        st = D.readout(last, store=False, lite=True)["stats"]
        size = 16 * mp.ReturnAiryRadius(last.wavelength, mp.ReturnNumericalAperture(last, 1))
        k = 2 * math.pi / last.wavelength
        sd = _abi.ArtFocalSpectrumDesc()
        fd = sd.f
        fd.det = D._desc()
        fd.k, fd.L_ref = k * (1 - 0.1 * (nk > 1)), st[1] / st[0]
        fd.x0 = fd.y0 = -0.5 * size
        fd.dx = fd.dy = size / (pix - 1)
        fd.nx = fd.ny = pix
        fd.planes = planes
        for q in range(planes):
            fd.shift[q] = 0.05 * q
        sd.dk = 0.2 * k / max(nk - 1, 1)
        sd.nk = nk
        view = last.view()
        ms = _time(lambda: be.focal_spectrum(sd, view, None, n), args.reps)
        flops = 8.0 * n * pix * pix * nk * planes
        print(f"{rays:.0e} rays ({n} slots, {len(last)} alive) x {pix}^2 x {nk} wavenumbers x {planes} planes: "
              f"art_focal_spectrum {ms:9.3f} ms/call {flops / ms * 1e-9:8.2f} TFLOP/s (8-flop count over all slots)",
              flush=True)
        if nk == 1:
            ms = _time(lambda: be.focal_field(fd, view, None, n), args.reps)
            print(f"{'':>{len(f'{rays:.0e}')}} same descriptor:  art_focal_field    {ms:9.3f} ms/call "
                  f"{flops / ms * 1e-9:8.2f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time art_focal_image on relay4's final bundle at 1e6 rays for the two shapes of DESIGN.md 5 -- 256^2 pixels with the
slots treated as groups of 4000 rays (250 groups), and the under-filled shape of 30 groups on one 64^2 tile -- one plane
each, against two baselines on the same device in the same run:

  1. the route without art_focal_image: one coherent field per group on slots() of the bundle and a torch abs()**2 sum,
     through Detector.get_FocalField (what a user would write) and through the backend's focal_field alone (no host
     copies: the leanest form of that route);
  2. ONE art_focal_field call over all rays: the floor, the same FMAs without the groups.

Every figure is bracketed by HIP events over `reps` back-to-back calls after `warmup` calls.  Prints one line per figure
and one JSON line per shape:

    python tools/image_bench.py [--reps 5] [--warmup 2] [--shapes 0,1]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RAYS = 10 ** 6
SHAPES = [(256, 250), (64, 30)]          # (pixels per side, groups)


def timed(torch, call, reps, warmup):
    for _ in range(warmup):
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="0,1")
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _lib, focal, image
    import ART.ModuleDetector as mdet
    import ART.ModuleProcessing as mp
    from tools.bench import workloads
    be = _lib.get_backend()
    chain, _ = workloads.build_scene(4, small_n=RAYS)
    last = chain.get_output_rays()[-1]
    n = last.n_slots
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    st = D.readout(last, store=False, lite=True)["stats"]
    size = 16 * mp.ReturnAiryRadius(last.wavelength, mp.ReturnNumericalAperture(last, 1))
    print(f"device: {torch.cuda.get_device_name(0)}; relay4, {n} slots, {len(last)} alive", flush=True)
    for s in (int(v) for v in args.shapes.split(",")):
        pix, groups = SHAPES[s]
        per = -(-n // groups)
        kw = dict(Size=size, Pixels=pix, Centre=(0.0, 0.0), RefPath=st[1] / st[0])
        seg, groups = image.segments(last, RaysPerSource=per)
        bounds = [(g * per, min((g + 1) * per, n)) for g in range(groups)]
        parts = [last.slots(lo, hi) for lo, hi in bounds]
        fd = focal.focal_desc(D, last, Shifts=None, Wavelength=None, **kw)[0]
        view = last.view()

        def per_group_api():
            total = torch.zeros((1, pix, pix), dtype=torch.float64, device=be.device)
            for p in parts:
                total += D.get_FocalField(p, **kw).field.abs() ** 2
            return total

        def per_group_backend():
            total = torch.zeros((1, pix, pix), dtype=torch.float64, device=be.device)
            for p in parts:
                total += be.focal_field(fd, p.view(), None, p.n_slots).abs() ** 2
            return total

        got = be.focal_image(fd, seg, groups, view, None, n)
        ref = per_group_backend()
        worst = float((got - ref).abs().max() / ref.max())
        res = {"shape": f"{n} slots x {pix}^2 x 1 plane, {groups} groups of {per}", "max_diff_over_peak": worst,
               "image_ms": timed(torch, lambda: be.focal_image(fd, seg, groups, view, None, n), args.reps, args.warmup),
               "image_api_ms": timed(torch, lambda: D.get_FocalImage(last, RaysPerSource=per, **kw), args.reps, args.warmup),
               "coherent_ms": timed(torch, lambda: be.focal_field(fd, view, None, n), args.reps, args.warmup),
               "per_group_backend_ms": timed(torch, per_group_backend, max(1, args.reps // 2), 1),
               "per_group_api_ms": timed(torch, per_group_api, max(1, args.reps // 2), 1)}
        res["image_over_coherent"] = res["image_ms"] / res["coherent_ms"]
        res["per_group_backend_over_image"] = res["per_group_backend_ms"] / res["image_ms"]
        res["per_group_api_over_image_api"] = res["per_group_api_ms"] / res["image_api_ms"]
        flops = 8.0 * n * pix * pix
        for key in ("image_ms", "image_api_ms", "coherent_ms", "per_group_backend_ms", "per_group_api_ms"):
            print(f"{res['shape']}: {key:22s} {res[key]:10.3f} ms {flops / res[key] * 1e-9:8.2f} TFLOP/s (8-flop count)",
                  flush=True)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time art_trace_quadric beside art_trace_element ("Quadrics"): a point source on an elliptical cylinder at
2 degrees grazing (p = 1000 mm, q = 300 mm), 1e7 rays by default, all alive before and after; the yardstick is
art_trace_element on a circular MirrorCylindrical of the same curvature in the same pose, for the same bundle, in the same
run.  Both kernels read 57 B and write 65 B per ray.  Every figure: HIP events around ONE call, after warm-up calls,
median and min..max over `reps` calls; the two kernels alternate (element, quadric, element again).

    python tools/quadric_bench.py [rays] [--reps 30]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rays", nargs="?", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    import ART.ModuleMirror as mm
    import ART.ModuleOpticalElement as moe
    import ART.ModuleProcessing as mp
    import ART.ModuleSource as msrc
    import ART.ModuleSupport as ms
    from attosecondraytracing_amd.bundle import RayBundle

    n = int(args.rays)
    p, q, graz = 1000.0, 300.0, 2.0
    src = msrc.PointSource(np.zeros(3), np.array([1.0, 0.0, 0.0]), 1e-3, n, Wavelength=30e-6)
    be = src.backend
    S = ms.SupportRectangle(200.0, 20.0)              # footprint: +-29 mm x +-1 mm -- every ray hits
    conic = mm.MirrorEllipticalCylinder(S, p, q, graz)
    # the circle that osculates the ellipse at its pole: R = 2 p q / ((p + q) sin(grazing)); MirrorCylindrical curves along
    # y, so it is placed with its major axis across the beam -- the yardstick only has to move the same bytes
    circ = mm.MirrorCylindrical(2 * p * q / ((p + q) * np.sin(np.deg2rad(graz))), S)
    th = np.deg2rad(90.0 - graz)
    pose = (np.array([p, 0.0, 0.0]), np.array([-np.cos(th), 0.0, np.sin(th)]), np.array([np.sin(th), 0.0, np.cos(th)]))
    d_conic, _ = mp.element_descriptor(moe.OpticalElement(conic, *pose), True, be)
    d_circ, _ = mp.element_descriptor(moe.OpticalElement(circ, *pose), True, be)
    out = RayBundle.allocate(n, like=src, backend=be)
    vin, vout = src.view(), out.view()
    co = conic._quadric_coefficients()

    def timed(call, warm=5):
        for _ in range(warm):
            call()
        ms_ = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms_.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(ms_)), "min_ms": float(min(ms_)), "max_ms": float(max(ms_))}

    res = {"rays": n, "reps": args.reps, "alive_before": int(src.alive.sum())}
    res["element_cylinder"] = timed(lambda: be.trace_element(d_circ, vin, vout, n))
    res["alive_after_element"] = int(out.alive.sum())
    res["quadric"] = timed(lambda: be.trace_quadric(d_conic, co, vin, vout, n))
    res["alive_after_quadric"] = int(out.alive.sum())
    res["element_cylinder_again"] = timed(lambda: be.trace_element(d_circ, vin, vout, n))
    res["quadric_again"] = timed(lambda: be.trace_quadric(d_conic, co, vin, vout, n))
    el = min(res["element_cylinder"]["median_ms"], res["element_cylinder_again"]["median_ms"])
    qu = min(res["quadric"]["median_ms"], res["quadric_again"]["median_ms"])
    res["ratio_quadric_over_element"] = qu / el
    res["bytes_per_ray"] = 57 + 65
    res["quadric_TB_per_s"] = n * (57 + 65) / (qu * 1e-3) / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()

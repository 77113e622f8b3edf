#!/usr/bin/env python3
"""Time art_trace_freeform beside art_trace_quadric ("Freeforms"): the scene of tools/quadric_bench.py -- a
point source on an elliptical cylinder at 2 degrees grazing (p = 1000 mm, q = 300 mm), 1e7 rays by default, all alive
before and after -- with figures of total degree 0 (none), 4, 8 and 16 on the same base.  The yardstick is
art_trace_quadric on the bare base for the same bundle, in the same run, alternating with the freeform calls.  Both
kernels read 57 B and write 65 B per ray.  Every figure: HIP events around ONE call, after warm-up calls, median and
min..max over `reps` calls.  The mean number of Newton steps per ray comes from the NumPy restatement of the device's
stopping rule (tests/freeform_common.py, fp64, device=True) on the first `sample` rays of the bundle.

    python tools/freeform_bench.py [rays] [--reps 30] [--sample 20000]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ORDERS = (0, 4, 8, 16)


def figure_of_order(md, S, order, scale=1e-5):
    """Every monomial up to `order` (total degree), sizes decaying by a factor of two per degree: about 10 nm."""
    if order == 0:
        return []
    return [md.Polynomial(S, {(p, q): scale * 0.5 ** (p + q) * np.cos(1.7 * p + 0.9 * q + 0.3)
                              for p in range(order + 1) for q in range(order + 1 - p)})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rays", nargs="?", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sample", type=int, default=20000)
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    import ART.ModuleDefects as md
    import ART.ModuleMirror as mm
    import ART.ModuleOpticalElement as moe
    import ART.ModuleProcessing as mp
    import ART.ModuleSource as msrc
    import ART.ModuleSupport as ms
    from attosecondraytracing_amd.bundle import RayBundle
    import freeform_common as fc

    n = int(args.rays)
    p, q, graz = 1000.0, 300.0, 2.0
    src = msrc.PointSource(np.zeros(3), np.array([1.0, 0.0, 0.0]), 1e-3, n, Wavelength=30e-6)
    be = src.backend
    S = ms.SupportRectangle(200.0, 20.0)              # footprint: +-29 mm x +-1 mm -- every ray hits
    conic = mm.MirrorEllipticalCylinder(S, p, q, graz)
    th = np.deg2rad(90.0 - graz)
    pose = (np.array([p, 0.0, 0.0]), np.array([-np.cos(th), 0.0, np.sin(th)]), np.array([np.sin(th), 0.0, np.cos(th)]))
    d_conic, _ = mp.element_descriptor(moe.OpticalElement(conic, *pose), True, be)
    co = conic._quadric_coefficients()
    out = RayBundle.allocate(n, like=src, backend=be)
    vin, vout = src.view(), out.view()

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

    res = {"rays": n, "reps": args.reps, "alive_before": int(src.alive.sum()), "bytes_per_ray": 57 + 65}
    quadric = lambda: be.trace_quadric(d_conic, co, vin, vout, n)
    res["quadric"] = [timed(quadric)]
    res["alive_after_quadric"] = int(out.alive.sum())
    k = min(args.sample, n)
    host = src.data[:, :k].cpu().numpy()
    sample = (host[0:3].T.copy(), host[3:6].T.copy(), host[6].copy(), src.alive[:k].cpu().numpy())
    for order in ORDERS:
        M = mm.MirrorFreeform(conic, figure_of_order(md, S, order))
        oe = moe.OpticalElement(M, *pose)
        d, _ = mp.element_descriptor(oe, True, be)
        table, R, N = M._freeform_figure()
        fig = (be.from_numpy(table), R, N)
        r = timed(lambda: be.trace_freeform(d, co, fig, vin, vout, n))
        r["alive_after"] = int(out.alive.sum())
        twin = fc.trace(fc.element_spec(oe), *sample, T=np.float64, device=True)
        r["newton_steps_mean"] = float(twin["nsteps"][twin["alive"]].mean())
        r["newton_steps_max"] = int(twin["nsteps"][twin["alive"]].max())
        res[f"freeform_order_{order}"] = r
        res["quadric"].append(timed(quadric))
    qu = min(t["median_ms"] for t in res["quadric"])
    res["quadric_median_ms"] = qu
    for order in ORDERS:
        r = res[f"freeform_order_{order}"]
        r["ratio_over_quadric"] = r["median_ms"] / qu
        r["TB_per_s"] = n * (57 + 65) / (r["median_ms"] * 1e-3) / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()

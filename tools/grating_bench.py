#!/usr/bin/env python3
"""Time art_trace_grating beside art_trace_element ("Gratings"): a point source on one toroid at grazing
incidence, 1e7 rays by default.  nw = 1 without groove output moves art_trace_element's bytes (57 B read, 65 B written
per ray); the fan-out (nw = 16 in one call) is set against 16 single-wavelength calls.  Every figure: HIP events around
ONE call, after warm-up calls, median and min..max over `reps` calls.

    python tools/grating_bench.py [rays] [--reps 30]"""
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
    ap.add_argument("--fan", type=int, default=16)
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
    src = msrc.PointSource(np.zeros(3), np.array([1.0, 0.0, 0.0]), 2e-3, n, Wavelength=30e-6)
    be = src.backend
    tor = mm.MirrorToroidal(5600.0, 50.0, ms.SupportRectangle(60.0, 10.0))
    G = mm.Grating(tor, 1200.0, -1)
    th = np.deg2rad(87.0)
    pose = (np.array([237.0, 0.0, 0.0]), np.array([-np.cos(th), 0.0, np.sin(th)]), np.array([np.sin(th), 0.0, np.cos(th)]))
    d_bare, _ = mp.element_descriptor(moe.OpticalElement(tor, *pose), True, be)
    d_grat, _ = mp.element_descriptor(moe.OpticalElement(G, *pose), True, be)
    wls = [float(w) for w in np.linspace(10e-6, 40e-6, args.fan)]
    outs = [RayBundle.allocate(n, like=src, backend=be) for _ in wls]
    q = G._groove_vector()

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

    vin, v0 = src.view(), outs[0].view()
    views = [b.view() for b in outs]
    import ctypes as C
    from attosecondraytracing_amd import _abi
    keep = []

    def grating_call(lo, hi):
        """art_trace_grating for wavelengths [lo, hi) with its device arrays built ONCE: the timed call is the launch alone."""
        k = hi - lo
        wl_host = (C.c_double * k)(*wls[lo:hi])
        varr = (_abi.ArtBundleView * k)(*views[lo:hi])
        wl_dev = be.from_numpy(np.asarray(wls[lo:hi], dtype=np.float64))
        v_dev = be.from_numpy(np.frombuffer(bytes(varr), dtype=np.uint8).copy())
        g = _abi.ArtGratingDesc()
        g.q[0], g.q[1] = q
        g.lines_per_mm, g.order, g.nw = G.lines_per_mm, G.order, k
        g.wavelengths, g.outs = wl_dev.data_ptr(), v_dev.data_ptr()
        keep.append((wl_host, varr, wl_dev, v_dev, g))
        sp = be.stream_ptr()
        return lambda: be.check(be.fn["art_trace_grating"](C.byref(d_grat), C.byref(g), wl_host, varr, C.byref(vin), n, sp),
                                "art_trace_grating")
    one, fan = grating_call(0, 1), grating_call(0, args.fan)
    each = [grating_call(j, j + 1) for j in range(args.fan)]
    res = {"rays": n, "alive_after": None, "reps": args.reps, "fan": args.fan}
    res["element"] = timed(lambda: be.trace_element(d_bare, vin, v0, n))
    res["grating_nw1"] = timed(one)
    res["alive_after"] = int(outs[0].alive.sum())
    res["element_again"] = timed(lambda: be.trace_element(d_bare, vin, v0, n))
    res["fan_one_call"] = timed(fan, warm=2)

    def singles():
        for call in each:
            call()
    res["fan_single_calls"] = timed(singles, warm=2)
    res["ratio_grating_over_element"] = res["grating_nw1"]["median_ms"] / res["element"]["median_ms"]
    res["ratio_fan_over_singles"] = res["fan_one_call"]["median_ms"] / res["fan_single_calls"]["median_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

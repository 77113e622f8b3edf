#!/usr/bin/env python3
"""Time art_wavefront on relay4's final bundle -- 1e6 and 1e7 rays at orders 4, 8 and 10, and one batch of 10 bundles x
1e6 rays at order 8 -- each bracketed by HIP events over `reps` back-to-back calls, and print the rate by the flop count
2 K (K + 1) / 2 per ray (one FMA per entry of G's upper triangle) against the 78.6 TF fp64 spec.  Beside it, a plain
torch reference on the device (the design matrix in chunks of 2^20 rays, then torch.matmul) is timed, and the two must
agree to 1e-10 of the largest coefficient.  Kernel times come from a rocprofv3 --kernel-trace --stats run of this
script:

    python tools/wavefront_bench.py [--reps 5] [--quick]"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEC_TF = 78.6
CASES = [(10 ** 6, 4), (10 ** 6, 8), (10 ** 6, 10), (10 ** 7, 4), (10 ** 7, 8), (10 ** 7, 10)]


def torch_gram(B, det, ref_path, order, radius, chunk=1 << 20):
    """G of wavefront.py's model with torch ops on the device: W, pupil coordinates, the Andersen recurrences, matmul."""
    import torch
    d = det._desc()
    C = torch.tensor(d.centre[:], dtype=torch.float64, device=B.data.device)
    nr = torch.tensor(d.normal[:], dtype=torch.float64, device=B.data.device)
    rot = torch.tensor(d.rot[:], dtype=torch.float64, device=B.data.device).reshape(3, 3)
    n = B.n_slots
    K = (order + 1) * (order + 2) // 2 + 2
    G = torch.zeros((K, K), dtype=torch.float64, device=B.data.device)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        alive = B.alive[lo:hi] != 0
        P, D, L = B.data[0:3, lo:hi], B.data[3:6, lo:hi], B.data[6, lo:hi]
        W = (L - ref_path) + (D * (C[:, None] - P)).sum(0)
        x, y = (rot[0] @ D) / radius, (rot[1] @ D) / radius
        w = B.intensity[lo:hi] if B.intensity is not None else torch.ones_like(W)
        w = torch.where(alive, w, 0.0)
        rows = [[torch.ones_like(x)], [y, x]]
        for k in range(2, order + 1):
            b, dd, r = rows[k - 1], rows[k - 2], []
            for m in range(k + 1):
                if m == 0:
                    z = x * b[0] + y * b[k - 1]
                elif m == k:
                    z = x * b[k - 1] - y * b[0]
                elif k % 2 and 2 * m == k - 1:
                    z = y * b[k - 1 - m] + x * b[m - 1] - y * b[k - m] - dd[m - 1]
                elif k % 2 and 2 * m == k + 1:
                    z = x * b[m] + y * b[k - 1 - m] + x * b[m - 1] - dd[m - 1]
                elif k % 2 == 0 and 2 * m == k:
                    z = 2.0 * x * b[m] + 2.0 * y * b[m - 1] - dd[m - 1]
                else:
                    z = x * b[m] + y * b[k - 1 - m] + x * b[m - 1] - y * b[k - m] - dd[m - 1]
                r.append(z)
            rows.append(r)
        V = torch.stack([z for r in rows[:order + 1] for z in r] + [nr @ D, W])
        V = torch.where(alive[None, :], V, 0.0)
        G += (V * w[None, :]) @ V.T
    return G


def timed(call, reps):
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
    ap.add_argument("--quick", action="store_true", help="1e6 rays only, no batch")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _lib, wavefront
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    be = _lib.get_backend()
    scenes = {}
    for rays, order in CASES if not args.quick else CASES[:3]:
        if rays not in scenes:
            chain, _ = workloads.build_scene(4, small_n=rays)
            last = chain.get_output_rays()[-1]
            D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
            D.autoplace(last, 600.0)
            scenes[rays] = (last, D)
        B, D = scenes[rays]
        wf = D.get_Wavefront(B, Order=order)
        item = [B, D, wavefront.resolve(Order=order), None]
        item[2]["ref_path"] = wf.ref_path
        jobs = [wavefront._job(item)]
        ms = timed(lambda: be.wavefront(jobs), args.reps)
        K = (order + 1) * (order + 2) // 2 + 2
        tf = 2.0 * K * (K + 1) / 2 * B.n_slots / ms * 1e-9
        Gt = torch_gram(B, D, wf.ref_path, order, wf.pupil_radius)
        ms_t = timed(lambda: torch_gram(B, D, wf.ref_path, order, wf.pupil_radius), max(1, args.reps // 2))
        ct = wavefront.solve(Gt.cpu().numpy(), wf.sum_w)[0]
        c = np.array(list(wf.coefficients.values()))
        err = np.abs(c - ct).max() / np.abs(c).max()
        print(f"{rays:.0e} rays ({B.n_slots} slots, {wf.count} used) order {order:2d} K {K:2d}: {ms:8.3f} ms/call "
              f"{tf:6.2f} TF ({tf / SPEC_TF:.3f} of spec) | torch reference {ms_t:8.3f} ms, x{ms_t / ms:.1f} | "
              f"coefficients agree to {err:.1e}", flush=True)
        assert err <= 1e-10, err
    if not args.quick:
        B, D = scenes[10 ** 6]
        reqs = [(B, D, {"Order": 8, "Shift": 0.05 * k}) for k in range(10)]
        items = []
        for wf, (_, _, kw) in zip(wavefront.wavefronts(reqs), reqs):
            p = wavefront.resolve(**kw)
            p["ref_path"] = wf.ref_path
            items.append([B, D, p, None])
        jobs = [wavefront._job(it) for it in items]
        ms = timed(lambda: be.wavefront(jobs), args.reps)
        K = 47
        tf = 2.0 * K * (K + 1) / 2 * B.n_slots * 10 / ms * 1e-9
        print(f"batch 10 x 1e6 rays order 8: {ms:8.3f} ms/call {tf:6.2f} TF ({tf / SPEC_TF:.3f} of spec)", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time art_sensitivities on relay4's history (1e7 rays x 4 toroids), PerRay off, beside art_ray_tubes on the same history
-- the pass whose transport it shares.  tools/tubes_time.py's protocol: each case is bracketed by HIP events over `reps`
back-to-back calls of the device entry point (job table built once); the cases alternate over `rounds` rounds and the
median, minimum and maximum are printed, with the bytes per ray the pass requests (every group reads the views from its own
element on), the distinct bytes among them (the history once) and the share of 8 TB/s that the requested bytes make of
the call time.

    python tools/sensitivity_time.py [--reps 20] [--rounds 5] [--quick]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.tubes_time import HBM_TBS, timed, tube_bytes  # noqa: E402


def sensitivity_bytes(K, live, w, parts=1):
    """Per slot and group the K + 1 alive bytes; for the slots that count the points and directions of the views from the
    group's own element on (K + 1 for the source and the first element, then one fewer each), w and the last path.
    Returns (requested over all groups, distinct)."""
    views = (K + 1) + sum(K - g + 2 for g in range(1, K + 1))
    per_group = (K + 1) + live * (16 if w else 8)
    return parts * ((K + 1) * per_group + live * 48 * views), (K + 1) + live * (48 * (K + 1) + (16 if w else 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1e6 rays instead of 1e7")
    ap.add_argument("--lib", help="a diagnostic build of the library to time art_sensitivities from, e.g. one compiled "
                                  "with -DART_SENS_PER_WG=3 (give --parts 2 with it)")
    ap.add_argument("--parts", type=int, default=1, help="workgroups per group of the build (6 / ART_SENS_PER_WG)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _abi, _lib, polarisation as pm, sensitivity, tubes
    from attosecondraytracing_amd.ModuleDetector import Detector
    from tools.bench import workloads
    be = _lib.get_backend()
    N = 10 ** 6 if args.quick else 10 ** 7
    chain, _ = workloads.build_scene(4, small_n=N)
    els = list(chain.optical_elements)
    K = len(els)
    bundles = pm.history(chain)
    live = float(torch.stack([b.alive for b in bundles]).all(dim=0).sum()) / N
    w = bundles[-1].intensity is not None
    chief = bundles[-1].data[0:6, 0].cpu().numpy()
    centre = chief[0:3] + 100.0 * chief[3:6]
    det = Detector(centre.copy(), centre, -chief[3:6] / np.linalg.norm(chief[3:6]))
    st = det.readout(bundles[-1], store=False)["stats"]
    origin = tuple(float(v / st[8]) for v in st[9:12])

    sj, sviews, selems, squadrics, _ = sensitivity._job((bundles, els, det, False), origin)
    tj, tviews, telems, tquadrics, keep = tubes._job((bundles, els, _abi.ART_TUBE_POINT, None, False))
    requested, distinct = sensitivity_bytes(K, live, w, args.parts)
    sbe = _lib.HipBackend(path=args.lib) if args.lib else be
    cases = [("art_sensitivities, PerRay off", lambda: sbe.sensitivities([sj], [sviews], [selems], [squadrics]), requested),
             ("art_ray_tubes, PerRay off", lambda: (be.ray_tubes([tj], [tviews], [telems], [tquadrics]), keep),
              tube_bytes(K, live, w, False))]
    for _, call, _ in cases:                                     # warm up every shape of the timed window
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, call, _ in cases:
            times[name].append(timed(call, args.reps))
    print(f"relay4 history, {N:.0e} rays x {K} toroids, {live:.3f} of the slots alive in every view, {args.rounds} rounds of "
          f"{args.reps} calls (call time: two launches and the job-table upload); {6 * (K + 1)} degrees of freedom")
    med = {}
    for name, _, B in cases:
        t = times[name]
        med[name] = m = statistics.median(t)
        print(f"  {name:34s} {m:8.3f} ms/call (min {min(t):.3f}, max {max(t):.3f}), {B:6.1f} B/ray requested, "
              f"{B * N / m * 1e-9:5.2f} TB/s = {B * N / m * 1e-9 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s", flush=True)
    a, b = (med[name] for name, _, _ in cases)
    print(f"  art_sensitivities: {a / b:.2f} x art_ray_tubes; {distinct:.1f} distinct B/ray (the history once): "
          f"{distinct * N / a * 1e-9 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s")


if __name__ == "__main__":
    main()

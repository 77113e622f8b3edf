#!/usr/bin/env python3
"""Time art_alignment_sums on relay4's history (1e7 rays x 4 toroids) at C = 2, 6 and 8 degrees of freedom, beside what it
replaces on the same build: art_sensitivities with the three per-ray arrays, the torch gather of the chosen rows and three
A @ A.T.  tools/sensitivity_time.py's protocol: each case is bracketed by HIP events over `reps` back-to-back calls (job
tables built once); the cases alternate over `rounds` rounds and the median, minimum and maximum are printed, with the
bytes per ray the pass requests.

    python tools/alignment_time.py [--reps 10] [--rounds 5] [--quick]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.tubes_time import HBM_TBS, timed  # noqa: E402

SETS = {2: [(0, "pitch"), (1, "pitch")],
        6: [(0, "pitch"), (1, "pitch"), (2, "pitch"), (3, "pitch"), (3, "yaw"), ("detector", "shift_normal")],
        8: [("source", "tilt_y"), (0, "pitch"), (1, "pitch"), (2, "pitch"), (3, "pitch"), (3, "yaw"), (3, "roll"),
            ("detector", "shift_normal")]}


def alignment_bytes(K, first, live, w):
    """Per slot the K + 1 alive bytes; for the slots that count the points and directions of the views from the earliest
    chosen element on, w and the last path.  The pilot adds the same for 1024 slots: nothing at this size."""
    return (K + 1) + live * ((16 if w else 8) + 48 * (K + 1 - first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1e6 rays instead of 1e7")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _lib, alignment, polarisation as pm, sensitivity
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

    cases = []
    for Cn, dofs in SETS.items():
        ids = alignment.dof_ids(dofs, K)
        made = alignment._job((bundles, els, det, ids, None), origin)
        first = min(K if c < 0 else max(c // 6 - 1, 0) for c in ids)
        cases.append((f"art_alignment_sums, C = {Cn}", lambda made=made: be.alignment_sums(*[[m] for m in made]),
                      alignment_bytes(K, first, live, w)))
    sj, sviews, selems, squadrics, arrays = sensitivity._job((bundles, els, det, True), origin)
    rows = torch.tensor([c for c in alignment.dof_ids(SETS[6], K) if c >= 0], device=arrays[0].device)

    def replaced():
        be.sensitivities([sj], [sviews], [selems], [squadrics])
        out = []
        for A in arrays:
            G = torch.nan_to_num(A.index_select(0, rows))
            out.append(G @ G.T)
        return out
    M = 6 * (K + 1)
    cases.append(("art_sensitivities PerRay + gather + 3 A @ A.T, C = 5", replaced, 3 * 8 * M + 3 * 8 * 5 * 3))
    for _, call, _ in cases:                                     # warm up every shape of the timed window
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, call, _ in cases:
            times[name].append(timed(call, args.reps))
    print(f"relay4 history, {N:.0e} rays x {K} toroids, {live:.3f} of the slots alive in every view, {args.rounds} rounds of "
          f"{args.reps} calls")
    for name, _, B in cases:
        t = times[name]
        m = statistics.median(t)
        print(f"  {name:52s} {m:9.3f} ms/call (min {min(t):.3f}, max {max(t):.3f}), {B:7.1f} B/ray requested"
              f"{' (stores and gathers alone)' if 'gather' in name else ''}, {B * N / m * 1e-9 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s",
              flush=True)


if __name__ == "__main__":
    main()

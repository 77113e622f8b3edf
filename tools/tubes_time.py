#!/usr/bin/env python3
"""Time art_ray_tubes on relay4's history (1e7 rays x 4 toroids) beside art_polarisation with the ideal coating on the
same history -- the pass that reads the same views and is the yardstick.  Each case is bracketed by HIP events over `reps`
back-to-back calls of the device entry point (job table built once); the three cases alternate over `rounds` rounds and
the median, minimum and maximum are printed, with the bytes per ray the pass must move (the streams it reads and writes)
and the share of 8 TB/s that they make of the call time.

    python tools/tubes_time.py [--reps 50] [--rounds 5] [--quick]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0


def timed(call, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def tube_bytes(K, live, w, per_ray):
    """Streams of one slot: K + 1 alive bytes; for the slots that count the K + 1 points and directions and w; the weight
    written for every slot, seven more doubles with PerRay."""
    return (K + 1) + live * (48 * (K + 1) + (8 if w else 0)) + 8 + (56 if per_ray else 0)


def polarisation_bytes(K, live, w):
    """tools/polarisation_bench.py's count: two alive bytes, w0 and w, K + 1 directions, w_out."""
    return 2 + 8 * (1 + live) * (1 if w else 0) + live * 24 * (K + 1) + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1e6 rays instead of 1e7")
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    from attosecondraytracing_amd import _abi, _lib, polarisation as pm, tubes
    from attosecondraytracing_amd.coating import Coating
    from tools.bench import workloads
    be = _lib.get_backend()
    N = 10 ** 6 if args.quick else 10 ** 7
    chain, _ = workloads.build_scene(4, small_n=N)
    els = list(chain.optical_elements)
    K = len(els)
    bundles = pm.history(chain)
    live = float(torch.stack([b.alive for b in bundles]).all(dim=0).sum()) / N
    w = bundles[-1].intensity is not None

    def tube_call(per_ray):
        j, views, elems, quadrics, keep = tubes._job((bundles, els, _abi.ART_TUBE_POINT, None, per_ray))
        return lambda: (be.ray_tubes([j], [views], [elems], [quadrics]), keep)

    ideal = Coating.ideal()
    coat_list, coat_pos = [], {}
    pj, pviews, pkeep = pm._job((bundles, pm.resolve_coatings(els, ideal), None, None, bundles[-1].wavelength, False),
                                coat_list, coat_pos)
    structs = [c._struct() for c in coat_list]
    cases = [("art_ray_tubes, PerRay off", tube_call(False), tube_bytes(K, live, w, False)),
             ("art_ray_tubes, PerRay on", tube_call(True), tube_bytes(K, live, w, True)),
             ("art_polarisation, ideal coating", lambda: be.polarisation([pj], [pviews], structs), polarisation_bytes(K, live, w))]
    for _, call, _ in cases:                                     # warm up every shape of the timed window
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, call, _ in cases:
            times[name].append(timed(call, args.reps))
    print(f"relay4 history, {N:.0e} rays x {K} toroids, {live:.3f} of the slots alive in every view, {args.rounds} rounds of "
          f"{args.reps} calls (call time: two launches and the job-table upload)")
    med = {}
    for name, _, B in cases:
        t = times[name]
        med[name] = m = statistics.median(t)
        print(f"  {name:34s} {m:8.3f} ms/call (min {min(t):.3f}, max {max(t):.3f}), {B:6.1f} B/ray, "
              f"{B * N / m * 1e-9:5.2f} TB/s = {B * N / m * 1e-9 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s", flush=True)
    ref = med["art_polarisation, ideal coating"]
    for name, _, _ in cases[:2]:
        print(f"  {name}: {med[name] / ref:.2f} x the polarisation pass")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time art_quantiles (Detector.get_EncircledEnergy's device call) on relay4's final bundle (1e7 rays) beside the same
answer by torch.sort + gather + cumsum + searchsorted on the same device tensors.  Three cases: one plane with three
fractions, 16 planes with three fractions, and a tight focus -- given keys that all lie within 1024 ulp of 1.0, so that
every slot shares its leading digits with every other: the case of maximal digit coincidence in the LDS bins.  The torch
path starts from the staged keys and the fixed-point weights (it is not charged for the read-out), the device call
includes the centroid sums and the staging.  Each case is bracketed by HIP events over `reps` back-to-back calls; the cases
alternate over `rounds` rounds and the median, minimum and maximum are printed, with the bytes per ray the device call
must move and the share of 8 TB/s they make of the call time.

    python tools/quantile_time.py [--reps 20] [--rounds 5] [--quick]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
FRACTIONS = (0.5, 0.8, 0.9)


def timed(call, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def metric_bytes(P):
    """Streams of one slot: the centroid sums read the bundle (7 doubles, alive, w) once per 4 planes, the staging reads it
    once (no w) and writes a key per plane, each of the six passes reads key, w and alive per plane."""
    return 65 * ((P + 3) // 4) + 57 + 8 * P + 6 * 17 * P


def given_bytes(P):
    return 6 * 17 * P


def torch_path(keys, q, fractions):
    """values [P, K] by a full sort: what the device call answers without sorting."""
    import torch
    sk, idx = torch.sort(keys, dim=1)
    cum = torch.cumsum(torch.gather(q.expand_as(keys), 1, idx), dim=1)
    W = cum[:, -1:]
    T = torch.clamp(torch.ceil(torch.tensor(fractions, dtype=torch.float64, device=keys.device)[None, :] * W.double()).long(), min=1)
    j = torch.searchsorted(cum, torch.minimum(T, W))
    return torch.gather(sk, 1, j.clamp(max=keys.shape[1] - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1e6 rays instead of 1e7")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    import ART.ModuleDetector as mdet
    from attosecondraytracing_amd import _abi, _lib, quantile
    from tools.bench import workloads
    be = _lib.get_backend()
    N = 10 ** 6 if args.quick else 10 ** 7
    chain, _ = workloads.build_scene(4, small_n=N)
    last = chain.get_output_rays()[-1]
    det = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    det.autoplace(last, 600.0)
    n = last.n_slots
    w = last.intensity
    shift = quantile._shift_from(n, None if w is None else quantile._weight_range(w[:n]).cpu().numpy())
    alive = last.alive[:n] != 0
    q = torch.where(alive, torch.ones(n, dtype=torch.int64, device=be.device) if w is None
                    else torch.round(torch.ldexp(w[:n], torch.tensor(shift, device=be.device))).long(), 0)

    def metric_case(shifts):
        d = quantile._desc(_abi.ART_QKEY_RADIUS, len(shifts), FRACTIONS, shift, None)
        d.det = det._desc()
        for p, s in enumerate(shifts):
            d.shift[p] = -s
        view = last.view()
        r = det.readout(last)
        keys = []
        for s in shifts:                                   # the torch path's keys: the radius^2 about the device's centres
            dd = det.copy_detector()
            dd.shiftByDistance(float(s))
            rr = dd.readout(last)
            keys.append((rr["X"], rr["Y"]))
        out = be.quantiles(d, view, w, n, None)
        c = out["centres"]
        K = torch.stack([torch.where(alive, (X - c[p, 0]) ** 2 + (Y - c[p, 1]) ** 2, torch.inf) for p, (X, Y) in enumerate(keys)])
        del r, keys
        return (lambda: be.quantiles(d, view, w, n, None)), (lambda: torch_path(K, q, FRACTIONS)), out, K

    def given_case():
        K = (1.0 + (torch.arange(n, device=be.device) % 1024).double() * 2.0 ** -52).reshape(1, n)
        d = quantile._desc(_abi.ART_QKEY_GIVEN, 1, FRACTIONS, shift, None)
        d.keys, d.alive = K.data_ptr(), last.alive.data_ptr()
        out = be.quantiles(d, None, w, n, None)
        return (lambda: be.quantiles(d, None, w, n, None)), (lambda: torch_path(torch.where(alive, K, torch.inf), q, FRACTIONS)), out, K

    cases = []
    for name, made, B in (("one plane", metric_case([0.0]), metric_bytes(1)),
                          ("16 planes", metric_case(list(np.linspace(-1.5, 1.5, 16))), metric_bytes(16)),
                          ("tight focus (given keys)", given_case(), given_bytes(1))):
        dev, ref, out, K = made
        got = out["values"].cpu().numpy()
        want = ref().cpu().numpy()
        want = np.sqrt(want) if "given" not in name else want
        agree = np.allclose(got, want, rtol=1e-12, atol=0)
        print(f"  {name}: device and torch answers agree: {agree}", flush=True)
        cases.append((name + ", art_quantiles", dev, B))
        cases.append((name + ", torch.sort path", ref, None))
    for _, call, _ in cases:
        for _ in range(2):
            call()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, call, _ in cases:
            times[name].append(timed(call, args.reps))
    print(f"relay4 final bundle, {N:.0e} rays, {float(alive.sum()) / n:.3f} alive, fractions {FRACTIONS}, {args.rounds} rounds of "
          f"{args.reps} calls")
    med = {}
    for name, _, B in cases:
        t = times[name]
        med[name] = m = statistics.median(t)
        line = f"  {name:42s} {m:9.3f} ms/call (min {min(t):.3f}, max {max(t):.3f})"
        if B is not None:
            line += f", {B:6.0f} B/ray, {B * N / m * 1e-9:5.2f} TB/s = {B * N / m * 1e-9 / HBM_TBS:.2f} of {HBM_TBS:.0f} TB/s"
        print(line, flush=True)
    for k in range(0, len(cases), 2):
        a, b = cases[k][0], cases[k + 1][0]
        print(f"  {a}: {med[b] / med[a]:.1f} x faster than the torch path" if med[a] < med[b]
              else f"  {a}: MISSES the bar, {med[a] / med[b]:.2f} x the torch path's time")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time art_focal_chromatic against art_focal_spectrum in ONE process, on the same bundle, grid and wavenumbers (relay4's
final bundle, 1e6 rays x 64^2 x 64 wavenumbers x 1 plane): the two calls alternate, `rounds` times, each
timing bracketed by HIP events over `reps` back-to-back calls after two warm-up calls, and the ratio of the medians is
printed.  The chromatic table has a divergence and a position in every row (no neutral row), so the ratio is the cost of
the two new terms.  Kernel times come from a rocprofv3 --kernel-trace --stats run of this script.

With --retrace the script instead measures the MODEL: the focal field of art_focal_chromatic with every source moved by
z along the axis (z / distance to the first optic = --ratio, default 1e-3) against the focal field of a point source
actually moved by z and traced again, as the relative L2 difference of the two fields (global phase removed) in three
planes.

With --vector the script times art_focal_vector_chromatic against art_focal_vector_spectrum the same way (same history,
grid and wavenumbers; 40-period Mo/Si of constant illustrative indices on relay4's four toroids; host tables included in
both): once with a NEUTRAL table, which is the cost of the table variant itself, and once with every fourth row of it
(a comb that keeps a quarter of the frequencies) over the full call.

    python tools/chromatic_bench.py [--reps 5] [--rounds 3] [--rays 1000000] [--retrace [--ratio 1e-3]] [--vector]"""
import argparse
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIXELS, NK = 64, 64


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


def _scene(rays):
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=rays)
    last = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 600.0)
    return chain, last, D


def _focal_desc(D, last, pix, shifts=None):
    from attosecondraytracing_amd import focal
    return focal.focal_desc(D, last, None, pix, None, shifts, None, None)[0]


def _axis(src):
    import ART.ModuleProcessing as mp
    a = np.asarray(mp.FindCentralRay(src).vector, dtype=float)
    return a / np.linalg.norm(a)


def bench(args):
    from attosecondraytracing_amd import _abi, _lib
    be = _lib.get_backend()
    chain, last, D = _scene(args.rays)
    src = chain.source_rays
    n = last.n_slots
    fd = _focal_desc(D, last, PIXELS)
    k = fd.k
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.f.k, sd.dk, sd.nk = 0.9 * k, 0.2 * k / (NK - 1), NK
    cd = _abi.ArtFocalChromaticDesc()
    cd.f = fd
    for i, v in enumerate(_axis(src)):
        cd.axis[i] = v
    kj = sd.f.k + np.arange(NK) * sd.dk
    theta = 0.015 * k / kj                                   # narrower with the order, as a harmonic's
    table = np.stack([kj, 2 / theta ** 2, np.linspace(-1.0, 1.0, NK), np.zeros(NK)], axis=1)
    fv, sv = last.view(), src.view()
    spectrum = lambda: be.focal_spectrum(sd, fv, last.intensity, n)
    chromatic = lambda: be.focal_chromatic(cd, fv, sv, last.intensity, n, table)
    ts, tc = [], []
    for _ in range(args.rounds):
        ts.append(_time(spectrum, args.reps))
        tc.append(_time(chromatic, args.reps))
    ms, mc = statistics.median(ts), statistics.median(tc)
    flops = 8.0 * n * PIXELS * PIXELS * NK
    print(f"{args.rays:.0e} rays ({n} slots, {len(last)} alive) x {PIXELS}^2 x {NK} wavenumbers x 1 plane, "
          f"{args.rounds} rounds of {args.reps} calls, alternating", flush=True)
    print(f"  art_focal_spectrum  {ms:9.3f} ms/call ({min(ts):.3f}-{max(ts):.3f}) {flops / ms * 1e-9:8.2f} TFLOP/s", flush=True)
    print(f"  art_focal_chromatic {mc:9.3f} ms/call ({min(tc):.3f}-{max(tc):.3f}) {flops / mc * 1e-9:8.2f} TFLOP/s", flush=True)
    print(f"  ratio chromatic / spectrum {mc / ms:.4f}", flush=True)


def vector(args):
    from attosecondraytracing_amd import _abi, polarisation, vector_pulse
    from attosecondraytracing_amd.coating import Coating
    chain, last, D = _scene(args.rays)
    bundles = polarisation.history(chain)
    n = last.n_slots
    fd = _focal_desc(D, last, PIXELS)
    k = fd.k
    sd = _abi.ArtFocalSpectrumDesc()
    sd.f = fd
    sd.f.k, sd.dk, sd.nk = 0.9 * k, 0.2 * k / (NK - 1), NK
    kj = sd.f.k + np.arange(NK) * sd.dk
    si, mo = (0.0010, 0.0018), (0.0769, 0.0064)              # illustrative (delta, beta) at 13.5 nm
    coat = Coating(si, [(si, 4.1e-6, 0.3e-6), (mo, 2.8e-6, 0.3e-6)] * 40, Roughness=0.3e-6)
    coats = polarisation.resolve_coatings(list(chain.optical_elements), coat)
    P = np.array([0.0, 1.0, 0.0], dtype=complex)
    axis = _axis(chain.source_rays)
    table = np.stack([kj, 0 * kj, 0 * kj, 0 * kj], axis=1)
    quarter = table[::4]
    sq = _abi.ArtFocalSpectrumDesc.from_buffer_copy(sd)
    sq.nk = len(quarter)
    spectrum = lambda: vector_pulse._vector_spectrum(bundles, coats, P, sd, 2 * np.pi / kj, None)
    chromatic = lambda: vector_pulse._vector_spectrum(bundles, coats, P, sd, 2 * np.pi / kj, None, chromatic=(axis, table))
    comb = lambda: vector_pulse._vector_spectrum(bundles, coats, P, sq, 2 * np.pi / quarter[:, 0], None,
                                                 chromatic=(axis, quarter))
    same = spectrum().cpu().numpy().tobytes() == chromatic().cpu().numpy().tobytes()
    ts, tc, tq = [], [], []
    for _ in range(args.rounds):
        ts.append(_time(spectrum, args.reps))
        tc.append(_time(chromatic, args.reps))
        tq.append(_time(comb, args.reps))
    ms, mc, mq = statistics.median(ts), statistics.median(tc), statistics.median(tq)
    print(f"{args.rays:.0e} rays ({n} slots, {len(last)} alive) x {PIXELS}^2 x {NK} wavenumbers x 1 plane x 3 components, "
          f"4 x 80 layers, {args.rounds} rounds of {args.reps} calls, alternating; neutral table = the spectrum's bytes: {same}",
          flush=True)
    print(f"  art_focal_vector_spectrum                {ms:9.3f} ms/call ({min(ts):.3f}-{max(ts):.3f})", flush=True)
    print(f"  art_focal_vector_chromatic, {NK} rows      {mc:9.3f} ms/call ({min(tc):.3f}-{max(tc):.3f})", flush=True)
    print(f"  art_focal_vector_chromatic, {len(quarter)} rows      {mq:9.3f} ms/call ({min(tq):.3f}-{max(tq):.3f})", flush=True)
    print(f"  ratio chromatic / spectrum {mc / ms:.4f}; comb of {len(quarter)} / all {NK} rows {mq / mc:.4f} "
          f"(kept fraction {len(quarter) / NK:.4f})", flush=True)


def retrace(args):
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd import ModuleGeometry as mgeo
    from attosecondraytracing_amd import _abi, _lib
    be = _lib.get_backend()
    chain, last, D = _scene(args.rays)
    src = chain.source_rays
    n = last.n_slots
    axis = _axis(src)
    first = np.asarray(chain.optical_elements[0].position, dtype=float)
    origin = np.asarray(mp.FindCentralRay(src).point, dtype=float)
    distance = float(np.linalg.norm(first - origin))
    print(f"{args.rays:.0e} rays, {PIXELS}^2 pixels; the first optic is {distance:.1f} mm from the source", flush=True)
    for sign in (1.0, -1.0):
        z = sign * args.ratio * distance
        planes = (-z, 0.0, z)
        fd = _focal_desc(D, last, PIXELS, planes)
        cd = _abi.ArtFocalChromaticDesc()
        cd.f = fd
        for i, v in enumerate(axis):
            cd.axis[i] = v
        model = be.focal_chromatic(cd, last.view(), src.view(), last.intensity, n, np.array([[fd.k, 0.0, z, 0.0]]))[:, 0]
        still = be.focal_field(fd, last.view(), last.intensity, n)
        moved = mp.RayTracingCalculation(mgeo.TranslationRayList(src, z * axis), chain.optical_elements)[-1]
        assert moved.n_slots == n
        truth = be.focal_field(fd, moved.view(), last.intensity, n)
        for q, v in enumerate(planes):
            t = truth[q].reshape(-1)

            def rel(e):      # min over a global phase of |e - exp(i phi) t| / |t|
                e = e.reshape(-1)
                num = (e.abs() ** 2).sum() + (t.abs() ** 2).sum() - 2 * (e.conj() * t).sum().abs()
                return math.sqrt(max(float(num), 0.0) / float((t.abs() ** 2).sum()))

            print(f"  z = {z:+.3f} mm (k z u_max = {fd.k * abs(z) * 0.5 * 0.02 ** 2:.1f} rad), plane shifted by {v:+.3f} mm: "
                  f"relative L2 difference model - retraced {rel(model[q]):.3e}; unmoved source - retraced {rel(still[q]):.3e}",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rays", type=int, default=10 ** 6)
    ap.add_argument("--retrace", action="store_true")
    ap.add_argument("--ratio", type=float, default=1e-3)
    ap.add_argument("--vector", action="store_true")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.ensure_built()
    (retrace if args.retrace else vector if args.vector else bench)(args)


if __name__ == "__main__":
    main()

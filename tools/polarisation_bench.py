#!/usr/bin/env python3
"""Time art_polarisation, each case bracketed by HIP events over `reps` back-to-back calls of the device entry point
(job table built once), and print bytes per ray -- the streams the kernel actually reads and writes -- with the share
of 8 TB/s, or for the multilayer case the fp64 work per ray and element.  Cases:

  (a) relay4's history, 1e7 rays x 4 toroids, a gold-like single-layer coating, unpolarised, no per-ray field
  (b) the same, polarised, PerRay=True
  (c) 1e7 rays x 1 normal-incidence plane mirror, a 40-period Mo/Si-like stack (80 layers, with roughness)
  (d) the 10 chains of C3 x 1e6 rays in one call

Kernel times (k_polarisation, k_polarisation_fold) come from a rocprofv3 --kernel-trace --stats run of this script:

    python tools/polarisation_bench.py [--reps 10] [--quick]"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 8.0


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


def bytes_per_ray(K, live, w, per_ray):
    """Streams of one slot: alive bytes of source and final bundle, w0 (source-alive) and w, the source's and K
    bundles' directions (alive slots), w_out written; the field (48 B) with PerRay.  `live`: the alive fraction."""
    return 2 + 8 * (1 + live) * (1 if w else 0) + live * 24 * (K + 1) + 8 + (48 if per_ray else 0)


def prepared(be, reqs):
    """The device call of polarisations(reqs) with its job table built once: a closure for the timing loop."""
    from attosecondraytracing_amd import polarisation as pm
    items = []
    for chain, coats, kw in reqs:
        els = chain.optical_elements
        out = chain.get_output_rays()
        bundles = [chain.source_rays] + [out[k] for k in range(len(els))]
        P = pm._state(kw.get("Polarisation"))
        items.append((bundles, pm.resolve_coatings(els, coats), P, kw.get("Detector"), bundles[-1].wavelength,
                      bool(kw.get("PerRay", False))))
    coat_list, coat_pos = [], {}
    made = [pm._job(it, coat_list, coat_pos) for it in items]
    jobs, views = [m[0] for m in made], [m[1] for m in made]
    structs = [c._struct() for c in coat_list]
    return lambda: be.polarisation(jobs, views, structs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="1e6 rays instead of 1e7")
    args = ap.parse_args()
    import torch
    import __graft_entry__
    __graft_entry__.ensure_built()
    import polarisation_common as pcm
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalElement as moe
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd import _lib
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain, trace_chain_list
    from tools.bench import workloads
    be = _lib.get_backend()
    N = 10 ** 6 if args.quick else 10 ** 7
    gold, mosi = pcm.gold(), pcm.mosi(40)

    chain, _ = workloads.build_scene(4, small_n=N)
    out = chain.get_output_rays()
    live = float(out[-1].alive.sum()) / N
    w = chain.source_rays.intensity is not None
    for tag, kw in (("a", {}), ("b", {"Polarisation": (1, 0, 0), "PerRay": True})):
        ms = timed(prepared(be, [(chain, gold, kw)]), args.reps)
        B = bytes_per_ray(4, live, w, tag == "b")
        print(f"({tag}) relay4 {N:.0e} rays x 4 toroids, gold, {'polarised + field' if kw else 'unpolarised'}: "
              f"{ms:8.3f} ms/call, {B:.0f} B/ray, {B * N / ms * 1e-9:6.2f} TB/s = {B * N / ms * 1e-9 / HBM_TBS:.2f} of "
              f"{HBM_TBS:.0f} TB/s (call time)", flush=True)
    del chain, out
    torch.cuda.empty_cache()

    # (c) a plane mirror at normal incidence: rays along +z onto a mirror facing -z (a stand-in source, in place)
    src = RayBundle.allocate(N, backend=be)
    src.data[0:2].uniform_(-1.0, 1.0)
    src.data[2].zero_()
    src.data[3:5].uniform_(-1e-3, 1e-3)
    src.data[5].fill_(1.0)
    src.data[3:6] /= torch.linalg.norm(src.data[3:6], dim=0)
    src.data[6:8].zero_()
    src.alive.fill_(1)
    src.wavelength = 13.5e-6
    src.touch()
    M = mmirror.MirrorPlane(msupp.SupportRectangle(40, 40))
    el = moe.OpticalElement(M, np.array([0.0, 0.0, 100.0]), np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0]))
    ch1 = OpticalChain(src, [el])
    live1 = float(ch1.get_output_rays()[-1].alive.sum()) / N
    ms = timed(prepared(be, [(ch1, mosi, {})]), args.reps)
    L = 80
    # per ray and layer: one interface (2 complex divisions, 2 products, the roughness factor: exp + sincos + 3
    # products) and one Parratt step for s and p (phase: exp + sincos; 4 products, 2 divisions)
    print(f"(c) 1 mirror at normal incidence, Mo/Si x 40 (80 layers, roughness), {N:.0e} rays (alive {live1:.2f}): "
          f"{ms:8.3f} ms/call = {ms * 1e9 / (N * L):.2f} ps per ray and layer (call time)", flush=True)
    del ch1, src
    torch.cuda.empty_cache()

    # (d) C3: mask + 2 toroids, 10 twists, one shared source of 1e6 rays
    SP = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": N // 10}
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 41e-3 / 2 * 500, 0, 0))
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    chains = mp.OEPlacement(SP, [Mask, Tor, Tor], [500, 100, 600], [0, 80, -80], [0, 0, np.linspace(-90, 90, 10).tolist()], "C3")
    trace_chain_list(chains)
    n3 = chains[0].source_rays.n_slots
    lv = np.mean([float(c.get_output_rays()[-1].alive.sum()) / n3 for c in chains])
    ms = timed(prepared(be, [(c, gold, {}) for c in chains]), args.reps)
    B = bytes_per_ray(3, lv, chains[0].source_rays.intensity is not None, False)
    print(f"(d) C3 10 chains x {n3:.0e} rays in one call: {ms:8.3f} ms/call, {B:.0f} B/ray, "
          f"{B * n3 * 10 / ms * 1e-9:6.2f} TB/s (call time)", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""In-process A/B of the row summaries (include/art_hip.h: art_bundle_row_summary): one eager SceneProgram per configuration
-- the same output bundles for every variant -- with ART_ROW_SUMMARY, which the library reads at every launch, alternating
round by round.  Variants: off, off again (what identical passes differ by), on.  tools/ab_kernel.py's protocol: 80 ms of
load first, one warm-up round, every launch (trace + fold) bracketed by HIP events.  Also times the summary kernel itself.

    python tools/ab_row_summary.py [relay4 C4 C5]

Prints one JSON line per configuration (profiles/r06_row_summary.md holds the recorded ones)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from tools.bench import workloads
    from attosecondraytracing_amd import _lib
    from attosecondraytracing_amd.graph import SceneProgram
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    be = _lib.get_backend()
    rounds, launches = 12, 20
    for cfg in sys.argv[1:] or ["relay4", "C4", "C5"]:
        W = workloads.select(cfg)
        els, n, ign = W["element_lists"][0], W["n"], W["ignore_defects"]
        src = bench.device_source(n, 0, n, be, W["src_kind"], W["wavelength"])
        out = mp.RayTracingCalculation(src, els, IgnoreDefects=ign)
        det = mdet.Detector(np.asarray(els[-1].position, dtype=float))
        det.autoplace(out[-1], W["det_dist"])
        del out
        prog = SceneProgram([src], [els], IgnoreDefects=ign, capture=False, detectors=[det])
        variants = [("off", "0"), ("off_again", "0"), ("on", None)]
        times = {v: [] for v, _ in variants}
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.08:
            prog.run()
        torch.cuda.synchronize()
        for rnd in range(rounds + 1):
            for v, env in variants:
                if env is None:
                    os.environ.pop("ART_ROW_SUMMARY", None)
                else:
                    os.environ["ART_ROW_SUMMARY"] = env
                be.trace_events = []
                for _ in range(launches):
                    prog.run()
                torch.cuda.synchronize()
                ev, be.trace_events = be.trace_events, None
                if rnd > 0:
                    times[v].append(float(np.mean([a.elapsed_time(b) for a, b in ev])))
        os.environ.pop("ART_ROW_SUMMARY", None)
        off, again, on = (np.array(times[v]) for v in ("off", "off_again", "on"))
        # the summary kernel itself
        buf = torch.empty(be.row_summary_bytes(), dtype=torch.uint8, device=be.device)
        ts = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            be.bundle_row_summary(src.view(), src.intensity, n, buf)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        raw = buf.cpu().numpy()
        res = {"rays": n, "elements": len(els), "rounds": rounds, "launches": launches,
                    "off_ms": [round(x, 4) for x in off], "off_again_ms": [round(x, 4) for x in again], "on_ms": [round(x, 4) for x in on],
                    "median_off": float(np.median(off)), "median_off_again": float(np.median(again)), "median_on": float(np.median(on)),
                    "ratio_on_off": float(np.median(on) / np.median(off)),
                    "ratio_again_off": float(np.median(again) / np.median(off)),
                    "per_round_ratio_again_off": [round(float(x), 4) for x in again / off],
                    "per_round_ratio_on_off": [round(float(x), 4) for x in on / off],
                    "summary_kernel_ms": [round(x, 4) for x in ts], "summary_differs": hex(int(raw[0:4].view(np.uint32)[0]))}
        print(cfg, json.dumps(res), flush=True)
        del prog, src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

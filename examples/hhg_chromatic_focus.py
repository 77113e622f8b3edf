#!/usr/bin/env python3
"""The attosecond pulse at the focus of a toroid pair when the source is a comb of high harmonics (orders 11 to 41 of
800 nm) that is NOT achromatic: every harmonic leaves a waist of 10 um with its own divergence, and its apparent source
slides along the axis with the order, from 10 mm upstream to 10 mm downstream.  The harmonics then focus in different
planes, and the plane of the shortest pulse is not the geometric focus.  One device call sums all lines and planes; the
frequencies between the lines cost nothing.

    python examples/hhg_chromatic_focus.py [--rays 100000] [--pixels 32] [--show]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ART.ModuleAnalysisAndPlots as mplots
import ART.ModuleDetector as mdet
import ART.ModuleMirror as mmirror
import ART.ModuleProcessing as mp
import ART.ModuleSupport as msupp
from attosecondraytracing_amd import chromatic

FUNDAMENTAL = 800e-6                 # mm
ORDERS = np.arange(11, 42, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=100000)
    ap.add_argument("--pixels", type=int, default=32)
    ap.add_argument("--show", action="store_true")
    args = ap.parse_args()
    centre = FUNDAMENTAL / 26                                # the middle of the comb
    source = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": centre, "DeltaFT": 0.24, "NumberRays": args.rays}
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    toroid = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    chain = mp.OEPlacement(source, [toroid, toroid], [600, 1200], [80, -80], [0, 0], "toroid pair, 1:1")
    det = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    det.autoplace(chain.get_output_rays()[-1], 600.0)

    omega1 = 2 * np.pi * chromatic.C_MM_PER_FS / FUNDAMENTAL
    comb = chromatic.harmonic_comb(FUNDAMENTAL, ORDERS, LineDeltaFT=10.0)
    position = lambda omega: 20.0 * (omega / omega1 - 26) / 30          # mm: -10 at order 11, +10 at order 41
    kw = dict(Divergence=chromatic.gaussian_divergence(0.01), Spectrum=comb, Pixels=args.pixels,
              Shifts=np.linspace(-15.0, 15.0, 13), TimeWindow=63.0, Times=1024)
    moving = chain.get_ChromaticFocalPulse(det, 0.24, Position=position, **kw)
    fixed = chain.get_ChromaticFocalPulse(det, 0.24, **kw)
    lines = int((np.abs(moving.weights) > 0).sum())
    print(f"{len(moving.omega)} frequencies on the grid, {lines} of them on the {len(ORDERS)} lines")
    print("shift (mm)   Strehl, duration (as): source fixed     source sliding with the order")
    for q, s in enumerate(moving.shifts):
        print(f"{s:9.2f}       {fixed.strehl[q]:8.4f} {fixed.duration[q] * 1e3:9.1f}        "
              f"{moving.strehl[q]:8.4f} {moving.duration[q] * 1e3:9.1f}")
    for order in (11, 21, 31, 41):
        j = int(np.argmin(np.abs(moving.omega - order * omega1)))
        print(f"harmonic {order}: divergence {moving.divergence[j] * 1e3:.3f} mrad, source at {moving.position[j]:+.2f} mm, "
              f"best focus at shift {moving.best_focus[j]:+.2f} mm")
    fig = mplots.ChromaticFocus(moving)
    if args.show:
        mplots.show()
    return fig


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The attosecond pulse train at the focus of a COATED toroid pair when the source is a comb of high harmonics (orders
11 to 41 of 800 nm) that is not achromatic: examples/hhg_chromatic_focus.py's source -- every harmonic with its own
divergence and its own apparent source position -- behind mirrors that do not reflect every harmonic alike.  The
chromatic source sets which harmonic focuses where, the coating which harmonics survive and with what group delay; one
device call (art_focal_vector_chromatic) sums both for all lines, planes and field components, and the frequencies
between the lines cost nothing.

The coatings are ILLUSTRATIVE: a thick B4C layer, or 40 periods of Mo/Si, whose (delta, beta) follow made-up smooth power
laws through plausible 13.5 nm values (coating.Material tables).  Put tabulated optical constants in their place for a
real mirror.

    python examples/hhg_coated_focus.py [--coating b4c|mosi] [--rays 100000] [--pixels 32] [--show]"""
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
from attosecondraytracing_amd.coating import Coating, Material

FUNDAMENTAL = 800e-6                 # mm
ORDERS = np.arange(11, 42, 2)


def power_law(delta0, beta0, wl0=13.5e-6, lo=15e-6, hi=90e-6, nodes=61):
    """An illustrative Material: delta ~ wavelength and beta ~ wavelength^1.5 through (delta0, beta0) at wl0."""
    wl = np.linspace(lo, hi, nodes)
    return Material(wl, delta=delta0 * (wl / wl0), beta=beta0 * (wl / wl0) ** 1.5)


def coating(name):
    if name == "b4c":
        b4c = power_law(0.0364, 0.0044)
        return Coating(power_law(0.0010, 0.0018), [(b4c, 30e-6, 0.5e-6)], Roughness=0.3e-6)     # 30 nm B4C on silicon
    si, mo = power_law(0.0010, 0.0018), power_law(0.0769, 0.0064)
    return Coating(si, [(si, 4.1e-6, 0.3e-6), (mo, 2.8e-6, 0.3e-6)] * 40, Roughness=0.3e-6)


def shares(pulse, omega1, plane):
    """The share of plane `plane`'s spectral energy (summed over pixels and components) that every harmonic holds."""
    sp = pulse.spectrum[plane].cpu().numpy()
    per_freq = (np.abs(sp) ** 2).reshape(sp.shape[0], -1).sum(axis=1)
    nearest = np.rint(pulse.omega / omega1)
    per_order = np.array([per_freq[nearest == q].sum() for q in ORDERS])
    return per_order / per_order.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--coating", choices=("b4c", "mosi"), default="b4c")
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
    kw = dict(Divergence=chromatic.gaussian_divergence(0.01), Position=position, Spectrum=comb, Pixels=args.pixels,
              Shifts=np.linspace(-15.0, 15.0, 13), TimeWindow=63.0, Times=1024)
    bare = chain.get_ChromaticFocalPulse(det, 0.24, **kw)
    coated = chain.get_ChromaticFocalPulse(det, 0.24, Coatings=coating(args.coating), Polarisation=(0.0, 1.0, 0.0), **kw)
    lines = int((np.abs(coated.weights) > 0).sum())
    print(f"{len(coated.omega)} frequencies on the grid, {lines} of them on the {len(ORDERS)} lines; coating: {args.coating}")
    print("shift (mm)   Strehl, duration (as): without coatings     behind the coated toroids")
    for q, s in enumerate(coated.shifts):
        print(f"{s:9.2f}       {bare.strehl[q]:8.4f} {bare.duration[q] * 1e3:9.1f}            "
              f"{coated.strehl[q]:8.4f} {coated.duration[q] * 1e3:9.1f}")
    plane = int(np.argmin(np.abs(coated.shifts)))
    before, after = shares(bare, omega1, plane), shares(coated, omega1, plane)
    print(f"share of the fluence per harmonic in the plane of shift {coated.shifts[plane]:+.2f} mm, and its best focus:")
    for i, order in enumerate(ORDERS):
        j = int(np.argmin(np.abs(coated.omega - order * omega1)))
        print(f"  harmonic {order}: without coatings {before[i]:6.3f}, coated {after[i]:6.3f}; best focus at shift "
              f"{coated.best_focus[j]:+.2f} mm")
    fig = mplots.ChromaticFocus(coated)
    if args.show:
        mplots.show()
    return fig


if __name__ == "__main__":
    main()

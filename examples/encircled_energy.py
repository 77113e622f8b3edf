#!/usr/bin/env python3
"""The foci of examples/kb_focus.py -- a Kirkpatrick-Baez pair of plane-elliptical cylinders at 2 degrees grazing and a
pair of toroids with the same conjugates -- by the figures such optics are specified with: the half-energy width (HEW, the
diameter that holds 50 % of the intensity) and W90, from Detector.get_EncircledEnergy, beside the rms spot; and the time
windows that hold 50 % and 90 % of the intensity.  A grazing-incidence focus has a sharp core and long tails: the rms
measures the tails, the HEW the core.

    python examples/encircled_energy.py [--rays 1000000]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ART.ModuleDetector as mdet
import ART.ModuleMirror as mmirror
import ART.ModuleProcessing as mp
import ART.ModuleSupport as msupp


def report(name, chain, focus_distance):
    last = chain.get_output_rays()[-1]
    u = np.array([1.0, 0.0, 0.0])                  # the central ray, mirrored at every element's normal (kb_focus.py)
    for oe in chain.optical_elements:
        u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(chain.optical_elements[-1].position, dtype=float)
    det = mdet.Detector(pole, pole + focus_distance * u, -u)
    h = det.get_Histogram(last, Bins=(256, 256))
    w = h.counts if h.intensity is None else h.intensity
    cx, cy = [0.5 * (e[1:] + e[:-1]) for e in h.edges]
    mx, my = (w.sum(1) * cx).sum() / w.sum(), (w.sum(0) * cy).sum() / w.sum()
    rms = np.sqrt(((w.sum(1) * (cx - mx) ** 2).sum() + (w.sum(0) * (cy - my) ** 2).sum()) / w.sum())
    spot = det.get_EncircledEnergy(last, Fractions=(0.5, 0.9))
    time = det.get_EncircledEnergy(last, Fractions=(0.5, 0.9), Metric="Delay")
    print(f"{name:28s} {len(last):8d} rays   rms spot {rms * 1e6:10.3f} nm   HEW {spot.hew[0] * 1e6:10.3f} nm   "
          f"W90 {2 * spot.radii[0, 1] * 1e6:10.3f} nm   50 % within +-{time.radii[0, 0] * 1e3:8.3f} as   "
          f"90 % within +-{time.radii[0, 1] * 1e3:8.3f} as")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1000000)
    args = ap.parse_args()
    graz, inc = 2.0, 88.0
    S = msupp.SupportRectangle(150.0, 20.0)
    point = {"Divergence": 1e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": args.rays}
    kb = [mmirror.MirrorEllipticalCylinder(S, 1000.0, 400.0, graz), mmirror.MirrorEllipticalCylinder(S, 1100.0, 300.0, graz)]
    report("KB pair (elliptical cyl.)", mp.OEPlacement(point, kb, [1000.0, 100.0], [inc, inc], [0.0, 90.0], "KB"), 300.0)
    tor = [mmirror.MirrorToroidal(*mmirror.ReturnOptimalToroidalRadii(f, inc), S) for f in (1000.0, 300.0)]
    report("toroid pair", mp.OEPlacement(point, tor, [1000.0, 100.0], [inc, -inc], [0.0, 0.0], "toroids"), 300.0)


if __name__ == "__main__":
    main()

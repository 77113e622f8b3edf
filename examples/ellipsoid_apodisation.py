#!/usr/bin/env python3
"""What the sine condition does to a diffraction-limited focus: a point source imaged 10:1 by an ellipsoid at 5 degrees
grazing.  Every ray of the source stands for the same solid angle in OBJECT space, but the Debye integral runs over
IMAGE-space solid angle, and on this mirror dOmega' / dOmega = (r1 / r2)^2 changes by more than a factor of two along the
footprint.  get_RayTubes gives that factor per ray (differential ray tracing, one device pass) and `tubes.rays`, the final
bundle re-weighted by it; the focal field of either bundle has its peak at the stigmatic focus with a Strehl ratio of 1
-- the phases are the same -- but the spot around it is that of another apodisation.

    python examples/ellipsoid_apodisation.py [--rays 200000]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ART.ModuleDetector as mdet
import ART.ModuleMirror as mmirror
import ART.ModuleProcessing as mp
import ART.ModuleSupport as msupp


def widths(ff):
    """rms half-widths (mm) of the focal intensity along the detector's two axes."""
    I = ff.intensity[0]
    px, py = I.sum(0) / I.sum(), I.sum(1) / I.sum()
    mx, my = (px * ff.x).sum(), (py * ff.y).sum()
    return np.sqrt((px * (ff.x - mx) ** 2).sum()), np.sqrt((py * (ff.y - my) ** 2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=200000)
    args = ap.parse_args()
    p, q, graz = 1000.0, 100.0, 5.0
    source = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": args.rays}
    M = mmirror.MirrorConic(msupp.SupportRectangle(120.0, 20.0), p, q, graz)
    chain = mp.OEPlacement(source, [M], [p], [90.0 - graz], [0.0], "ellipsoid 10:1")
    last = chain.get_output_rays()[-1]
    oe = chain.optical_elements[0]
    u = np.array([1.0, 0.0, 0.0])
    u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(oe.position, dtype=float)
    det = mdet.Detector(pole, pole + q * u, -u)
    tubes = chain.get_RayTubes()          # (no Detector: curvatures at the mirror; on the focal plane they are a caustic's)
    c = tubes.chief
    print(f"{tubes.count} rays; dOmega'/dOmega over the aperture: {tubes.solid_angle_min:.1f} .. {tubes.solid_angle_max:.1f} "
          f"(paraxial (p/q)^2 = {(p / q) ** 2:.0f}), a factor of {tubes.solid_angle_max / tubes.solid_angle_min:.2f}")
    print(f"central ray: focal lines {c['foci'][0]:.6f} and {c['foci'][1]:.6f} mm behind the mirror (q = {q:g}: stigmatic)")
    for name, rays in (("rays (equal weight per source ray)", last), ("tubes.rays (image-space weight)", tubes.rays)):
        ff = det.get_FocalField(rays, Size=0.02, Pixels=129, Centre=(0.0, 0.0))
        wx, wy = widths(ff)
        print(f"{name:36s} Strehl {ff.strehl[0]:.6f}  peak at ({ff.peak[0][0] * 1e6:+.1f}, {ff.peak[0][1] * 1e6:+.1f}) nm  "
              f"rms half-width {wx * 1e6:7.1f} x {wy * 1e6:7.1f} nm")


if __name__ == "__main__":
    main()

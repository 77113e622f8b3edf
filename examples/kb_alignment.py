#!/usr/bin/env python3
"""Aligning a Kirkpatrick-Baez pair: the two crossed elliptical cylinders of examples/kb_focus.py with both pitches off
by tens of microradians.  get_Compensation says which moves of the two pitch adjusters make the spot smallest and how
small, from one device pass over the traced history; align repeats solve, move and re-trace until the re-traced spot no
longer shrinks.  Printed: the solve, and the rms spot and the half-energy width (get_EncircledEnergy) before and after.

    python examples/kb_alignment.py [--rays 1000000]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ART.ModuleDetector as mdet
import ART.ModuleMirror as mmirror
import ART.ModuleProcessing as mp
import ART.ModuleSupport as msupp


def spot(chain, det, dofs):
    """rms spot (nm) from the second moments and the half-energy width (nm) from the exact median radius."""
    c = chain.get_Compensation(det, dofs)
    hew = 2.0 * chain.get_EncircledEnergy(det, Fractions=(0.5,)).radii[0][0]
    return np.sqrt(c.variance[0] + c.variance[1]) * 1e6, hew * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1000000)
    args = ap.parse_args()
    graz, inc = 2.0, 88.0
    S = msupp.SupportRectangle(150.0, 20.0)
    point = {"Divergence": 1e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": args.rays}
    kb = [mmirror.MirrorEllipticalCylinder(S, 1000.0, 400.0, graz), mmirror.MirrorEllipticalCylinder(S, 1100.0, 300.0, graz)]
    chain = mp.OEPlacement(point, kb, [1000.0, 100.0], [inc, inc], [0.0, 90.0], "KB")
    u = np.array([1.0, 0.0, 0.0])
    for oe in chain.optical_elements:
        u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(chain.optical_elements[-1].position, dtype=float)
    det = mdet.Detector(pole, pole + 300.0 * u, -u)
    dofs = [(0, "pitch"), (1, "pitch")]
    applied = (2e-5, -3e-5)
    off = chain.copy_chain()
    for k, v in enumerate(applied):
        off.rotate_OE(k, "pitch", float(np.rad2deg(v)))
    print(f"nominal chain:    rms spot {spot(chain, det, dofs)[0]:10.3f} nm   HEW {spot(chain, det, dofs)[1]:10.3f} nm")
    print(f"pitches off by {applied} rad: rms spot {spot(off, det, dofs)[0]:10.3f} nm   HEW {spot(off, det, dofs)[1]:10.3f} nm")
    c = off.get_Compensation(det, dofs)
    print(f"solve: moves {c.moves} rad, singular values {c.singular_values}, rank {c.rank}; variances {c.variance} -> "
          f"{c.variance_predicted} mm^2 predicted; centroid moves by {c.centroid_shift * 1e3} um, arrival by {c.delay_shift:.4f} fs")
    aligned, det2, report = off.align(det, dofs, Tolerance=1e-6)
    print(f"align: {report.iterations} iterations, steps {report.step[1:]}, rejected {report.rejected}, objective "
          f"{report.objective}, moves {report.moves[-1]} rad")
    print(f"aligned chain:    rms spot {spot(aligned, det2, dofs)[0]:10.3f} nm   HEW {spot(aligned, det2, dofs)[1]:10.3f} nm")


if __name__ == "__main__":
    main()

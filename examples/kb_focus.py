#!/usr/bin/env python3
"""Focusing an XUV point source with a Kirkpatrick-Baez pair -- two crossed plane-elliptical cylinders at 2 degrees
grazing, the first focusing in the vertical, the second in the horizontal plane -- beside a pair of toroids with the same
conjugates (the first collimates, the second focuses), and a Wolter-I pair (paraboloid + hyperboloid) on a collimated
beam.  For each: the rms spot from the binned image (get_Histogram) and the Strehl ratio of the coherent focal field
(get_FocalField).

    python examples/kb_focus.py [--rays 1000000]"""
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
    # the detector sits normal to the central ray, `focus_distance` behind the last pole: that ray leaves the source
    # along +x and is mirrored at every element's normal (autoplace would measure from the mean hit point instead, which
    # at grazing incidence is millimetres away from the pole)
    u = np.array([1.0, 0.0, 0.0])
    for oe in chain.optical_elements:
        u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(chain.optical_elements[-1].position, dtype=float)
    det = mdet.Detector(pole, pole + focus_distance * u, -u)
    h = det.get_Histogram(last, Bins=(64, 64))
    w = h.counts if h.intensity is None else h.intensity
    cx, cy = [0.5 * (e[1:] + e[:-1]) for e in h.edges]
    mx, my = (w.sum(1) * cx).sum() / w.sum(), (w.sum(0) * cy).sum() / w.sum()
    rms = np.sqrt(((w.sum(1) * (cx - mx) ** 2).sum() + (w.sum(0) * (cy - my) ** 2).sum()) / w.sum())
    ff = det.get_FocalField(last, Pixels=65)       # odd: one pixel sits on the centre
    print(f"{name:28s} {len(last):8d} rays   rms spot {rms * 1e6:10.3f} nm   Strehl {ff.strehl[0]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1000000)
    args = ap.parse_args()
    graz, inc = 2.0, 88.0
    S = msupp.SupportRectangle(150.0, 20.0)
    point = {"Divergence": 1e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": args.rays}
    # source -> 1000 mm -> M1 -> 100 mm -> M2 -> 300 mm -> focus
    kb = [mmirror.MirrorEllipticalCylinder(S, 1000.0, 400.0, graz), mmirror.MirrorEllipticalCylinder(S, 1100.0, 300.0, graz)]
    report("KB pair (elliptical cyl.)", mp.OEPlacement(point, kb, [1000.0, 100.0], [inc, inc], [0.0, 90.0], "KB"), 300.0)
    tor = [mmirror.MirrorToroidal(*mmirror.ReturnOptimalToroidalRadii(f, inc), S) for f in (1000.0, 300.0)]
    report("toroid pair", mp.OEPlacement(point, tor, [1000.0, 100.0], [inc, -inc], [0.0, 0.0], "toroids"), 300.0)
    # Wolter-I on a collimated beam: the paraboloid's focus lies 600 mm behind it; the hyperboloid, 200 mm downstream, takes
    # that virtual object at 400 mm to a real focus at 150 mm
    beam = dict(point, Divergence=0, SourceSize=4.0)
    wolter = [mmirror.MirrorConic(S, np.inf, 600.0, graz), mmirror.MirrorHyperboloidal(S, -400.0, 150.0, graz)]
    report("Wolter-I (parab. + hyperb.)", mp.OEPlacement(beam, wolter, [100.0, 200.0], [inc, inc], [0.0, 0.0], "Wolter"), 150.0)


if __name__ == "__main__":
    main()

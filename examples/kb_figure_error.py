#!/usr/bin/env python3
"""How much figure error does a Kirkpatrick-Baez focus tolerate?  The KB pair of examples/kb_focus.py -- two crossed
plane-elliptical cylinders at 2 degrees grazing -- with a polynomial figure error of a few nm rms on each mirror
(ModuleMirror.MirrorFreeform: the rays meet the figured surface exactly).  For each amplitude: the rms spot from the binned
image, the rms wavefront error about the nominal focus (get_Wavefront; beside it the first-order -2 h cos(incidence)
summed over both mirrors, and the rms about the best reference point) and the Strehl ratio of the coherent focal field
(get_FocalField, its peak over the grid) at 30 nm, beside the Marechal estimate exp(-(2 k sigma sin(grazing))^2) with sigma
the intensity-weighted rms height over the rays' footprints on both mirrors, added in quadrature.

    python examples/kb_figure_error.py [--rays 1000000]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ART.ModuleDefects as mdef
import ART.ModuleDetector as mdet
import ART.ModuleMirror as mmirror
import ART.ModuleProcessing as mp
import ART.ModuleSupport as msupp
from attosecondraytracing_amd import ModuleGeometry as mgeo

GRAZING, WAVELENGTH = 2.0, 30e-6


def weighted_rms(v, w):
    mean = (w * v).sum() / w.sum()
    return float(np.sqrt((w * (v - mean) ** 2).sum() / w.sum()))


def heights(oe, bundle, keep):
    """(h, cos of the incidence angle) where the rays `keep` met the mirror."""
    fwd, _ = mgeo.frame_maps(oe.normal, oe.majoraxis)
    d = bundle.data.cpu().numpy()
    local = (d[0:3].T[keep] - np.asarray(oe.position, dtype=float)) @ np.asarray(fwd).T
    return oe.type._figure(local[:, 0], local[:, 1]), np.cos(d[7][keep])


def report(amplitude_nm, chain, focus_distance):
    rays = chain.get_output_rays()
    last = rays[-1]
    u = np.array([1.0, 0.0, 0.0])                 # the nominal central ray, mirrored at every element's normal
    for oe in chain.optical_elements:
        u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(chain.optical_elements[-1].position, dtype=float)
    det = mdet.Detector(pole, pole + focus_distance * u, -u)
    h = det.get_Histogram(last, Bins=(64, 64))
    w = h.counts if h.intensity is None else h.intensity
    cx, cy = [0.5 * (e[1:] + e[:-1]) for e in h.edges]
    mx, my = (w.sum(1) * cx).sum() / w.sum(), (w.sum(0) * cy).sum() / w.sum()
    spot = np.sqrt(((w.sum(1) * (cx - mx) ** 2).sum() + (w.sum(0) * (cy - my) ** 2).sum()) / w.sum())
    wf = det.get_Wavefront(last, Order=6)
    ff = det.get_FocalField(last, Pixels=65)
    # the rays that reach the focus, with the weights of get_Wavefront and get_FocalField: their intensities
    keep = last.alive.cpu().numpy() != 0
    wgt = np.ones(int(keep.sum())) if last.intensity is None else last.intensity.cpu().numpy()[keep]
    hc = [heights(oe, b, keep) for oe, b in zip(chain.optical_elements, rays)]
    sigma = np.sqrt(sum(weighted_rms(h, wgt) ** 2 for h, _ in hc))
    first_order = weighted_rms(-2 * sum(h * c for h, c in hc), wgt)          # OPD = -2 h cos(incidence), mirror by mirror
    k = 2 * np.pi / WAVELENGTH
    marechal = np.exp(-(2 * k * sigma * np.sin(np.deg2rad(GRAZING))) ** 2)
    print(f"{amplitude_nm:6.1f} nm   height rms {sigma * 1e6:6.2f} nm   rms spot {spot * 1e6:9.3f} nm   wavefront rms "
          f"{wf.rms * 1e6:7.3f} nm (-2 h cos: {first_order * 1e6:7.3f} nm, best point {wf.rms_best * 1e6:7.3f} nm)   "
          f"Strehl {ff.strehl[0]:.4f}   Marechal {marechal:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1000000)
    args = ap.parse_args()
    inc = 90.0 - GRAZING
    S = msupp.SupportRectangle(150.0, 20.0)
    point = {"Divergence": 1e-3, "SourceSize": 0, "Wavelength": WAVELENGTH, "DeltaFT": 0.5, "NumberRays": args.rays}
    print("figure amplitude; KB pair at 2 degrees grazing, 30 nm, source -> 1000 mm -> M1 -> 100 mm -> M2 -> 300 mm -> focus")
    for nm in (0.0, 1.0, 2.0, 5.0, 10.0, 20.0):
        a = nm * 1e-6
        # polynomial ripples along each mirror (x / 40 mm) WITHOUT a slope at the pole: OEPlacement sends its guide ray along
        # the real reflected central ray, so a pole slope would re-align the optics behind it instead of showing up here
        fig1 = [mdef.Polynomial(S, {(3, 0): 4 * a, (4, 0): 4 * a, (2, 0): -4 * a, (0, 0): 0.5 * a}, Radius=40.0)]
        fig2 = [mdef.Polynomial(S, {(5, 0): 8 * a, (3, 0): -10 * a}, Radius=40.0)]
        kb = [mmirror.MirrorFreeform(mmirror.MirrorEllipticalCylinder(S, 1000.0, 400.0, GRAZING), fig1),
              mmirror.MirrorFreeform(mmirror.MirrorEllipticalCylinder(S, 1100.0, 300.0, GRAZING), fig2)]
        report(nm, mp.OEPlacement(point, kb, [1000.0, 100.0], [inc, inc], [0.0, 90.0], "KB"), 300.0)


if __name__ == "__main__":
    main()

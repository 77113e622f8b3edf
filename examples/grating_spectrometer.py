#!/usr/bin/env python3
"""A flat-field XUV spectrometer: a point source, a spherical grating at grazing incidence and a detector across the
diffracted beams.  One trace per wavelength would read the source bundle once each; `get_SpectralRays` fans the bundle
out into all wavelengths in one launch.

    python examples/grating_spectrometer.py [--rays 1000000] [--show]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1000000)
    ap.add_argument("--show", action="store_true")
    args = ap.parse_args()
    source = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": 25e-6, "DeltaFT": 0.5, "NumberRays": args.rays}
    grating = mmirror.Grating(mmirror.MirrorSpherical(5649.0, msupp.SupportRectangle(60.0, 10.0)), LinesPerMm=1200.0,
                              Order=-1, GrooveAngle=0.0)
    chain = mp.OEPlacement(source, [grating], [237.0], [87.0], [0.0], "flat-field spectrometer")
    centre = chain.get_output_rays()[-1]                      # the bundle at the placement wavelength, 25 nm
    det = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    det.autoplace(centre, 235.0)
    wavelengths = np.linspace(10e-6, 40e-6, 16)
    bundles = chain.get_SpectralRays(wavelengths)
    for wl, b in zip(wavelengths, bundles):
        xy = det.get_PointList2D(b)
        delays = det.get_Delays(b)
        print(f"{wl * 1e6:5.1f} nm: {len(b):8d} rays, centroid X = {xy[:, 0].mean():9.4f} mm, spot sd = "
              f"{xy[:, 0].std() * 1e3:8.2f} um, delay spread (pulse-front tilt) = {np.ptp(delays):8.1f} fs")
    fig, hist = mplots.SpectrometerImage(chain, det, wavelengths, Bins=(512, 64), Show=args.show)
    print("spectrometer image:", hist.counts.shape, "bins,", int(hist.counts.sum()), "rays binned")
    if args.show:
        mplots.show()


if __name__ == "__main__":
    main()

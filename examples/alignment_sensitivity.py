#!/usr/bin/env python3
"""The tolerancing table of a Kirkpatrick-Baez pair (the KB pair of examples/kb_focus.py): how far the spot moves, how
much later the pulse arrives and how much the spot grows per unit of each of the 18 rigid degrees of freedom -- six of
the source, six per mirror -- from ONE device pass over the traced history (OpticalChain.get_Sensitivities), beside one
column obtained the old way: a loop list of re-traced chains (get_OE_loop_list) and a central difference.

    python examples/alignment_sensitivity.py [--rays 1000000]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ART.ModuleDetector as mdet
import ART.ModuleMirror as mmirror
import ART.ModuleProcessing as mp
import ART.ModuleSupport as msupp


def centroid_and_path(chain, det):
    st = det.readout(chain.get_output_rays()[-1], store=False)["stats"]
    return np.array([st[9] / st[8], st[10] / st[8], st[11] / st[8]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1000000)
    args = ap.parse_args()
    graz, inc = 2.0, 88.0
    S = msupp.SupportRectangle(150.0, 20.0)
    point = {"Divergence": 1e-3, "SourceSize": 0, "Wavelength": 30e-6, "DeltaFT": 0.5, "NumberRays": args.rays}
    # source -> 1000 mm -> M1 -> 100 mm -> M2 -> 300 mm -> focus
    kb = [mmirror.MirrorEllipticalCylinder(S, 1000.0, 400.0, graz), mmirror.MirrorEllipticalCylinder(S, 1100.0, 300.0, graz)]
    chain = mp.OEPlacement(point, kb, [1000.0, 100.0], [inc, inc], [0.0, 90.0], "KB")
    u = np.array([1.0, 0.0, 0.0])
    for oe in chain.optical_elements:
        u = u - 2 * u.dot(oe.normal) * oe.normal
    pole = np.asarray(chain.optical_elements[-1].position, dtype=float)
    det = mdet.Detector(pole, pole + 300.0 * u, -u)

    s = chain.get_Sensitivities(det)
    print(f"{s.count} rays, {len(s.names)} degrees of freedom; per um of shift and per urad of rotation:")
    print(f"{'element':>8s} {'motion':>13s} {'dX (nm)':>11s} {'dY (nm)':>11s} {'delay (as)':>11s} {'spot growth (nm)':>17s}")
    for c, ((who, dof), unit) in enumerate(zip(s.names, s.units)):
        k = 1e-3 if unit == "mm" else 1e-6
        grow = np.hypot(s.spread[c, 0], s.spread[c, 1]) * k
        print(f"{str(who):>8s} {dof:>13s} {s.centroid[c, 0] * k * 1e6:11.3f} {s.centroid[c, 1] * k * 1e6:11.3f} "
              f"{s.delay[c] * k * 1e3:11.4f} {grow * 1e6:17.4f}")

    # one column the old way: four re-traces of the whole chain and a central difference
    h = 1e-4                                                     # rad
    steps = [float(np.rad2deg(v)) for v in (h, -h, h / 2, -h / 2)]
    m = [centroid_and_path(c, det) for c in chain.get_OE_loop_list(1, "pitch", steps)]
    one, two = (m[0] - m[1]) / (2 * h), (m[2] - m[3]) / h
    fd = (4 * two - one) / 3
    c = s.index(1, "pitch")
    print(f"pitch of mirror 2, per rad: dX {s.centroid[c, 0]:.6f} mm, dY {s.centroid[c, 1]:.6f} mm, "
          f"path {s.delay[c] * 299792458000 / 1e15:.6f} mm (one pass)")
    print(f"      the same from four re-traces: dX {fd[0]:.6f} mm, dY {fd[1]:.6f} mm, path {fd[2]:.6f} mm")
    p = s.predict(rotate_OE=(1, "pitch", float(np.rad2deg(1e-6))), shift_OE=(0, "normal", 1e-3))
    print(f"1 urad of that pitch with mirror 1 pushed 1 um along its normal: spot moves by "
          f"({p['centroid'][0] * 1e6:.2f}, {p['centroid'][1] * 1e6:.2f}) nm, its arrival by {p['delay'] * 1e3:.3f} as")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record the reference's `RayTracingCalculation` calls for tests/test_reference_with_binding.py: the scene of that test
(mask, two toroids, an off-axis parabola) is placed and traced by the reference's own OEPlacement / OpticalChain, every
call of its RayTracingCalculation (the 1-ray alignment traces of the placement, then the 400-ray trace) is stored with
its inputs (the rays' public attributes, the optics' type, support, parameters and pose) and its result; beside them the
reference Detector's delays on the last bundle.  Output: tests/golden/reference_binding.json.gz.

TEST INFRASTRUCTURE.  Run where a reference tree exists:
    ART_REFERENCE=<reference tree> python tests/golden/generate_binding_goldens.py
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _floats(v):
    return [float(x) for x in v]


def _opt(f, v):
    return None if v is None else f(v)


def _support(S):
    keys = ("radius", "radiushole", "centerholeX", "centerholeY", "dimX", "dimY", "holeX", "holeY")
    return {"class": type(S).__name__, "attrs": {k: float(getattr(S, k)) for k in keys if hasattr(S, k)}}


def _optic(o):
    keys = ("radius", "p", "majorradius", "minorradius", "a", "b")
    return {"type": o.type, "support": _support(o.support), "centre": _floats(o.get_centre()),
            "params": {k: float(getattr(o, k)) for k in keys if isinstance(getattr(o, k, None), (int, float))}}


def _element(oe):
    return {"optic": _optic(oe.type), "position": _floats(oe.position), "normal": _floats(oe.normal),
            "majoraxis": _floats(oe.majoraxis)}


def _rays(rays):
    return {"point": [_floats(r.point) for r in rays], "vector": [_floats(r.vector) for r in rays],
            "path": [_floats(r.path) for r in rays], "number": [_opt(int, r.number) for r in rays],
            "wavelength": [_opt(float, r.wavelength) for r in rays], "incidence": [_opt(float, r.incidence) for r in rays],
            "intensity": [_opt(float, r.intensity) for r in rays]}


def main():
    ref_tree = os.environ.get("ART_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref_tree or not os.path.isdir(ref_tree):
        sys.exit("usage: ART_REFERENCE=<reference tree> python tests/golden/generate_binding_goldens.py")
    sys.path[:0] = [ref_tree, os.path.join(HERE, "_standin")]
    import matplotlib
    matplotlib.use("Agg")
    import ART.ModuleProcessing as mp, ART.ModuleMirror as mmirror, ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp, ART.ModuleDetector as mdet
    assert mp.__file__.startswith(os.path.abspath(ref_tree))

    calls = []
    original = mp.RayTracingCalculation

    def recording(source_rays, optical_elements, IgnoreDefects=True):
        out = original(source_rays, optical_elements, IgnoreDefects)
        calls.append({"source": _rays(source_rays), "elements": [_element(oe) for oe in optical_elements],
                      "IgnoreDefects": bool(IgnoreDefects), "result": [_rays(o) for o in out]})
        return out

    mp.RayTracingCalculation = recording
    SP = {"Divergence": 50e-3 / 2, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": 400}
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 41e-3 / 2 * 500, 0, 0))
    R, r = mmirror.ReturnOptimalToroidalRadii(600, 80)
    Tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(200, 30))
    oap = mmirror.MirrorParabolic(150, 45, msupp.SupportRound(40))
    chain = mp.OEPlacement(SP, [Mask, Tor, Tor, oap], [500, 100, 600, 400], [0, 80, -80, 0], [0, 0, 30.0, 0], "stub")
    out = chain.get_output_rays()
    det = mdet.Detector(chain.optical_elements[-1].position)
    det.autoplace(out[-1], 150)
    rec = {"calls": calls, "poses": [_element(oe) for oe in chain.optical_elements],
           "delays": _floats(det.get_Delays(out[-1])), "n_out": [len(o) for o in out]}
    path = os.path.join(HERE, "reference_binding.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(rec, sort_keys=True).encode())
    print(f"[golden] {len(calls)} calls, survivors {rec['n_out']}: wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

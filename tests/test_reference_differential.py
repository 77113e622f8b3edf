"""CPU: the product's host shell against the reference ITSELF on seeded
random chains (1-4 optics of every mirror class + masks, random distances, incidence angles and incidence-plane
rotations, point and plane-wave sources):
  * `OEPlacement` -> poses and exception types;
  * `FindOptimalDistance`, `GetResultSummary`, `getETransmission` on the traced bundles;
  * random sequences of `OpticalChain` operations and the loop-list generators.
The reference runs in a subprocess (its package is also called `ART`) and reports its results as JSON; both sides
build their scenes from the same generator text below.  Its results for the default seeds are recorded in
tests/golden/reference_differential.json.gz (tests/golden/generate_reference_differential.py); with ART_REFERENCE naming
a reference tree the scripts run live there instead, for any seed range.  Seeds per test: ART_FUZZ_PLACEMENTS / ART_FUZZ_FOCUS /
ART_FUZZ_OPS / ART_FUZZ_METHODS / ART_FUZZ_DETECTOR / ART_FUZZ_GEOMETRY / ART_FUZZ_MAIN (defaults keep the suite short;
4000 / 700 / 1500 / 3000 / 1500 / 5000 / 500 were run offline)."""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = os.path.join(ROOT, "tests", "golden", "reference_differential.json.gz")


def script_key(script, stdin):
    """Identifies what a recorded result was computed from: the reference-side script and the text fed to it."""
    return hashlib.sha256((script + "\0" + stdin).encode()).hexdigest()


def run_reference(ref_tree, script, stdin, lo, hi):
    """Run one of the scripts below on the reference tree `ref_tree`; returns its JSON result."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    argv = [sys.executable, "-c", script, ROOT, ref_tree] + ([] if lo is None else [str(lo), str(hi)])
    r = subprocess.run(argv, input=stdin, capture_output=True, text=True, timeout=3000, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout[r.stdout.index("RESULT") + 6:])


def reference_results(key, script, stdin, lo, hi):
    """The reference's results for one test on the seeds [lo, hi): run live on the tree ART_REFERENCE names, else the
    recorded ones (which exist for the default seed range of each test)."""
    if os.environ.get("ART_REFERENCE"):
        return run_reference(os.environ["ART_REFERENCE"], script, stdin, lo, hi)
    with gzip.open(RECORDED, "rt") as f:
        rec = json.load(f)[key]
    assert rec["script_sha256"] == script_key(script, stdin), \
        "the reference-side script or generator changed: rerun tests/golden/generate_reference_differential.py"
    if rec["range"] != [lo, hi]:
        pytest.fail(f"seeds [{lo}, {hi}) of '{key}' are not recorded (recorded: {rec['range']}): set ART_REFERENCE to a "
                    "reference tree to run them")
    return rec["result"]

GENERATOR = textwrap.dedent('''
    import numpy as np

    def make_case(seed, mmirror, mmask, msupp):
        """(SourceProperties, optics, distances, incidence angles, plane angles) of one seeded random chain."""
        rng = np.random.default_rng(seed)
        n_el = int(rng.integers(1, 5))
        optics, dist, inc, plane = [], [], [], []
        for k in range(n_el):
            kind = int(rng.integers(0, 8))
            sup = [msupp.SupportRound(float(rng.uniform(15, 40))),
                   msupp.SupportRectangle(float(rng.uniform(60, 200)), float(rng.uniform(20, 60)))][int(rng.integers(0, 2))]
            theta = float(rng.uniform(-75, 75))
            if kind == 0:
                o = mmirror.MirrorPlane(sup)
            elif kind == 1:
                o = mmirror.MirrorSpherical(float(rng.uniform(300, 3000)) * (1 if rng.uniform() < 0.7 else -1), sup)
            elif kind == 2:
                o = mmirror.MirrorParabolic(float(rng.uniform(80, 500)), float(rng.uniform(0, 100)), sup)
                theta = 0.0     # off-axis parabolas are aligned on their own axis
            elif kind == 3:
                f, a = float(rng.uniform(200, 800)), float(rng.uniform(60, 82))
                R, r = mmirror.ReturnOptimalToroidalRadii(f, a)
                o = mmirror.MirrorToroidal(R, r, sup)
                theta = a * (1 if rng.uniform() < 0.5 else -1)
            elif kind == 4:
                o = mmirror.MirrorCylindrical(float(rng.uniform(300, 3000)), sup)
            elif kind == 5:
                a_ = float(rng.uniform(300, 800))
                o = mmirror.MirrorEllipsoidal(sup, SemiMajorAxis=a_, SemiMinorAxis=a_ * float(rng.uniform(0.5, 0.9)),
                                              OffAxisAngle=float(rng.uniform(50, 120)))
                theta = 0.0
            elif kind == 6:
                # hole on the axis, as in the shipped configs.  (With an opaque centre the reference loses its own
                # alignment ray at the NEXT mirror -- its transparent stand-in mask is dropped when the auxiliary chain
                # is rebuilt, ART/ModuleProcessing.py:108-125 -- and raises IndexError; the product keeps the stand-in.)
                o = mmask.Mask(msupp.SupportRoundHole(30.0, float(rng.uniform(0.5, 3)), 0.0, 0.0))
                theta = 0.0
            else:
                o = mmirror.MirrorSpherical(float(rng.uniform(300, 3000)), sup)
                theta = 0.0     # normal incidence: RotationPoint's antiparallel special case on the way back
            optics.append(o)
            dist.append(float(rng.uniform(50, 900)))
            inc.append(theta)
            plane.append(float(rng.choice([0.0, 90.0, 180.0, -90.0, float(rng.uniform(-180, 180))])))
        point = rng.uniform() < 0.6
        SP = {"Divergence": float(rng.uniform(1e-3, 2e-2)) if point else 0, "SourceSize": 0 if point else float(rng.uniform(2, 20)),
              "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": 60}
        return SP, optics, dist, inc, plane
''')

REF_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleProcessing as mp, ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp
    assert mp.__file__.startswith(REF)
    exec(sys.stdin.read())
    out = {}
    for seed in range(lo, hi):
        SP, optics, dist, inc, plane = make_case(seed, mmirror, mmask, msupp)
        try:
            ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
            out[seed] = {"poses": [[list(map(float, oe.position)), list(map(float, oe.normal)), list(map(float, oe.majoraxis))]
                                   for oe in ch.optical_elements],
                         "n_src": len(ch.source_rays)}
        except Exception as e:       # e.g. the alignment ray falls into a hole: IndexError in the reference
            out[seed] = {"error": type(e).__name__}
    print("RESULT" + json.dumps(out))
''')


@pytest.fixture(scope="module")
def twin():
    from twin_backend import TwinBackend
    from attosecondraytracing_amd import _lib
    old = _lib._BACKEND
    _lib._BACKEND = TwinBackend()
    yield _lib._BACKEND
    _lib._BACKEND = old


def test_oeplacement_random_chains_match_reference(twin):
    lo, hi = 0, int(os.environ.get("ART_FUZZ_PLACEMENTS", "60"))
    ref = reference_results("placements", REF_SCRIPT, GENERATOR, lo, hi)
    import ART.ModuleProcessing as mp
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    ns = {}
    exec(GENERATOR, ns)
    compared = 0
    for seed in range(lo, hi):
        SP, optics, dist, inc, plane = ns["make_case"](seed, mmirror, mmask, msupp)
        expect = ref[str(seed)]
        if "error" in expect:
            with pytest.raises(Exception) as ei:
                mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
            assert type(ei.value).__name__ == expect["error"], (seed, ei.value, expect)
            continue
        ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
        assert len(ch.source_rays) == expect["n_src"]
        for oe, (p, n, m) in zip(ch.optical_elements, expect["poses"]):
            scale = max(1.0, np.abs(p).max())
            assert np.abs(np.asarray(oe.position, float) - p).max() <= 1e-10 * scale, (seed, oe.position, p)
            assert np.abs(np.asarray(oe.normal, float) - n).max() <= 1e-10, (seed, oe.normal, n)
            assert np.abs(np.asarray(oe.majoraxis, float) - m).max() <= 1e-10, (seed, oe.majoraxis, m)
        compared += 1
    assert compared >= 40


FOCUS_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleProcessing as mp, ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp
    import ART.ModuleDetector as mdet, ART.ModuleAnalysisAndPlots as mplots
    exec(sys.stdin.read())
    out = {}
    for seed in range(lo, hi):
        SP, optics, dist, inc, plane = make_case(seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 150
        try:
            ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
            last = ch.get_output_rays()[-1]
        except Exception as e:
            out[seed] = {"skip": type(e).__name__}
            continue
        if len(last) < 30:
            out[seed] = {"skip": "few rays"}
            continue
        rng = np.random.default_rng(seed + 9_000_000)
        d0 = float(rng.uniform(50, 600))
        optfor = ["intensity", "duration"][seed % 2]
        weighted = bool((seed // 2) % 2)
        D = mdet.Detector(ch.optical_elements[-1].position)
        D.autoplace(last, d0)
        try:
            Dopt, spot, dur = mp.FindOptimalDistance(D, last, optfor, None, 2, weighted)
            s_sum, d_sum = mplots.GetResultSummary(Dopt, last, False)
            out[seed] = {"d0": d0, "optfor": optfor, "weighted": weighted, "n": len(last), "distance": Dopt.get_distance(),
                         "spot": float(spot), "dur": float(dur), "sum_spot": float(s_sum), "sum_dur": float(d_sum),
                         "et": float(mplots.getETransmission(ch.source_rays, last))}
        except Exception as e:
            out[seed] = {"d0": d0, "optfor": optfor, "weighted": weighted, "error": type(e).__name__}
    print("RESULT" + json.dumps(out))
''')


def test_autofocus_and_summary_random_chains_match_reference(twin):
    """FindOptimalDistance (both working OptFor values, weighted or not), GetResultSummary and getETransmission on the
    bundles of random chains: the product's device-side moment scan against the reference's per-position loops."""
    lo, hi = 0, int(os.environ.get("ART_FUZZ_FOCUS", "24"))
    ref = reference_results("focus", FOCUS_SCRIPT, GENERATOR, lo, hi)
    import ART.ModuleProcessing as mp
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleDetector as mdet
    import ART.ModuleAnalysisAndPlots as mplots
    ns = {}
    exec(GENERATOR, ns)
    compared = 0
    compared_inside = [0]
    for seed in range(lo, hi):
        e = ref[str(seed)]
        if "skip" in e:
            continue
        SP, optics, dist, inc, plane = ns["make_case"](seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 150
        ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
        last = ch.get_output_rays()[-1]
        assert len(last) == e["n"], seed
        D = mdet.Detector(np.asarray(ch.optical_elements[-1].position, float))
        D.autoplace(last, e["d0"])
        if "error" in e:
            with pytest.raises(Exception) as ei:
                mp.FindOptimalDistance(D, last, e["optfor"], None, 2, e["weighted"])
            assert type(ei.value).__name__ == e["error"], (seed, ei.value, e)
            continue
        Dopt, spot, dur = mp.FindOptimalDistance(D, last, e["optfor"], None, 2, e["weighted"])
        # search range of the reference's algorithm (ART/ModuleProcessing.py:430-433)
        size = 2 * mp.StandardDeviation(D.get_PointList2DCentre(last))
        A = min(4 * np.ceil(size / np.tan(np.arcsin(mp.ReturnNumericalAperture(last, 1)))), e["d0"])
        # Each level scans n = int(2 A_k / Step_k) positions; that quotient is 20 or 19.999999999999996 depending on
        # the last bit of the detector distance, so the two implementations may scan 19 or 20 positions: when the
        # fitness has no minimum inside the range ("There`s no minimum ... in the searched range") they stop one
        # coarse step apart.  Inside the range they agree to the final grid (A * 1e-3).
        if not np.isnan(e["dur"]) and e["dur"] < 1e-6:
            compared += 1      # all optical paths equal (e.g. a plane wave on plane mirrors): the duration is rounding
            continue           # noise (1e-10 fs) and so is the position of its "minimum"
        at_edge = min(abs(e["distance"] - (e["d0"] - A)), abs(e["distance"] - (e["d0"] + A))) <= 0.25 * A
        tol_d = 0.125 * A if at_edge else 3e-3 * A + 1e-9
        assert abs(Dopt.get_distance() - e["distance"]) <= tol_d, (seed, Dopt.get_distance(), A, e)
        if not at_edge:
            if not np.isnan(e["spot"]):
                assert abs(spot - e["spot"]) <= 1e-3 * max(e["spot"], 1e-6), (seed, spot, e)
            if not np.isnan(e["dur"]):
                assert abs(dur - e["dur"]) <= 1e-3 * max(e["dur"], 1e-3), (seed, dur, e)
            compared_inside[0] += 1
        assert abs(mplots.getETransmission(ch.source_rays, last) - e["et"]) <= 1e-9, seed
        compared += 1
    assert compared >= (hi - lo) // 3 and compared_inside[0] >= (hi - lo) // 8, (compared, compared_inside)


OPS_GEN = textwrap.dedent('''
    def make_ops(seed, n_el):
        """Seeded random sequence of OpticalChain operations + one loop-list request."""
        rng = np.random.default_rng(seed + 123456)
        ops = []
        for _ in range(int(rng.integers(1, 6))):
            k = int(rng.integers(0, 4))
            if k == 0:
                ax = [("vert",), ("horiz",), (rng.normal(size=3),)][int(rng.integers(0, 3))][0]
                ops.append(("shift_source", ax, float(rng.uniform(-2, 2))))
            elif k == 1:
                ax = [("in_plane",), ("out_plane",), (rng.normal(size=3),)][int(rng.integers(0, 3))][0]
                ops.append(("tilt_source", ax, float(rng.uniform(-0.2, 0.2))))
            elif k == 2:
                ops.append(("rotate_OE", int(rng.integers(-n_el, n_el)), ["pitch", "roll", "yaw"][int(rng.integers(0, 3))],
                            float(rng.uniform(-0.3, 0.3))))
            else:
                ops.append(("shift_OE", int(rng.integers(-n_el, n_el)), ["normal", "major", "cross"][int(rng.integers(0, 3))],
                            float(rng.uniform(-0.5, 0.5))))
        if rng.uniform() < 0.5:
            loop = ("source", ["tilt_in_plane", "tilt_out_plane", "shift_vert", "shift_horiz", "divergence"][int(rng.integers(0, 5))],
                    [float(v) for v in rng.uniform(0.001, 0.02, 3)])
        else:
            loop = ("OE", int(rng.integers(0, n_el)), ["pitch", "roll", "yaw", "shift_normal", "shift_major", "shift_cross"][int(rng.integers(0, 6))],
                    [float(v) for v in rng.uniform(-0.2, 0.2, 3)])
        return ops, loop

    def run_ops(ch, ops, loop, points_of):
        """Apply the operations; returns a JSON-able record of the resulting state (or of the exception)."""
        rec = {"steps": []}
        try:
            for op in ops:
                getattr(ch, op[0])(*op[1:])
                rec["steps"].append(op[0])
            chains = ch.get_source_loop_list(loop[1], loop[2]) if loop[0] == "source" else ch.get_OE_loop_list(loop[1], loop[2], loop[3])
        except Exception as e:
            rec["error"] = type(e).__name__
            return rec
        rec["chains"] = []
        for c in [ch] + list(chains):
            P, V = points_of(c.source_rays)
            out = c.get_output_rays()
            Pl, Vl = points_of(out[-1])
            rec["chains"].append({"name": c.loop_variable_name, "value": None if c.loop_variable_value is None else float(c.loop_variable_value),
                                  "src_p": P, "src_v": V, "n_out": [len(o) for o in out], "last_p": Pl, "last_v": Vl,
                                  "poses": [[list(map(float, oe.position)), list(map(float, oe.normal)), list(map(float, oe.majoraxis))]
                                            for oe in c.optical_elements]})
        return rec
''')

OPS_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleProcessing as mp, ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp
    exec(sys.stdin.read())
    def points_of(rays):
        return [[float(v) for v in r.point] for r in rays], [[float(v) for v in r.vector] for r in rays]
    out = {}
    for seed in range(lo, hi):
        SP, optics, dist, inc, plane = make_case(seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 40
        try:
            ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
        except Exception as e:
            out[seed] = {"skip": type(e).__name__}
            continue
        ops, loop = make_ops(seed, len(optics))
        out[seed] = run_ops(ch, ops, loop, points_of)
    print("RESULT" + json.dumps(out))
''')


def test_chain_operations_random_sequences_match_reference(twin):
    """shift/tilt of the source, rotate/shift of optical elements and the loop-list generators (ART/ModuleOpticalChain.py:
    219-615) applied in random sequences to random chains: same resulting sources, poses, loop-variable names, survivor
    counts, final rays and exception types as the reference."""
    lo, hi = 0, int(os.environ.get("ART_FUZZ_OPS", "30"))
    ref = reference_results("ops", OPS_SCRIPT, GENERATOR + OPS_GEN, lo, hi)
    import ART.ModuleProcessing as mp
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    ns = {}
    exec(GENERATOR + OPS_GEN, ns)

    def points_of(rays):
        return rays.points().tolist(), rays.vectors().tolist()

    compared = 0
    for seed in range(lo, hi):
        e = ref[str(seed)]
        if "skip" in e:
            continue
        SP, optics, dist, inc, plane = ns["make_case"](seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 40
        ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
        ops, loop = ns["make_ops"](seed, len(optics))
        mine = ns["run_ops"](ch, ops, loop, points_of)
        assert mine["steps"] == e["steps"], (seed, mine, e.get("error"))
        assert mine.get("error") == e.get("error"), (seed, mine.get("error"), e.get("error"), ops, loop)
        if "error" in e:
            continue
        assert len(mine["chains"]) == len(e["chains"])
        for a, b in zip(mine["chains"], e["chains"]):
            assert a["name"] == b["name"] and a["value"] == b["value"], (seed, a["name"], b["name"])
            assert a["n_out"] == b["n_out"], (seed, a["n_out"], b["n_out"])
            scale = max(1.0, np.abs(np.array(b["src_p"])).max(), *(np.abs(np.array(p[0])).max() for p in b["poses"]))
            for key, tol in (("src_p", 1e-10 * scale), ("src_v", 1e-10), ("last_p", 1e-9 * scale), ("last_v", 1e-9)):
                if len(b[key]):
                    assert np.abs(np.array(a[key]) - np.array(b[key])).max() <= tol, (seed, key, ops, loop)
            for pa, pb in zip(a["poses"], b["poses"]):
                assert np.abs(np.array(pa[0]) - np.array(pb[0])).max() <= 1e-10 * scale, (seed, "position", ops)
                assert np.abs(np.array(pa[1:]) - np.array(pb[1:])).max() <= 1e-10, (seed, "axes", ops)
        compared += 1
    assert compared >= (hi - lo) // 3


METHODS_GEN = textwrap.dedent('''
    def make_mirror_and_rays(seed, mmirror, mmask, msupp, mray, mdef):
        """One optic (any class, any aperture) and 12 rays given in ITS OWN frame, some missing it."""
        rng = np.random.default_rng(seed + 424242)
        size = float(rng.uniform(10, 40))
        sup = [msupp.SupportRound(size), msupp.SupportRoundHole(size, size / 4, size / 5, 0.0),
               msupp.SupportRectangle(2 * size, size), msupp.SupportRectangleHole(2 * size, size, size / 5, 1.0, -2.0),
               msupp.SupportRectangleRectHole(2 * size, size, size / 2, size / 4, 2.0, 1.0)][int(rng.integers(0, 5))]
        k = seed % 9
        if k == 0: o = mmirror.MirrorPlane(sup)
        elif k == 1: o = mmirror.MirrorSpherical(float(rng.uniform(100, 2000)), sup)
        elif k == 2: o = mmirror.MirrorSpherical(-float(rng.uniform(100, 2000)), sup)
        elif k == 3: o = mmirror.MirrorParabolic(float(rng.uniform(60, 400)), float(rng.uniform(0, 110)), sup)
        elif k == 4:
            R, r = mmirror.ReturnOptimalToroidalRadii(float(rng.uniform(200, 800)), float(rng.uniform(50, 82)))
            o = mmirror.MirrorToroidal(R, r, sup)
        elif k == 5: o = mmirror.MirrorCylindrical(float(rng.uniform(100, 2000)) * (1 if rng.uniform() < 0.5 else -1), sup)
        elif k == 6: o = mmirror.MirrorEllipsoidal(sup, f_object=float(rng.uniform(200, 600)), f_image=float(rng.uniform(200, 600)),
                                                   OffAxisAngle=float(rng.uniform(40, 120)))
        elif k == 7: o = mmask.Mask(sup)
        else:
            base = mmirror.MirrorParabolic(float(rng.uniform(60, 400)), float(rng.uniform(0, 90)), sup) if rng.uniform() < 0.5 \
                else mmirror.MirrorSpherical(float(rng.uniform(200, 2000)), sup)
            defects = [mdef.Zernike(sup, {(int(n), int(rng.integers(0, n + 1))): float(rng.uniform(-1, 1) * 3e-4)
                                          for n in rng.integers(1, 8, size=3)}) for _ in range(int(rng.integers(1, 3)))]
            o = mmirror.DeformedMirror(base, defects)
        C = np.asarray(o.get_centre(), dtype=float)
        rays = []
        for j in range(12):
            target = C + np.array([rng.uniform(-1.3, 1.3) * size, rng.uniform(-1.3, 1.3) * size, 0.0])
            d = rng.normal(size=3); d[2] = abs(d[2]) + 0.3; d /= np.linalg.norm(d)
            A = target + float(rng.uniform(50, 500)) * d
            rays.append(mray.Ray(A, -d, (0.0, float(rng.uniform(0, 10))), j, 50e-6, None, float(rng.uniform(0, 1))))
        return o, rays
''')

METHODS_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp, ART.ModuleOpticalRay as mray
    import ART.ModuleSource as msource, ART.ModuleDefects as mdef
    exec(sys.stdin.read())
    out = {}
    for seed in range(lo, hi):
        o, rays = make_mirror_and_rays(seed, mmirror, mmask, msupp, mray, mdef)
        pts = [o._get_intersection(r) for r in rays]
        lst = mmask.TransmitMaskRayList(o, rays) if o.type == "Mask" else mmirror.ReflectionMirrorRayList(o, rays)
        single = []
        for r, p in zip(rays, pts):
            if p is None:
                single.append(None)
                continue
            q = mmask._TransmitMaskRay(o, p, r) if o.type == "Mask" else mmirror._ReflectionMirrorRay(o, p, r)
            single.append([list(map(float, q.point)), list(map(float, q.vector)), float(q.incidence), [float(v) for v in q.path]])
        out[seed] = {"type": o.type, "pts": [None if p is None else list(map(float, p)) for p in pts],
                     "normals": [None if p is None else list(map(float, o.get_normal(p))) for p in pts],
                     "offsets": [[float(d.get_offset(p - o.get_centre())) for d in getattr(o, "DeformationList", [])]
                                 for p in pts if p is not None],
                     "list": [[r.number, list(map(float, r.point)), list(map(float, r.vector)), float(r.incidence),
                               [float(v) for v in r.path], r.wavelength, r.intensity] for r in lst],
                     "single": single}
    sq = {}
    for n in (0, 1, 2, 3, 4, 9, 50):
        try:
            b = msource.PlaneWaveSquare(np.array([1.0, 2.0, 3.0]), np.array([0.2, -0.5, 0.8]), 7.0, n, 800e-6)
            sq[n] = [[list(map(float, r.point)), list(map(float, r.vector))] for r in b]
        except Exception as e:
            sq[n] = type(e).__name__
    print("RESULT" + json.dumps({"mirrors": out, "square": sq}))
''')


def test_single_ray_methods_and_square_source_match_reference(twin):
    """`_get_intersection`, `_ReflectionMirrorRay` / `_TransmitMaskRay`, `ReflectionMirrorRayList` /
    `TransmitMaskRayList` of every optic class on rays given in the optic's own frame, and `PlaneWaveSquare`
    (which the reference only runs for NbRays < 4)."""
    lo, hi = 0, int(os.environ.get("ART_FUZZ_METHODS", "48"))
    ref = reference_results("methods", METHODS_SCRIPT, METHODS_GEN, lo, hi)
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalRay as mray
    import ART.ModuleSource as msource
    import ART.ModuleDefects as mdef
    ns = {"np": np}
    exec(METHODS_GEN, ns)
    n_hits = 0
    for seed in range(lo, hi):
        e = ref["mirrors"][str(seed)]
        o, rays = ns["make_mirror_and_rays"](seed, mmirror, mmask, msupp, mray, mdef)
        assert o.type == e["type"]
        pts = [o._get_intersection(q) for q in rays]
        assert [p is None for p in pts] == [p is None for p in e["pts"]], (seed, e["type"])
        for p, pe in zip(pts, e["pts"]):
            if pe is not None:
                assert np.abs(p - np.array(pe)).max() <= 1e-9 * max(1.0, np.abs(pe).max()), (seed, e["type"])
                n_hits += 1
        hit_pts = [p for p in pts if p is not None]
        for p, nrm in zip(hit_pts, [x for x in e["normals"] if x is not None]):
            assert np.abs(np.asarray(o.get_normal(p), float) - np.array(nrm)).max() <= 1e-9, (seed, e["type"])
        for p, offs in zip(hit_pts, e["offsets"]):
            mine = [d.get_offset(p - o.get_centre()) for d in getattr(o, "DeformationList", [])]
            assert np.allclose(mine, offs, rtol=0, atol=1e-13), (seed, mine, offs)
        lst = mmask.TransmitMaskRayList(o, rays) if o.type == "Mask" else mmirror.ReflectionMirrorRayList(o, rays)
        assert [q.number for q in lst] == [x[0] for x in e["list"]]
        for q, x in zip(lst, e["list"]):
            assert np.abs(q.point - np.array(x[1])).max() <= 1e-9 * max(1.0, np.abs(x[1]).max())
            assert np.abs(q.vector - np.array(x[2])).max() <= 1e-9
            assert abs(q.incidence - x[3]) <= 1e-9
            assert len(q.path) == len(x[4]) and np.abs(np.array(q.path) - np.array(x[4])).max() <= 1e-9 * max(1.0, max(x[4]))
            assert q.wavelength == x[5] and abs(q.intensity - x[6]) <= 1e-15
        for q, p, x in zip(rays, pts, e["single"]):
            if x is None:
                continue
            s = mmask._TransmitMaskRay(o, p, q) if o.type == "Mask" else mmirror._ReflectionMirrorRay(o, p, q)
            assert np.abs(s.point - np.array(x[0])).max() <= 1e-9 * max(1.0, np.abs(x[0]).max())
            assert np.abs(s.vector - np.array(x[1])).max() <= 1e-9 and abs(s.incidence - x[2]) <= 1e-9
            assert np.abs(np.array(s.path) - np.array(x[3])).max() <= 1e-9 * max(1.0, max(x[3]))
    assert n_hits >= 2 * (hi - lo)
    for n, expect in ref["square"].items():
        args = (np.array([1.0, 2.0, 3.0]), np.array([0.2, -0.5, 0.8]), 7.0, int(n), 800e-6)
        if isinstance(expect, str):
            with pytest.raises(Exception) as ei:
                msource.PlaneWaveSquare(*args)
            assert type(ei.value).__name__ == expect
        else:
            b = msource.PlaneWaveSquare(*args)
            assert len(b) == len(expect)
            assert np.abs(b.points() - np.array([x[0] for x in expect])).max() <= 1e-12
            assert np.abs(b.vectors() - np.array([x[1] for x in expect])).max() <= 1e-12


DET_GEN = textwrap.dedent('''
    def detector_session(seed, mdet, last, refpoint):
        """Random sequence of Detector operations on the last bundle of a chain; returns a JSON-able log."""
        rng = np.random.default_rng(seed + 777)
        log = []
        def state(D, tag):
            log.append([tag, None if D.centre is None else [float(v) for v in D.centre],
                        None if D.normal is None else [float(v) for v in D.normal], [float(v) for v in D.refpoint]])
        def attempt(tag, fn):
            try:
                v = fn()
                log.append([tag, "ok" if v is None else v])
            except Exception as e:
                log.append([tag, "raises " + type(e).__name__])
        D = mdet.Detector(np.asarray(refpoint, dtype=float))
        attempt("incomplete.get_distance", lambda: float(D.get_distance()))
        attempt("incomplete.points", lambda: len(D.get_PointList2D(last)))
        attempt("bad centre", lambda: setattr(D, "centre", [1.0, 2.0, 3.0]))
        attempt("bad normal", lambda: setattr(D, "normal", np.zeros(3)))
        attempt("bad refpoint", lambda: setattr(D, "refpoint", np.zeros(2)))
        D.autoplace(last, float(rng.uniform(30, 500)))
        state(D, "autoplace")
        for _ in range(int(rng.integers(2, 6))):
            k = int(rng.integers(0, 4))
            if k == 0:
                D.shiftByDistance(float(rng.uniform(-20, 40)))
            elif k == 1:
                D.shiftToDistance(float(rng.uniform(5, 400)))
            elif k == 2:
                D = D.copy_detector()
            else:
                n = D.normal + 0.2 * rng.normal(size=3)
                D.normal = n
                D.centre = D.centre + rng.normal(size=3)
            state(D, "op%d" % k)
            log.append(["distance", float(D.get_distance())])
        P3 = np.array([np.asarray(p, dtype=float) for p in D.get_PointList3D(last)])
        P2 = np.array([np.asarray(p, dtype=float) for p in D.get_PointList2D(last)])
        PC = np.array([np.asarray(p, dtype=float) for p in D.get_PointList2DCentre(last)])
        dl = np.array([float(v) for v in D.get_Delays(last)])
        log.append(["readout", P3.tolist(), P2.tolist(), PC.tolist(), dl.tolist()])
        return log
''')

DET_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleProcessing as mp, ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp
    import ART.ModuleDetector as mdet
    exec(sys.stdin.read())
    out = {}
    for seed in range(lo, hi):
        SP, optics, dist, inc, plane = make_case(seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 60
        try:
            ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
            last = ch.get_output_rays()[-1]
        except Exception as e:
            out[seed] = {"skip": type(e).__name__}
            continue
        if len(last) < 10:
            out[seed] = {"skip": "few rays"}
            continue
        out[seed] = {"log": detector_session(seed, mdet, last, ch.optical_elements[-1].position)}
    print("RESULT" + json.dumps(out))
''')


def test_detector_sessions_match_reference(twin):
    """Detector construction errors, autoplace, shiftBy/shiftTo/copy, manual re-posing, and the four read-out
    methods in random sequences (ART/ModuleDetector.py:47-279)."""
    lo, hi = 0, int(os.environ.get("ART_FUZZ_DETECTOR", "40"))
    ref = reference_results("detector", DET_SCRIPT, GENERATOR + DET_GEN, lo, hi)
    import ART.ModuleProcessing as mp
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleDetector as mdet
    ns = {}
    exec(GENERATOR + DET_GEN, ns)
    compared = 0
    for seed in range(lo, hi):
        e = ref[str(seed)]
        if "skip" in e:
            continue
        SP, optics, dist, inc, plane = ns["make_case"](seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 60
        ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
        last = ch.get_output_rays()[-1]
        mine = ns["detector_session"](seed, mdet, last, ch.optical_elements[-1].position)
        assert len(mine) == len(e["log"]), seed
        for a, b in zip(mine, e["log"]):
            assert a[0] == b[0], (seed, a[0], b[0])
            if a[0] == "readout":
                scale = max(1.0, np.abs(np.array(b[1])).max())
                # delays are path differences: tolerance relative to the travel time over the scene scale
                travel_fs = scale / 299792458000.0 * 1e15
                for x, y, tol in zip(a[1:4], b[1:4], (1e-9 * scale,) * 3):
                    assert np.abs(np.array(x) - np.array(y)).max() <= tol, (seed, a[0])
                assert np.abs(np.array(a[4]) - np.array(b[4])).max() <= 1e-9 * travel_fs, seed
            elif a[0] == "distance" or isinstance(b[1], float):
                assert abs(a[1] - b[1]) <= 1e-9 * max(1.0, abs(b[1])), (seed, a, b)
            elif isinstance(b[1], str) or b[1] is None or isinstance(b[1], int):
                assert a[1] == b[1], (seed, a, b)
            else:
                for x, y in zip(a[1:], b[1:]):
                    assert (x is None) == (y is None), (seed, a, b)
                    if x is not None:
                        assert np.abs(np.array(x) - np.array(y)).max() <= 1e-9 * max(1.0, np.abs(y).max()), (seed, a[0])
        compared += 1
    assert compared >= (hi - lo) // 3


ERR_CASES = [
    "mray.Ray([0, 0, 0], np.array([0, 0, 1.0]))",
    "mray.Ray(np.zeros(3), np.zeros(3))",
    "mray.Ray(np.zeros(3), np.array([0, 0, 1e-12]))",
    "mray.Ray(np.zeros(3), np.array([0, 0, 2.0]), Number=1.5)",
    "mray.Ray(np.zeros(3), np.array([0, 0, 2.0]), Number=np.int64(3)).number",
    "tuple(mray.Ray(np.zeros(3), np.array([0, 3.0, 4.0])).vector)",
    "setattr(ray, 'wavelength', 'red')",
    "setattr(ray, 'wavelength', 5)",
    "setattr(ray, 'incidence', 1)",
    "setattr(ray, 'incidence', 0.5)",
    "setattr(ray, 'intensity', None)",
    "setattr(ray, 'intensity', np.float64(0.5))",
    "setattr(ray, 'number', 4)",
    "setattr(ray, 'point', [1, 2, 3])",
    "setattr(ray, 'vector', np.zeros(3))",
    "hash(ray) == hash(ray.copy_ray())",
    "moe.OpticalElement(plane, [0, 0, 0], np.array([0, 0, 1.0]), np.array([1.0, 0, 0]))",
    "moe.OpticalElement(plane, np.zeros(3), np.array([0, 0, 0.0]), np.array([1.0, 0, 0]))",
    "moe.OpticalElement(plane, np.zeros(3), np.array([0, 0, 1.0]), np.array([0, 0, 1.0]))",
    "tuple(moe.OpticalElement(plane, np.zeros(3), np.array([0, 0, 2.0]), np.array([3.0, 0, 1.0])).majoraxis)",
    "moe.OpticalElement('mirror', np.zeros(3), np.array([0, 0, 1.0]), np.array([1.0, 0, 0])).type",
    "moc.OpticalChain([], [])",
    "moc.OpticalChain('rays', [oe])",
    "moc.OpticalChain([ray], 'elements')",
    "moc.OpticalChain([ray], [plane])",
    "moc.OpticalChain([ray], [oe], 5)",
    "moc.OpticalChain([ray], [oe], 'x', 7, 1.0)",
    "len(moc.OpticalChain([ray], [oe]).get_output_rays()[0])",
    "mmirror.MirrorEllipsoidal(sup)",
    "mmirror.MirrorEllipsoidal(sup, SemiMajorAxis=300)",
    "mmirror.MirrorEllipsoidal(sup, f_object=300, f_image=200)",
    "round(mmirror.MirrorEllipsoidal(sup, f_object=300, f_image=200, OffAxisAngle=60).b, 9)",
    "round(mmirror.MirrorEllipsoidal(sup, SemiMajorAxis=300, SemiMinorAxis=200)._offaxisangle, 12)",
    "round(mmirror.MirrorEllipsoidal(sup, SemiMajorAxis=300, SemiMinorAxis=200, f_object=350, f_image=250)._offaxisangle, 12)",
    "mmirror.MirrorSpherical(-100, sup).type",
    "mmirror.MirrorCylindrical(-100, sup).type",
    "[round(v, 9) for v in mmirror.ReturnOptimalToroidalRadii(500, 75)]",
    "round(mmirror.MirrorParabolic(100, 90, sup)._p, 12)",
    "mdef.MeasuredMap(sup, {})",
    "mp.FindOptimalDistance(det, chain.get_output_rays()[-1], 'spotsize')",
    "mp.FindOptimalDistance(det, chain.get_output_rays()[-1], 'size')",
    "chain.shift_source('diagonal', 1.0)",
    "chain.shift_source('vert', '1')",
    "chain.tilt_source('sideways', 1.0)",
    "chain.tilt_source('in_plane', [1])",
    "chain.rotate_OE(7, 'pitch', 1.0)",
    "chain.rotate_OE(0, 'spin', 1.0)",
    "chain.rotate_OE(0, 'pitch', '1')",
    "chain.shift_OE(0, 'sideways', 1.0)",
    "chain.shift_OE(-9, 'normal', 1.0)",
    "chain.get_OE_loop_list(0, 'bad', [1.0])",
    "chain.get_OE_loop_list(0, 'pitch', 1.0)",
    "chain.get_source_loop_list('tilt_in_plane', 5)",
    "chain.get_source_loop_list('zoom', [1.0])",
    "[c.loop_variable_name for c in chain.get_source_loop_list('shift_vert', [0.1, 0.2])]",
    "[c.loop_variable_name for c in chain.get_OE_loop_list(-1, 'shift_major', [0.1])]",
    "planechain.shift_source('vert', 1.0)",
    "mp.OEPlacement(dict(SP), [tor, tor], [[100, 200], 300], [[80, 70], -80])",
    "len(mp.OEPlacement(dict(SP), [tor, tor], [[100, 200], 300], [80, -80]))",
    "mp.OEPlacement(dict(SP), [tor, tor], [100, 300], [80, [-80, -70]])[1].loop_variable_name",
    "mp.OEPlacement(dict(SP), [tor, 'lens'], [100, 300], [80, -80])",
    "mp.RayTracingCalculation([ray], [moe.OpticalElement(Odd(), np.zeros(3), np.array([0, 0, 1.0]), np.array([1.0, 0, 0]))])",
    "mp.ReturnNumericalAperture(chain.get_output_rays()[-1], 1) > 0",
    "round(mp.ReturnAiryRadius(50e-6, 0.01), 12)",
    "mp.ReturnAiryRadius(50e-6, 1e-4)",
    "round(mp.StandardDeviation([np.array([0.0, 1.0]), np.array([2.0, 5.0])]), 12)",
    "round(mp.WeightedStandardDeviation([1.0, 2.0, 4.0], [1.0, 1.0, 2.0]), 12)",
    "mdet.Detector([0, 0, 0])",
    "mdet.Detector(np.zeros(3), np.zeros(3), np.zeros(3))",
    "mdet.Detector(np.zeros(3)).get_distance()",
    "msupp.SupportRoundHole(10, 2, 1, 1)._IncludeSupport(np.array([1.0, 1.0, 0]))",
    "msupp.SupportRectangleRectHole(10, 8, 2, 2, 1, 1)._IncludeSupport(np.array([4.9, -4.0, 0]))",
    "[round(v, 12) for v in msupp.SupportRectangle(6, 8)._CircumRect()] + [round(msupp.SupportRectangle(6, 8)._CircumCirc(), 12)]",
    "mgeo.SolverQuadratic(0, 2, -4)",
    "mgeo.SolverQuadratic(1, 0, 1)",
    "[round(v, 10) for v in mgeo.SolverQuartic(1, 0, -5, 0, 4)]",
    "mgeo.KeepPositiveSolution([-1, 0, 1e-13, 2])",
    "mgeo.IncludeRectangle(-4, 2, np.array([2.0, -1.0, 0]))",
    "[round(v, 12) for v in mgeo.RotationPoint(np.array([1.0, 2, 3]), np.array([0, 0, 1.0]), np.array([0, 0, -1.0]))]",
    "[round(v, 12) for v in mgeo.VectorPerpendicular(np.array([0.0, 0, 2]))]",
    "[round(v, 12) for v in mgeo.VectorPerpendicular(np.array([1.0, 2, 0]))]",
    "round(mgeo.AngleBetweenTwoVectors(np.array([1.0, 0, 0]), np.array([-1.0, 1e-9, 0])), 12)",
    "mgeo.DiameterPointList([])",
    "round(mgeo.DiameterPointList([np.array([0.0, 0]), np.array([3.0, 4])]), 12)",
    # seeded random operations: the same NumPy draws in the same order on both sides
    "(np.random.seed(3), chain.shift_source('random', 1.5), [float(x) for x in chain.source_rays[5].point])[-1]",
    "(np.random.seed(4), chain.tilt_source('random', 0.2), [float(x) for x in chain.source_rays[5].vector])[-1]",
    "(np.random.seed(5), oe.rotate_random_by(2.0), [float(x) for x in oe.normal] + [float(x) for x in oe.majoraxis])[-1]",
    "(np.random.seed(6), oe.shift_along_random(0.7), [float(x) for x in oe.position])[-1]",
    "(np.random.seed(7), chain.rotate_OE(1, 'random', 0.3), [float(x) for x in chain.optical_elements[1].normal])[-1]",
    "(np.random.seed(8), chain.shift_OE(0, 'random', 0.3), [float(x) for x in chain.optical_elements[0].position])[-1]",
    "(np.random.seed(9), [[float(x) for x in c.optical_elements[1].normal] + [float(x) for x in c.optical_elements[0].position] "
    "for c in chain.get_OE_random_loop_list(0.1, 0.05, 3)])[-1][2]",
    "(np.random.seed(9), [c.loop_variable_name for c in chain.get_OE_random_loop_list(0.1, 0.05, 2)])[-1]",
    "(np.random.seed(10), [[float(x) for x in c.source_rays[3].vector] for c in chain.get_source_loop_list('tilt_random', [0.1, 0.2])])[-1][1]",
    "(np.random.seed(11), [[float(x) for x in c.source_rays[3].point] for c in chain.get_source_loop_list('shift_random', [0.1, 0.2])])[-1][0]",
    "[round(float(x), 12) for x in chain.get_source_loop_list('divergence', [0.005, 0.02])[1].source_rays[7].vector]",
    "[round(float(c.source_rays[7].intensity), 12) for c in chain.get_source_loop_list('divergence', [0.005, 0.02])]",
    "oe.rotate_pitch_by('1')",
    "oe.shift_along_normal([1])",
    "(oe.rotate_pitch_by(1.0), oe.rotate_roll_by(-2.0), oe.rotate_yaw_by(3.0), oe.shift_along_major(0.5), oe.shift_along_cross(-0.5), "
    "[float(x) for x in oe.position] + [float(x) for x in oe.normal] + [float(x) for x in oe.majoraxis])[-1]",
    "hash(oe) == hash(moe.OpticalElement(plane, np.array([0.0, 0.0, 10.0]), np.array([0.0, 0.6, -0.8]), np.array([1.0, 0.0, 0.0])))",
]

ERR_PRELUDE = textwrap.dedent('''
    import numpy as np
    import ART.ModuleOpticalRay as mray, ART.ModuleOpticalElement as moe, ART.ModuleOpticalChain as moc
    import ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp, ART.ModuleDefects as mdef
    import ART.ModuleProcessing as mp, ART.ModuleDetector as mdet, ART.ModuleGeometry as mgeo
    class Odd:
        type = "Lens"
        support = msupp.SupportRound(5)
        def get_centre(self): return np.zeros(3)
    def run_cases(cases):
        out = []
        for c in cases:
            sup = msupp.SupportRound(20.0)
            plane = mmirror.MirrorPlane(sup)
            ray = mray.Ray(np.zeros(3), np.array([0.0, 0.0, 1.0]), (0.0,), 1, 50e-6, 0.1, 1.0)
            oe = moe.OpticalElement(plane, np.array([0.0, 0.0, 10.0]), np.array([0.0, 0.6, -0.8]), np.array([1.0, 0.0, 0.0]))
            R, r = mmirror.ReturnOptimalToroidalRadii(300, 80)
            tor = mmirror.MirrorToroidal(R, r, msupp.SupportRectangle(150, 30))
            SP = {"Divergence": 0.01, "SourceSize": 0, "Wavelength": 50e-6, "DeltaFT": 0.5, "NumberRays": 30}
            chain = mp.OEPlacement(dict(SP), [tor, tor], [300, 600], [80, -80])
            planechain = mp.OEPlacement(dict(SP), [mmirror.MirrorPlane(msupp.SupportRound(50))], [100], [0])
            det = mdet.Detector(chain.optical_elements[-1].position)
            det.autoplace(chain.get_output_rays()[-1], 300)
            try:
                v = eval(c)
                if isinstance(v, (np.bool_, bool)): v = bool(v)
                elif isinstance(v, (np.integer,)): v = int(v)
                elif isinstance(v, (np.floating,)): v = float(v)
                elif isinstance(v, tuple): v = [float(x) for x in v]
                elif isinstance(v, list): v = [x if isinstance(x, str) else float(x) for x in v]
                elif not isinstance(v, (int, float, str, type(None))): v = type(v).__name__
                out.append(["value", v])
            except Exception as e:
                out.append(["raises", type(e).__name__])
        return out
''')

ERR_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF = sys.argv[1], sys.argv[2]
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    src = sys.stdin.read()
    prelude, cases = src.split("#CASES#")
    exec(prelude)
    print("RESULT" + json.dumps(run_cases(json.loads(cases))))
''')


def test_values_and_exception_types_of_the_host_api_match_reference(twin, capsys):
    """A table of small API calls -- constructors with bad arguments, validating setters, helper functions, chain
    operations with wrong axis names or indices -- evaluated by the reference and by the product: same values, same
    exception TYPES ("same names, argument meaning and error behaviour")."""
    ref = reference_results("errors", ERR_SCRIPT, ERR_PRELUDE + "#CASES#" + json.dumps(ERR_CASES), None, None)
    ns = {}
    exec(ERR_PRELUDE, ns)
    mine = ns["run_cases"](ERR_CASES)
    bad = []
    for c, a, b in zip(ERR_CASES, mine, ref):
        same = a[0] == b[0] and (a[1] == b[1] or (isinstance(b[1], (float, list)) and np.allclose(a[1], b[1], rtol=0, atol=1e-9)))
        if not same:
            bad.append((c, a, b))
    assert not bad, "\\n".join(f"{c}\\n    product:   {a}\\n    reference: {b}" for c, a, b in bad)


GEO_GEN = textwrap.dedent('''
    def geometry_session(seed, mgeo, mray):
        """Every helper of ModuleGeometry on seeded random inputs (incl. the RotationPoint special cases); a flat list
        of numbers."""
        rng = np.random.default_rng(seed + 31337)
        v = lambda: rng.normal(size=3)
        out = []
        def put(x):
            out.extend(np.asarray(x, dtype=float).ravel().tolist())
        a, b, c, p = v(), v(), v(), v() * 50
        put(mgeo.Normalize(a)); put(mgeo.VectorPerpendicular(a)); put([mgeo.AngleBetweenTwoVectors(a, b)])
        n = mgeo.Normalize(c)
        if abs(np.dot(a, n)) > 0.05:
            put(mgeo.IntersectionLinePlane(p, a, b * 10, n))
        put(mgeo.SpiralVogel(int(rng.integers(1, 40)), float(rng.uniform(0.1, 9))))
        put(sorted(mgeo.SolverQuadratic(1.0, float(rng.uniform(-9, 9)), float(rng.uniform(-9, 2)))))
        r = np.sort(rng.uniform(-5, 5, 4))
        co = np.poly(r)
        put(sorted(np.round(mgeo.SolverQuartic(*co), 7)))
        vals = list(rng.uniform(-1, 1, 6))
        put(mgeo.KeepPositiveSolution(vals)); put(mgeo.KeepNegativeSolution(vals))
        put(mgeo.ClosestPoint(p, p + a, p + 2 * b)); put(mgeo.FarestPoint(p, p + a, p + 2 * b))
        pts2 = [rng.uniform(-5, 5, 2) for _ in range(7)]
        put([mgeo.DiameterPointList(pts2)]); put(mgeo.CentrePointList(pts2))
        pts3 = [v() for _ in range(5)]
        put([mgeo.DiameterPointList(pts3)])
        put([float(mgeo.IncludeRectangle(4.0, 3.0, v() * 2)), float(mgeo.IncludeDisk(2.0, v() * 2))])
        put(mgeo.SymmetricalVector(a, b))
        put(mgeo.TranslationPoint(p, a)); put(mgeo.TranslationPointList(pts3, a))
        ang = float(rng.uniform(-3.5, 3.5))
        put(mgeo.RotationAroundAxis(a, ang, b)); put(mgeo.RotationAroundAxis(a, 0.0, b)); put(mgeo.RotationAroundAxis(a, np.pi, b))
        for ax1, ax2 in ((a, b), (a, a * 2.5), (a, -a), (np.array([0.0, 0, 1]), np.array([0.0, 0, -1]))):
            put(mgeo.RotationPoint(p, ax1, ax2))
        put(mgeo.RotationPointList(pts3, a, b))
        ray = mray.Ray(p.copy(), mgeo.Normalize(c), (0.0, 1.5), 3, 50e-6, 0.2, 0.7)
        for q in (mgeo.TranslationRay(ray, a), mgeo.RotationRay(ray, a, b), mgeo.RotationRay(ray, a, -a)):
            put(q.point); put(q.vector); put(q.path); put([q.number, q.incidence, q.intensity])
        rl = [mray.Ray(v() * 10, mgeo.Normalize(v()), (0.0,), k) for k in range(4)]
        for lst in (mgeo.TranslationRayList(rl, a), mgeo.RotationRayList(rl, a, b), mgeo.RotationAroundAxisRayList(rl, a, ang)):
            for q in lst:
                put(q.point); put(q.vector)
        put(mgeo.normal_add(np.array([0.1, -0.2, 1.0]), np.array([-0.05, 0.3, 0.9])))
        return out
''')

GEO_SCRIPT = textwrap.dedent('''
    import sys, json
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import numpy as np
    import ART.ModuleGeometry as mgeo, ART.ModuleOpticalRay as mray
    exec(sys.stdin.read())
    print("RESULT" + json.dumps({s: geometry_session(s, mgeo, mray) for s in range(lo, hi)}))
''')


def test_geometry_helpers_match_reference(twin):
    """All 27 functions of ModuleGeometry on random inputs (rotations incl. the identity / point-inversion special
    cases, ray and ray-list transforms, solvers, point-list statistics)."""
    lo, hi = 0, int(os.environ.get("ART_FUZZ_GEOMETRY", "60"))
    ref = reference_results("geometry", GEO_SCRIPT, GEO_GEN, lo, hi)
    import ART.ModuleGeometry as mgeo
    import ART.ModuleOpticalRay as mray
    ns = {"np": np}
    exec(GEO_GEN, ns)
    for seed in range(lo, hi):
        mine = np.array(ns["geometry_session"](seed, mgeo, mray))
        want = np.array(ref[str(seed)])
        assert mine.shape == want.shape, (seed, mine.shape, want.shape)
        err = np.abs(mine - want) / np.maximum(1.0, np.abs(want))
        assert err.max() <= 1e-9, (seed, int(err.argmax()), mine[err.argmax()], want[err.argmax()])


MAIN_GEN = textwrap.dedent('''
    def main_options(seed, ch):
        """Random DetectorOptions / AnalysisOptions for ARTmain.main (auto or manual detector, autofocus on or off)."""
        rng = np.random.default_rng(seed + 2024)
        det = {"ReflectionNumber": -1, "AutoDetectorDistance": bool(rng.uniform() < 0.5),
               "OptFor": ["intensity", "duration"][int(rng.integers(0, 2))]}
        if rng.uniform() < 0.3:
            last = ch.optical_elements[-1]
            det.update(ManualDetector=True, DetectorCentre=np.asarray(last.position, dtype=float) + np.array([30.0, -20.0, 10.0]),
                       DetectorNormal=np.array([-0.3, 0.2, -0.9]))
        else:
            det.update(ManualDetector=False, DistanceDetector=float(rng.uniform(40, 500)))
        if rng.uniform() < 0.1:
            det.pop("DistanceDetector", None)
            det["ManualDetector"] = False
            det["DistanceDetector"] = None           # -> RuntimeError in setup_detector
        ana = {"verbose": False, "save_results": False}
        return det, ana
''')

MAIN_SCRIPT = textwrap.dedent('''
    import sys, json, copy
    sys.dont_write_bytecode = True
    ROOT, REF, lo, hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
    sys.path[:0] = [REF, ROOT + "/tests/golden/_standin"]
    import matplotlib; matplotlib.use("Agg")
    import numpy as np
    import ART.ModuleProcessing as mp, ART.ModuleMirror as mmirror, ART.ModuleMask as mmask, ART.ModuleSupport as msupp
    import ART.DefaultOptions as DO
    import ARTmain
    assert ARTmain.__file__.startswith(REF)
    exec(sys.stdin.read())
    defaults = {k: dict(getattr(DO, k)) for k in ("DefaultSourceProperties", "DefaultDetectorOptions", "DefaultAnalysisOptions")}
    out = {}
    for seed in range(lo, hi):
        for k, v in defaults.items():            # complete_defaults mutates the module-level dicts
            getattr(DO, k).clear(); getattr(DO, k).update(v)
        SP, optics, dist, inc, plane = make_case(seed, mmirror, mmask, msupp)
        SP["NumberRays"] = 120
        try:
            ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
        except Exception as e:
            out[seed] = {"skip": type(e).__name__}
            continue
        det, ana = main_options(seed, ch)
        try:
            kept = ARTmain.main(ch, SP, det, ana)
            D = kept["Detector"][0]
            out[seed] = {"et": float(kept["ETransmission"][0]), "spot": float(kept["SpotSizeSD"][0]), "dur": float(kept["DurationSD"][0]),
                         "distance": float(D.get_distance()), "auto": det["AutoDetectorDistance"], "optfor": det["OptFor"],
                         "n": len(kept["OpticalChain"][0].get_output_rays()[-1])}
        except Exception as e:
            out[seed] = {"error": type(e).__name__}
    print("RESULT" + json.dumps(out))
''')


def test_artmain_main_matches_reference(twin):
    """`ARTmain.main` end to end (trace, transmission, detector set-up -- automatic, manual or invalid --, autofocus or
    summary) on random chains with <= 1000 rays, where the reference's autofocus also uses every ray."""
    lo, hi = 0, int(os.environ.get("ART_FUZZ_MAIN", "24"))
    ref = reference_results("main", MAIN_SCRIPT, GENERATOR + MAIN_GEN, lo, hi)
    import ART.ModuleProcessing as mp
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ARTmain
    from attosecondraytracing_amd import DefaultOptions as DO
    defaults = {k: dict(getattr(DO, k)) for k in ("DefaultSourceProperties", "DefaultDetectorOptions", "DefaultAnalysisOptions")}
    ns = {}
    exec(GENERATOR + MAIN_GEN, ns)
    compared = 0
    try:
        for seed in range(lo, hi):
            e = ref[str(seed)]
            if "skip" in e:
                continue
            for k, v in defaults.items():
                getattr(DO, k).clear()
                getattr(DO, k).update(v)
            SP, optics, dist, inc, plane = ns["make_case"](seed, mmirror, mmask, msupp)
            SP["NumberRays"] = 120
            ch = mp.OEPlacement(SP, optics, dist, inc, plane, "fuzz")
            det, ana = ns["main_options"](seed, ch)
            if "error" in e:
                with pytest.raises(Exception) as ei:
                    ARTmain.main(ch, SP, det, ana)
                assert type(ei.value).__name__ == e["error"], (seed, ei.value, e)
                continue
            kept = ARTmain.main(ch, SP, det, ana)
            assert len(kept["OpticalChain"][0].get_output_rays()[-1]) == e["n"], seed
            assert abs(kept["ETransmission"][0] - e["et"]) <= 1e-9, (seed, kept["ETransmission"][0], e)
            D = kept["Detector"][0]
            if e["auto"] and (e["n"] < 30 or (not np.isnan(e["dur"]) and e["dur"] < 1e-6)):
                compared += 1          # a handful of rays, or all optical paths equal: the fitness is flat up to
                continue               # rounding noise (ties decide), nothing to compare
            if not e["auto"]:
                assert abs(D.get_distance() - e["distance"]) <= 1e-9 * max(1.0, e["distance"]), seed
                assert abs(kept["SpotSizeSD"][0] - e["spot"]) <= 1e-9 * max(1.0, e["spot"]), (seed, kept["SpotSizeSD"][0], e)
                assert abs(kept["DurationSD"][0] - e["dur"]) <= 1e-7 * max(1.0, e["dur"]), (seed, kept["DurationSD"][0], e)
            else:
                # autofocus: same caveat as in the FindOptimalDistance test (19 or 20 scan positions per level)
                assert abs(D.get_distance() - e["distance"]) <= 0.13 * max(1.0, abs(e["distance"])) + 1.0, (seed, D.get_distance(), e)
            compared += 1
    finally:
        for k, v in defaults.items():
            getattr(DO, k).clear()
            getattr(DO, k).update(v)
    assert compared >= (hi - lo) // 3

"""Spot size and duration against a long-double truth.  TEST INFRASTRUCTURE shared by tests/test_readout_truth_host.py (CPU
twin) and tests/test_gpu_readout_truth.py (MI355X): the truth, the scenes, the detector poses, the bars and the checks.

The truth is NumPy longdouble (64-bit significand) throughout, written from the formulas of the read-out -- the reference's
ART/ModuleDetector.py:191-279 and the comments of csrc/art_device.h -- not from the header's code:

  t = n.(C - p) / (d.n),  I = p + t d,  (X, Y) = (rot (I - C))[0:2],  opl = path + |t| |d|

on the bundle's fp64 state (points, directions, paths, alive, weights) and the detector's fp64 centre, normal and rot
(Detector._desc()), all taken as exact; EVERY alive ray counts.  Standard deviations are two-pass, sum w (x - mu_w)^2 / sum w.
A plane shifted by s (Detector.shiftByDistance: centre - s normal) is moved itself and read out again; the slopes d/ds
of the linear model only enter the bars.

Bars (none of them comes from the code under test):
  per-ray X, Y, opl     1e-10 of span (the project's parity bar); span_xy = the largest distance from a ray's origin to
                        the plane, span_L = the largest opl
  spot, duration, s=0   |sigma - truth| <= 1e-6 truth + 16 eps span      (1e-6: what tests/test_host_shell.py asks of the
                        moment form; 16 eps span: the floor of sensitivity_common.compare_table -- no fp64 trace knows a
                        coordinate better -- which is also what a single ray or a perfect focus is held to)
  variances at s != 0   |var - truth| <= 2e-6 truth + 16 eps (sqrt V0 + |s| sqrt Vs)^2 + (16 eps span)^2, V0 the truth's
                        variance of that coordinate at s = 0, Vs the truth's mean square of its slope as the kernels sum it
                        (dX/ds, dY/ds, dO/ds - 1): the rounding of CENTRED sums of the size N (X0 + s X')^2.
The reference's own algorithm -- a two-pass fp64 StandardDeviation of get_PointList2DCentre and get_Delays -- is held to
the same bars in every case: a bar it cannot meet is a broken test, not a product failure."""
import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 1e-18
EPS = LD(np.finfo(np.float64).eps)
PARITY = 1e-10
REL = 1e-6
FLOOR = 16 * EPS
LIGHT = LD(299792458000)            # mm/s
FS = LD(10) ** 15 / LIGHT           # mm of path -> fs
SHIFTS = (0.0, 1e-3, -1e-3, 0.1, -0.1, 5.0, -5.0)
SIZES = (1, 2, 3, 257, 20001, 300001)
WORST = {}                          # path -> worst ratio to its bar, over everything checked in this process


def ld(a):
    return np.asarray(a, dtype=LD)


def note(path, ratio):
    WORST[path] = max(WORST.get(path, 0.0), float(ratio))


def worst_lines(backend):
    return [f"[readout truth, {backend}] worst error / bar:  " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items()))]


# ------------------------------------------------------------------------------------------------------------- the truth
def state_of(B):
    """The bundle's fp64 state on the host: P, D [n, 3], path [n], alive [n] (bool), w [n] or None."""
    d = B.data.cpu().numpy()
    w = None if B.intensity is None else B.intensity.cpu().numpy().copy()
    return {"P": d[0:3].T.copy(), "D": d[3:6].T.copy(), "path": d[6].copy(), "alive": B.alive.cpu().numpy() != 0, "w": w}


def plane_of(det):
    d = det._desc()
    return {"C": np.array(d.centre[:]), "n": np.array(d.normal[:]), "rot": np.array(d.rot[:]).reshape(3, 3)}


def readout(st, pl, s=0.0):
    """X, Y, opl of the alive rays on the plane moved by s along -normal, and t."""
    a = st["alive"]
    P, D, path = ld(st["P"][a]), ld(st["D"][a]), ld(st["path"][a])
    n, rot = ld(pl["n"]), ld(pl["rot"])
    C = ld(pl["C"]) - LD(s) * n
    t = ((C - P) @ n) / (D @ n)
    I = P + t[:, None] * D
    R = (I - C) @ rot.T
    return R[:, 0], R[:, 1], path + np.abs(t) * np.sqrt((D * D).sum(axis=1)), t


def slopes(st, pl):
    """d/ds of X, Y and opl - s at s = 0: t' = -(n.n) / (d.n), (I - C_s)' = t' d + n, opl' = sign(t) t' |d|."""
    a = st["alive"]
    P, D = ld(st["P"][a]), ld(st["D"][a])
    n, rot, C = ld(pl["n"]), ld(pl["rot"]), ld(pl["C"])
    den = D @ n
    dt = -(n @ n) / den
    R = (dt[:, None] * D + n) @ rot.T
    t = ((C - P) @ n) / den
    return R[:, 0], R[:, 1], np.where(t >= 0, dt, -dt) * np.sqrt((D * D).sum(axis=1)) - 1


def weights_of(st, weighted):
    a = st["alive"]
    return ld(st["w"][a]) if weighted else np.ones(int(a.sum()), dtype=LD)


def variance(x, w):
    mu = (w * x).sum() / w.sum()
    return (w * (x - mu) ** 2).sum() / w.sum()


def truth(st, pl, s, weighted):
    """dict: var (X, Y, opl in mm^2), spot (mm), dur (fs) on the plane moved by s."""
    X, Y, O, _ = readout(st, pl, s)
    w = weights_of(st, weighted)
    v = [variance(q, w) for q in (X, Y, O)]
    return {"var": v, "spot": np.sqrt(v[0] + v[1]), "dur": np.sqrt(v[2]) * FS}


def spans(st, pl):
    """(span_xy, span_L): the largest distance from a ray's origin to the plane, the largest opl."""
    _, _, O, t = readout(st, pl)
    a = st["alive"]
    return (np.abs(t) * np.sqrt((ld(st["D"][a]) ** 2).sum(axis=1))).max(), np.abs(O).max()


def bars0(tr, sp):
    """Bars of (spot in mm, duration in fs) at s = 0."""
    return REL * tr["spot"] + FLOOR * sp[0], REL * tr["dur"] + FLOOR * sp[1] * FS


def start_pose(st, pl, weighted):
    """(V0, Vs): the truth's variances at s = 0 and the mean squares of the slopes, per coordinate."""
    w = weights_of(st, weighted)
    return truth(st, pl, 0.0, weighted)["var"], [(w * q * q).sum() / w.sum() for q in slopes(st, pl)]


def bars_var(base, s, tr, sp):
    """Bars of (spot^2 = var X + var Y, var opl), mm^2, on the plane moved by s; base = start_pose(...)."""
    V0, Vs = base
    b = [2 * REL * tr["var"][k] + FLOOR * (np.sqrt(V0[k]) + abs(LD(s)) * np.sqrt(Vs[k])) ** 2 + (FLOOR * sp[0 if k < 2 else 1]) ** 2
         for k in range(3)]
    return b[0] + b[1], b[2]


def judge0(path, what, got, tr, sp):
    """(spot, duration) of one path at s = 0 against the truth."""
    for name, g, t, bar in zip(("spot", "duration"), got, (tr["spot"], tr["dur"]), bars0(tr, sp)):
        err = abs(LD(g) - t)
        print(f"{path:>10} {what}: {name} {float(g):.12e} truth {float(t):.12e} err/bar {float(err / bar):.2e}")
        note(path, err / bar)
        assert err <= bar, f"{path} {what}: {name} {float(g):.12e} against {float(t):.12e}: error {float(err):.3e}, bar {float(bar):.3e}"


def judge_var(path, what, got, tr, base, s, sp):
    """(spot, duration) of one path on the plane moved by s, judged on the variances; tr = truth(..., s, .)."""
    bxy, bo = bars_var(base, s, tr, sp)
    gxy, go = LD(got[0]) ** 2, (LD(got[1]) / FS) ** 2
    for name, g, t, bar in (("var XY", gxy, tr["var"][0] + tr["var"][1], bxy), ("var opl", go, tr["var"][2], bo)):
        err = abs(g - t)
        print(f"{path:>10} {what} s={s:g}: {name} {float(g):.12e} truth {float(t):.12e} err/bar {float(err / bar):.2e}")
        note(path + " s", err / bar)
        assert err <= bar, f"{path} {what} s={s:g}: {name} {float(g):.12e} against {float(t):.12e}: error {float(err):.3e}, bar {float(bar):.3e}"


# ------------------------------------------------------------------------------------------------------------- the scenes
def seeded_weights(n):
    """The seeded Gaussian weights of tests/test_gpu_focal.py's relay4 fixture (host tensor)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(7)
    return torch.exp(-0.5 * torch.randn(n, generator=g, dtype=torch.float64) ** 2)


def _set_weights(B):
    B.intensity = B.backend.from_numpy(seeded_weights(B.n_slots).numpy())
    B.touch()


def tight(angle, n=19999):
    """The parabola of test_autofocus_of_a_tight_focus (f = 100, round 15 mm support, plane wave of diameter 20) at a field
    angle of `angle` degrees; the detector near the focus, found once by the autofocus search."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    import ART.ModuleDetector as mdet
    SP = {"Divergence": 0, "SourceSize": 20, "Wavelength": 800e-6, "DeltaFT": 0.5, "NumberRays": n}
    ch = mp.OEPlacement(SP, [mmirror.MirrorParabolic(100, 0, msupp.SupportRound(15))], [300], [angle], Description="tight")
    last = ch.get_output_rays()[-1]
    det = mdet.Detector(np.asarray(ch.optical_elements[-1].position, float))
    det.autoplace(last, 100.0)
    D, _, _ = mp.FindOptimalDistance(det, last, "intensity", 2.0, 3, False, False)
    return {"chain": ch, "B": last, "det": D}


def relay4(n=20001):
    import ART.ModuleDetector as mdet
    from tools.bench import workloads
    ch, _ = workloads.build_scene(4, small_n=n)
    last = ch.get_output_rays()[-1]
    _set_weights(last)
    det = mdet.Detector(np.asarray(ch.optical_elements[-1].position, float))
    det.autoplace(last, 600.0)
    return {"chain": ch, "B": last, "det": det, "weighted": True}


def masked(n):
    """The masked twisted toroids with every 7th source slot dead; the eight data rows of every dead slot -- of the source
    before the trace, of the result after it -- hold NaN: the kernels promise to select them away."""
    import ART.ModuleDetector as mdet
    import tubes_common as tb
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    els, rays, det = tb.twisted(n, mask=True)
    src = RayBundle.from_arrays(*rays, np.arange(n), 0.5 + ((np.arange(n) * 0.6180339887498949) % 1.0), 50e-6)
    src.alive[6::7] = 0
    src.data[:, 6::7] = float("nan")
    src.touch()
    ch = OpticalChain(src, els)
    last = ch.get_output_rays()[-1]
    dead = last.alive == 0
    last.data[:, dead] = float("nan")
    last.touch()
    D = mdet.Detector(np.asarray(det[0], float), np.asarray(det[0], float), np.asarray(det[1], float))
    return {"chain": ch, "B": last, "det": D, "weighted": True}


def build_scenes():
    S = {"tight_2nm": tight(0.0005), "tight_180nm": tight(0.05), "relay4": relay4()}
    _set_weights(S["tight_2nm"]["B"])                  # tight_2nm carries relay4's weights
    S["tight_2nm"]["weighted"] = True
    for sc in S.values():
        sc["st"] = state_of(sc["B"])
        sc["poses"] = poses(sc["det"])
    return S


def poses(det):
    """name -> Detector: the scene's own, then manual ones with the centre moved IN the plane by 0, 1 and 100 mm along
    rot[0], 100 mm along the diagonal of rot[0] and rot[1], and one with the normal tilted by 5 degrees."""
    import ART.ModuleDetector as mdet
    pl = plane_of(det)
    C, n, ex, ey = pl["C"], pl["n"], pl["rot"][0], pl["rot"][1]
    mk = lambda c, nrm: mdet.Detector(np.array(det.refpoint, dtype=float), np.array(c, dtype=float), np.array(nrm, dtype=float))
    a = np.deg2rad(5.0)
    return {"auto": det, "off0": mk(C, n), "off1": mk(C + ex, n), "off100": mk(C + 100.0 * ex, n),
            "diag100": mk(C + 100.0 * (ex + ey) / np.sqrt(2.0), n), "tilt5": mk(C, np.cos(a) * n + np.sin(a) * ey)}


# ------------------------------------------------------------------------------------------------------------- the checks
def modes_of(sc):
    return (False, True) if sc.get("weighted") else (False,)


def reference_sd(det, B, weighted):
    """The reference's own algorithm: two-pass fp64 standard deviations of get_PointList2DCentre and get_Delays."""
    import ART.ModuleProcessing as mp
    P, dl = list(det.get_PointList2DCentre(B)), list(det.get_Delays(B))
    if weighted:
        w = list(B.intensities())
        return mp.WeightedStandardDeviation(P, w), mp.WeightedStandardDeviation(dl, w)
    return mp.StandardDeviation(P), mp.StandardDeviation(dl)


def check_per_ray(name, sc):
    """(e): X, Y, opl of Detector.readout on every pose, 1e-10 of span."""
    st, B = sc["st"], sc["B"]
    a = st["alive"]
    for pose, det in sc["poses"].items():
        pl = plane_of(det)
        sp = spans(st, pl)
        r = det.readout(B)
        X, Y, O, _ = readout(st, pl)
        for key, ref, span in (("X", X, sp[0]), ("Y", Y, sp[0]), ("opl", O, sp[1])):
            err = np.abs(ld(r[key].cpu().numpy()[a]) - ref).max()
            print(f"   per ray {name}/{pose}: {key} worst {float(err / (EPS * span)):.2f} ulp of span {float(span):.4g}")
            note("per-ray", err / (PARITY * span))
            assert err <= PARITY * span, (name, pose, key, float(err), float(span))


def fused_variances(s, weighted, centres):
    """(spot, duration) from the fused read-out's statistics (include/art_hip.h: 16..21 are second moments about
    `centres`), the way the examples form them: var = sum w (x - c)^2 / sum w - (mean - c)^2."""
    m0 = s[8] if weighted else s[0]
    sums = (s[9], s[10], s[11]) if weighted else (s[6], s[7], s[1])
    sq = s[19:22] if weighted else s[16:19]
    v = [max(sq[k] / m0 - (sums[k] / m0 - centres[k]) ** 2, 0.0) for k in range(3)]
    return float(np.sqrt(v[0] + v[1])), float(np.sqrt(v[2]) / 299792458000 * 1e15)


def check_at_the_detector(name, sc):
    """Paths (a) - (d) and the reference's algorithm at s = 0 on every pose."""
    import ART.ModuleAnalysisAndPlots as mplots
    import ART.ModuleDetector as mdet
    import ART.ModuleProcessing as mp
    from attosecondraytracing_amd import analysis
    st, B = sc["st"], sc["B"]
    be = B.backend
    for pose, det in sc["poses"].items():
        pl = plane_of(det)
        sp = spans(st, pl)
        what = f"{name}/{pose}"
        mom = det._scan_moments(B)
        ana = analysis.analyse([(B, "manual", det)])[0]
        # a first look for the centres of (d): the means of a statistics-only read-out
        s1 = det.readout(B, store=False)["stats"]
        c = (s1[6] / s1[0], s1[7] / s1[0], s1[1] / s1[0])
        s2 = be.detector_readout(det._desc(), B.view(), B.intensity, B.n_slots, c, None, None, None)
        # Detector.readout hands in the path centre only: X and Y stay about Detector.centre, so they are
        # judged where that centre lies inside the spot
        s3 = det.readout(B, store=False, path_centre=float(c[2]))["stats"]
        for weighted in modes_of(sc):
            tr = truth(st, pl, 0.0, weighted)
            tag = what + (" w" if weighted else "")
            judge0("reference", tag, reference_sd(det, B, weighted), tr, sp)
            judge0("(a) scan", tag, det._spot_duration_from_moments(mom, 0.0, weighted), tr, sp)
            judge0("(b) manual", tag, ana.spot_duration(0.0, weighted), tr, sp)
            judge0("(d) fused", tag, fused_variances(s2, weighted, c), tr, sp)
            got = fused_variances(s3, weighted, (0.0, 0.0, c[2]))
            if pose in ("auto", "off0", "tilt5"):
                judge0("(d) fused", tag + " readout()", got, tr, sp)
            else:
                judge0("(d) fused", tag + " readout() duration", (tr["spot"], got[1]), tr, sp)
        judge0("(c) summary", what, mplots.GetResultSummary(det.copy_detector(), B), truth(st, pl, 0.0, False), sp)
    # (b) auto-placing: the truth is taken on whatever plane results
    det = sc["poses"]["auto"]
    ana = analysis.analyse([(B, "autoplace", float(det.get_distance()))])[0]
    placed = mdet.Detector(np.zeros(3))
    placed._adopt(ana)
    pl = plane_of(placed)
    assert not ana.cxy.any()
    for weighted in modes_of(sc):
        judge0("(b) auto", name + (" w" if weighted else ""), ana.spot_duration(0.0, weighted), truth(st, pl, 0.0, weighted), spans(st, pl))
    # (d) from a trace with detector=: statistics formed by the tracing launch, the path centre from the first look
    s1 = det.readout(B, store=False)["stats"]
    co = float(s1[1] / s1[0])
    ch = sc["chain"]
    last = mp.RayTracingCalculation(ch.source_rays, ch.optical_elements, detector=det, path_centre=co)[-1]
    assert getattr(last, "_fused_readout", None) is not None
    s4 = det.readout(last, path_centre=co)["stats"]
    assert np.array_equal(last.alive.cpu().numpy() != 0, st["alive"])
    pl, sp = plane_of(det), spans(st, plane_of(det))
    judge0("(d) fused", name + " trace(detector=)", fused_variances(s4, False, (0.0, 0.0, co)), truth(st, pl, 0.0, False), sp)
    # ... and by a resident scene program (examples/pose_scan.py: path_centres = the aligned setup's mean path)
    from attosecondraytracing_amd.graph import SceneProgram
    last = SceneProgram([ch.source_rays], [ch.optical_elements], detectors=[det], path_centres=[co]).run()[0][-1]
    s5 = det.readout(last, path_centre=co)["stats"]
    assert getattr(last, "_fused_readout", None) is not None and np.array_equal(last.alive.cpu().numpy() != 0, st["alive"])
    judge0("(d) fused", name + " SceneProgram", fused_variances(s5, False, (0.0, 0.0, co)), truth(st, pl, 0.0, False), sp)


def check_shifted(name, sc):
    """BundleAnalysis.spot_duration(s, .) on every pose against the truth on the MOVED plane (no linear model on that side),
    and the reference's algorithm on the moved detector."""
    from attosecondraytracing_amd import analysis
    st, B = sc["st"], sc["B"]
    names = list(sc["poses"])
    anas = analysis.analyse([(B, "manual", sc["poses"][p]) for p in names])
    for pose, ana in zip(names, anas):
        det = sc["poses"][pose]
        pl = plane_of(det)
        sp = spans(st, pl)
        assert ana.linear_over(min(SHIFTS), max(SHIFTS)), (name, pose, ana.kink_below, ana.kink_above)
        for weighted in modes_of(sc):
            base = start_pose(st, pl, weighted)
            tag = f"{name}/{pose}" + (" w" if weighted else "")
            for s in SHIFTS:
                tr = truth(st, pl, s, weighted)
                judge_var("(b) manual", tag, ana.spot_duration(s, weighted), tr, base, s, sp)
                if s != 0.0:       # (s = 0: check_at_the_detector; the moved detector's fp64 centre is C - s n rounded)
                    here = det.copy_detector()
                    here.shiftByDistance(float(s))
                    judge_var("reference", tag, reference_sd(here, B, weighted), tr, base, s, sp)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_size(n):
    """The masked scene with n source slots: (a) and (b) on its tilted detector and on the same moved 100 mm in its plane;
    one alive ray: both results within the floor; two calls: the same bytes."""
    from attosecondraytracing_amd import analysis
    sc = masked(n)
    st, B = state_of(sc["B"]), sc["B"]
    count = int(st["alive"].sum())
    assert count >= 1 and (n < 7 or count < n)
    for v in (st["P"], st["D"], st["path"]):
        assert np.isnan(v[~st["alive"]]).all() and np.isfinite(v[st["alive"]]).all()
    ps = poses(sc["det"])
    for pose in ("off0", "off100"):
        det = ps[pose]
        pl = plane_of(det)
        sp = spans(st, pl)
        rows = [analysis.analyse([(B, "manual", det)])[0] for _ in range(2)]
        moms = [det._scan_moments(B) for _ in range(2)]
        assert same_bytes(rows[0].row, rows[1].row) and same_bytes(moms[0]["m"], moms[1]["m"]), (n, pose)
        assert rows[0].count == count
        for weighted in (False, True):
            tr = truth(st, pl, 0.0, weighted)
            tag = f"masked {n}/{pose}" + (" w" if weighted else "")
            if count == 1:
                assert tr["spot"] == 0 and tr["dur"] == 0
            judge0("(a) scan", tag, det._spot_duration_from_moments(moms[0], 0.0, weighted), tr, sp)
            judge0("(b) manual", tag, rows[0].spot_duration(0.0, weighted), tr, sp)
            judge0("reference", tag, reference_sd(det, B, weighted), tr, sp)


def check_batches(S):
    """One analyse call holding all poses of one bundle, an auto-placing job and a bundle of another size, and the same
    requests reversed: every row has the bytes of its single call."""
    from attosecondraytracing_amd import analysis
    a, b = S["tight_2nm"], S["relay4"]
    assert a["B"].n_slots != b["B"].n_slots
    reqs = [(a["B"], "manual", d) for d in a["poses"].values()] + [(a["B"], "autoplace", float(a["det"].get_distance()))]
    reqs += [(b["B"], "manual", b["poses"]["off100"]), (b["B"], "autoplace", 600.0)]
    single = [analysis.analyse([r])[0].row for r in reqs]
    together = [x.row for x in analysis.analyse(reqs)]
    backwards = [x.row for x in analysis.analyse(reqs[::-1])][::-1]
    for k, (s, t, r) in enumerate(zip(single, together, backwards)):
        assert same_bytes(s, t) and same_bytes(s, r), k

"""GPU (-m gpu): art_alignment_sums, OpticalChain.get_Compensation and OpticalChain.align -- every entry of the table
against the long-double sums of tests/alignment_common.py on the device's own traced histories, about the centres the
table reports; the detector alone against the autofocus quadratic; the shapes and edges of the kernels; consistency with
get_Sensitivities; and the KB alignment experiment end to end."""
import ctypes as C

import numpy as np
import pytest

import alignment_common as al
import sensitivity_common as sn
import tubes_common as tb
from test_gpu_sensitivity import _chain, _detector, _device_detector, _history, _reference

pytestmark = pytest.mark.gpu
NAMES = ["a_toroid", "c_kb", "d_twisted", "e_masked", "h_mixed8", "h_rotated_quadric"]
PITCH = sn.ELEMENT_DOFS.index("pitch")


@pytest.fixture(scope="module")
def hip():
    import torch
    import __graft_entry__
    from attosecondraytracing_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    __graft_entry__.ensure_built()
    _lib._BACKEND = None
    be = _lib.get_backend()
    assert be.name == "hip"
    return be


def dof_sets(K):
    """C = 1; C = 8 over the source, the first and the last element and the detector; an unsorted set; a set whose earliest
    group is the last element; the detector alone."""
    last = ["yaw", "roll", "shift_cross"]
    return {"one": [(K - 1, "pitch")],
            "eight": [("source", "tilt_y"), (0, "pitch"), al.DETECTOR, (K - 1, last[0]), ("source", "shift_x"),
                      (0, "shift_normal"), (K - 1, last[1]), (K - 1, last[2])],
            "unsorted": [(K - 1, "pitch"), ("source", "tilt_x"), (0, "yaw")],
            "last_first": [(K - 1, "roll"), (K - 1, "pitch")],
            "detector": [al.DETECTOR]}


def truth(chain, det, D, comp, ref):
    """The long-double table of comp's degrees of freedom about the centres comp's table reports, and the pilot's means."""
    K = len(chain.optical_elements)
    ids = [al.id_of(d, K) for d in comp.names]
    bundles = _history(chain)
    Dl = bundles[-1].data[3:6].cpu().numpy().T.copy()
    rot = np.array(list(D._desc().rot)).reshape(3, 3)
    w = bundles[-1].intensity
    w = np.ones(len(Dl)) if w is None else w.cpu().numpy()
    cols = al.columns(ref, ids, Dl, det, rot)
    centres = comp.table[al.CENTRES:al.MEANS].reshape(3, 8)[:, :len(ids)]
    return al.truth_table(ref, cols, w, centres), al.pilot_centres(ref, cols, w), cols


def check(chain, det, D, comp, ref, what):
    want, pilot, cols = truth(chain, det, D, comp, ref)
    Cn = len(comp.names)
    f = al.column_floor(cols, comp.names, ref["alive"], ref["span"])
    worst = al.compare_table(comp.table, want, Cn, what, ref["span"], f)
    got = comp.table[al.CENTRES:al.MEANS].reshape(3, 8)[:, :Cn]
    a = ref["alive"].copy()
    a[al.PILOT:] = False
    for q in range(3):
        for k in range(Cn):
            scale = np.abs(cols[q, k][a]).max() if a.any() else 0
            assert abs(got[q, k] - pilot[q, k]) <= tb.PARITY * scale + f[k], (what, "centre", q, k)
    return worst


@pytest.fixture(scope="module")
def runs(hip):
    """name -> (scene, chain, (centre, normal), Detector, {set: Compensation}, restatement), traced once."""
    S = sn.all_scenes()
    out = {}
    for name in NAMES:
        sc = S[name]
        chain = _chain(sc)
        det = _device_detector(chain, sc)
        D = _detector(det)
        comps = {k: chain.get_Compensation(D, dofs) for k, dofs in dof_sets(len(sc["els"])).items()}
        origin = comps["one"].origin
        assert all(np.array_equal(c.origin, origin) for c in comps.values())
        out[name] = (sc, chain, det, D, comps, _reference(chain, det, D, origin))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_table_against_the_long_double_sums(runs, name):
    sc, chain, det, D, comps, ref = runs[name]
    for key, comp in comps.items():
        worst = check(chain, det, D, comp, ref, f"{name} {key}")
        print(f"{name} {key}: {comp.count} rays, {len(comp.names)} degrees of freedom, worst deviation {worst:.2e}")
        assert comp.count == int(ref["alive"].sum())
    assert comps["eight"].names[2] == al.DETECTOR and len(comps["eight"].names) == 8
    if name == "e_masked":
        assert 100 < comps["one"].count < len(sc["rays"][0]) - 100


def test_detector_alone_is_the_autofocus_quadratic(runs):
    """sigma_X^2 + sigma_Y^2 of the detector shifted by s is a quadratic in s whose sums Detector._scan_moments forms; its
    minimiser against moves[0], to 1e-9 of the detector's distance from the last element."""
    for name in ("d_twisted", "a_toroid"):
        sc, chain, det, D, comps, ref = runs[name]
        last = chain.get_output_rays()[-1]
        mom = D._scan_moments(last)
        m = mom["m"][16:] if last.intensity is not None else mom["m"][:16]
        num = den = 0.0
        for k in range(2):
            q, sq, qq, qs, ss = m[1 + 5 * k: 6 + 5 * k]
            num += qs / m[0] - q * sq / m[0] ** 2
            den += ss / m[0] - (sq / m[0]) ** 2
        want = -num / den
        got = comps["detector"].moves[0]
        print(f"{name}: detector shift {got!r}, autofocus quadratic {want!r}")
        assert abs(got - want) <= 1e-9 * ref["span"][0], (name, got, want)
        assert comps["detector"].rank == 1 and comps["detector"].units == ["mm"]


# ------------------------------------------------------------------------------------------- the kernels' shapes and edges
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
SIZED_DOFS = [(2, "pitch"), ("source", "tilt_y"), al.DETECTOR, (0, "roll"), (0, "shift_normal")]   # (five: a spare column)
PAD, GUARD = 512, -7.25


def _sized_scene(n, extra=0):
    els, rays, det = tb.twisted(n, mask=True)
    if extra:
        more = tb.twisted(extra, mask=True)[1]
        rays = (np.concatenate([rays[0], more[0]]), np.concatenate([rays[1], more[1]]))
    n += extra
    return dict(els=els, rays=rays, det=det, w=0.5 + ((np.arange(n) * 0.6180339887498949) % 1.0))


@pytest.fixture(scope="module")
def sized(hip):
    """n -> (chain, det, Detector, Compensation, restatement): the masked twisted toroids with n source slots of which every
    7th is dead; 1300: 300 further rays behind 1000 (beyond the pilot's prefix); "dark": 1300 with the first 1024 dead."""
    out = {}
    for key in SIZES + [1300, "dark"]:
        if key == "dark":
            sc, dead = _sized_scene(1000, 300), slice(0, al.PILOT)
        else:
            sc, dead = (_sized_scene(1000, 300) if key == 1300 else _sized_scene(key)), slice(6, None, 7)
        chain = _chain(sc, dead=dead)
        D = _detector(sc["det"])
        comp = chain.get_Compensation(D, SIZED_DOFS)
        out[key] = (chain, sc["det"], D, comp, _reference(chain, sc["det"], D, comp.origin))
    return out


@pytest.mark.parametrize("n", SIZES + [1300])
def test_bundle_sizes_with_dead_source_slots(sized, n):
    chain, det, D, comp, ref = sized[n]
    dead = ~ref["alive"]
    assert not dead[0] and dead[6::7].all() and 0 < comp.count == int((~dead).sum())
    worst = check(chain, det, D, comp, ref, f"n = {n}")
    again = chain.get_Compensation(D, SIZED_DOFS)
    assert again.table.tobytes() == comp.table.tobytes(), n
    print(f"n = {n}: {comp.count} rays count, worst deviation {worst:.2e}")


def test_a_prefix_without_counted_rays_gives_zero_centres(sized):
    chain, det, D, comp, ref = sized["dark"]
    assert not ref["alive"][:al.PILOT].any() and comp.count == int(ref["alive"].sum()) > 100
    assert not comp.table[al.CENTRES:al.MEANS].any()
    worst = check(chain, det, D, comp, ref, "dark prefix")
    # uncentred sums still carry the covariances: the bar holds about centres of 0 at the scale of the raw second moments
    print(f"first {al.PILOT} slots dead: {comp.count} rays count, worst deviation {worst:.2e}")


def _made(chain, D, dofs, origin):
    from attosecondraytracing_amd import alignment
    from attosecondraytracing_amd.polarisation import history
    els = list(chain.optical_elements)
    return alignment._job((history(chain), els, D, alignment.dof_ids(dofs, len(els)), None), tuple(origin))


def test_no_slots_at_all(hip, sized):
    chain, det, D, comp, ref = sized[257]
    made = _made(chain, D, SIZED_DOFS, comp.origin)
    made[0].n = 0
    table = hip.alignment_sums(*[[m] for m in made]).cpu().numpy()
    assert table.shape == (1, al.DOUBLES) and not table.any()


def test_guard_bands_around_the_table_and_the_scratch(hip, sized):
    import torch
    from attosecondraytracing_amd import _abi
    for n in (1, 257, 1300):
        chain, det, D, comp, ref = sized[n]
        made = _made(chain, D, SIZED_DOFS, comp.origin)
        jh = (_abi.ArtAlignmentJob * 1)(made[0])
        jh[0].views, jh[0].elems = 8, C.addressof(made[2])
        ns = hip.fn["art_alignment_sums_scratch_doubles"](jh, 1)
        tiles = (n + 255) // 256
        assert ns == tiles * (8 + 3 * (12 + 21)) + 4 * 25          # six columns' sums per tile, the pilot's behind them
        key = ("alignment_sums", hip.stream_key())
        saved = hip._scratch.get(key)
        big = torch.full((ns + PAD,), GUARD, dtype=torch.float64, device=hip.device)
        out = torch.full((al.DOUBLES + 2 * PAD,), GUARD, dtype=torch.float64, device=hip.device)
        try:
            hip._scratch[key] = big
            table = hip.alignment_sums(*[[m] for m in made], out=out[PAD:PAD + al.DOUBLES].view(1, al.DOUBLES)).cpu().numpy()
        finally:
            hip._scratch[key] = saved
        assert (big[ns:] == GUARD).all() and (out[:PAD] == GUARD).all() and (out[-PAD:] == GUARD).all(), n
        assert not (table == GUARD).any() and table[0].tobytes() == comp.table.tobytes(), n


def test_a_ray_dead_in_a_middle_view_only_does_not_count(runs):
    import torch
    sc, chain, det, D, comps, ref = runs["e_masked"]
    out = chain.get_output_rays()
    mid = out[1]
    live = np.flatnonzero(ref["alive"])
    chosen = live[np.linspace(0, len(live) - 1, 50).astype(int)]
    assert len(set(chosen)) == 50 and len(set(chosen // 256)) > 1
    idx = torch.from_numpy(chosen).to(mid.alive.device)
    saved = mid.alive[idx].clone()
    dofs = dof_sets(3)["eight"]
    try:
        mid.alive[idx] = 0
        got = chain.get_Compensation(D, dofs)
        ref2 = _reference(chain, det, D, got.origin)
        assert (out[2].alive[idx] != 0).all() and (chain.source_rays.alive[idx] != 0).all()
    finally:
        mid.alive[idx] = saved
    assert got.count == comps["eight"].count - 50 == int(ref2["alive"].sum())
    worst = check(chain, det, D, got, ref2, "e_masked with 50 rays dead in the middle view")
    assert chain.get_Compensation(D, dofs).table.tobytes() == comps["eight"].table.tobytes()
    print(f"e_masked, 50 rays dead in the middle view only: {got.count} count, worst deviation {worst:.2e}")


def test_unequal_chains_in_one_call_equal_single_calls(runs, sized):
    """K = 3, 1, 8 and 2 with 1 to 8 degrees of freedom and 1 to 1300 slots, in two orders: every job runs in the kernel of
    its own width at its own stride of the scratch, whichever jobs share its call."""
    from attosecondraytracing_amd import alignment
    cases = [(runs[n][1], runs[n][3], dof_sets(len(runs[n][0]["els"]))[k], runs[n][4][k])
             for n, k in (("e_masked", "eight"), ("a_toroid", "one"), ("h_mixed8", "unsorted"), ("c_kb", "last_first"),
                          ("h_mixed8", "eight"), ("d_twisted", "detector"))]
    cases += [(sized[n][0], sized[n][2], SIZED_DOFS, sized[n][3]) for n in (257, 1, 1300)]
    for order in (list(range(len(cases))), [8, 2, 4, 0, 7, 3, 1, 6, 5]):
        res = alignment.compensations([(cases[k][0], dict(Detector=cases[k][1], DOFs=cases[k][2])) for k in order])
        for pos, k in enumerate(order):
            assert res[pos].table.tobytes() == cases[k][3].table.tobytes(), f"job {k} at place {pos} of {order}"


def test_more_requests_than_one_call_holds(sized):
    from attosecondraytracing_amd import alignment
    chain, det, D, comp, ref = sized[257]
    assert alignment.MAX_JOBS_PER_CALL == 64
    res = alignment.compensations([(chain, dict(Detector=D, DOFs=SIZED_DOFS))] * 65)
    assert len(res) == 65 and all(r.table.tobytes() == comp.table.tobytes() for r in res)


# --------------------------------------------------------------------------------------- consistency with what exists
def test_means_and_squares_agree_with_get_sensitivities_and_leave_it_alone(runs):
    for name in ("d_twisted", "h_mixed8"):
        sc, chain, det, D, comps, ref = runs[name]
        K = len(chain.optical_elements)
        before = chain.get_Sensitivities(D)
        comp = chain.get_Compensation(D, dof_sets(K)["eight"])
        after = chain.get_Sensitivities(D)
        assert before.table.tobytes() == after.table.tobytes(), name
        T, sw = before.table, before.table[0, 1]
        assert comp.sum_w == sw and comp.count == before.count
        for a, dof in enumerate(comp.names):
            if dof == al.DETECTOR:
                continue
            row = T[1 + al.id_of(dof, K)]
            for q in range(3):
                scale = np.sqrt(sw * row[6 + q])
                assert abs(comp.means[q, a] * sw - row[q]) <= 1e-9 * scale, (name, dof, q)
                square = sw * (comp.gram[q, a, a] + comp.means[q, a] ** 2)
                assert abs(square - row[6 + q]) <= 1e-9 * row[6 + q], (name, dof, q)


# ---------------------------------------------------------------------------------------------------------- end to end
APPLIED = np.array([2e-5, -3e-5])
PITCHES = [(0, "pitch"), (1, "pitch")]
SHIFTS = [(0, "shift_normal"), (1, "shift_normal")]


@pytest.fixture(scope="module")
def kb(hip):
    """The KB pair of c_kb with a detector at its focus, 500 mm along the chief ray, its normal against it; the chain with
    both pitches off; the nominal chain's own solve."""
    sc = sn.all_scenes()["c_kb"]
    chain = _chain(sc)
    last = _history(chain)[-1].data[0:6, 0].cpu().numpy()
    det = (last[0:3] + 500.0 * last[3:6], -last[3:6])
    D = _detector(det)
    off = chain.copy_chain()
    for k, v in enumerate(APPLIED):
        off.rotate_OE(k, "pitch", float(np.rad2deg(v)))
    return chain, off, D


@pytest.mark.parametrize("dofs, rank", [(PITCHES, 2), (PITCHES + SHIFTS, 2)])
def test_align_recovers_the_kb_pair(kb, dofs, rank):
    chain, off, D = kb
    nominal = chain.get_Compensation(D, dofs)
    before = off.get_Sensitivities(D).table.tobytes()
    start = off.get_Compensation(D, dofs)
    # Tolerance: X and Y are differences of fp64 numbers of the size of the 500 mm to the detector, known to 16 eps x 500 mm
    # = 1.8e-12 mm each, and the aligned spot is 1.5e-7 mm wide: its variance resolves relative changes of 1e-5 / sqrt(n),
    # 1e-6 with the 1000 rays.  Below that a re-trace cannot tell a step that helps from one that does not.
    aligned, det, report = off.align(D, dofs, Iterations=4, Tolerance=1e-6)
    print(f"nominal objective {nominal.objective:.3e}, misaligned {start.objective:.3e}, re-traced {report.objective}, "
          f"steps {report.step}, ranks {report.rank}, moves {report.moves[-1]}, singular values {start.singular_values}")
    assert off.get_Sensitivities(D).table.tobytes() == before      # (self is never changed)
    assert start.objective > 1e3 * nominal.objective
    assert 1 <= report.iterations <= 4 and min(report.objective) <= nominal.objective
    assert report.objective[-1] <= nominal.objective
    assert report.rejected == 0 and all(s == 1.0 for s in report.step[1:])
    assert start.rank == rank and all(r == rank for r in report.rank[1:])
    assert aligned is not off and report.names == start.names
    if dofs is PITCHES:
        err = np.abs(report.moves[-1] + APPLIED - nominal.moves)
        print(f"|moves + applied - nominal solve| {err}")
        assert (err <= 1e-3 * np.abs(APPLIED).max()).all(), err
    # the chain align returns holds the moves: its own re-trace gives the last objective
    again = aligned.get_Compensation(det, dofs)
    assert again.objective == report.objective[-1]

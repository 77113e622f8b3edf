"""GPU (-m gpu): art_polarisation against the mpmath truth of tests/coating_truth.py, on chains built through the
public API.  One plane mirror met by a fan of rays at every angle of the coating x angle matrix (tests/coating_cases.py)
for every coating of it, s and p inputs with PerRay=True; one job whose three mirrors carry three different coatings
with a mask between them; several jobs in one call; relay4 at 1e7 rays under the 256-layer coating.  Bars as on the
CPU (tests/test_coating_truth.py): 1e-14 absolute on the field of a unit input (so on rs, rp), widened within 1e-6 rad
of a lossless medium's critical angle by the rounding of cos t."""
import math

import numpy as np
import pytest

import coating_cases as cc
import coating_truth as ct
from conftest import report

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BAR = 1e-14


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


def _history(chain):
    """Directions of the source and of every bundle of the history [K + 1][n, 3], and the final alive bytes."""
    src, out = chain.source_rays, chain.get_output_rays()
    bundles = [src] + [out[k] for k in range(len(chain.optical_elements))]
    return [b.data[3:6].cpu().numpy().T.copy() for b in bundles], bundles[-1].alive.cpu().numpy().astype(bool)


def _field(pol):
    return pol.field.cpu().numpy().T          # [n, 3] complex


def _detector(chain):
    import ART.ModuleDetector as mdet
    last = chain.get_output_rays()[-1]
    D = mdet.Detector(np.asarray(chain.optical_elements[-1].position, dtype=float))
    D.autoplace(last, 300.0)
    d = D._desc()
    rot = np.array(d.rot[:]).reshape(3, 3)
    return D, (tuple(rot[0]), tuple(rot[1]), tuple(d.normal[:]))


# ------------------------------------------------------------------------------------------- one plane mirror, a fan
FAN_ANGLES = cc.angles(cc.COATINGS["lossless"][2])


def _fan(hip, n=1037):
    """One plane mirror facing -z at z = 100, plane of incidence x-z; ray i at FAN_ANGLES[i % A], mirrored in x every
    other round, hitting within 1 mm of the centre.  n = 1037: the last 256-slot tile holds 13 rays."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleSupport as msupp
    import ART.ModuleOpticalElement as moe
    from attosecondraytracing_amd.bundle import RayBundle
    from attosecondraytracing_amd.ModuleOpticalChain import OpticalChain
    rng = np.random.default_rng(21)
    A = len(FAN_ANGLES)
    j = np.arange(n) % A
    sign = np.where((np.arange(n) // A) % 2 == 0, 1.0, -1.0)
    s = np.array([FAN_ANGLES[q][1] for q in j]) * sign
    c = np.array([FAN_ANGLES[q][2] for q in j])
    vec = np.stack([s, np.zeros(n), c], axis=1)
    hit = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.full((n, 1), 100.0)], axis=1)
    src = RayBundle.from_arrays(hit - 10.0 * vec, vec, np.arange(n), np.ones(n), 13.5e-6, backend=hip)
    M = mmirror.MirrorPlane(msupp.SupportRectangle(40, 40))
    el = moe.OpticalElement(M, np.array([0.0, 0.0, 100.0]), np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0]))
    return OpticalChain(src, [el]), j


@pytest.fixture(scope="module")
def fan(hip):
    chain, j = _fan(hip)
    dirs, alive = _history(chain)
    assert alive.all()
    return chain, j, dirs


@pytest.mark.parametrize("name", list(cc.COATINGS))
def test_plane_mirror_fan(fan, name):
    chain, j, dirs = fan
    make, k, _ = cc.COATINGS[name]
    coat = make()
    wl = 2 * math.pi / k
    k = 2 * math.pi / wl                                  # (the job's wave number)
    pair = np.concatenate([dirs[0], dirs[1]], axis=1)
    rows, inv = np.unique(pair, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.array([np.nonzero(inv == r)[0][0] for r in range(len(rows))])
    bars = np.full(len(rows), BAR)
    if name == "lossless":
        for r in range(len(rows)):
            if FAN_ANGLES[j[first[r]]][3]:
                cm = ct.cos_incidence(rows[r, :3], rows[r, 3:])
                bars[r] += 4 * EPS * float(cm * cm * ct.drdc2(coat, cm, k))
    worst = {}
    for P in ((0, 1, 0), (1, 0, 0)):                      # s, p (the fallback-frame rays mix them)
        E = _field(chain.get_Polarisation(coat, Polarisation=P, Wavelength=wl, PerRay=True))
        want = np.array([[ct.to_complex(z) for z in ct.chain([rows[r, :3], rows[r, 3:]], [coat], k, P)["E"][0]]
                         for r in range(len(rows))])
        err = np.abs(E - want[inv]).max(axis=1)
        bad = np.nonzero(err > bars[inv])[0]
        assert len(bad) == 0, [(FAN_ANGLES[j[i]][0], float(err[i]), float(bars[inv[i]])) for i in bad[:8]]
        for i in range(len(err)):
            lab, _, cos_t, near = FAN_ANGLES[j[i]]
            reg = "critical" if near else ("grazing <= 3 mrad" if cos_t <= 3.01e-3 else "other")
            worst[reg] = max(worst.get(reg, 0.0), float(err[i] / bars[inv[i]]))
    report(f"[coating truth, plane mirror fan, {name}] worst |E - truth| / bar: " +
           "  ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------- chains with a mask
def _mixed(hip, n, twist=90.0):
    """Plane mirror at 3.5 mrad grazing, a mask with a hole that stops some rays, plane mirrors at 45 and 70 deg."""
    import ART.ModuleMirror as mmirror
    import ART.ModuleMask as mmask
    import ART.ModuleSupport as msupp
    import ART.ModuleProcessing as mp
    SP = {"Divergence": 2e-3, "SourceSize": 0, "Wavelength": 13.5e-6, "DeltaFT": 0.5, "NumberRays": n}
    Mask = mmask.Mask(msupp.SupportRoundHole(30, 0.9, 0, 0))
    M = mmirror.MirrorPlane(msupp.SupportRectangle(800, 60))
    return mp.OEPlacement(SP, [M, Mask, M, M], [400, 100, 100, 300], [89.8, 0, 45, 70], [0, 0, twist, 0], "mixed")


def _weights(b):
    return np.ones(b.n_slots) if b.intensity is None else b.intensity.cpu().numpy()


def _chain_truth(chain, coats, P, det=None):
    dirs, alive = _history(chain)
    idx = np.nonzero(alive)[0]
    last = chain.get_output_rays()[-1]
    w = _weights(last)[idx]
    res = ct.chain_many([[d[i] for d in dirs] for i in idx], coats, 2 * math.pi / last.wavelength, P, det, w)
    return idx, alive, w, res


def _check_job(pol, chain, coats, P, det, truth, tag):
    idx, alive, w, res = truth
    T = pol.throughput.cpu().numpy()                      # w_out = w T
    Tt = np.array([r[1] for r in res])
    assert np.all(T[~alive] == 0)
    eT = (np.abs(T[idx] - w * Tt) / w).max()
    assert eT <= 2 * BAR, (tag, eT)
    eE = 0.0
    if P is not None:
        E = _field(pol)
        Et = np.array([r[0][0] for r in res])
        eE = np.abs(E[idx] - Et).max()
        assert eE <= BAR, (tag, eE)
        assert np.all(E[~alive] == 0)
    m = len(idx)
    src = chain.source_rays
    assert pol.count == m
    assert pol.sum_w_source == pytest.approx(math.fsum(_weights(src)[src.alive.cpu().numpy().astype(bool)]), rel=1e-14)
    assert abs(pol.sum_w_out - math.fsum(w * Tt)) <= 2 * BAR * math.fsum(w)
    assert abs(pol.t_min - Tt.min()) <= 2 * BAR and abs(pol.t_max - Tt.max()) <= 2 * BAR
    eS = 0.0
    if det is not None:
        S = [math.fsum(r[2][q] for r in res) for q in range(5)]
        got = list(pol.stokes) + [pol.longitudinal_sum]
        eS = max(abs(g - s) for g, s in zip(got, S))
        assert eS <= 4 * BAR * math.fsum(w), (tag, got, S)
    return eT, eE, eS / max(m, 1)


def _three():
    return [cc.mosi(128), None, cc.six_materials(), cc.COATINGS["metal633"][0]()]


@pytest.fixture(scope="module")
def mixed(hip):
    chain = _mixed(hip, 600)
    _, alive = _history(chain)
    assert 0.3 * len(alive) < alive.sum() < len(alive)    # the mask stops some rays, most pass
    return chain


@pytest.mark.parametrize("P", [None, (0, 1, 0), (0, 0, 1), (0, 1 / math.sqrt(2), 1j / math.sqrt(2))])
def test_one_job_three_coatings(mixed, P):
    D, det = _detector(mixed)
    coats = _three()
    pol = mixed.get_Polarisation(coats, Polarisation=P, Detector=D, PerRay=P is not None)
    eT, eE, eS = _check_job(pol, mixed, coats, P, det, _chain_truth(mixed, coats, P, det), "three coatings")
    report(f"[coating truth, one job, 256 layers + 6 materials + metal, P={P}] worst |T - truth| {eT:.1e}  "
           f"|E - truth| {eE:.1e}  Stokes per ray {eS:.1e}")


def test_several_jobs_in_one_call(hip, mixed, fan):
    from attosecondraytracing_amd import polarisation as pmod
    other = _mixed(hip, 300, twist=-30.0)
    metal = cc.COATINGS["metal633"][0]()
    reqs = [(mixed, _three(), {"Polarisation": (0, 1, 0), "PerRay": True}),
            (other, [cc.gold(), None, cc.COATINGS["lossless"][0](), cc.mosi(40)], {"Polarisation": (1, 1j, 0),
                                                                                  "PerRay": True}),
            (fan[0], [cc.COATINGS["zero_thickness"][0]()], {"Polarisation": (0, 1, 0), "PerRay": True}),
            (other, [metal, None, cc.COATINGS["absorber_1mm"][0](), cc.six_materials()], {})]
    many = pmod.polarisations(reqs)
    worst = 0.0
    for p, (ch, coats, kw) in zip(many, reqs):
        single = ch.get_Polarisation(coats, **kw)
        assert np.array_equal(p.throughput.cpu().numpy(), single.throughput.cpu().numpy())
        assert p.sum_w_out == single.sum_w_out and p.t_min == single.t_min and p.t_max == single.t_max
        if p.field is not None:
            assert np.array_equal(p.field.cpu().numpy(), single.field.cpu().numpy())
        P = kw.get("Polarisation")
        eT, eE, _ = _check_job(p, ch, coats, P, None, _chain_truth(ch, coats, P), "batched")
        worst = max(worst, eT, eE)
    report(f"[coating truth, {len(reqs)} jobs in one call] worst |T, E - truth| {worst:.1e}; bytes as single calls")


# ------------------------------------------------------------------------------------------- a large job
def test_relay4_1e7_256_layers(hip):
    import torch
    from tools.bench import workloads
    chain, _ = workloads.build_scene(4, small_n=10 ** 7)
    coat = cc.mosi(128)
    pol = chain.get_Polarisation(coat)
    out = chain.get_output_rays()
    alive = out[-1].alive.cpu().numpy().astype(bool)
    n = len(alive)
    T = pol.throughput.cpu().numpy()
    live = np.nonzero(alive)[0]
    assert len(live) > n // 2 and live[-1] >= n - 256           # (the last tile holds live rays)
    pick = np.unique(np.concatenate([live[np.linspace(0, len(live) - 1, 1900).astype(np.int64)], live[-100:]]))
    k = 2 * math.pi / out[-1].wavelength
    sel = torch.from_numpy(pick).to(out[-1].data.device)
    dirs = [b.data[3:6][:, sel].cpu().numpy().T for b in [chain.source_rays] + [out[e] for e in range(4)]]
    res = ct.chain_many([[d[i] for d in dirs] for i in range(len(pick))], [coat] * 4, k)
    w = _weights(out[-1])
    err = np.abs(T[pick] / w[pick] - np.array([r[1] for r in res]))        # (T here is w_out = w T)
    assert err.max() <= 2 * BAR, err.max()
    assert pol.count == len(live) and np.all(T[~alive] == 0)
    ref = float(T[alive].astype(np.longdouble).sum())
    assert abs(pol.sum_w_out - ref) <= 1e-13 * ref
    Tk = T[alive] / w[alive]
    assert pol.t_min == pytest.approx(Tk.min(), rel=1e-15) and pol.t_max == pytest.approx(Tk.max(), rel=1e-15)
    report(f"[coating truth, relay4 1e7 x 256 layers] {len(pick)} slots: worst |T - truth| {err.max():.1e}; "
           f"sum w_out vs long double {abs(pol.sum_w_out - ref) / ref:.1e} rel")

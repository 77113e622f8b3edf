"""mpmath truth of art_polarisation at 40 significant digits: the coefficients rs, rp of a coating and
the 3x3 polarisation ray-tracing step along a chain.  TEST INFRASTRUCTURE (the judge of tests/test_coating_truth.py and
tests/test_gpu_coating_truth.py).

Inputs are the exact fp64 values a job holds -- the unit directions before and after each element, n and kappa of
every material, thicknesses, roughnesses and the wave number k -- and everything after them is done in mp:

  cos t = |b - a| / 2 (never 1 - sin^2 t), kz_j / k = sqrt(N_j^2 - 1 + cos^2 t) on the branch Im >= 0, vacuum kz / k = cos t;
  interfaces with the Nevot-Croce factor exp(-2 kz_a kz_b sigma^2); Parratt from the substrate up;
  s = normalize(a x b) (|a x b| < 1e-12: normalize(a x e), e the lab axis of a's smallest |component|, the first of
  equals), p_in = a x s, p_out = b x s;  E' = rs (E.s) s + rp (E.p_in) p_out (bilinear dot products).

A coating is anything with the fields of coating.Coating: is_ideal, substrate, layers [(N, thickness, roughness)],
roughness.  Results are mpc / mpf; `to_complex` rounds them."""
from mpmath import mp, mpc, mpf

DPS = 40


def _v(x):
    return [mpf(float(t)) for t in x]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(v):
    return mp.sqrt(sum(t * t for t in v))


def cos_incidence(a, b):
    """cos t = |b - a| / 2 of the reflection from direction a to b (fp64 triples), in mp."""
    with mp.workdps(DPS):
        a, b = _v(a), _v(b)
        return _norm([y - x for x, y in zip(a, b)]) / 2


def _mpN(N):
    N = complex(N)
    return mpc(mpf(N.real), mpf(N.imag))


def _kz(N, c):
    """kz / k of medium N at cos t = c, Im >= 0 (N = None: vacuum, kz / k = c)."""
    if N is None:
        return mpc(c, 0)
    q = mp.sqrt(N * N - 1 + c * c)
    return -q if q.imag < 0 else q


def rs_rp_at(coat, c, k):
    """(rs, rp) as mpc of `coat` at cos t = c (an mpf), wave number k (fp64, 1/mm)."""
    with mp.workdps(DPS):
        if coat.is_ideal:
            return mpc(-1), mpc(1)
        c = mpf(c)
        k = mpf(float(k))
        media = [None] + [_mpN(ly[0]) for ly in coat.layers] + [_mpN(coat.substrate)]
        thick = [None] + [mpf(float(ly[1])) for ly in coat.layers] + [None]
        sigma = [mpf(float(ly[2])) for ly in coat.layers] + [mpf(float(coat.roughness))]
        kzc, ifc, phc = {}, {}, {}

        def kz(j):
            key = None if media[j] is None else (media[j].real, media[j].imag)
            if key not in kzc:
                kzc[key] = _kz(media[j], c)
            return kzc[key]

        def eps(j):
            return mpc(1) if media[j] is None else media[j] * media[j]

        def interface(j):
            """r^s, r^p of the interface between media j and j + 1, with its roughness."""
            qa, qb = kz(j), kz(j + 1)
            key = (str(qa), str(qb), sigma[j])
            if key not in ifc:
                ea, eb = eps(j), eps(j + 1)
                rs = (qa - qb) / (qa + qb)
                rp = (eb * qa - ea * qb) / (eb * qa + ea * qb)
                if sigma[j] > 0:
                    f = mp.exp(-2 * qa * qb * (k * sigma[j]) ** 2)
                    rs, rp = rs * f, rp * f
                ifc[key] = (rs, rp)
            return ifc[key]

        L = len(coat.layers)
        Rs, Rp = interface(L)
        for j in range(L - 1, -1, -1):
            r_s, r_p = interface(j)
            key = (str(kz(j + 1)), thick[j + 1])
            if key not in phc:
                phc[key] = mp.exp(2j * kz(j + 1) * k * thick[j + 1])
            X = phc[key]
            Rs = (r_s + Rs * X) / (1 + r_s * Rs * X)
            Rp = (r_p + Rp * X) / (1 + r_p * Rp * X)
        return Rs, Rp


def rs_rp(coat, a, b, k):
    """One reflection: (rs, rp) as mpc of `coat` for the fp64 directions a (before) and b (after)."""
    return rs_rp_at(coat, cos_incidence(a, b), k)


def drdc2(coat, c, k, h=mpf("1e-24")):
    """max(|d rs / d c^2|, |d rp / d c^2|) at cos t = c, a central difference in mp (the conditioning of r in c^2)."""
    with mp.workdps(DPS):
        c2 = mpf(c) ** 2
        up = rs_rp_at(coat, mp.sqrt(c2 + h), k)
        dn = rs_rp_at(coat, mp.sqrt(c2 - h), k)
        return max(abs(up[0] - dn[0]), abs(up[1] - dn[1])) / (2 * h)


def _perp_unit(d, dm):
    """normalize(d x e), e the lab axis of d's smallest |component| (the first of equals); d fp64, dm its mp copy."""
    ax, ay, az = (abs(float(t)) for t in d)
    if ax <= ay and ax <= az:
        s = [mpf(0), dm[2], -dm[1]]
    elif ay <= az:
        s = [-dm[2], mpf(0), dm[0]]
    else:
        s = [dm[1], -dm[0], mpf(0)]
    m = _norm(s)
    return [t / m for t in s]


def frame(a, b):
    """s, p_in, p_out (mp 3-vectors) of the reflection from a to b (fp64 triples)."""
    with mp.workdps(DPS):
        am, bm = _v(a), _v(b)
        s = _cross(am, bm)
        m = _norm(s)
        s = _perp_unit(a, am) if m < mpf("1e-12") else [t / m for t in s]
        return s, _cross(am, s), _cross(bm, s)


def _dot(u, v):
    return sum(x * y for x, y in zip(u, v))


def reflect(Es, coat, a, b, k):
    """E' = rs (E.s) s + rp (E.p_in) p_out for one element, each E (3 mpc) of the list Es."""
    with mp.workdps(DPS):
        rs, rp = rs_rp(coat, a, b, k)
        s, pi, po = frame(a, b)
        out = []
        for E in Es:
            es, ep = rs * _dot(E, s), rp * _dot(E, pi)
            out.append([es * x + ep * y for x, y in zip(s, po)])
        return out


def input_states(d0, P=None):
    """The input field(s) at the source direction d0: [E0] for a polarised P (3 complex), else the two states
    u1 = perp_unit(d0), u2 = d0 x u1."""
    with mp.workdps(DPS):
        dm = _v(d0)
        if P is not None:
            Pm = [_mpN(p) for p in P]
            pd = _dot(Pm, dm)
            E = [p - pd * d for p, d in zip(Pm, dm)]
            m = mp.sqrt(sum(abs(t) ** 2 for t in E))
            return [[t / m for t in E]]
        u1 = _perp_unit(d0, dm)
        return [[mpc(t) for t in u1], [mpc(t) for t in _cross(dm, u1)]]


def chain(dirs, coats, k, P=None):
    """One ray through a chain: dirs = K + 1 fp64 directions (the source's, then after each element), coats = K
    coatings (None: a mask).  Returns {"E": the output field of each input state, "T": |E|^2 (the mean of the two
    states when unpolarised)}."""
    with mp.workdps(DPS):
        out = input_states(dirs[0], P)
        for e, c in enumerate(coats):
            if c is not None:
                out = reflect(out, c, dirs[e], dirs[e + 1], k)
        T = sum(sum(abs(t) ** 2 for t in E) for E in out) / len(out)
        return {"E": out, "T": T}


def stokes(Es, det, w=1.0):
    """[S0, S1, S2, S3, sum |E.nd|^2] of one ray's output state(s) with weight w (averaged over the states) in a
    detector's frame det = (e1, e2, nd): as art_polarisation's statistics row [5..9]."""
    with mp.workdps(DPS):
        e1, e2, nd = (_v(v) for v in det)
        acc = [mpf(0)] * 5
        ws = mpf(float(w)) / len(Es)
        for E in Es:
            x, y, z = _dot(E, e1), _dot(E, e2), _dot(E, nd)
            ix, iy = abs(x) ** 2, abs(y) ** 2
            xy = mp.conj(x) * y
            for q, v in enumerate((ix + iy, ix - iy, 2 * xy.real, 2 * xy.imag, abs(z) ** 2)):
                acc[q] += ws * v
        return acc


def to_complex(z):
    return complex(float(z.real), float(z.imag))


class Plain:
    """A coating's fields only (picklable, no package import): what the truth reads."""

    def __init__(self, c):
        self.is_ideal = bool(c.is_ideal)
        self.substrate = complex(c.substrate)
        self.layers = [(complex(N), float(t), float(s)) for N, t, s in c.layers]
        self.roughness = float(c.roughness)


def ray_job(args):
    """One ray of chain(), rounded for transport: (E of each state as complex triples, T, stokes row or None)."""
    dirs, coats, k, P, det, w = args
    r = chain(dirs, coats, k, P)
    st = None if det is None else [float(v) for v in stokes(r["E"], det, w)]
    return [[to_complex(z) for z in E] for E in r["E"]], float(r["T"]), st


def chain_many(rays, coats, k, P=None, det=None, w=None, workers=None):
    """chain() of many rays (rays[i] = the K + 1 directions of ray i): a list of ray_job's results.  The rays are
    shared among `workers` fresh Python processes (default: up to 16) that run this file on pickled job lists.
    w: per-ray weights for the Stokes sums (default 1)."""
    import os
    import pickle
    import subprocess
    import sys
    import tempfile
    coats = [None if c is None else Plain(c) for c in coats]
    jobs = [([tuple(float(t) for t in d) for d in dirs], coats, float(k), P, det, 1.0 if w is None else float(w[i]))
            for i, dirs in enumerate(rays)]
    workers = min(workers or min(16, os.cpu_count() or 1), max(1, len(jobs) // 8))
    if workers <= 1:
        return [ray_job(j) for j in jobs]
    with tempfile.TemporaryDirectory() as td:
        procs = []
        for q in range(workers):
            src, dst = os.path.join(td, "in%d" % q), os.path.join(td, "out%d" % q)
            with open(src, "wb") as f:
                pickle.dump(jobs[q::workers], f)
            procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__), src, dst]), dst))
        res = [None] * len(jobs)
        for q, (p, dst) in enumerate(procs):
            assert p.wait(timeout=3000) == 0, "a truth worker failed"
            with open(dst, "rb") as f:
                res[q::workers] = pickle.load(f)
    return res


if __name__ == "__main__":          # a worker of chain_many: ray_job over a pickled list
    import pickle
    import sys
    with open(sys.argv[1], "rb") as f:
        work = pickle.load(f)
    with open(sys.argv[2], "wb") as f:
        pickle.dump([ray_job(j) for j in work], f)

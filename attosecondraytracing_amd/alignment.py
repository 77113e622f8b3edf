"""Compensator solves on the device (art_hip.h, art_alignment_sums): OpticalChain.get_Compensation and OpticalChain.align.

get_Sensitivities answers the forward question of tolerancing: a mirror moves by u, the spot and the arrival time change
by so much.  The inverse question -- "the spot is aberrated; which moves of these few adjusters make it smallest, and how
small?" -- needs the products BETWEEN the columns of a handful of degrees of freedom, per ray:
    G_ab = Cov_w(dQ_a, dQ_b),  c_a = Cov_w(Q, dQ_a)        for Q = X, Y and the path L.
One pass over the history a traced chain already holds forms them (C <= 8 columns travel in one lane), and the solve
    minimise  sum_q Weights_q Var_w(Q + sum_a u_a dQ_a)   <=>   G u = -c,  G = sum_q Weights_q G_q,  c = sum_q Weights_q c_q
happens on the host by a truncated SVD.  `align` is Gauss-Newton on re-traces around it.

Degrees of freedom: those of sensitivity.py, ("source", "shift_x" ...), (k, "pitch" ...), and ("detector", "shift_normal"):
the detector shifted along its normal by Detector.shiftByDistance, in mm.

Limits: first order per iteration; the counted rays are those of the nominal trace; at most 8 degrees of freedom;
DeformedMirror, Grating and MirrorFreeform elements raise NotImplementedError; the objective is second moments, not
encircled energy or Strehl."""
import ctypes as C

import numpy as np

from . import _abi
from .sensitivity import ELEMENT_DOFS, SOURCE_DOFS, _FS_PER_MM

MAX_JOBS_PER_CALL = _abi.ART_TUBE_MAX_JOBS
MAX_DOFS = _abi.ART_ALIGN_MAX_DOFS
DETECTOR_DOFS = ("shift_normal",)


def dof_ids(DOFs, K):
    """The column ids of a list of (who, name) for a chain of K elements; ValueError for what the list may not hold."""
    DOFs = list(DOFs)
    if not 1 <= len(DOFs) <= MAX_DOFS:
        raise ValueError(f"DOFs must name 1..{MAX_DOFS} degrees of freedom")
    ids = []
    for item in DOFs:
        try:
            who, name = item
        except (TypeError, ValueError):
            raise ValueError(f"a degree of freedom is (who, name), not {item!r}") from None
        if isinstance(who, str) and who == "source" and name in SOURCE_DOFS:
            ids.append(SOURCE_DOFS.index(name))
        elif isinstance(who, str) and who == "detector" and name in DETECTOR_DOFS:
            ids.append(_abi.ART_ALIGN_DOF_DETECTOR)
        elif isinstance(who, (int, np.integer)) and not isinstance(who, bool) and -K <= who < K and name in ELEMENT_DOFS:
            ids.append(_abi.ART_SENS_COLS * (int(who) % K + 1) + ELEMENT_DOFS.index(name))
        else:
            raise ValueError(f"unknown degree of freedom {item!r}: (\"source\", one of {SOURCE_DOFS}), (element index, one of "
                             f"{ELEMENT_DOFS}) or (\"detector\", \"shift_normal\")")
    if len(set(ids)) != len(ids):
        raise ValueError("DOFs names a degree of freedom twice (duplicate)")
    return ids


def canonical(DOFs, K):
    """DOFs with element indices counted from the front."""
    return [(int(who) % K if not isinstance(who, str) else who, name) for who, name in DOFs]


def pair_index(a, b):
    """The place of sum w d'Q_a d'Q_b (a <= b) among the 36 pairs of one coordinate of the table."""
    a, b = min(a, b), max(a, b)
    return a * (2 * MAX_DOFS + 1 - a) // 2 + (b - a)


def unpack(table, n_dofs):
    """The [ART_ALIGN_DOUBLES] block of art_alignment_sums as count, sum_w, and about the origin the mean [3] and variance
    [3] of X, Y, L; the true means [3, C] of the columns, gram [3, C, C] = Cov_w(dQ_a, dQ_b) and rhs [3, C] =
    Cov_w(Q, dQ_a)."""
    t = np.asarray(table, dtype=float)
    if t.shape != (_abi.ART_ALIGN_DOUBLES,):
        raise ValueError(f"an alignment table has {_abi.ART_ALIGN_DOUBLES} entries")
    Cn = int(n_dofs)
    count, sw = int(t[0]), float(t[1])
    s = sw if sw > 0 else np.nan
    m = t[2:5] / s
    var = t[5:8] / s - m * m
    block = lambda at: t[at:at + 3 * MAX_DOFS].reshape(3, MAX_DOFS)[:, :Cn]
    centres, lin, cross = block(_abi.ART_ALIGN_CENTRES), block(_abi.ART_ALIGN_MEANS) / s, block(_abi.ART_ALIGN_CROSS) / s
    pairs = t[_abi.ART_ALIGN_PAIRS:_abi.ART_ALIGN_PAIRS + 3 * 36].reshape(3, 36) / s
    gram = np.empty((3, Cn, Cn))
    for a in range(Cn):
        for b in range(Cn):
            gram[:, a, b] = pairs[:, pair_index(a, b)] - lin[:, a] * lin[:, b]
    return dict(count=count, sum_w=sw, mean=m, variance=var, means=centres + lin, gram=gram, rhs=cross - m[:, None] * lin)


class Compensation:
    """What solve returns.  moves [C]: the moves of `names` (units[c]: "mm" or "rad") that minimise the objective;
    singular_values of the solved matrix (largest first) and the `rank` kept above Rcond x the largest; variance [3]: the
    variances of X, Y (mm^2) and the path (mm^2) before, variance_predicted [3] after the moves, to first order;
    objective = Weights . variance and objective_predicted; centroid_shift [2] (mm) and delay_shift (fs): what the moves do
    to the centroid and the arrival time; gram [3, C, C], rhs [3, C], means [3, C], count, sum_w: the sums they come from."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def apply(self, chain, Detector, moves=None):
        """Performs `moves` (default self.moves) on a COPY of the chain and of the detector -- shift_OE, rotate_OE (degrees),
        shift_source, tilt_source (degrees) and shiftByDistance -- and returns both."""
        u = self.moves if moves is None else np.asarray(moves, dtype=float)
        new = chain.copy_chain()                              # (its own copies of the elements and of the source)
        det = Detector.copy_detector()
        for (who, name), v in zip(self.names, u):
            v = float(v)
            if who == "source":
                axis = np.eye(3)[SOURCE_DOFS.index(name) % 3]
                if name.startswith("shift"):
                    new.shift_source(axis, v)
                else:
                    new.tilt_source(axis, float(np.rad2deg(v)))
            elif who == "detector":
                det.shiftByDistance(v)
            elif name.startswith("shift"):
                new.shift_OE(who, name[6:], v)
            else:
                new.rotate_OE(who, name, float(np.rad2deg(v)))
        return new, det


def _weights(Weights, Rcond):
    alpha = np.asarray(Weights, dtype=float)
    if alpha.shape != (3,) or not np.isfinite(alpha).all() or (alpha < 0).any() or not alpha.any():
        raise ValueError("Weights are three non-negative numbers, not all zero: of the variances of X, Y and the path")
    if not 0 <= float(Rcond) < 1:
        raise ValueError("Rcond must be in [0, 1)")
    return alpha


def solve(table, names, Weights=(1, 1, 0), Rcond=1e-9, HoldCentroid=False):
    """The compensator solve on one block of art_alignment_sums (pure NumPy, no device).  names: the degrees of freedom of
    the block's columns, in order.  Weights: of the variances of X, Y and L in the objective, (0, 0, 1) minimises the path
    spread, i.e. the duration.  G u = -c is solved by an SVD truncated at Rcond x the largest singular value; with
    HoldCentroid the solve is restricted to the moves that leave the centroid where it is (the null space of the two rows
    mean dX, mean dY)."""
    names = [tuple(n) for n in names]
    Cn = len(names)
    if not 1 <= Cn <= MAX_DOFS:
        raise ValueError(f"names must hold 1..{MAX_DOFS} degrees of freedom")
    alpha = _weights(Weights, Rcond)
    p = unpack(table, Cn)
    G = np.einsum("q,qab->ab", alpha, p["gram"])
    c = alpha @ p["rhs"]
    basis = np.eye(Cn)
    if HoldCentroid and np.isfinite(p["means"]).all():
        A = p["means"][0:2]
        _, sv, Vt = np.linalg.svd(A)
        held = int((sv > 1e-12 * sv[0]).sum()) if sv.size and sv[0] > 0 else 0
        basis = Vt[held:].T                                   # [C, C - held]: an orthonormal basis of the null space
    u = np.zeros(Cn)
    sing, rank = np.zeros(0), 0
    if basis.shape[1] and np.isfinite(G).all() and np.isfinite(c).all():      # (no counted ray: nothing to solve)
        Gr, cr = basis.T @ G @ basis, basis.T @ c
        U, sing, Vt = np.linalg.svd(Gr)
        rank = int((sing > float(Rcond) * sing[0]).sum()) if sing[0] > 0 else 0
        y = -(Vt[:rank].T @ ((U[:, :rank].T @ cr) / sing[:rank]))
        u = basis @ y
    predicted = p["variance"] + 2.0 * (p["rhs"] @ u) + np.einsum("a,qab,b->q", u, p["gram"], u)
    units = ["mm" if n[1].startswith("shift") else "rad" for n in names]
    return Compensation(moves=u, names=names, units=units, singular_values=sing, rank=rank, variance=p["variance"],
                        variance_predicted=predicted, objective=float(alpha @ p["variance"]),
                        objective_predicted=float(alpha @ predicted), centroid_shift=p["means"][0:2] @ u,
                        delay_shift=float(p["means"][2] @ u) * _FS_PER_MM, gram=p["gram"], rhs=p["rhs"], means=p["means"],
                        count=p["count"], sum_w=p["sum_w"], weights=alpha, table=np.asarray(table, dtype=float))


_KEYS = {"Detector", "DOFs", "Weights", "Rcond", "HoldCentroid"}


def compensations(requests):
    """requests: [(chain, kwargs)], kwargs those of OpticalChain.get_Compensation.  One Compensation per request, in order;
    all chains of one backend go to the device in ONE enqueue sequence of art_alignment_sums (blocks of MAX_JOBS_PER_CALL),
    and the one copy back to the host per call is the table.  The origins come from the detector's read-out statistics of
    the final bundle, as for sensitivity.sensitivities."""
    from .polarisation import history
    from .tubes import _refuse
    items = []
    for chain, kw in requests:
        kw = dict(kw or {})
        unknown = set(kw) - _KEYS
        if unknown:
            raise TypeError(f"unknown arguments {sorted(unknown)}")
        det = kw.get("Detector")
        if det is None:
            raise TypeError("a compensation needs a Detector")
        det._iscomplete()
        els = list(chain.optical_elements)
        if not 1 <= len(els) <= _abi.ART_TUBE_MAX_ELEMS:
            raise ValueError(f"a chain needs 1..{_abi.ART_TUBE_MAX_ELEMS} optical elements")
        if kw.get("DOFs") is None:
            raise ValueError("DOFs must name 1..8 degrees of freedom")
        ids = dof_ids(kw["DOFs"], len(els))
        _weights(kw.get("Weights", (1, 1, 0)), kw.get("Rcond", 1e-9))   # (argument errors come before the history is touched)
        for k, oe in enumerate(els):
            _refuse(k, oe)
        items.append((chain, els, det, ids, kw))
    items = [(history(chain), els, det, ids, kw) for chain, els, det, ids, kw in items]
    stats = [det.readout(bundles[-1], sync=False, store=False) for bundles, _, det, _, _ in items]
    origins = []
    for st in stats:
        s = st["stats"] if "stats" in st else st["stats_dev"].cpu().numpy()
        origins.append(tuple(float(v) / float(s[8]) for v in s[9:12]) if s[8] > 0 and np.isfinite(s[8:12]).all()
                       else (0.0, 0.0, 0.0))
    groups = {}
    for pos, it in enumerate(items):
        groups.setdefault(id(it[0][-1].backend), []).append(pos)
    results = [None] * len(items)
    for positions in groups.values():
        be = items[positions[0]][0][-1].backend
        for lo in range(0, len(positions), MAX_JOBS_PER_CALL):
            part = positions[lo:lo + MAX_JOBS_PER_CALL]
            made = [_job(items[pos], origins[pos]) for pos in part]
            rows = be.alignment_sums(*[[m[q] for m in made] for q in range(4)]).cpu().numpy()
            for k, pos in enumerate(part):
                _, els, _, _, kw = items[pos]
                res = solve(rows[k].copy(), canonical(kw["DOFs"], len(els)), kw.get("Weights", (1, 1, 0)),
                            kw.get("Rcond", 1e-9), bool(kw.get("HoldCentroid", False)))
                res.origin = np.asarray(origins[pos], dtype=float)
                results[pos] = res
    return results


def _job(item, origin):
    from . import ModuleProcessing as mp
    bundles, els, det, ids, _ = item
    last = bundles[-1]
    be, n = last.backend, last.n_slots
    K = len(els)
    descs = [mp.element_descriptor(oe, True, be)[0] for oe in els]
    elems = (_abi.ArtElementDesc * K)()
    for k, d in enumerate(descs):
        C.memmove(C.addressof(elems[k]), C.addressof(d), C.sizeof(_abi.ArtElementDesc))
    quadrics = None
    if any(d.flags & _abi.ART_FLAG_QUADRIC for d in descs):
        quadrics = (_abi.ArtQuadricDesc * K)()
        for k, d in enumerate(descs):
            if d.flags & _abi.ART_FLAG_QUADRIC:
                quadrics[k] = be._quadric_desc(d.quadric._quadric_coefficients())
    j = _abi.ArtAlignmentJob()
    j.n_elems, j.n, j.n_dofs = K, n, len(ids)
    j.dofs[:len(ids)] = ids
    j.det = det._desc()
    j.origin[:] = origin
    j.w = None if last.intensity is None else last.intensity.data_ptr()
    views = (_abi.ArtBundleView * (K + 1))(*[b.view() for b in bundles])
    return j, views, elems, quadrics


def compensation(chain, Detector, DOFs, Weights=(1, 1, 0), Rcond=1e-9, HoldCentroid=False):
    """OpticalChain.get_Compensation (see the module's docstring)."""
    return compensations([(chain, dict(Detector=Detector, DOFs=DOFs, Weights=Weights, Rcond=Rcond,
                                       HoldCentroid=HoldCentroid))])[0]


class AlignmentReport:
    """What align returns beside the chain and the detector.  names, units: the degrees of freedom; per accepted iteration
    (entry 0: the chain as given) objective and variance [3] of the RE-TRACED chain, step (1: the full Gauss-Newton step;
    0.5 ...: halved), moves [C] cumulative, rank of the solve that led there, predicted: what that solve expected;
    rejected: the trial steps whose re-traced objective grew; converged: the relative decrease fell below Tolerance."""

    def __init__(self, names, units):
        self.names, self.units = names, units
        self.objective, self.variance, self.step, self.moves, self.rank, self.predicted = [], [], [], [], [], []
        self.rejected, self.converged, self.last = 0, False, None

    @property
    def iterations(self):
        return len(self.objective) - 1


def align(chain, Detector, DOFs, Weights=(1, 1, 0), Iterations=5, Tolerance=1e-9, Rcond=1e-9, HoldCentroid=False):
    """OpticalChain.align: Gauss-Newton on re-traces.  Each iteration solves (get_Compensation), applies the moves to a
    copy and re-traces; a step is accepted only if the re-traced objective does not grow, otherwise it is halved, at most
    4 times; the loop stops when the relative decrease falls below Tolerance.  Returns (chain, detector, AlignmentReport);
    the chain and the detector passed in are never changed."""
    if not (isinstance(Iterations, (int, np.integer)) and Iterations >= 1):
        raise ValueError("Iterations must be a positive integer")
    if not float(Tolerance) >= 0:
        raise ValueError("Tolerance must be non-negative")
    kw = dict(DOFs=list(DOFs), Weights=Weights, Rcond=Rcond, HoldCentroid=HoldCentroid)
    cur_chain, cur_det = chain.copy_chain(), Detector.copy_detector()
    comp = compensation(cur_chain, cur_det, **kw)
    report = AlignmentReport(comp.names, comp.units)
    total = np.zeros(len(comp.names))

    def record(c, step, rank, predicted):
        report.objective.append(c.objective)
        report.variance.append(c.variance.copy())
        report.step.append(step)
        report.moves.append(total.copy())
        report.rank.append(rank)
        report.predicted.append(predicted)

    record(comp, 0.0, 0, comp.objective)
    for _ in range(int(Iterations)):
        if comp.objective > 0 and comp.objective - comp.objective_predicted < float(Tolerance) * comp.objective:
            report.converged = True                           # (the solve itself expects less than Tolerance: no re-trace)
            break
        step, trial = 1.0, None
        for _ in range(5):
            t_chain, t_det = comp.apply(cur_chain, cur_det, step * comp.moves)
            trial = compensation(t_chain, t_det, **kw)
            if trial.objective <= comp.objective:
                break
            report.rejected += 1
            trial, step = None, step / 2
        if trial is None:
            break
        decrease = (comp.objective - trial.objective) / comp.objective if comp.objective > 0 else 0.0
        total = total + step * comp.moves
        record(trial, step, comp.rank, comp.objective_predicted if step == 1.0 else float("nan"))
        cur_chain, cur_det, comp = t_chain, t_det, trial
        if decrease < float(Tolerance):
            report.converged = True
            break
    report.last = comp
    return cur_chain, cur_det, report

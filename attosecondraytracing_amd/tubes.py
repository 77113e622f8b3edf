"""Ray tubes on the device (art_hip.h, art_ray_tubes): OpticalChain.get_RayTubes.

Differential ("generalised") ray tracing: one streaming pass over a traced chain's history carries, beside every ray, the
first-order change of its point and direction with respect to two source parameters through every surface (DESIGN.md 3,
csrc/art_tubes.h).  Three things come out of that one quantity, per ray and exactly instead of from a histogram or a fit:

  solid_angle   dOmega' / dmu, the image-space solid angle per unit source measure mu (steradians for a point source, mm^2
                for a plane wave).  The focal sums (get_FocalField and its kin) weigh every ray as sqrt(intensity) and so
                assume equal solid angle per ray, which holds in OBJECT space; `rays`, an alias of the final bundle whose
                intensity carries |solid_angle| (total power kept), hands them the image-space apodisation instead.
  curvature     the two principal wavefront curvatures behind the last element (1 / mm, negative = converging), their
                focal lines foci = -1 / curvature along the ray, and the direction of the first: the tangential and
                sagittal foci of a toroid per ray, Coddington's equations on the chief ray.
  area          the tube's cross-section on the detector (or at the last hit point) per unit mu: irradiance = w / |area|.

Limits: no DeformedMirror, Grating or MirrorFreeform elements (NotImplementedError); first order only; at a caustic the
curvatures, foci and axis are +-inf or NaN (nothing is clamped; solid_angle is always finite); the re-weighting is the
scalar Debye factor and does not replace the polarisation pass -- for both, multiply: w_eff = throughput * |solid_angle|,
i.e. rays.intensity = chain.get_Polarisation(...).throughput * chain.get_RayTubes().solid_angle.abs()."""
import ctypes as C
import math

from . import _abi
from .polarisation import history

MAX_JOBS_PER_CALL = _abi.ART_TUBE_MAX_JOBS
_SEEDS = {"point": _abi.ART_TUBE_POINT, "plane": _abi.ART_TUBE_PLANE}


class RayTubes:
    """What get_RayTubes returns.  count: rays alive in every bundle of the history; sum_w, sum_weight: sum w and
    sum w |solid_angle| over them; magnification = sum_weight / sum_w; solid_angle_min, solid_angle_max: the range of
    |solid_angle|; sum_area: sum w |area|; mean_curvature: the w-weighted means (kappa1, kappa2) over the finite_count
    rays where both are finite; asymmetry: max |C12 - C21| / (|kappa1| + |kappa2|) over them (Malus-Dupin: rounding);
    weight: DEVICE [n] w |solid_angle| (0 for the rays that do not count); rays: an alias of the final bundle with
    intensity = weight * sum_w / sum_weight; with PerRay: DEVICE solid_angle [n], area [n], curvature [2, n], axis [3, n]
    (NaN for the rays that do not count), foci = -1 / curvature, irradiance = w / |area| and chief, the values of slot 0 (a
    Vogel source's central ray); without: None."""

    def __init__(self, row, weight, rays, per_ray, w):
        self.count = int(row[0])
        self.sum_w, self.sum_weight = float(row[1]), float(row[2])
        self.magnification = self.sum_weight / self.sum_w if self.sum_w > 0 else math.nan
        self.solid_angle_min, self.solid_angle_max = float(row[3]), float(row[4])
        self.sum_area = float(row[5])
        self.mean_curvature = (float(row[6]), float(row[7]))
        self.finite_count = int(row[9])
        self.asymmetry = float(row[10])
        self.weight, self.rays, self._w = weight, rays, w
        self.solid_angle = self.area = self.curvature = self.axis = None
        if per_ray is not None:
            self.solid_angle, self.area, self.curvature, self.axis = per_ray

    @property
    def foci(self):
        return None if self.curvature is None else -1.0 / self.curvature

    @property
    def irradiance(self):
        if self.area is None:
            return None
        inv = 1.0 / self.area.abs()
        return inv if self._w is None else self._w * inv

    @property
    def chief(self):
        if self.solid_angle is None or self.solid_angle.numel() == 0:
            return None
        k = self.curvature[:, 0].cpu().numpy()
        return {"solid_angle": float(self.solid_angle[0]), "area": float(self.area[0]), "curvature": (float(k[0]), float(k[1])),
                "foci": (-1.0 / k[0] if k[0] != 0 else math.inf, -1.0 / k[1] if k[1] != 0 else math.inf),
                "axis": tuple(float(v) for v in self.axis[:, 0].cpu().numpy())}


def _refuse(k, oe):
    optic = oe.type
    name = type(optic).__name__
    if hasattr(optic, "lines_per_mm"):
        raise NotImplementedError(f"ray tubes: element {k} ({name}) is a grating")
    if hasattr(optic, "_freeform_figure"):
        raise NotImplementedError(f"ray tubes: element {k} ({name}) is a freeform: its Hessian needs the second "
                                  "derivatives of the figure")
    if len(getattr(optic, "DeformationList", ())) > 0:
        raise NotImplementedError(f"ray tubes: element {k} ({name}) has defects")


def _seed(chain, Source):
    if Source is None:
        Source = getattr(chain.source_rays, "source_kind", None)
        if Source is None:
            raise ValueError("the source bundle does not say whether it is a point source or a plane wave: "
                             "pass Source='point' or Source='plane'")
    if Source not in _SEEDS:
        raise ValueError("Source must be 'point', 'plane' or None")
    return _SEEDS[Source]


def ray_tubes(requests):
    """requests: [(chain, kwargs)], kwargs those of OpticalChain.get_RayTubes.  One RayTubes per request, in order; all
    chains of one backend go to the device in ONE call of art_ray_tubes (blocks of MAX_JOBS_PER_CALL), and the one copy
    back to the host is the table of sums."""
    items = []
    for chain, kw in requests:
        kw = dict(kw or {})
        unknown = set(kw) - {"Detector", "Source", "PerRay"}
        if unknown:
            raise TypeError(f"unknown arguments {sorted(unknown)}")
        els = list(chain.optical_elements)
        if not 1 <= len(els) <= _abi.ART_TUBE_MAX_ELEMS:
            raise ValueError(f"a chain needs 1..{_abi.ART_TUBE_MAX_ELEMS} optical elements")
        for k, oe in enumerate(els):
            _refuse(k, oe)
        seed = _seed(chain, kw.get("Source"))
        det = kw.get("Detector")
        if det is not None:
            det._iscomplete()
        items.append((history(chain), els, seed, det, bool(kw.get("PerRay", True))))
    groups = {}
    for pos, it in enumerate(items):
        groups.setdefault(id(it[0][-1].backend), []).append(pos)
    results = [None] * len(items)
    for positions in groups.values():
        be = items[positions[0]][0][-1].backend
        for lo in range(0, len(positions), MAX_JOBS_PER_CALL):
            part = positions[lo:lo + MAX_JOBS_PER_CALL]
            made = [_job(items[pos]) for pos in part]
            rows_dev = be.ray_tubes(*[[m[q] for m in made] for q in range(4)])
            rows = rows_dev.cpu().numpy()
            for k, pos in enumerate(part):
                last = items[pos][0][-1]
                weight, per_ray = made[k][4]
                rays = last.alias()
                # total power kept, apodisation changed: formed on the device from the device's own sums
                rays.intensity = weight * (rows_dev[k, 1] / rows_dev[k, 2]) if rows[k][2] > 0 else weight
                rays.touch()                       # (new weights: drop what was cached for the original ones)
                results[pos] = RayTubes(rows[k], weight, rays, per_ray, last.intensity)
    return results


def _job(item):
    from . import ModuleProcessing as mp
    bundles, els, seed, det, per_ray = item
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
    j = _abi.ArtTubeJob()
    j.n_elems, j.seed, j.n = K, seed, n
    if det is not None:
        j.has_detector = 1
        j.det = det._desc()
    j.w = None if last.intensity is None else last.intensity.data_ptr()
    weight = be.empty(max(n, 1))[:n]
    j.weight = weight.data_ptr()
    arrays = None
    if per_ray:
        buf = be.empty(7 * max(n, 1))
        rows = [buf[q * n:(q + 1) * n] for q in range(7)]
        j.solid_angle, j.area, j.kappa1, j.kappa2, j.axis = (rows[q].data_ptr() for q in (0, 1, 2, 3, 4))
        arrays = (rows[0], rows[1], buf[2 * n:4 * n].reshape(2, n), buf[4 * n:7 * n].reshape(3, n))
    views = (_abi.ArtBundleView * (K + 1))(*[b.view() for b in bundles])
    return j, views, elems, quadrics, (weight, arrays)


def tubes(chain, Detector=None, Source=None, PerRay=True):
    """OpticalChain.get_RayTubes (see the module's docstring)."""
    return ray_tubes([(chain, dict(Detector=Detector, Source=Source, PerRay=PerRay))])[0]

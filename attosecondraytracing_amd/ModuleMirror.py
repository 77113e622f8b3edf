"""Mirror surfaces, API of ART/ModuleMirror.py.

The classes are parameter holders for the HIP kernels: each exposes `_abi_kind` / `_abi_params()` (layout in
include/art_hip.h) plus the reference's host-side helpers `get_centre()` and `get_normal(Point)` for a single
point.  Ray/surface intersection, aperture test and reflection of a *bundle* never run in Python; see
ModuleProcessing.RayTracingCalculation -> libart_hip.so.  `get_grid3D` samples the surface for the 3-D render
(host, a few thousand points)."""
import math

import numpy as np

from . import _abi
from . import ModuleGeometry as mgeo


def _IntersectionRayMirror(PointMirror, ListPointIntersectionMirror):
    """Two candidate points -> the one closer to PointMirror, one -> it, otherwise None (ART/ModuleMirror.py:27-38).
    Host helper kept for API parity; the kernels apply the same rule per ray (art_device.h `consider`)."""
    if len(ListPointIntersectionMirror) == 2:
        return mgeo.ClosestPoint(PointMirror, ListPointIntersectionMirror[0], ListPointIntersectionMirror[1])
    if len(ListPointIntersectionMirror) == 1:
        return ListPointIntersectionMirror[0]
    return None


def _ReflectionMirrorRay(Mirror, PointMirror, Ray):
    """Reflect ONE ray at a given surface point (ART/ModuleMirror.py:878-906), on the host; bundles go through
    ReflectionMirrorRayList / RayTracingCalculation on the device."""
    NormalMirror = Mirror.get_normal(PointMirror)
    out = Ray.copy_ray()
    out.point = PointMirror
    out.vector = mgeo.SymmetricalVector(-Ray.vector, NormalMirror)
    out.incidence = mgeo.AngleBetweenTwoVectors(-Ray.vector, NormalMirror)
    out.path = Ray.path + (np.linalg.norm(PointMirror - Ray.point),)
    return out


class _Mirror:
    __deepcopy__ = mgeo.flat_deepcopy

    _abi_kind = None

    def _abi_params(self):
        raise NotImplementedError

    def _get_intersection(self, Ray):
        """Intersection point of ONE ray, given in the mirror's own frame, with the surface inside its support, or
        None (the `_get_intersection` of every mirror class of ART/ModuleMirror.py): a one-ray trace on the device."""
        hit = ReflectionMirrorRayList(self, [Ray], IgnoreDefects=True)
        return hit[0].point if len(hit) == 1 else None

    def _content_hash(self):
        return hash((self.type, hash(self.support)) + tuple(float(v) for v in self._abi_params()))

    def __hash__(self):
        return mgeo.memo_hash(self, self._content_hash)      # (recomputed from the contents, once per hash epoch)

    _cloud_has_outline = True      # the point cloud of get_grid3D starts with the outline of the support

    def _sag(self, x, y):
        """Surface height z(x, y) in the mirror's own frame (arrays; NaN where the surface does not exist)."""
        return np.zeros_like(x)

    def get_grid3D(self, NbPoint: int, **kwargs):
        """About NbPoint points of the surface inside its support, in the mirror's own frame: a tenth of them on the
        outline of the support (and of its hole), the rest on the support's grid (the `get_grid3D` of every optic
        class of ART/ModuleMirror.py, e.g. :93-113).  With edges=True also the closed index loops of the hole outlines.
        Points where the surface does not exist under the support are left out."""
        return _surface_cloud(self, self._sag, self._cloud_has_outline, NbPoint, bool(kwargs.get("edges")))


def _surface_cloud(optic, sag, with_outline, NbPoint, want_edges):
    n_outline = int(round(0.1 * NbPoint))
    outline, loops = optic.support._Contour_points(n_outline, edges=True)
    outline = np.asarray(outline, dtype=float).reshape(-1, 2)
    grid = optic.support._grid_xy(NbPoint - n_outline)
    centre = optic.get_centre()

    def lift(xy):
        x, y = xy[:, 0] + centre[0], xy[:, 1] + centre[1]
        with np.errstate(invalid="ignore"):
            z = sag(x, y)
        return np.column_stack((x, y, z)), np.isfinite(z)

    if with_outline:
        P, ok = lift(np.concatenate((outline, grid)))
        new_index = np.cumsum(ok) - 1
        loops = [[int(new_index[i]) for i in loop if ok[i]] for loop in loops]
        P = P[ok]
    else:
        # the ellipsoid's cloud (ART/ModuleMirror.py:716-751): grid points first, then only the outline points an edge
        # loop refers to (the hole), in loop order -- the loop's closing index is a point of its own
        G, okg = lift(grid)
        O, oko = lift(outline)
        parts, first, new_loops = [G[okg]], int(okg.sum()), []
        for loop in loops:
            keep = [i for i in loop if oko[i]]
            parts.append(O[keep])
            new_loops.append(list(range(first, first + len(keep))))
            first += len(keep)
        P, loops = np.concatenate(parts), new_loops
    cloud = list(P)
    return (cloud, loops) if want_edges else cloud


class MirrorPlane(_Mirror):
    """Plane mirror in the xy-plane of its own frame (ART/ModuleMirror.py:42-113)."""
    _abi_kind = _abi.ART_PLANE

    def __init__(self, Support):
        self.support = Support
        self.type = "Plane Mirror"

    def _abi_params(self):
        return []

    def get_normal(self, Point):
        return np.array([0, 0, 1])

    def get_centre(self):
        return np.array([0, 0, 0])


class MirrorSpherical(_Mirror):
    """Sphere x^2+y^2+z^2 = R^2; negative Radius = convex (ART/ModuleMirror.py:117-208)."""
    _abi_kind = _abi.ART_SPHERE

    def __init__(self, Radius, Support):
        if Radius < 0:
            self.type = "SphericalCX Mirror"
            self.radius = -Radius
        else:
            self.type = "SphericalCC Mirror"
            self.radius = Radius
        self.support = Support

    def _abi_params(self):
        return [self.radius]

    def get_normal(self, Point):
        return mgeo.Normalize(-np.asarray(Point, dtype=float))

    def get_centre(self):
        return np.array([0, 0, -self.radius])

    def _sag(self, x, y):
        return -np.sqrt(self.radius ** 2 - (x * x + y * y))


class MirrorParabolic(_Mirror):
    """Paraboloid x^2+y^2 = 2 p z with the support centre off-axis (ART/ModuleMirror.py:212-387).
    `offaxisangle` is given in degrees and stored/returned in radians, like the reference."""
    _abi_kind = _abi.ART_PARABOLA

    def __init__(self, FocalEffective: float, OffAxisAngle: float, Support):
        self._offaxisangle = np.deg2rad(OffAxisAngle)
        self.support = Support
        self.type = "Parabolic Mirror"
        self._feff = FocalEffective
        self._p = FocalEffective * (1 + np.cos(self._offaxisangle))

    @property
    def offaxisangle(self):
        return self._offaxisangle

    @offaxisangle.setter
    def offaxisangle(self, OffAxisAngle):
        self._offaxisangle = np.deg2rad(OffAxisAngle)
        self._p = self._feff * (1 + np.cos(self._offaxisangle))

    @property
    def feff(self):
        return self._feff

    @feff.setter
    def feff(self, FocalEffective):
        self._feff = FocalEffective
        self._p = self._feff * (1 + np.cos(self._offaxisangle))

    @property
    def p(self):
        return self._p

    @p.setter
    def p(self, SemiLatusRectum):
        self._p = SemiLatusRectum
        self._feff = self._p / (1 + np.cos(self._offaxisangle))

    def _abi_params(self):
        return [self._p]

    def get_normal(self, Point):
        return mgeo.Normalize(np.array([-Point[0], -Point[1], self._p]))

    def get_centre(self):
        return np.array([self.feff * np.sin(self.offaxisangle), 0,
                         self._p * 0.5 - self.feff * np.cos(self.offaxisangle)])

    def _sag(self, x, y):
        return (x * x + y * y) / (2 * self._p)


class MirrorToroidal(_Mirror):
    """Torus (sqrt(x^2+z^2) - R)^2 + y^2 = r^2 (ART/ModuleMirror.py:391-527)."""
    _abi_kind = _abi.ART_TORUS

    def __init__(self, MajorRadius, MinorRadius, Support):
        self.majorradius = MajorRadius
        self.minorradius = MinorRadius
        self.support = Support
        self.type = "Toroidal Mirror"

    def _abi_params(self):
        return [self.majorradius, self.minorradius]

    def get_normal(self, Point):
        x, y, z = Point
        R2, r2 = self.majorradius ** 2, self.minorradius ** 2
        S = x * x + y * y + z * z
        return mgeo.Normalize(-np.array([x * (S - R2 - r2), y * (S + R2 - r2), z * (S - R2 - r2)]))

    def get_centre(self):
        return np.array([0, 0, -self.majorradius - self.minorradius])

    def _sag(self, x, y):
        return -np.sqrt((np.sqrt(self.minorradius ** 2 - y * y) + self.majorradius) ** 2 - x * x)


def ReturnOptimalToroidalRadii(Focal: float, AngleIncidence: float):
    """Major/minor radii giving focal length `Focal` at `AngleIncidence` (deg) without astigmatism
    (ART/ModuleMirror.py:533-561)."""
    c = np.cos(AngleIncidence * np.pi / 180)
    return 2 * Focal * (1 / c - c), 2 * Focal * c


class MirrorEllipsoidal(_Mirror):
    """Ellipsoid (x/a)^2 + (y/b)^2 + (z/b)^2 = 1 (ART/ModuleMirror.py:565-751); same ctor variants."""
    _abi_kind = _abi.ART_ELLIPSOID

    def __init__(self, Support, SemiMajorAxis=None, SemiMinorAxis=None, OffAxisAngle=None, f_object=None,
                 f_image=None):
        self.type = "Ellipsoidal Mirror"
        self.support = Support
        self.a = None
        self.b = None
        self._offaxisangle = None
        if SemiMajorAxis is not None and SemiMinorAxis is not None:
            self.a = SemiMajorAxis
            self.b = SemiMinorAxis
        have_f = f_object is not None and f_image is not None
        if OffAxisAngle is not None:
            self._offaxisangle = np.deg2rad(OffAxisAngle)
            if have_f:
                foci_sq = f_object ** 2 + f_image ** 2 - 2 * f_object * f_image * np.cos(self._offaxisangle)
                self.a = (f_image + f_object) / 2
                self.b = np.sqrt(self.a ** 2 - foci_sq / 4)
        elif self.a is not None and self.b is not None:
            foci = 2 * np.sqrt(self.a ** 2 - self.b ** 2)
            if have_f:
                self._offaxisangle = np.arccos((f_image ** 2 + f_object ** 2 - foci ** 2) / (2 * f_image * f_object))
            else:
                self._offaxisangle = np.arccos(1 - foci ** 2 / (2 * self.a ** 2))
        if self.a is None or self.b is None or self._offaxisangle is None:
            raise ValueError("Invalid mirror parameters")

    def _abi_params(self):
        return [self.a, self.b]

    def get_normal(self, Point):
        return mgeo.Normalize(np.array([-Point[0] / self.a ** 2, -Point[1] / self.b ** 2, -Point[2] / self.b ** 2]))

    def get_centre(self):
        """Point of the surface at the centre of the support (ART/ModuleMirror.py:695-714)."""
        foci = 2 * np.sqrt(self.a ** 2 - self.b ** 2)
        h = -foci / 2 / np.tan(self._offaxisangle)
        R = np.sqrt(foci ** 2 / 4 + h ** 2)
        sign = 1
        if math.isclose(self._offaxisangle, np.pi / 2):
            h = 0
        elif self._offaxisangle > np.pi / 2:
            h = -h
            sign = -1
        qa = 1 - self.a ** 2 / self.b ** 2
        qb = -2 * h
        qc = self.a ** 2 + h ** 2 - R ** 2
        z = (-qb + sign * np.sqrt(qb ** 2 - 4 * qa * qc)) / (2 * qa)
        if math.isclose(z ** 2, self.b ** 2):
            return np.array([0, 0, -self.b])
        return np.array([self.a * np.sqrt(1 - z ** 2 / self.b ** 2), 0, sign * z])

    _cloud_has_outline = False

    def _sag(self, x, y):
        return -self.b * np.sqrt(1 - (x / self.a) ** 2 - (y / self.b) ** 2)


def ReturnOptimalEllipsoidalAxes(Focal: float, AngleIncidence: float):
    """ART/ModuleMirror.py:755-777."""
    return Focal, Focal * np.cos(np.deg2rad(AngleIncidence))


class MirrorCylindrical(_Mirror):
    """Cylinder y^2 + z^2 = R^2; negative Radius = convex (ART/ModuleMirror.py:781-874)."""
    _abi_kind = _abi.ART_CYLINDER

    def __init__(self, Radius, Support):
        if Radius < 0:
            self.type = "CylindricalCX Mirror"
            self.radius = -Radius
        else:
            self.type = "CylindricalCC Mirror"
            self.radius = Radius
        self.support = Support

    def _abi_params(self):
        return [self.radius]

    def get_normal(self, Point):
        return mgeo.Normalize(np.array([0, -Point[1], -Point[2]]))

    def get_centre(self):
        return np.array([0, 0, -self.radius])

    def _sag(self, x, y):
        return -np.sqrt(self.radius ** 2 - y * y) + 0.0 * x


class MirrorQuadric(_Mirror):
    """General quadric mirror in its own POLE frame (no counterpart in the reference): the surface
        F(P) = P^T Q P + 2 b.P + c = 0
    with the origin on the surface (c = 0) and grad F(0) = 2b along -z; the reflecting sheet is the one with dF/dz < 0,
    its normal n = -grad F / |grad F| is +z at the pole, so `OEPlacement`'s IncidenceAngle is the true incidence angle
    there.  Q: symmetric 3x3 matrix.  The coefficients are rescaled to grad F(0) = (0, 0, -1).  Traced by
    art_trace_quadric (include/art_hip.h), one element per launch; no defects, no gratings."""
    _abi_kind = _abi.ART_PLANE            # by convention: art_trace_quadric ignores the kind

    def __init__(self, Support, Q, b, c=0.0):
        Q = np.asarray(Q, dtype=np.longdouble)
        b = np.asarray(b, dtype=np.longdouble)
        if Q.shape != (3, 3) or b.shape != (3,):
            raise ValueError("MirrorQuadric: Q must be a 3x3 matrix and b a 3-vector")
        if not (np.isfinite(Q).all() and np.isfinite(b).all() and np.isfinite(c)):
            raise ValueError("MirrorQuadric: every coefficient must be finite")
        if np.abs(Q - Q.T).max() > 1e-14 * max(float(np.abs(Q).max()), 1e-300):
            raise ValueError("MirrorQuadric: Q must be symmetric")
        if not b[2] < 0 or max(abs(b[0]), abs(b[1])) > 1e-14 * abs(b[2]):
            raise ValueError("MirrorQuadric: grad F(0) = 2b must point along -z (the mirror's normal at its pole is +z)")
        if abs(c) > 1e-14 * abs(b[2]):
            raise ValueError("MirrorQuadric: the origin must lie on the surface (c = 0)")
        k = -1 / (2 * b[2])
        self._set(Support, [Q[0, 0] * k, Q[1, 1] * k, Q[2, 2] * k, Q[0, 1] * k, Q[0, 2] * k, Q[1, 2] * k, 0.0, 0.0, -0.5,
                            np.longdouble(c) * k], "Quadric Mirror")

    def _set(self, Support, coefficients, tname):
        self.support = Support
        self.type = tname
        self._coeff = tuple(float(v) for v in coefficients)      # q[6] (xx yy zz xy xz yz), b[3], c: ArtQuadricDesc

    def _abi_params(self):
        return []

    def _quadric_coefficients(self):
        return self._coeff

    def _content_hash(self):
        return hash((self.type, hash(self.support)) + self._coeff)

    def get_centre(self):
        return np.array([0.0, 0.0, 0.0])

    def _half_gradient(self, P):
        q, x, y, z = self._coeff, P[0], P[1], P[2]
        return np.array([q[0] * x + q[3] * y + q[4] * z + q[6], q[3] * x + q[1] * y + q[5] * z + q[7],
                         q[4] * x + q[5] * y + q[2] * z + q[8]])

    def get_normal(self, Point):
        return mgeo.Normalize(-self._half_gradient(np.asarray(Point, dtype=float)))

    def _sag(self, x, y):
        """The root in z of F(x, y, z) = A z^2 + B z + C on the sheet with dF/dz = 2 A z + B < 0, i.e. the root
        (-B - sqrt(D)) / (2A), in the form that does not cancel; NaN where there is none."""
        q = self._coeff
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        A = q[2] + 0.0 * x
        B = 2 * (q[4] * x + q[5] * y + q[8])
        Cc = q[0] * x * x + q[1] * y * y + 2 * q[3] * x * y + 2 * (q[6] * x + q[7] * y) + q[9]
        with np.errstate(all="ignore"):
            D = B * B - 4 * A * Cc
            s = np.sqrt(np.where(D > 0, D, np.nan))
            w = -0.5 * (B + np.where(B < 0, -s, s))             # B < 0: (-B + s) / 2, B >= 0: (-B - s) / 2
            z = np.where(B < 0, Cc / w, w / A)
            return np.where(A == 0, np.where(B < 0, -Cc / B, np.nan), z)


class MirrorConic(MirrorQuadric):
    """Conic mirror between two conjugate points, in its pole frame: origin on the surface, z the normal there, x
    tangential in the plane of incidence and pointing downstream, `GrazingAngle` (degrees, in (0, 90]) between the
    central ray and the surface.  The signs of the two distances select the surface:
        f_object, f_image > 0, finite      ellipse    (point to point)
        one of them np.inf                 parabola   (collimated in, or collimating out)
        one of them < 0                    hyperbola  (virtual object or virtual image)
    With foci F1, F2 and s = f_object + f_image the surface is (g.P + h)^2 - 4 s^2 |P - F1|^2 = 0, g = -2 (F2 - F1),
    h = |F2|^2 - |F1|^2 - s^2 (hyperbola: s = |f_object| - |f_image|); a real object sits at p (-cos t, 0, sin t), a real
    image at q (cos t, 0, sin t), a virtual focus mirrored behind the surface; the parabola for a beam along
    d = (cos t, 0, -+sin t) is |P|^2 - (d.P)^2 - 4 f sin t z = 0.  Cylindrical=True: y drops out of every squared distance
    (a plane-elliptical, parabolic or hyperbolic cylinder with its generators along y).  The coefficients are formed in
    np.longdouble, c = 0 exactly, scaled to grad F(0) = (0, 0, -1)."""

    def __init__(self, Support, f_object, f_image, GrazingAngle, Cylindrical=False):
        L = np.longdouble
        p, q, deg = float(f_object), float(f_image), float(GrazingAngle)
        if not (0 < deg <= 90):
            raise ValueError("MirrorConic: GrazingAngle must lie in (0, 90] degrees")
        if p == 0 or q == 0 or np.isnan(p) or np.isnan(q):
            raise ValueError("MirrorConic: f_object and f_image must not be zero")
        if np.isinf(p) and np.isinf(q):
            raise ValueError("MirrorConic: f_object and f_image are both infinite: that is a MirrorPlane")
        if (p < 0 and q < 0) or ((np.isinf(p) or np.isinf(q)) and min(p, q) < 0):
            raise ValueError("MirrorConic: at most one of f_object, f_image may be negative, and then both are finite")
        th = np.deg2rad(L(deg))
        ct, st = (L(0), L(1)) if deg == 90 else (np.cos(th), np.sin(th))
        I = np.diag([L(1), L(0) if Cylindrical else L(1), L(1)])
        if np.isinf(p) or np.isinf(q):
            d = np.array([ct, L(0), -st if np.isinf(p) else st])
            f = L(q if np.isinf(p) else p)
            k = 1 / (4 * f * st)
            Q = (I - np.outer(d, d)) * k
            kind = "Parabolic"
        else:
            if p < 0 or q < 0:
                if abs(p) == abs(q):
                    raise ValueError("MirrorConic: a hyperbola with |f_object| = |f_image| degenerates into a MirrorPlane")
                s = L(abs(p)) - L(abs(q))
                kind = "Hyperbolic"
            else:
                s = L(p) + L(q)
                kind = "Elliptical"
            F1 = L(abs(p)) * (np.array([-ct, L(0), st]) if p > 0 else np.array([ct, L(0), -st]))
            F2 = L(abs(q)) * (np.array([ct, L(0), st]) if q > 0 else np.array([-ct, L(0), -st]))
            g = -2 * (F2 - F1)
            h = F2.dot(F2) - F1.dot(F1) - s * s
            bz = h * g[2] + 4 * s * s * F1[2]               # b = h g + 4 s^2 F1; its x component vanishes analytically
            k = -1 / (2 * bz)
            Q = (np.outer(g, g) - 4 * s * s * I) * k
        self._set(Support, [Q[0, 0], Q[1, 1], Q[2, 2], Q[0, 1], Q[0, 2], Q[1, 2], 0.0, 0.0, -0.5, 0.0],
                  kind + (" Cylinder Mirror" if Cylindrical else " Conic Mirror"))
        self.f_object, self.f_image, self.grazingangle, self.cylindrical = p, q, deg, bool(Cylindrical)


def MirrorEllipticalCylinder(Support, f_object, f_image, GrazingAngle):
    """Plane-elliptical cylinder (one mirror of a Kirkpatrick-Baez pair): focuses in its plane of incidence only."""
    if not (0 < f_object < np.inf and 0 < f_image < np.inf):
        raise ValueError("MirrorEllipticalCylinder: f_object and f_image must be positive and finite")
    return MirrorConic(Support, f_object, f_image, GrazingAngle, Cylindrical=True)


def MirrorParabolicCylinder(Support, Focal, GrazingAngle, Collimating=False):
    """Parabolic cylinder: focuses a collimated beam onto a line at `Focal` (Collimating=True: the reverse)."""
    if not 0 < Focal < np.inf:
        raise ValueError("MirrorParabolicCylinder: Focal must be positive and finite")
    return MirrorConic(Support, Focal if Collimating else np.inf, np.inf if Collimating else Focal, GrazingAngle, Cylindrical=True)


def _hyperbolic(Support, f_object, f_image, GrazingAngle, Cylindrical, name):
    if not (np.isfinite(f_object) and np.isfinite(f_image) and min(f_object, f_image) < 0):
        raise ValueError(name + ": one of f_object, f_image must be negative (a virtual focus), both finite")
    return MirrorConic(Support, f_object, f_image, GrazingAngle, Cylindrical=Cylindrical)


def MirrorHyperboloidal(Support, f_object, f_image, GrazingAngle):
    """Hyperboloid of revolution between a real and a virtual focus (the secondary of a Wolter or Cassegrain pair)."""
    return _hyperbolic(Support, f_object, f_image, GrazingAngle, False, "MirrorHyperboloidal")


def MirrorHyperbolicCylinder(Support, f_object, f_image, GrazingAngle):
    return _hyperbolic(Support, f_object, f_image, GrazingAngle, True, "MirrorHyperbolicCylinder")


class MirrorFreeform(_Mirror):
    """Freeform mirror (no counterpart in the reference): a quadric base in its pole frame plus a polynomial height figure,
        z = sag_base(x, y) + h(x, y),   implicitly  Phi(P) = F(x, y, z - h(x, y)) = 0 ,
    with h in mm and h > 0 a bump towards the incoming light.  Base: a MirrorQuadric or anything built on it (MirrorConic,
    MirrorEllipticalCylinder, ...).  Figure: a list of ModuleDefects.Zernike (order <= 16) and / or
    ModuleDefects.Polynomial; they are summed here into ONE polynomial of total degree <= 16 with one normalisation radius.
    Terms with different radii cannot be merged exactly and are refused (a constant term has no radius and merges with
    anything).  The rays are intersected with Phi exactly, by Newton's iteration on the device (art_trace_freeform,
    include/art_hip.h): nanometres of figure error and millimetres of aspheric departure are the same code."""
    _abi_kind = _abi.ART_PLANE            # by convention: art_trace_freeform ignores the kind

    def __init__(self, Base, Figure):
        from . import ModuleDefects as mdef
        if not isinstance(Base, MirrorQuadric):
            raise TypeError("MirrorFreeform: Base must be a MirrorQuadric or one of the mirrors built on it (MirrorConic, ...)")
        if isinstance(Figure, (mdef.Defect, dict)) or not hasattr(Figure, "__iter__"):
            raise TypeError("MirrorFreeform: Figure must be a list of ModuleDefects.Zernike and / or ModuleDefects.Polynomial")
        Dm = _abi.ART_ZERN_DIM
        A, R, N = np.zeros((Dm, Dm)), None, 0
        for term in Figure:
            if isinstance(term, mdef.Polynomial):
                M, order = term._matrix(), term.max_order
            elif isinstance(term, mdef.Zernike):
                if term.max_order > _abi.ART_ZERN_MAX_ORDER:
                    raise ValueError(f"MirrorFreeform: a Zernike figure of order {term.max_order} exceeds the maximum "
                                     f"{_abi.ART_ZERN_MAX_ORDER} of a freeform's figure")
                order = max(2, term.max_order)            # the generator's lowest table (ModuleDefects.zernike_table)
                M = np.zeros((Dm, Dm))
                Zm = mdef.zernike_monomials(order)
                for key, c in term.coefficients.items():
                    Z = Zm[key][:Dm, :Dm]
                    M[:Z.shape[0], :Z.shape[1]] += c * Z
            else:
                raise ValueError(f"MirrorFreeform: a figure term of type {type(term).__name__} is not supported (gridded "
                                 "Fourrier maps and measured maps are not polynomials): use Zernike or Polynomial")
            flat = M.copy()
            flat[0, 0] = 0.0
            if flat.any():                                  # only a constant is free of the radius
                if R is not None and float(term.R) != R:
                    raise ValueError(f"MirrorFreeform: figure terms with the normalisation radii {R:g} and {float(term.R):g} "
                                     "cannot be merged exactly: give them one Radius")
                R = float(term.R)
            A += M
            N = max(N, order)
        if not np.isfinite(A).all():
            raise ValueError("MirrorFreeform: every figure coefficient must be finite")
        self.Base = Base
        self.support = Base.support
        self.type = "Freeform Mirror"
        self._fig_A, self._fig_R, self._fig_N = A, float(Base.support._CircumCirc()) if R is None else R, int(N)

    def _abi_params(self):
        return []

    def _base_coefficients(self):
        return self.Base._quadric_coefficients()

    def _freeform_figure(self):
        """(table in the dense layout of include/art_hip.h, radius, order)."""
        from .ModuleDefects import dense_table
        return dense_table(self._fig_R, self._fig_N, self._fig_A), self._fig_R, self._fig_N

    def _content_hash(self):
        return hash((self.type, hash(self.Base), self._fig_R, self._fig_N, self._fig_A.tobytes()))

    def get_centre(self):
        return np.array([0.0, 0.0, 0.0])

    def _figure(self, x, y, derivatives=False):
        """h (and its two slopes) at pole-frame points, in the float type of x."""
        from .ModuleDefects import dense_eval
        return dense_eval(self._fig_R, self._fig_A, x, y, derivatives)

    def get_normal(self, Point):
        """The true normal -grad Phi / |grad Phi| at ONE point of the surface: grad Phi = (F_x - F_z h_x, F_y - F_z h_y,
        F_z) with the base's gradient taken at (x, y, z - h)."""
        P = np.asarray(Point, dtype=float)
        h, hx, hy = self._figure(P[0], P[1], derivatives=True)
        g = self.Base._half_gradient(np.array([P[0], P[1], P[2] - float(h)]))
        return mgeo.Normalize(-np.array([g[0] - g[2] * float(hx), g[1] - g[2] * float(hy), g[2]]))

    def _sag(self, x, y):
        """Base + figure: the surface the rays meet (the render shows the figure, unlike DeformedMirror's)."""
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        return self.Base._sag(x, y) + self._figure(x, y)


def MirrorEvenAsphere(Support, Radius, Conic=0.0, Coefficients=()):
    """The standard even asphere in its vertex frame, reflecting side towards +z,
        z = c r^2 / (1 + sqrt(1 - (1 + k) c^2 r^2)) + sum_i alpha_i r^(2 i + 2),   i = 1, 2, ...   (c = 1 / Radius),
    Radius > 0 concave (np.inf: a plane base), Conic = k, Coefficients = (alpha_1, alpha_2, ...) in mm^-(2i+1), at most seven
    (r^16).  A MirrorFreeform whose base is the conicoid x^2 + y^2 + (1 + k) z^2 - 2 R z = 0 and whose figure is the alpha
    polynomial, normalised to a power of two >= the support's circumscribed radius (scaling by it is exact)."""
    from .ModuleDefects import Polynomial
    R, k = float(Radius), float(Conic)
    alphas = [float(a) for a in Coefficients]
    if R == 0 or np.isnan(R) or not np.isfinite(k):
        raise ValueError("MirrorEvenAsphere: Radius must not be zero and Conic must be finite")
    if 2 * len(alphas) + 2 > _abi.ART_ZERN_MAX_ORDER:
        raise ValueError("MirrorEvenAsphere: at most seven coefficients (r^4 ... r^16)")
    L = np.longdouble
    s = L(1) if R > 0 else L(-1)
    c2 = L(0) if np.isinf(R) else s / (2 * abs(L(R)))         # F = s (x^2 + y^2 + (1 + k) z^2) / (2 |R|) - z
    Q = np.diag([c2, c2, (1 + L(k)) * c2])
    base = MirrorQuadric(Support, Q, [0.0, 0.0, -0.5])
    Rn = 2.0 ** math.ceil(math.log2(float(Support._CircumCirc())))
    co = {}
    for i, a in enumerate(alphas, start=1):
        m = i + 1                                                   # alpha_i r^(2m) = alpha_i sum_j C(m, j) x^(2j) y^(2(m-j))
        for j in range(m + 1):
            co[(2 * j, 2 * (m - j))] = float(L(a) * math.comb(m, j) * L(Rn) ** (2 * m))
    M = MirrorFreeform(base, [Polynomial(Support, co, Radius=Rn)])
    M.type = "Even Asphere Mirror"
    M.radius, M.conic, M.alphas = R, k, tuple(alphas)
    return M


class DeformedMirror(_Mirror):
    """A mirror with surface defects (ART/ModuleMirror.py:945-980).  The defect offset always shifts the hit
    point; the perturbed normal is used only when tracing with IgnoreDefects=False (reference default: True)."""

    def __init__(self, Mirror, DeformationList):
        if hasattr(Mirror, "_quadric_coefficients"):
            raise ValueError("DeformedMirror: defects on a MirrorQuadric / MirrorConic are not supported")
        if hasattr(Mirror, "_freeform_figure"):
            raise ValueError("DeformedMirror: defects on a MirrorFreeform are not supported: put them into its Figure")
        self.Mirror = Mirror
        self.DeformationList = list(DeformationList)
        self.type = Mirror.type
        self.support = self.Mirror.support
        for d in self.DeformationList:
            if not (hasattr(d, "_abi_table") or hasattr(d, "_abi_grid")):
                raise NotImplementedError(f"defect type {type(d).__name__} has no device implementation yet")
        # Any number of Zernike defects: offsets and slopes of defects with the same normalisation radius add up
        # (ART/ModuleMirror.py:952-980), so they are merged into ONE table per radius (_zernike_groups).  What stays
        # limited is the number of tables per mirror: distinct radii, and gridded height maps.
        if len(self._zernike_groups()) > _abi.ART_MAX_DEFECTS:
            raise NotImplementedError(f"Zernike defects with more than {_abi.ART_MAX_DEFECTS} different normalisation radii on one mirror")
        if len(self._grid_defects()) > _abi.ART_MAX_DEFECTS:
            raise NotImplementedError(f"at most {_abi.ART_MAX_DEFECTS} gridded defects per mirror are supported")

    @property
    def _abi_kind(self):
        return self.Mirror._abi_kind

    def _abi_params(self):
        return self.Mirror._abi_params()

    def _zernike_defects(self):
        return [d for d in self.DeformationList if hasattr(d, "_abi_table")]

    def _grid_defects(self):
        return [d for d in self.DeformationList if hasattr(d, "_abi_grid")]

    def _zernike_groups(self):
        """{R: summed coefficient dict} of the Zernike defects, by normalisation radius, in order of first appearance."""
        groups = {}
        for d in self._zernike_defects():
            g = groups.setdefault(float(d.R), {})
            for k, c in d.coefficients.items():
                g[k] = g.get(k, 0.0) + c
        return groups

    def _abi_defect_table(self):
        """(device table of all Zernike groups, number of tables, recurrence layout?) -- see ModuleDefects.zernike_table.
        One group above order 16 puts all of the mirror's tables into the recurrence layout, padded to one order."""
        from .ModuleDefects import zernike_table
        groups = self._zernike_groups()
        top = max(max(k[0] for k in g) for g in groups.values())
        rec = top > _abi.ART_ZERN_MAX_ORDER
        return (np.concatenate([zernike_table(R, g, recurrence=rec, order=max(2, top)) for R, g in groups.items()]),
                len(groups), rec)

    def get_normal(self, PointMirror):
        """Normal of the deformed surface at ONE point, host side (ART/ModuleMirror.py:952-961): the base normal
        folded with each defect's normal by slope addition."""
        normal = np.asarray(self.Mirror.get_normal(PointMirror), dtype=float)
        C = self.get_centre()
        for d in self.DeformationList:
            normal = mgeo.normal_add(normal, d.get_normal(PointMirror - C))
            normal = normal / np.linalg.norm(normal)
        return normal

    def get_centre(self):
        return self.Mirror.get_centre()

    def get_grid3D(self, NbPoint, **kwargs):
        """The undeformed surface: the render does not show the defects (ART/ModuleMirror.py:966-967)."""
        return self.Mirror.get_grid3D(NbPoint, **kwargs)

    def __hash__(self):
        return hash((hash(self.Mirror),) + tuple(hash(d) for d in self.DeformationList))


class Grating(_Mirror):
    """A classical ruled diffraction grating on any of the six mirror surfaces (no counterpart in the reference, whose
    optics are achromatic).  The grooves are the intersections of the surface with equally spaced parallel planes,
    `LinesPerMm` of them per millimetre along q0 = (cos GrooveAngle, sin GrooveAngle, 0) of the optic's own frame:
    GrooveAngle (degrees) is measured from the optic's x axis, the element's `majoraxis`, which `OEPlacement` puts into
    the plane of incidence -- 0 is the classical in-plane mount, 90 the conical (off-plane) mount.  `Order` is the
    diffraction order m; LinesPerMm = 0 or Order = 0 is the bare mirror.  Traced by art_trace_grating
    (include/art_hip.h); the wavelength is the traced bundle's."""

    def __init__(self, Mirror, LinesPerMm, Order=1, GrooveAngle=0.0):
        if isinstance(Mirror, (DeformedMirror, Grating)) or hasattr(Mirror, "DeformationList"):
            raise ValueError("Grating: mirrors with defects (DeformedMirror) or gratings are not supported as substrates")
        if hasattr(Mirror, "_quadric_coefficients") or hasattr(Mirror, "_freeform_figure"):
            raise ValueError("Grating: a MirrorQuadric / MirrorConic / MirrorFreeform is not supported as a substrate")
        tname = getattr(Mirror, "type", None)
        if not (isinstance(tname, str) and "Mirror" in tname) or getattr(Mirror, "_abi_kind", None) is None:
            raise ValueError("Grating: the substrate must be one of the mirror classes (a Mask cannot carry a grating)")
        N = float(LinesPerMm)
        if not (math.isfinite(N) and N >= 0):
            raise ValueError("Grating: LinesPerMm must be finite and >= 0")
        if int(Order) != Order:
            raise ValueError("Grating: Order must be an integer")
        if not math.isfinite(float(GrooveAngle)):
            raise ValueError("Grating: GrooveAngle must be finite")
        self.Mirror = Mirror
        self.lines_per_mm = N
        self.order = int(Order)
        self.groove_angle = float(GrooveAngle)
        self.type = Mirror.type              # passes the '"Mirror" in type' checks, convex substrates included
        self.support = Mirror.support

    @property
    def _abi_kind(self):
        return self.Mirror._abi_kind

    def _abi_params(self):
        return self.Mirror._abi_params()

    def _groove_vector(self):
        """q0 in the optic's xy plane (exact for the two mounts: cos 90 deg is not 6e-17 here)."""
        a = self.groove_angle % 360.0
        exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
        if a in exact:
            return exact[a]
        return (math.cos(math.radians(a)), math.sin(math.radians(a)))

    def get_normal(self, Point):
        return self.Mirror.get_normal(Point)

    def get_centre(self):
        return self.Mirror.get_centre()

    def _sag(self, x, y):
        return self.Mirror._sag(x, y)

    def get_grid3D(self, NbPoint, **kwargs):
        return self.Mirror.get_grid3D(NbPoint, **kwargs)

    def __hash__(self):
        return hash((hash(self.Mirror), "grating", self.lines_per_mm, self.order, self.groove_angle))


def ReflectionMirrorRayList(Mirror, ListRay, IgnoreDefects=False):
    """Reflect a bundle given in the mirror's own frame (ART/ModuleMirror.py:912-939): one identity-pose
    element on the device."""
    from . import ModuleProcessing as mp
    from .ModuleOpticalElement import OpticalElement
    # position = get_centre() with identity axes makes lab frame == optic frame (P_opt = P - pos + centre)
    oe = OpticalElement(Mirror, np.asarray(Mirror.get_centre(), dtype=float), np.array([0.0, 0.0, 1.0]),
                        np.array([1.0, 0.0, 0.0]))
    return mp.RayTracingCalculation(ListRay, [oe], IgnoreDefects=IgnoreDefects)[0]

// art_tubes.h -- the per-ray math of art_ray_tubes (include/art_hip.h): differential ("generalised") ray tracing.
//
// Beside each ray of a traced chain's history travel the first-order changes of its point and direction with respect to
// two source parameters a, b: four 3-vectors dP_j, dD_j (j = a, b) in the lab frame, 12 doubles.  The source parameters
// span the plane perpendicular to the source direction D0, (u, v) = perp_pair(D0):
//   ART_TUBE_POINT  dP = 0, dD = (u, v)   the source measure mu is solid angle (steradians)
//   ART_TUBE_PLANE  dP = (u, v), dD = 0   the source measure mu is area (mm^2)
// Every quantity read out below is independent of the choice of (u, v).
//
// A surface is the zero set of an implicit form with gradient g(P) and Hessian H(P) in the optic frame,
// P_o = fwd (P - pos) + centre (tangents rotate by fwd alone); the forms are those whose gradients base_normal
// (art_device.h) and quadric_trace normalise:
//   plane, mask  g = (0, 0, 1)              H = 0
//   sphere       g = P                      H = I
//   parabola     g = (x, y, -p)             H = diag(1, 1, 0)
//   ellipsoid    g = (x b^2, y a^2, z a^2)  H = diag(b^2, a^2, a^2)
//   cylinder     g = (0, y, z)              H = diag(0, 1, 1)
//   torus        g = (x kxz, y ky, z kxz)   H = diag(kxz, ky, kxz) + 2 P P^T,  kxz = |P|^2 - (R^2 + r^2), ky = |P|^2 + (R^2 - r^2)
//   quadric      g = Q P + b                H = Q        (half of the form's own 2 (Q P + b), 2 Q: a common factor cancels)
// Every kind but the torus is g = H P + g0 with a constant symmetric H: `Surface` holds H, g0 and the torus' two constants.
//
// Step at a mirror: D the incoming direction, P_prev the previous point, P the hit point (from the history), n = -g / |g|
// (the sign of g cancels: the reflection is even in n and dn follows n):
//   t    = (P - P_prev) . D
//   a_j  = dP_j + t dD_j                                   the tangent carried to the hit point's transverse plane
//   dt_j = -(n . a_j) / (n . D),  dQ_j = a_j + D dt_j      ... and along the ray onto the surface's tangent plane
//   dn_j = -(H dQ_j - n (n . H dQ_j)) / |g|                the normal's change along the surface
//   dD'_j = dD_j - 2 [(dD_j . n + D . dn_j) n + (D . n) dn_j]
// and the state becomes (dQ_j, dD'_j).  A mask is the plane rule without the reflection: dD stays, dP becomes dQ.
//
// Read-out behind the last element, D' the final direction: with a detector plane (centre C, normal nd) the same transport
// onto the plane gives dX_j; without one dX_j = dQ_j (the section at the last hit point).
//   solid_angle = D' . (dD_a x dD_b)                       dOmega' / dmu, signed, always finite
//   area        = nd . (dX_a x dX_b)   (detector)   or   D' . (dQ_a x dQ_b)   (none): mm^2 per unit mu, signed
//   curvature   C = B A^-1,  A = [v_i . dX_j],  B = [v_i . dD_j],  (v_1, v_2) = perp_pair(D')
//               (v_i . D' = 0, so dX_j needs no projection first); kappa_1 <= kappa_2 the eigenvalues of (C + C^T) / 2 in
//               1 / mm, negative = converging, the focal line at -1 / kappa along the ray; axis = the unit eigenvector of
//               kappa_1 in the lab frame (v_1 where the two are equal); asymmetry = |C_12 - C_21|, zero by Malus-Dupin.
// At a caustic A is singular and nothing is clamped: the curvatures, the axis and the asymmetry come out +-inf or NaN.
#pragma once

#include <math.h>

#include "../../include/art_hip.h"

#ifndef ART_HD
#if (defined(__HIPCC__) || defined(__CUDACC__)) && !defined(ART_HOST_TWIN)
#define ART_HD __host__ __device__ __forceinline__
#else
#define ART_HD inline
#endif
#endif

namespace artt {

struct Surface {
  double fwd[9], pos[3], centre[3];
  double H[6];        // h00, h11, h22, h01, h02, h12 (every kind but the torus)
  double g0[3];
  double sum2, dif2;  // torus: R^2 + r^2, R^2 - r^2
  int torus, mask;
};

struct Tube {
  double dP[2][3], dD[2][3];
};

struct Readout {
  double solid_angle, area, kappa1, kappa2, axis[3], asymmetry;
};

ART_HD double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ART_HD void cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
ART_HD double triple(const double* a, const double* b, const double* c) {   // a . (b x c)
  double x[3];
  cross(b, c, x);
  return dot(a, x);
}
ART_HD void rot(const double* M, const double* v, double* r) {      // r = M v
  r[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
  r[1] = M[3] * v[0] + M[4] * v[1] + M[5] * v[2];
  r[2] = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
}
ART_HD void rot_t(const double* M, const double* v, double* r) {    // r = M^T v
  r[0] = M[0] * v[0] + M[3] * v[1] + M[6] * v[2];
  r[1] = M[1] * v[0] + M[4] * v[1] + M[7] * v[2];
  r[2] = M[2] * v[0] + M[5] * v[1] + M[8] * v[2];
}

// An orthonormal pair (u, v) perpendicular to the unit vector d, d = u x v: u = d x e / |d x e| with e the coordinate axis
// of d's smallest component (selects, no branch), v = d x u.
ART_HD void perp_pair(const double* d, double* u, double* v) {
  const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
  const bool ex = ax <= ay && ax <= az, ey = !ex && ay <= az;
  // d x ex = (0, dz, -dy), d x ey = (-dz, 0, dx), d x ez = (dy, -dx, 0)
  u[0] = ex ? 0.0 : (ey ? -d[2] : d[1]);
  u[1] = ex ? d[2] : (ey ? 0.0 : -d[0]);
  u[2] = ex ? -d[1] : (ey ? d[0] : 0.0);
  const double r = 1.0 / sqrt(dot(u, u));
  u[0] *= r; u[1] *= r; u[2] *= r;
  cross(d, u, v);
}

// The surface of an element as the caller filled it (NOT a prepared descriptor); q: its ArtQuadricDesc, read when
// ART_FLAG_QUADRIC is set.  Pointer types are template parameters so that the kernel can hand in constant-address-space
// pointers (scalar loads).
template <typename EP, typename QP>
ART_HD void load_surface(const EP e, const QP q, Surface& s) {
#pragma unroll
  for (int i = 0; i < 9; ++i) s.fwd[i] = e->fwd[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { s.pos[i] = e->pos[i]; s.centre[i] = e->centre[i]; s.g0[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 6; ++i) s.H[i] = 0.0;
  s.sum2 = s.dif2 = 0.0;
  const int kind = e->kind;
  s.torus = 0;
  s.mask = kind == ART_MASK;
  if (e->flags & ART_FLAG_QUADRIC) {
#pragma unroll
    for (int i = 0; i < 6; ++i) s.H[i] = q->q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) s.g0[i] = q->b[i];
  } else if (kind == ART_SPHERE) {
    s.H[0] = s.H[1] = s.H[2] = 1.0;
  } else if (kind == ART_PARABOLA) {
    s.H[0] = s.H[1] = 1.0;
    s.g0[2] = -e->mp[0];
  } else if (kind == ART_ELLIPSOID) {
    const double a2 = e->mp[0] * e->mp[0], b2 = e->mp[1] * e->mp[1];
    s.H[0] = b2; s.H[1] = a2; s.H[2] = a2;
  } else if (kind == ART_CYLINDER) {
    s.H[1] = s.H[2] = 1.0;
  } else if (kind == ART_TORUS) {
    const double R = e->mp[0], r = e->mp[1];
    s.torus = 1;
    s.sum2 = R * R + r * r;
    s.dif2 = R * R - r * r;
  } else {                                  // plane, mask
    s.g0[2] = 1.0;
  }
}

// H v at the optic-frame point P
ART_HD void hessian_apply(const Surface& s, const double* P, const double* v, double* r) {
  if (s.torus) {
    const double S = dot(P, P), kxz = S - s.sum2, ky = S + s.dif2, pv = 2.0 * dot(P, v);
    r[0] = kxz * v[0] + pv * P[0];
    r[1] = ky * v[1] + pv * P[1];
    r[2] = kxz * v[2] + pv * P[2];
  } else {
    r[0] = s.H[0] * v[0] + s.H[3] * v[1] + s.H[4] * v[2];
    r[1] = s.H[3] * v[0] + s.H[1] * v[1] + s.H[5] * v[2];
    r[2] = s.H[4] * v[0] + s.H[5] * v[1] + s.H[2] * v[2];
  }
}

ART_HD void gradient(const Surface& s, const double* P, double* g) {
  if (s.torus) {
    const double S = dot(P, P), kxz = S - s.sum2, ky = S + s.dif2;
    g[0] = P[0] * kxz; g[1] = P[1] * ky; g[2] = P[2] * kxz;
  } else {
    hessian_apply(s, P, P, g);
    g[0] += s.g0[0]; g[1] += s.g0[1]; g[2] += s.g0[2];
  }
}

ART_HD void seed(const int kind, const double* D0, Tube& T) {
  double u[3], v[3];
  perp_pair(D0, u, v);
  const bool point = kind == ART_TUBE_POINT;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    T.dD[0][q] = point ? u[q] : 0.0;
    T.dD[1][q] = point ? v[q] : 0.0;
    T.dP[0][q] = point ? 0.0 : u[q];
    T.dP[1][q] = point ? 0.0 : v[q];
  }
}

// The tangents carried over t along D onto the plane with unit normal n: dQ_j = a_j - D (n . a_j) / (n . D)
ART_HD void onto_plane(const Tube& T, const double t, const double* D, const double* n, double (&dQ)[2][3]) {
  const double inD = 1.0 / dot(n, D);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double a[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = T.dP[j][q] + t * T.dD[j][q];
    const double dt = -dot(n, a) * inD;
#pragma unroll
    for (int q = 0; q < 3; ++q) dQ[j][q] = a[q] + D[q] * dt;
  }
}

// One element: D the incoming direction, Pprev the previous point, P the hit point, all lab frame
ART_HD void step(const Surface& s, const double* D, const double* Pprev, const double* P, Tube& T) {
  const double rel[3] = {P[0] - s.pos[0], P[1] - s.pos[1], P[2] - s.pos[2]};
  double Po[3], g[3], no[3], n[3];
  rot(s.fwd, rel, Po);
  Po[0] += s.centre[0]; Po[1] += s.centre[1]; Po[2] += s.centre[2];
  gradient(s, Po, g);
  const double ig = 1.0 / sqrt(dot(g, g));
  no[0] = -g[0] * ig; no[1] = -g[1] * ig; no[2] = -g[2] * ig;
  rot_t(s.fwd, no, n);
  const double leg[3] = {P[0] - Pprev[0], P[1] - Pprev[1], P[2] - Pprev[2]};
  double dQ[2][3];
  onto_plane(T, dot(leg, D), D, n, dQ);
  const double Dn = dot(D, n);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!s.mask) {
      double qo[3], Hq[3], dno[3], dn[3];
      rot(s.fwd, dQ[j], qo);
      hessian_apply(s, Po, qo, Hq);
      const double nHq = dot(no, Hq);
#pragma unroll
      for (int q = 0; q < 3; ++q) dno[q] = -(Hq[q] - no[q] * nHq) * ig;
      rot_t(s.fwd, dno, dn);
      const double c = dot(T.dD[j], n) + dot(D, dn);
#pragma unroll
      for (int q = 0; q < 3; ++q) T.dD[j][q] -= 2.0 * (c * n[q] + Dn * dn[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) T.dP[j][q] = dQ[j][q];
  }
}

// Behind the last element: D the final direction, P the last hit point; the detector plane (centre C, unit normal nd)
// is read when has_det is set
ART_HD void readout(const Tube& T, const double* D, const double* P, const bool has_det, const double* C, const double* nd,
                    Readout& R) {
  R.solid_angle = triple(D, T.dD[0], T.dD[1]);
  double dX[2][3];
  if (has_det) {
    const double toC[3] = {C[0] - P[0], C[1] - P[1], C[2] - P[2]};
    onto_plane(T, dot(nd, toC) / dot(nd, D), D, nd, dX);
    R.area = triple(nd, dX[0], dX[1]);
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) dX[j][q] = T.dP[j][q];
    R.area = triple(D, dX[0], dX[1]);
  }
  double v1[3], v2[3];
  perp_pair(D, v1, v2);
  const double A11 = dot(v1, dX[0]), A12 = dot(v1, dX[1]), A21 = dot(v2, dX[0]), A22 = dot(v2, dX[1]);
  const double B11 = dot(v1, T.dD[0]), B12 = dot(v1, T.dD[1]), B21 = dot(v2, T.dD[0]), B22 = dot(v2, T.dD[1]);
  const double idet = 1.0 / (A11 * A22 - A12 * A21);
  // C = B A^-1, A^-1 = [A22, -A12; -A21, A11] / det
  const double C11 = (B11 * A22 - B12 * A21) * idet, C12 = (B12 * A11 - B11 * A12) * idet;
  const double C21 = (B21 * A22 - B22 * A21) * idet, C22 = (B22 * A11 - B21 * A12) * idet;
  R.asymmetry = fabs(C12 - C21);
  const double m = 0.5 * (C11 + C22), d = 0.5 * (C11 - C22), o = 0.5 * (C12 + C21);
  const double r = sqrt(d * d + o * o);
  R.kappa1 = m - r;
  R.kappa2 = m + r;
  // the eigenvector of m - r: (-o, d + r) or (r - d, -o), whichever does not cancel
  const bool pos = d >= 0.0;
  double e1 = pos ? -o : r - d, e2 = pos ? d + r : -o;
  const double len = sqrt(e1 * e1 + e2 * e2);
  const bool umbilic = len == 0.0;
  e1 = umbilic ? 1.0 : e1 / len;
  e2 = umbilic ? 0.0 : e2 / len;
#pragma unroll
  for (int q = 0; q < 3; ++q) R.axis[q] = e1 * v1[q] + e2 * v2[q];
}

// ------------------------------------------------------------------------------------------- alignment sensitivities
// art_sensitivities (include/art_hip.h): the same transport differentiates a ray with respect to a rigid motion of one
// element or of the source.  A column is the state (dP, dD, dL) of one degree of freedom, dL the change of the path.
// Element k's surface point at X moves by the field s(X); r_0, r_1, r_2 are the rows of its fwd (major axis,
// normal x major, normal):
//   columns 0..2  shift along r_i              s = r_i              theta = 0
//   columns 3..5  rotation about r_i at pos    s = r_i x (X - pos)  theta = r_i      (per radian)
// At the element that moves, with a = dP + t dD as in step:
//   dt = -n . (a - s(P)) / (n . D),  dQ = a + D dt,  dn = dn_surf(dQ - s(P)) + theta x n   (dn_surf: step's rule)
//   dD' = dD - 2 [(dD . n + D . dn) n + (D . n) dn],  dP' = dQ,  dL += dt
// (the leg's length changes by D . (dQ - dP_prev) = dt, because D . dD = 0).  Every other element is the same with
// s = theta = 0: step plus the path term.  The source's columns: 0..2 shifts along lab x, y, z (dP = e_i), 3..5 tilts
// about them with the points held (dD = e_i x D0).  On the detector (centre C, unit normal nd, rot) the transport onto its
// plane gives dX_lab and dL += dt; (dX, dY) = (rot dX_lab)[0:2].
struct Column {
  double dP[3], dD[3], dL;
};

// What every column of a ray shares at one element: the unit normal and the Hessian in the LAB frame (Hl = fwd^T H fwd:
// h00, h11, h22, h01, h02, h12 -- formed once, so that a column needs no rotation there and back), 1 / |g|, the leg t and
// the two products with the incoming direction
struct Hit {
  double n[3], Hl[6], ig, t, Dn, inD;
};

ART_HD void clear(Column& c) {
#pragma unroll
  for (int q = 0; q < 3; ++q) c.dP[q] = c.dD[q] = 0.0;
  c.dL = 0.0;
}

// column i (0..5) of the source group; D0 the source direction
ART_HD void seed_source(const int i, const double* D0, Column& c) {
  clear(c);
  const int m = i % 3;                                    // (selects: no indexed access to registers)
  const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
  if (i < 3) {
#pragma unroll
    for (int q = 0; q < 3; ++q) c.dP[q] = e[q];
  } else {
    cross(e, D0, c.dD);
  }
}

// column i (0..5) of the element s at the lab point P: the motion field sv = s(P) and the rotation vector th
ART_HD void motion(const Surface& s, const int i, const double* P, double* sv, double* th) {
  const int m = i % 3;
  double r[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) r[q] = m == 0 ? s.fwd[q] : (m == 1 ? s.fwd[3 + q] : s.fwd[6 + q]);
  if (i < 3) {
#pragma unroll
    for (int q = 0; q < 3; ++q) { sv[q] = r[q]; th[q] = 0.0; }
  } else {
    const double rel[3] = {P[0] - s.pos[0], P[1] - s.pos[1], P[2] - s.pos[2]};
    cross(r, rel, sv);
#pragma unroll
    for (int q = 0; q < 3; ++q) th[q] = r[q];
  }
}

// D the incoming direction, Pprev the previous point, P the hit point, all lab frame (the first lines of step)
ART_HD void hit_of(const Surface& s, const double* D, const double* Pprev, const double* P, Hit& h) {
  const double rel[3] = {P[0] - s.pos[0], P[1] - s.pos[1], P[2] - s.pos[2]};
  double Po[3], g[3], no[3];
  rot(s.fwd, rel, Po);
  Po[0] += s.centre[0]; Po[1] += s.centre[1]; Po[2] += s.centre[2];
  gradient(s, Po, g);
  h.ig = 1.0 / sqrt(dot(g, g));
  no[0] = -g[0] * h.ig; no[1] = -g[1] * h.ig; no[2] = -g[2] * h.ig;
  rot_t(s.fwd, no, h.n);
  // Hl_ab = f_a . H f_b with f_a the columns of fwd (the lab axes seen in the optic frame)
  double Hf[3][3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const double f[3] = {s.fwd[b], s.fwd[3 + b], s.fwd[6 + b]};
    hessian_apply(s, Po, f, Hf[b]);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int a = k < 3 ? k : (k == 5 ? 1 : 0), b = k < 3 ? k : (k == 3 ? 1 : 2);
    h.Hl[k] = s.fwd[a] * Hf[b][0] + s.fwd[3 + a] * Hf[b][1] + s.fwd[6 + a] * Hf[b][2];
  }
  const double leg[3] = {P[0] - Pprev[0], P[1] - Pprev[1], P[2] - Pprev[2]};
  h.t = dot(leg, D);
  h.Dn = dot(D, h.n);
  h.inD = 1.0 / h.Dn;
}

// One column through an element; kMoves: the element moves by (sv, th) = motion(...), else both are ignored
template <bool kMoves>
ART_HD void step_column(const Surface& s, const Hit& h, const double* D, const double* sv, const double* th, Column& c) {
  double a[3], v[3], dQ[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a[q] = c.dP[q] + h.t * c.dD[q];
    v[q] = kMoves ? a[q] - sv[q] : a[q];
  }
  const double dt = -dot(h.n, v) * h.inD;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    dQ[q] = a[q] + D[q] * dt;
    v[q] = kMoves ? dQ[q] - sv[q] : dQ[q];
  }
  if (!s.mask) {
    const double Hv[3] = {h.Hl[0] * v[0] + h.Hl[3] * v[1] + h.Hl[4] * v[2], h.Hl[3] * v[0] + h.Hl[1] * v[1] + h.Hl[5] * v[2],
                          h.Hl[4] * v[0] + h.Hl[5] * v[1] + h.Hl[2] * v[2]};
    const double nHv = dot(h.n, Hv);
    double dn[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) dn[q] = -(Hv[q] - h.n[q] * nHv) * h.ig;
    if (kMoves) {
      double tn[3];
      cross(th, h.n, tn);
#pragma unroll
      for (int q = 0; q < 3; ++q) dn[q] += tn[q];
    }
    const double k = dot(c.dD, h.n) + dot(D, dn);
#pragma unroll
    for (int q = 0; q < 3; ++q) c.dD[q] -= 2.0 * (k * h.n[q] + h.Dn * dn[q]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) c.dP[q] = dQ[q];
  c.dL += dt;
}

// One column through the element that moves by (sv, th) = motion(...)
ART_HD void step_moved(const Surface& s, const Hit& h, const double* D, const double* sv, const double* th, Column& c) {
  step_column<true>(s, h, D, sv, th, c);
}

// One column through an element that stays: step's rule plus the path term
ART_HD void step_path(const Surface& s, const Hit& h, const double* D, Column& c) {
  step_column<false>(s, h, D, nullptr, nullptr, c);
}

// Behind the last element: D the final direction, P the last hit point, the detector (centre C, unit normal nd, rot).
// dX, dY: the change of the detector coordinates; c.dL gains the last leg's term; c.dP becomes dX_lab, c.dD stays dD'.
ART_HD void readout_column(const double* D, const double* P, const double* C, const double* nd, const double* rotm,
                           Column& c, double& dX, double& dY) {
  const double toC[3] = {C[0] - P[0], C[1] - P[1], C[2] - P[2]};
  const double inD = 1.0 / dot(nd, D), t = dot(nd, toC) * inD;
  double a[3], r[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) a[q] = c.dP[q] + t * c.dD[q];
  const double dt = -dot(nd, a) * inD;
#pragma unroll
  for (int q = 0; q < 3; ++q) c.dP[q] = a[q] + D[q] * dt;
  c.dL += dt;
  rot(rotm, c.dP, r);
  dX = r[0];
  dY = r[1];
}

// ------------------------------------------------------------------------------------------- compensator sums
// art_alignment_sums (include/art_hip.h) carries a CHOSEN handful of the columns above in one lane.  A column id is
// art_sensitivities' c = 6 g + i, or -1 (ART_ALIGN_DOF_DETECTOR): the detector shifted along its normal by u with
// Detector.shiftByDistance's sign, C' = C - u nd.  That column is closed form, dP = dD = 0 up to the read-out: the hit
// moves along the ray by -u / (nd . D), so about the moved centre
//   dX_lab = nd - D / (nd . D),  dL = -1 / (nd . D)        (exactly linear in u)
ART_HD void detector_column(const double* D, const double* nd, const double* rotm, Column& c, double& dX, double& dY) {
  const double inD = 1.0 / dot(nd, D);
  double r[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    c.dP[q] = nd[q] - D[q] * inD;
    c.dD[q] = 0.0;
  }
  c.dL = -inD;
  rot(rotm, c.dP, r);
  dX = r[0];
  dY = r[1];
}

// the group of a column id: 0 the source, g >= 1 element g - 1, -1 the detector
ART_HD int dof_group(const int id) { return id < 0 ? -1 : id / 6; }

// the first element a lane that carries column `id` has to visit (K: none, the last view alone serves the detector)
ART_HD int dof_first(const int id, const int K) {
  const int g = dof_group(id);
  return g < 0 ? K : (g ? g - 1 : 0);
}

// column `id` at the source view (D0: the source direction there; read only by a source column)
ART_HD void seed_selected(const int id, const double* D0, Column& c) {
  clear(c);
  if (dof_group(id) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k)                  // (a constant column per branch, as in step_selected)
      if (id == k) seed_source(k, D0, c);
  }
}

// column `id` through element e (its surface s, the hit h at the lab point P): it moves there, it passes (the source or
// an earlier element moved), or it is still clear (a later element, the detector) and stays so
ART_HD void step_selected(const Surface& s, const Hit& h, const double* D, const double* P, const int id, const int e,
                          Column& c) {
  const int g = dof_group(id);
  if (g == e + 1) {
    double sv[3], th[3];
    const int i = id % 6;
#pragma unroll
    for (int k = 0; k < 6; ++k)                  // (a constant column per branch: no indexed access to the surface)
      if (i == k) motion(s, k, P, sv, th);
    step_moved(s, h, D, sv, th, c);
  } else if (g >= 0 && g <= e) {
    step_path(s, h, D, c);
  }
}

ART_HD void readout_selected(const int id, const double* D, const double* P, const double* C, const double* nd,
                             const double* rotm, Column& c, double& dX, double& dY) {
  if (id < 0) detector_column(D, nd, rotm, c, dX, dY);
  else readout_column(D, P, C, nd, rotm, c, dX, dY);
}

}  // namespace artt

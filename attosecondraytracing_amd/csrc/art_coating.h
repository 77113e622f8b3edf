// art_coating.h -- the per-ray math of art_polarisation (include/art_hip.h): the reflection coefficients rs, rp of a
// coated mirror (Fresnel interfaces with Nevot-Croce roughness, Parratt's recursion from the substrate up) and the 3x3
// polarisation ray-tracing step E' = rs (E.s) s + rp (E.p_in) p_out.
//
// Conventions: time dependence exp(-i w t); N = n + i kappa with kappa >= 0; kz_j = k sqrt(N_j^2 - sin^2 t)
// on the branch Im kz_j >= 0, formed from cos t as k sqrt((n - 1)(n + 1) - kappa^2 + cos^2 t + 2 i n kappa), vacuum k cos t
// (never from sin^2 t = 1 - cos^2 t, which at a grazing angle g loses log10(1 / g^2) digits); medium 0 is vacuum,
// layers 1..L run top down, L + 1 is the substrate;
//   r^s_{j,j+1} = (kz_j - kz_{j+1}) / (kz_j + kz_{j+1})
//   r^p_{j,j+1} = (N_{j+1}^2 kz_j - N_j^2 kz_{j+1}) / (N_{j+1}^2 kz_j + N_j^2 kz_{j+1})
//   each times exp(-2 kz_j kz_{j+1} sigma_{j,j+1}^2) where the interface has a roughness sigma;
//   R_{L+1} = 0,  R_j = (r_{j,j+1} + R_{j+1} X_{j+1}) / (1 + r_{j,j+1} R_{j+1} X_{j+1}),  X_{j+1} = exp(2 i kz_{j+1} t_{j+1});
//   rs = R^s_0, rp = R^p_0.  At normal incidence rp = -rs; the ideal coating (perfect conductor) is rs = -1, rp = +1.
// A coating names at most ART_COATING_MAX_MATERIALS materials and its layers refer to them by index, so kz -- the
// complex square root that depends only on the material and the angle -- is formed once per material and ray; a
// 40-period Mo/Si stack costs two square roots, then one Parratt step per layer.  The material table is wave-uniform
// (scalar loads); the kz of a layer's material is read back from a per-lane table (LDS in the kernel).
#pragma once

#include <math.h>

#include "../../include/art_hip.h"

#ifndef ART_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define ART_HD __host__ __device__ __forceinline__
#else
#define ART_HD inline
#endif
#endif

namespace artc {

struct cplx {
  double re, im;
};
ART_HD cplx cmk(const double re, const double im) { cplx c; c.re = re; c.im = im; return c; }
ART_HD cplx cadd(const cplx a, const cplx b) { return cmk(a.re + b.re, a.im + b.im); }
ART_HD cplx csub(const cplx a, const cplx b) { return cmk(a.re - b.re, a.im - b.im); }
ART_HD cplx cmul(const cplx a, const cplx b) { return cmk(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
ART_HD cplx cscale(const cplx a, const double s) { return cmk(a.re * s, a.im * s); }
// a / b, scaled by the larger component of b (Smith's method, branch-free: selects and one reciprocal)
ART_HD cplx cdiv(const cplx a, const cplx b) {
  const bool big = fabs(b.re) >= fabs(b.im);
  const double p = big ? b.re : b.im, q = big ? b.im : b.re;
  const double x = big ? a.re : a.im, y = big ? a.im : a.re;
  const double r = q / p, inv = 1.0 / (p + q * r);
  const double im = (y - x * r) * inv;
  return cmk((x + y * r) * inv, big ? im : -im);
}
// sin x, cos x: Cody-Waite reduction by pi/2 with FMAs (pi/2 = P1 + P2 to 2^-107; accurate while |x| / (pi/2) is an
// exact integer in a double, |x| < 2^50) and fdlibm's kernel polynomials on [-pi/4, pi/4], branch-free.  The library
// sincos carries a Payne-Hanek path for huge arguments that costs the kernel ~30 registers; phases here are small.
ART_HD void sincos_cw(const double x, double& sn, double& cs) {
  const double n = rint(x * 0.6366197723675814);
  double r = fma(-n, 1.5707963267948966, x);
  r = fma(-n, 6.123233995736766e-17, r);
  const double z = r * r;
  const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                    z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
  const double s = r + r * z * ps;
  const double pc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                    z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double c = w + (((1.0 - w) - hz) + z * pc);
  const int q = (int)(long long)n & 3;
  const double a = (q & 1) ? c : s, b = (q & 1) ? s : c;   // sin, cos of r + q pi/2
  sn = (q & 2) ? -a : a;
  cs = ((q + 1) & 2) ? -b : b;
}
// e^x: reduction by ln 2 with FMAs, |r| <= ln 2 / 2, Taylor polynomial to r^13 (truncation < 5e-18), ldexp; for the
// arguments met here (|x| < 700).  The library exp costs the kernel ~18 registers more.
ART_HD double exp_cw(const double x) {
  const double n = rint(x * 1.4426950408889634);
  double r = fma(-n, 0.6931471805599453, x);
  r = fma(-n, 2.3190468138462996e-17, r);
  double p = 1.6059043836821613e-10;
  p = fma(p, r, 2.08767569878681e-09);
  p = fma(p, r, 2.505210838544172e-08);
  p = fma(p, r, 2.755731922398589e-07);
  p = fma(p, r, 2.7557319223985893e-06);
  p = fma(p, r, 2.48015873015873e-05);
  p = fma(p, r, 0.0001984126984126984);
  p = fma(p, r, 0.001388888888888889);
  p = fma(p, r, 0.008333333333333333);
  p = fma(p, r, 0.041666666666666664);
  p = fma(p, r, 0.16666666666666666);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)fmax(-2100.0, fmin(2100.0, n)));
}
ART_HD cplx cexp(const cplx a) {
  const double m = exp_cw(a.re);
  double s, c;
  sincos_cw(a.im, s, c);
  return cmk(m * c, m * s);
}
// the square root w of z with Im w >= 0 (the decaying / outgoing branch of kz)
ART_HD cplx csqrt_up(const cplx z) {
  const double m = sqrt(z.re * z.re + z.im * z.im);
  const double t = sqrt(0.5 * (m + fabs(z.re)));
  if (t == 0.0) return cmk(0.0, 0.0);
  if (z.re >= 0.0) {
    const double u = z.im / (2.0 * t);          // w = +-(t, u): the sign that makes Im w >= 0
    return z.im >= 0.0 ? cmk(t, u) : cmk(-t, -u);
  }
  return cmk(z.im / (2.0 * t), t);              // Re z < 0: |Im w| = t, Re w = Im z / (2 Im w)
}
ART_HD cplx eps_of(const ArtCoatingMaterial& m) { return cmk(m.n * m.n - m.kappa * m.kappa, 2.0 * m.n * m.kappa); }
// (kz / k)^2 = N^2 - 1 + cos^2 t, with N^2 - 1 as (n - 1)(n + 1) - kappa^2: no cancellation for n near 1 or small cos t
ART_HD cplx kz2_of(const ArtCoatingMaterial& m, const double ct) {
  return cmk((m.n - 1.0) * (m.n + 1.0) - m.kappa * m.kappa + ct * ct, 2.0 * m.n * m.kappa);
}

// kz / k of every material of a coating, into kz[m * stride]: the caller's per-lane table (the kernel keeps it in LDS,
// one column per lane, so a wave-uniform material index is one read; no selects).  Vacuum (index -1) is formed where used.
// The `_at` forms take the optical constants from `mats` (n_materials entries) in place of c.materials: a dispersive
// coating is one ArtCoating (layers, thicknesses, roughnesses) and one material table per frequency.
ART_HD void kz_table_at(const ArtCoating& c, const ArtCoatingMaterial* mats, const double ct, cplx* kz, const int stride) {
  for (int m = 0; m < c.n_materials; ++m) kz[m * stride] = csqrt_up(kz2_of(mats[m], ct));
}
ART_HD void kz_table(const ArtCoating& c, const double ct, cplx* kz, const int stride) {
  kz_table_at(c, c.materials, ct, kz, stride);
}
ART_HD cplx kz_of(const cplx* kz, const int stride, const int m, const double ct) {
  return m < 0 ? cmk(ct, 0.0) : kz[m * stride];     // (vacuum: kz / k = cos t >= 0)
}
ART_HD cplx eps_pick_at(const ArtCoatingMaterial* mats, const int m) {
  return m < 0 ? cmk(1.0, 0.0) : eps_of(mats[m]);
}
ART_HD cplx eps_pick(const ArtCoating& c, const int m) { return eps_pick_at(c.materials, m); }

// the interface between material slots a (above) and b (below); qa, qb = kz / k; sigk = k sigma (dimensionless)
ART_HD void interface_rs_rp(const cplx qa, const cplx qb, const cplx ea, const cplx eb, const double sigk, cplx& rs,
                            cplx& rp) {
  rs = cdiv(csub(qa, qb), cadd(qa, qb));
  const cplx pa = cmul(eb, qa), pb = cmul(ea, qb);
  rp = cdiv(csub(pa, pb), cadd(pa, pb));
  if (sigk > 0.0) {
    const cplx f = cexp(cscale(cmul(qa, qb), -2.0 * sigk * sigk));
    rs = cmul(rs, f);
    rp = cmul(rp, f);
  }
}

// rs, rp of coating c with the optical constants `mats` at cos t = ct, wave number k (1/mm).  Everything is done in
// units of k: kz / k, k t, k sigma.  ct (and the frame of prt_step) belong to the ray and the element, not to k: a
// caller that runs many frequencies forms them once and calls this per frequency with that frequency's k and mats.
ART_HD void coating_rs_rp_at(const ArtCoating& c, const ArtCoatingMaterial* mats, const double ct, const double k,
                             cplx* kz, const int stride, cplx& rs, cplx& rp) {
  if (c.ideal) {
    rs = cmk(-1.0, 0.0);
    rp = cmk(1.0, 0.0);
    return;
  }
  kz_table_at(c, mats, ct, kz, stride);
  const int L = c.n_layers;
  int mb = c.substrate;
  int ma = L > 0 ? c.layers[L - 1].material : -1;
  cplx qb = kz_of(kz, stride, mb, ct);
  cplx qa = kz_of(kz, stride, ma, ct);
  interface_rs_rp(qa, qb, eps_pick_at(mats, ma), eps_pick_at(mats, mb), k * c.roughness, rs, rp);
#pragma unroll 1
  for (int l = L - 1; l >= 0; --l) {
    const ArtCoatingLayer& ly = c.layers[l];
    mb = ma;
    qb = qa;
    ma = l > 0 ? c.layers[l - 1].material : -1;
    qa = kz_of(kz, stride, ma, ct);
    cplx r_s, r_p;
    interface_rs_rp(qa, qb, eps_pick_at(mats, ma), eps_pick_at(mats, mb), k * ly.roughness, r_s, r_p);
    const double kt = 2.0 * k * ly.thickness;
    const cplx X = cexp(cmk(-qb.im * kt, qb.re * kt));
    const cplx Xs = cmul(rs, X), Xp = cmul(rp, X);
    rs = cdiv(cadd(r_s, Xs), cadd(cmk(1.0, 0.0), cmul(r_s, Xs)));
    rp = cdiv(cadd(r_p, Xp), cadd(cmk(1.0, 0.0), cmul(r_p, Xp)));
  }
}
// the same with the coating's own (constant) optical constants
ART_HD void coating_rs_rp(const ArtCoating& c, const double ct, const double k, cplx* kz, const int stride, cplx& rs,
                          cplx& rp) {
  coating_rs_rp_at(c, c.materials, ct, k, kz, stride, rs, rp);
}

// normalize(d x a), a the lab axis of d's smallest |component| (the first of equals): a unit vector perpendicular to d
ART_HD void perp_unit(const double dx, const double dy, const double dz, double& sx, double& sy, double& sz) {
  const double ax = fabs(dx), ay = fabs(dy), az = fabs(dz);
  // d x ex = (0, dz, -dy), d x ey = (-dz, 0, dx), d x ez = (dy, -dx, 0)
  if (ax <= ay && ax <= az) { sx = 0.0; sy = dz; sz = -dy; }
  else if (ay <= az) { sx = -dz; sy = 0.0; sz = dx; }
  else { sx = dy; sy = -dx; sz = 0.0; }
  const double r = 1.0 / sqrt(sx * sx + sy * sy + sz * sz);
  sx *= r; sy *= r; sz *= r;
}

// cos t of the reflection from a to b: |b - a| / 2 (accurate to a few ulp at any angle, grazing included)
ART_HD double cos_incidence(const double* a, const double* b) {
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
  return 0.5 * sqrt(ux * ux + uy * uy + uz * uz);
}
// The reflection frame of one element: s, p_in, p_out from the unit directions before (a) and after (b)
struct Frame {
  double s[3], pi[3], po[3];
};
ART_HD void reflection_frame(const double* a, const double* b, Frame& f) {
  double sx = a[1] * b[2] - a[2] * b[1], sy = a[2] * b[0] - a[0] * b[2], sz = a[0] * b[1] - a[1] * b[0];
  const double m = sqrt(sx * sx + sy * sy + sz * sz);
  if (m < 1e-12) {
    perp_unit(a[0], a[1], a[2], sx, sy, sz);
  } else {
    const double r = 1.0 / m;
    sx *= r; sy *= r; sz *= r;
  }
  f.s[0] = sx; f.s[1] = sy; f.s[2] = sz;
  f.pi[0] = a[1] * sz - a[2] * sy; f.pi[1] = a[2] * sx - a[0] * sz; f.pi[2] = a[0] * sy - a[1] * sx;
  f.po[0] = b[1] * sz - b[2] * sy; f.po[1] = b[2] * sx - b[0] * sz; f.po[2] = b[0] * sy - b[1] * sx;
}

// E' = rs (E.s) s + rp (E.p_in) p_out, E complex (re[3], im[3]), bilinear dot products
ART_HD void prt_step(const Frame& f, const cplx rs, const cplx rp, double* er, double* ei) {
  const cplx es = cmk(er[0] * f.s[0] + er[1] * f.s[1] + er[2] * f.s[2], ei[0] * f.s[0] + ei[1] * f.s[1] + ei[2] * f.s[2]);
  const cplx ep = cmk(er[0] * f.pi[0] + er[1] * f.pi[1] + er[2] * f.pi[2],
                      ei[0] * f.pi[0] + ei[1] * f.pi[1] + ei[2] * f.pi[2]);
  const cplx a = cmul(rs, es), b = cmul(rp, ep);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    er[q] = a.re * f.s[q] + b.re * f.po[q];
    ei[q] = a.im * f.s[q] + b.im * f.po[q];
  }
}

// The polarised input state of a ray: E0 = P - (P.d) d over its norm (P = pol: re x, im x, re y, im y, re z, im z; d the
// source direction).  Returns |P - (P.d) d| (0: P is parallel to d and E0 is not finite).
ART_HD double transverse_state(const double* P, const double* d, double* er, double* ei) {
  const double pr = P[0] * d[0] + P[2] * d[1] + P[4] * d[2], pi = P[1] * d[0] + P[3] * d[1] + P[5] * d[2];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    er[q] = P[2 * q] - pr * d[q];
    ei[q] = P[2 * q + 1] - pi * d[q];
  }
  const double m = sqrt(er[0] * er[0] + er[1] * er[1] + er[2] * er[2] + ei[0] * ei[0] + ei[1] * ei[1] + ei[2] * ei[2]);
#pragma unroll
  for (int q = 0; q < 3; ++q) { er[q] /= m; ei[q] /= m; }
  return m;
}

}  // namespace artc

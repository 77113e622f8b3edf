// Test stub (tests/test_vector_pulse_host.py compiles it with g++ into a shared object of its own): the per-ray,
// per-frequency math of art_focal_vector_spectrum from csrc/art_coating.h, organised as the header means it to be used
// at many frequencies -- the frame and cos t of every element are formed once per ray, then every frequency runs the
// chain with its own k and material table.
#include "../attosecondraytracing_amd/csrc/art_coating.h"

extern "C" {

// rs, rp of one coating for n (a, b) direction pairs at nk frequencies: out_rs, out_rp [n][nk][2].
// mats: [nk][ART_COATING_MAX_MATERIALS]
void vps_rs_rp(const ArtCoating* c, const ArtCoatingMaterial* mats, const double* k, int nk, const double* A,
               const double* B, int n, double* out_rs, double* out_rp) {
  artc::cplx kz[ART_COATING_MAX_MATERIALS];
  for (int i = 0; i < n; ++i) {
    const double ct = artc::cos_incidence(A + 3 * i, B + 3 * i);        // once per ray and element
    for (int j = 0; j < nk; ++j) {
      artc::cplx rs, rp;
      artc::coating_rs_rp_at(*c, mats + (long)j * ART_COATING_MAX_MATERIALS, ct, k[j], kz, 1, rs, rp);
      double* o = out_rs + 2 * ((long)i * nk + j);
      o[0] = rs.re; o[1] = rs.im;
      o = out_rp + 2 * ((long)i * nk + j);
      o[0] = rp.re; o[1] = rp.im;
    }
  }
}

// One ray through a chain of K elements at nk frequencies.  dirs: [K + 1][3]; coating[e]: index into coats or -1;
// mats: [nk][n_coatings][ART_COATING_MAX_MATERIALS]; pol: re x, im x, ...; out: [nk][3][2] (lab-frame field, re, im).
int vps_ray(const ArtCoating* coats, const ArtCoatingMaterial* mats, int n_coatings, const int* coating, int K,
            const double* dirs, const double* pol, const double* k, int nk, double* out) {
  if (K > ART_POLARISATION_MAX_ELEMS) return -1;
  static thread_local artc::Frame frames[ART_POLARISATION_MAX_ELEMS];
  double ct[ART_POLARISATION_MAX_ELEMS];
  for (int e = 0; e < K; ++e) {
    if (coating[e] < 0) continue;
    ct[e] = artc::cos_incidence(dirs + 3 * e, dirs + 3 * e + 3);
    artc::reflection_frame(dirs + 3 * e, dirs + 3 * e + 3, frames[e]);
  }
  artc::cplx kz[ART_COATING_MAX_MATERIALS];
  for (int j = 0; j < nk; ++j) {
    double er[3], ei[3];
    artc::transverse_state(pol, dirs, er, ei);
    for (int e = 0; e < K; ++e) {
      const int c = coating[e];
      if (c < 0) continue;
      artc::cplx rs, rp;
      artc::coating_rs_rp_at(coats[c], mats + ((long)j * n_coatings + c) * ART_COATING_MAX_MATERIALS, ct[e], k[j], kz, 1,
                             rs, rp);
      artc::prt_step(frames[e], rs, rp, er, ei);
    }
    for (int q = 0; q < 3; ++q) { out[6 * j + 2 * q] = er[q]; out[6 * j + 2 * q + 1] = ei[q]; }
  }
  return 0;
}

}  // extern "C"

// art_quantile.h -- the kernels of art_quantiles (include/art_hip.h): exact weighted quantiles by a most-significant-digit
// radix select, rank sums at given thresholds, and the staging of detector metrics as keys.
//
// A key is one fp64 value per slot and plane, mapped to an order-preserving uint64 (key_bits: -0 becomes +0, then the
// sign bit of a non-negative value is set and a negative value is complemented); a NaN key makes the slot invalid.  The
// weight of a slot is art_histogram's fixed-point integer q = (int64) rint(ldexp(w, wshift)) (1 without weights; a
// negative q counts as 0), and every sum below is a sum of such integers: integer atomics in LDS and in global memory,
// integer folds, so the result is the same bytes whatever the grid, the order of arrival or the plane blocking.
//
// Select: six passes over the keys, digits of 9, 11, 11, 11, 11, 11 bits from the top.  Pass p histograms digit p of
// the slots whose higher digits equal the prefix a (plane, fraction) pair has chosen so far (k_select_hist: the bins in
// LDS, flushed with one global atomic per non-zero bin), then k_select_pick walks the 2048 bins to the digit that holds
// the residual target, keeps the sum below it and clears the bins.  Fractions of one plane that still share their prefix
// share one histogram (the `leader` of a fraction is the first fraction with its prefix: in pass 0 all of them; at a
// tight focus most of them down to the last digits), so a slot costs one LDS atomic per pass, not one per fraction.
// Within a wave the slots that go to the bin of the wave's first active lane are summed across the wave first and added
// by that one lane: at a focus, where nearly all keys share their leading digits, a wave makes one LDS atomic instead of
// 64 to the same address.  Nothing is read back between the passes: the state lives in device memory.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/art_hip.h"
#include "art_device.h"

namespace artq {

typedef unsigned long long u64;

constexpr int kBlock = 256;
constexpr int kPasses = 6;
constexpr int kBins = 2048;           // bins of one digit (pass 0 uses the first 512)
constexpr int kGroups = 4;            // prefixes per select launch: 4 x 2048 x 8 B = 64 KiB of LDS at most
constexpr int kSelBlocks = 768;       // persistent grid per plane, 3 workgroups per CU: each zeroes and flushes its bins once
constexpr int kUnroll = 8;            // slots per thread and iteration, their loads requested up front
constexpr int kMomBlocks = 1024;      // partials per plane of the centroid sums (4 workgroups per CU)
constexpr int kMomPlanes = 4;         // planes per workgroup of the centroid sums (accumulators in registers)
constexpr int kMomSlots = 5;

__host__ __device__ constexpr int digit_shift(const int pass) { return 55 - 11 * pass; }
__host__ __device__ constexpr int digit_bits(const int pass) { return pass == 0 ? 9 : 11; }

// per (plane, fraction), 40 bytes
struct SelState {
  u64 prefix;          // the digits chosen so far, in place; lower bits 0
  long long T;         // the residual target: 1 <= T <= the sum of q over the slots that match the prefix
  long long below;     // sum of q over the keys below every key that matches the prefix
  long long upto;      // after the last pass: below + the sum of q over the slots whose key IS the result
  int32_t leader;      // the first fraction of this plane with the same prefix
  int32_t reserved;
};

__host__ __device__ __forceinline__ u64 key_bits(double v) {
  if (v == 0.0) v = 0.0;                                       // -0 -> +0
  u64 b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double key_value(const u64 u) {
  const u64 b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

template <typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
  typedef const T __attribute__((address_space(1)))* gptr_t;
  return __builtin_nontemporal_load((gptr_t)p);
}

// the fixed-point weight of a slot that counts (art_histogram's rule; a negative weight counts as 0)
__device__ __forceinline__ u64 fixed_weight(const double w, const int wshift) {
  const long long q = (long long)rint(ldexp(w, wshift));
  return q > 0 ? (u64)q : 0ull;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// bins[bin] += q for the lanes with bin >= 0: the lanes that share the bin of the first such lane are summed across the
// wave and added by that lane alone; the others add for themselves
__device__ __forceinline__ void wave_add(u64* bins, const int bin, const u64 q) {
  const u64 act = __ballot(bin >= 0);
  if (act == 0ull) return;
  const int lead = __ffsll((long long)act) - 1;
  const int lb = __shfl(bin, lead, 64);
  const bool same = bin == lb;
  const u64 s = wave_sum(same ? q : 0ull);
  if ((int)(threadIdx.x & 63) == lead) atomicAdd(&bins[lb], s);
  else if (!same && bin >= 0) atomicAdd(&bins[bin], q);
}

__global__ __launch_bounds__(kBlock) void k_select_init(SelState* st, const int count) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < count) {
    SelState s;
    s.prefix = 0ull; s.T = 0; s.below = 0; s.upto = 0; s.leader = 0; s.reserved = 0;
    st[i] = s;
  }
}

// One pass of the select for the fractions [k0, k0 + G) of the planes of a block.  grid (x, planes of the block).
// keys [planes][n] (plane stride n), alive [n] or NULL, w [n] or NULL; state [planes][K]; hist [planes][K][kBins];
// counts [planes][2] (valid, invalid slots: pass 0, k0 = 0 only).
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_select_hist(const double* keys, const uint8_t* alive, const double* w,
                                                        const int64_t n, const int wshift, const int pass, const int K,
                                                        const int k0, const SelState* state, u64* hist, u64* counts) {
  extern __shared__ u64 s_bins[];                       // [G][kBins]
  const int plane = blockIdx.y;
  const int G = (K - k0) < kGroups ? (K - k0) : kGroups;
  u64 pref[kGroups];
  bool lead[kGroups];
  bool any = false;
#pragma unroll
  for (int g = 0; g < kGroups; ++g) {
    const bool in = g < G;
    const SelState* s = state + (int64_t)plane * K + k0 + (in ? g : 0);
    lead[g] = in && (FIRST ? (k0 + g == 0) : (s->leader == k0 + g && s->T > 0));
    pref[g] = FIRST ? 0ull : s->prefix;
    any = any || lead[g];
  }
  if (!any) return;                                     // (uniform: every fraction of this launch follows a leader elsewhere)
  for (int i = threadIdx.x; i < G * kBins; i += kBlock) s_bins[i] = 0ull;
  __syncthreads();
  const int sh = digit_shift(pass), hs = sh + digit_bits(pass);
  const unsigned mask = (1u << digit_bits(pass)) - 1u;
  const double* kp = keys + (int64_t)plane * n;
  unsigned n_valid = 0, n_invalid = 0;
  constexpr int kU = FIRST ? kUnroll / 2 : kUnroll;     // (pass 0 also counts the slots: eight slots' lane masks would spill SGPRs)
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int lane = threadIdx.x & 63;                    // (the trip count is the wave's: wave_add talks across all 64 lanes)
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 - lane < n; i0 += kU * stride) {
    double kv[kU], wv[kU];
    uint8_t al[kU];                                  // (the flags stay in VGPRs: eight lane masks would crowd the SGPRs)
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t i = i0 + u * stride, c = i < n ? i : n - 1;
      kv[u] = ld_stream(kp + c);
      wv[u] = w ? ld_stream(w + c) : 1.0;
      al[u] = alive ? ld_stream(alive + c) : (uint8_t)1;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool live = (i0 + u * stride < n) && al[u] != 0;
      const bool nan = kv[u] != kv[u];
      const bool valid = live && !nan;
      if (FIRST) {
        n_valid += valid ? 1u : 0u;
        n_invalid += (live && nan) ? 1u : 0u;
      }
      const u64 q = fixed_weight(valid ? wv[u] : 0.0, wshift);       // (a dead slot's weight is unspecified: selected away)
      const u64 uk = key_bits(kv[u]);
      int g_of = -1;
#pragma unroll
      for (int g = 0; g < kGroups; ++g) {
        const bool m = FIRST ? true : ((uk >> hs) == (pref[g] >> hs));
        g_of = (lead[g] && m) ? g : g_of;                              // (leaders have distinct prefixes: at most one matches)
      }
      const int bin = (valid && q != 0ull && g_of >= 0) ? g_of * kBins + (int)((unsigned)(uk >> sh) & mask) : -1;
      wave_add(s_bins, bin, q);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < G * kBins; i += kBlock) {
    const u64 v = s_bins[i];
    if (v != 0ull) atomicAdd(&hist[((int64_t)plane * K + k0 + i / kBins) * kBins + (i % kBins)], v);
  }
  if (FIRST) {
    const u64 a = wave_sum((u64)n_valid), b = wave_sum((u64)n_invalid);
    if ((threadIdx.x & 63) == 0) {
      if (a) atomicAdd(&counts[2 * plane], a);
      if (b) atomicAdd(&counts[2 * plane + 1], b);
    }
  }
}

struct PickArg {
  double fraction[ART_QUANTILE_MAX_FRACTIONS];
};

// The digit of every fraction of one plane (grid: the planes of a block, one workgroup each); clears the plane's bins.
// After the last pass the results are written: values / below / upto [planes][K], totals [planes][3] = (W, valid slots,
// invalid slots).  root: the value is the square root of the key (the RADIUS metric).
__global__ __launch_bounds__(kBlock) void k_select_pick(SelState* state, u64* hist, const u64* counts, const int K,
                                                        const int pass, const PickArg fr, const int root, double* values,
                                                        long long* below, long long* upto, long long* totals) {
  __shared__ u64 s_scan[kBlock];
  __shared__ u64 s_found[3];                 // digit, the sum below it inside the prefix, the bin itself
  __shared__ SelState s_new[ART_QUANTILE_MAX_FRACTIONS];
  __shared__ long long s_W;
  const int plane = blockIdx.x, t = threadIdx.x;
  constexpr int kPer = kBins / kBlock;       // 8 bins per thread
  for (int j = 0; j < K; ++j) {
    const SelState cur = state[(int64_t)plane * K + j];
    const int L = pass == 0 ? 0 : cur.leader;
    const u64* h = hist + ((int64_t)plane * K + L) * kBins;
    u64 loc[kPer], sum = 0ull;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { loc[k] = h[t * kPer + k]; sum += loc[k]; }
    s_scan[t] = sum;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {                   // inclusive scan
      const u64 add = t >= off ? s_scan[t - off] : 0ull;
      __syncthreads();
      s_scan[t] += add;
      __syncthreads();
    }
    if (pass == 0 && j == 0 && t == kBlock - 1) s_W = (long long)s_scan[t];
    if (t == 0) s_found[0] = ~0ull;
    __syncthreads();
    long long T = cur.T;
    if (pass == 0) {
      const long long W = s_W;
      const double want = ceil(fr.fraction[j] * (double)W);         // (one product: nothing to contract)
      long long c = (long long)want;
      c = c < 1 ? 1 : c;
      T = W < c ? W : c;                                            // W == 0: T = 0, no digit is found
    }
    const u64 incl = s_scan[t], excl = incl - sum;
    if (T > 0 && excl < (u64)T && (u64)T <= incl) {                 // one thread at most
      u64 run = excl;
      int d = 0;
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const bool here = run < (u64)T && (u64)T <= run + loc[k];
        if (here) { d = k; s_found[1] = run; s_found[2] = loc[k]; }
        run += loc[k];
      }
      s_found[0] = (u64)(t * kPer + d);
    }
    __syncthreads();
    if (t == 0) {
      SelState nw = cur;
      if (pass == 0) { nw.prefix = 0ull; nw.below = 0; }
      nw.T = T;
      if (s_found[0] != ~0ull) {
        nw.prefix |= s_found[0] << digit_shift(pass);
        nw.T = T - (long long)s_found[1];
        nw.below += (long long)s_found[1];
        nw.upto = nw.below + (long long)s_found[2];
      } else {
        nw.T = 0; nw.below = 0; nw.upto = 0;
      }
      s_new[j] = nw;
    }
    __syncthreads();
  }
  if (t < K) {
    SelState nw = s_new[t];
    int L = t;
    for (int i = t - 1; i >= 0; --i) L = (s_new[i].prefix == nw.prefix && (s_new[i].T > 0) == (nw.T > 0)) ? i : L;
    nw.leader = L;
    state[(int64_t)plane * K + t] = nw;
    if (pass == kPasses - 1) {
      const bool has = nw.T > 0;
      const double v = key_value(nw.prefix);
      values[(int64_t)plane * K + t] = has ? (root ? sqrt(v) : v) : NAN;
      below[(int64_t)plane * K + t] = has ? nw.below : 0;
      upto[(int64_t)plane * K + t] = has ? nw.upto : 0;
    }
  }
  if (pass == 0 && t == 0) {
    totals[3 * plane] = s_W;
    totals[3 * plane + 1] = (long long)counts[2 * plane];
    totals[3 * plane + 2] = (long long)counts[2 * plane + 1];
  }
  for (int i = t; i < K * kBins; i += kBlock) hist[(int64_t)plane * K * kBins + i] = 0ull;
}

// Rank sums: for every threshold of a plane (sorted ascending, [planes][R]) the sum of q and the number of valid slots
// whose key (root: its square root) is <= the threshold.  One pass: a slot adds to the bin of the FIRST threshold that is
// >= its key (bin R: above all of them), k_rank_finish forms the running sums.  bins [planes][2][R + 1], zero on entry.
__global__ __launch_bounds__(kBlock) void k_rank_bins(const double* keys, const uint8_t* alive, const double* w,
                                                      const int64_t n, const int wshift, const int R, const int root,
                                                      const double* thresholds, u64* bins) {
  __shared__ double s_thr[ART_QUANTILE_MAX_THRESHOLDS];
  __shared__ u64 s_bins[2 * (ART_QUANTILE_MAX_THRESHOLDS + 1)];
  const int plane = blockIdx.y;
  for (int i = threadIdx.x; i < R; i += kBlock) s_thr[i] = thresholds[(int64_t)plane * R + i];
  for (int i = threadIdx.x; i < 2 * (R + 1); i += kBlock) s_bins[i] = 0ull;
  __syncthreads();
  const double* kp = keys + (int64_t)plane * n;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int lane = threadIdx.x & 63;                    // (the trip count is the wave's: wave_add talks across all 64 lanes)
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 - lane < n; i0 += kUnroll * stride) {
    double kv[kUnroll], wv[kUnroll];
    uint8_t al[kUnroll];                                  // (the flags stay in VGPRs: eight lane masks would crowd the SGPRs)
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t i = i0 + u * stride, c = i < n ? i : n - 1;
      kv[u] = ld_stream(kp + c);
      wv[u] = w ? ld_stream(w + c) : 1.0;
      al[u] = alive ? ld_stream(alive + c) : (uint8_t)1;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const bool valid = (i0 + u * stride < n) && al[u] != 0 && kv[u] == kv[u];
      const u64 q = fixed_weight(valid ? wv[u] : 0.0, wshift);
      const double v = root ? sqrt(kv[u]) : kv[u];
      int lo = 0, hi = R;                                   // the first threshold >= v
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_thr[mid] >= v) hi = mid; else lo = mid + 1;
      }
      wave_add(s_bins, valid ? lo : -1, q);
      wave_add(s_bins + (R + 1), valid ? lo : -1, 1ull);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * (R + 1); i += kBlock) {
    const u64 v = s_bins[i];
    if (v != 0ull) atomicAdd(&bins[(int64_t)plane * 2 * (R + 1) + i], v);
  }
}

__global__ __launch_bounds__(64) void k_rank_finish(const u64* bins, const int R, long long* sums, long long* counts) {
  const int plane = blockIdx.x;
  if (threadIdx.x != 0) return;
  const u64* b = bins + (int64_t)plane * 2 * (R + 1);
  u64 s = 0ull, c = 0ull;
  for (int r = 0; r < R; ++r) {
    s += b[r];
    c += b[R + 1 + r];
    sums[(int64_t)plane * R + r] = (long long)s;
    counts[(int64_t)plane * R + r] = (long long)c;
  }
}

// ------------------------------------------------------------------------------------------- detector metrics
// Plane p of a call is the detector moved to centre + shift[p] * normal: a detector of its own, read with detector_ray
// like every other read-out, so that X, Y and the path are the values Detector.get_PointList2D and get_OpticalPaths give
// on a detector moved there.  centres [planes][4] in device memory: cx, cy, c (fs), and the path (mm) the delays are
// measured from.
struct PlaneArg {
  ArtDetectorDesc det;                               // rot and normal; the centre of plane p is pc[p]
  double pc[ART_FOCAL_MAX_PLANES][3];
};

__device__ __forceinline__ ArtDetectorDesc plane_detector(const PlaneArg& a, const int p) {
  ArtDetectorDesc d = a.det;
  d.centre[0] = a.pc[p][0]; d.centre[1] = a.pc[p][1]; d.centre[2] = a.pc[p][2];
  return d;
}

__device__ __forceinline__ double delay_fs(const double opl, const double zero) {
  return ((opl - zero) / 299792458000.0) * 1e15;     // Detector.get_Delays' expression
}

__device__ __forceinline__ art::Ray load_ray(const ArtBundleView& b, const int64_t c) {
  art::Ray r;
  r.ox = ld_stream(b.ox + c); r.oy = ld_stream(b.oy + c); r.oz = ld_stream(b.oz + c);
  r.dx = ld_stream(b.dx + c); r.dy = ld_stream(b.dy + c); r.dz = ld_stream(b.dz + c);
  r.path = ld_stream(b.path + c);
  return r;
}

// Centroid sums of kMomPlanes planes per workgroup (grid: (kMomBlocks or fewer, ceil(planes / kMomPlanes))).
// stage 0: per plane [0] alive slots [1] sum opl [2] sum w [3] sum w X [4] sum w Y;
// stage 1: [2] sum w [3] sum w delay, the delay measured from centres[p][3].  partials [planes][gridDim.x][kMomSlots].
__global__ __launch_bounds__(kBlock) void k_metric_moments(const PlaneArg a, const int planes, const int stage,
                                                           const ArtBundleView b, const double* w, const int64_t n,
                                                           const double* centres, double* partials) {
  __shared__ double s_red[kBlock / 64][kMomPlanes * kMomSlots];
  const int p0 = blockIdx.y * kMomPlanes;
  double acc[kMomPlanes][kMomSlots];
  double zero[kMomPlanes];
#pragma unroll
  for (int j = 0; j < kMomPlanes; ++j) {
#pragma unroll
    for (int k = 0; k < kMomSlots; ++k) acc[j][k] = 0.0;
    zero[j] = (stage == 1 && p0 + j < planes) ? centres[4 * (p0 + j) + 3] : 0.0;
  }
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const bool live = ld_stream(b.alive + i) != 0;
    const art::Ray r = load_ray(b, i);
    const double wi = live ? (w ? ld_stream(w + i) : 1.0) : 0.0;
#pragma unroll
    for (int j = 0; j < kMomPlanes; ++j) {
      if (p0 + j < planes) {
        double Ix, Iy, Iz, X, Y, o;
        art::detector_ray(plane_detector(a, p0 + j), r, Ix, Iy, Iz, X, Y, o);
        if (stage == 0) {
          acc[j][0] += live ? 1.0 : 0.0;
          acc[j][1] += live ? o : 0.0;
          acc[j][2] += wi;
          acc[j][3] += live ? wi * X : 0.0;
          acc[j][4] += live ? wi * Y : 0.0;
        } else {
          acc[j][2] += wi;
          acc[j][3] += live ? wi * delay_fs(o, zero[j]) : 0.0;
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kMomPlanes; ++j)
#pragma unroll
    for (int k = 0; k < kMomSlots; ++k) {
      double v = acc[j][k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) s_red[wv][j * kMomSlots + k] = v;
    }
  __syncthreads();
  if (threadIdx.x < kMomPlanes * kMomSlots) {
    const int j = threadIdx.x / kMomSlots, k = threadIdx.x % kMomSlots;
    if (p0 + j < planes) {
      double v = s_red[0][threadIdx.x];
      for (int q = 1; q < kBlock / 64; ++q) v += s_red[q][threadIdx.x];
      partials[((int64_t)(p0 + j) * gridDim.x + blockIdx.x) * kMomSlots + k] = v;
    }
  }
}

struct CentreArg {
  double c[ART_FOCAL_MAX_PLANES][3];                 // the caller's centres (cx, cy, c in fs), read where `given`
};

// One workgroup of 64 lanes per plane folds the nb partials in a fixed order and writes the plane's centres.
// stage 0: [3] = the mean path; [0], [1] = the weighted centroid or the caller's; stage 1: [2] = the weighted mean delay.
// A given centre of stage 1 is written by stage 0 already.
__global__ __launch_bounds__(64) void k_metric_centres(const double* partials, const int nb, const int stage, const int given,
                                                       const CentreArg ca, double* centres) {
  const int plane = blockIdx.x, lane = threadIdx.x;
  double acc[kMomSlots];
#pragma unroll
  for (int k = 0; k < kMomSlots; ++k) {
    double v = 0.0;
    for (int q = lane; q < nb; q += 64) v += partials[((int64_t)plane * nb + q) * kMomSlots + k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    acc[k] = v;
  }
  if (lane != 0) return;
  double* c = centres + 4 * plane;
  if (stage == 0) {
    c[0] = given ? ca.c[plane][0] : acc[3] / acc[2];
    c[1] = given ? ca.c[plane][1] : acc[4] / acc[2];
    c[2] = given ? ca.c[plane][2] : 0.0;
    c[3] = acc[1] / acc[0];
  } else {
    c[2] = acc[3] / acc[2];
  }
}

// the caller's centres without any sum (X, Y, RADIUS with given centres)
__global__ __launch_bounds__(64) void k_metric_centres_given(const CentreArg ca, const int planes, double* centres) {
  const int p = threadIdx.x;
  if (p < planes) {
    centres[4 * p] = ca.c[p][0]; centres[4 * p + 1] = ca.c[p][1]; centres[4 * p + 2] = ca.c[p][2]; centres[4 * p + 3] = 0.0;
  }
}

// The keys of the planes [p0, p0 + pb) of every slot, keys [pb][n]: one read of the bundle per block of planes.
//   RADIUS (X - cx)^2 + (Y - cy)^2    X |X - cx|    Y |Y - cy|    DELAY |delay_fs - c|
// A dead slot's key is NaN (it is skipped by its alive flag, not by its key).
__global__ __launch_bounds__(kBlock) void k_stage_keys(const PlaneArg a, const int metric, const int p0, const int pb,
                                                       const ArtBundleView b, const int64_t n, const double* centres,
                                                       double* keys) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const bool live = ld_stream(b.alive + i) != 0;
    const art::Ray r = load_ray(b, i);
    for (int j = 0; j < pb; ++j) {
      const double* c = centres + 4 * (p0 + j);
      double Ix, Iy, Iz, X, Y, o;
      art::detector_ray(plane_detector(a, p0 + j), r, Ix, Iy, Iz, X, Y, o);
      const double ex = X - c[0], ey = Y - c[1];
      double key;
      if (metric == ART_QKEY_RADIUS) key = ex * ex + ey * ey;
      else if (metric == ART_QKEY_X) key = fabs(ex);
      else if (metric == ART_QKEY_Y) key = fabs(ey);
      else key = fabs(delay_fs(o, c[3]) - c[2]);
      __builtin_nontemporal_store(live ? key : (double)NAN, keys + (int64_t)j * n + i);
    }
  }
}

}  // namespace artq

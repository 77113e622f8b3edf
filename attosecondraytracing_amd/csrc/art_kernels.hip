// art_kernels.hip -- gfx950 kernels + the C ABI of libart_hip.so (include/art_hip.h).
//
// One ray per lane, SoA fp64 streams read and written with coalesced, non-temporal 8-byte accesses (64 lanes x
// 8 B = 512 B per wave instruction and per array; 16 B per lane in the read-out), element descriptors in kernel
// arguments or in a device-resident scene table (either way scalar loads -> SGPRs, broadcast for free), Zernike
// coefficient tables read through the scalar cache as well (wave-uniform; -DART_ZERN_LDS stages them in LDS instead),
// wavefront ballot on the torus Newton loop.  No MFMA: the path is streaming fp64 VALU work against HBM.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "art_device.h"
#include "art_coating.h"
#include "art_tubes.h"
#include "art_quantile.h"
#include "art_scene.h"

// The -DART_ZERN_LDS comparison build keeps a persistent grid whose last pass may leave part of a workgroup idle: no
// workgroup barriers there, i.e. the 8-byte store path.
#if defined(ART_ZERN_LDS) && !defined(ART_STORE_DIRECT)
#define ART_STORE_DIRECT 1
#endif

namespace {

constexpr int kBlock = 256;          // 4 waves per workgroup
constexpr int kMaxBlocks = 256 * 8;  // reductions: 256 CUs x 8 workgroups, grid-stride beyond that (one partial each)
constexpr int kReadoutBlocks = kMaxBlocks;  // fused read-out: persistent workgroups -- every workgroup ends with a 24-slot
                                           // reduction, so MORE workgroups cost more (16384: 244 us instead of 176 us)

thread_local char g_err[512] = "";

int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
int fail_hip(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return ART_ERR_HIP;
}

// The two trace kernels get one workgroup per 256 rays, NOT a persistent grid with a grid-stride loop: measured on
// relay4, 1e7 rays, the fused kernel takes 0.686 ms with 2048 workgroups and 0.653 ms with 39063 (per-element kernel
// 0.243 -> 0.222 ms; at 1e8 rays 7.33 -> 6.35 ms).  Consecutive workgroups then sweep every stream linearly (DRAM
// pages, TLB), and the hardware's workgroup dispatch hides latency at least as well as a software prefetch did.
// It is not a general rule (all per 1e7 rays, launches back to back): the bundle transform also gains (263 -> 226 us),
// the source generator (plain stores behind heavy trigonometry) loses (138 -> 158 us) and the fused read-out loses
// (every workgroup ends in a 24-slot reduction), so those keep the persistent grid_for().
inline int grid_stream(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > (int64_t)1 << 22) b = (int64_t)1 << 22;   // 2^28 rays per launch at most: never reached
  return (int)b;
}

// Workgroup -> tile mapping of the streaming kernels (`xmap`, a kernel argument).  The hardware deals consecutive
// workgroup ids round-robin to the 8 XCDs, so with the identity mapping each XCD's L2 sees every 8th 2-KiB piece of
// every stream.  xmap = k > 0 hands each XCD runs of 2^(k-1) CONSECUTIVE tiles instead (groups of 8 * 2^(k-1) tiles are
// shared out among the XCDs); xmap < 0 gives every XCD one contiguous eighth of the launch; 0 = identity.  The grid is
// rounded up to a whole number of groups (grid_stream_mapped); tiles beyond the bundle fall outside every buffer
// descriptor and do nothing.  Measured in DESIGN.md 5 (round 2).
__device__ __forceinline__ int64_t tile_of(const unsigned b, const unsigned nb, const int xmap) {
  if (xmap == 0) return b;
  if (xmap < 0) return (int64_t)(b & 7u) * (nb >> 3) + (b >> 3);
  const unsigned sh = (unsigned)(xmap - 1), span_sh = sh + 3u;
  const unsigned r = b & ((1u << span_sh) - 1u);
  return (int64_t)(((b >> span_sh) << span_sh) + ((r & 7u) << sh) + (r >> 3));
}

// ART_XCD_MAP: "0" identity (default: no mapping measured faster than run-to-run noise), "-1" eighths, "k" runs of
// 2^(k-1) tiles per XCD
inline int xcd_map() {
  static const int v = [] {
    const char* e = getenv("ART_XCD_MAP");
    const int x = e ? atoi(e) : 0;
    return (x < -1 || x > 8) ? 0 : x;     // runs of at most 128 tiles: the grid is rounded up by < 1024 workgroups
  }();
  return v;
}

inline int grid_stream_mapped(int64_t n, int xmap) {
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  const int64_t span = (xmap == 0) ? 1 : (xmap < 0 ? 8 : ((int64_t)8 << (xmap - 1)));
  b = (b + span - 1) / span * span;
  return (int)b;   // <= 2^20 + span workgroups for 2^28 rays
}

inline int grid_for(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}

// ---- buffer-resource access -----------------------------------------------------------------------------
// Every stream is addressed through a 128-bit buffer descriptor (base, byte count) with the per-lane byte offset
// in a 32-bit VGPR.  The hardware range check gives branch-free predication: a lane whose offset is out of range
// loads 0 / stores nothing.  That is what lets dead rays skip their 8 output stores WITHOUT a branch around the
// stores -- a branch would make the compiler drain every outstanding store (s_waitcnt vmcnt(0)) at the join, between
// the elements of a chain -- and the tail of a launch (slots >= n) needs no branch either.  One launch covers at most 2^28 rays (32-bit byte offsets); the C ABI splits
// larger bundles into several launches.
typedef int v2i32 __attribute__((ext_vector_type(2)));
// Cache-policy bits of the buffer instructions (gfx942/gfx950 aux operand: 1 = sc0, 2 = nt, 16 = sc1).  Every ray
// stream is touched exactly once per kernel, so both directions are marked non-temporal: measured on relay4
// (bench.py, 1e7 rays) 0.937 -> 0.874 ms per step against the default policy; sc0/sc1 combinations made no further
// difference.  The macros exist so that the experiment can be repeated (-DART_LD_AUX=0 -DART_ST_AUX=0).
#ifndef ART_LD_AUX
#define ART_LD_AUX 2
#endif
#ifndef ART_ST_AUX
#define ART_ST_AUX 2
#endif
constexpr int64_t kMaxRaysPerLaunchHw = (int64_t)1 << 28;  // 2^28 rays * 8 B = 2 GiB per stream
// Offset of a store that must be dropped by the range check: 2^31.  num_records never exceeds 2^31 (2^28 rays x 8 B), so
// it is out of range for every descriptor; it is 16-byte aligned, and the component offsets of a 16-byte store (+4, +8,
// +12) cannot wrap around 2^32 into the first slots of the stream (0xFFFFFFFF, used before, relied on that not happening).
constexpr unsigned kDropOffset = 0x80000000u;

struct BundleRsrc {
  __amdgpu_buffer_rsrc_t ox, oy, oz, dx, dy, dz, path, inc, alive;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)bytes, 0x00020000);
}
// descriptors of the n slots [first, first + n) of a view
__device__ __forceinline__ BundleRsrc make_rsrc(const ArtBundleView& v, int64_t n, int64_t first = 0) {
  const unsigned b8 = (unsigned)(n * 8), b1 = (unsigned)n;
  BundleRsrc r;
  r.ox = rsrc_of(v.ox + first, b8); r.oy = rsrc_of(v.oy + first, b8); r.oz = rsrc_of(v.oz + first, b8);
  r.dx = rsrc_of(v.dx + first, b8); r.dy = rsrc_of(v.dy + first, b8); r.dz = rsrc_of(v.dz + first, b8);
  r.path = rsrc_of(v.path + first, b8); r.inc = rsrc_of(v.incidence + first, b8);
  r.alive = rsrc_of(v.alive + first, b1);
  return r;
}
__device__ __forceinline__ double ld_f64(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  const v2i32 d = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, ART_LD_AUX);
  double v;
  __builtin_memcpy(&v, &d, 8);
  return v;
}
__device__ __forceinline__ void st_f64(__amdgpu_buffer_rsrc_t rs, unsigned off, double v) {
  v2i32 d;
  __builtin_memcpy(&d, &v, 8);
  __builtin_amdgcn_raw_buffer_store_b64(d, rs, (int)off, 0, ART_ST_AUX);
}
typedef int v4i32 __attribute__((ext_vector_type(4)));
struct D2 { double a, b; };
__device__ __forceinline__ D2 ld_2f64(__amdgpu_buffer_rsrc_t rs, unsigned off) {   // 16 B per lane: two consecutive slots
  const v4i32 d = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, ART_LD_AUX);
  D2 v;
  __builtin_memcpy(&v, &d, 16);
  return v;
}
__device__ __forceinline__ void st_2f64(__amdgpu_buffer_rsrc_t rs, unsigned off, double a, double b) {
  D2 v = {a, b};
  v4i32 d;
  __builtin_memcpy(&d, &v, 16);
  __builtin_amdgcn_raw_buffer_store_b128(d, rs, (int)off, 0, ART_ST_AUX);
}

// slot index -> byte offsets; out-of-range slots (i >= n) fall outside every descriptor automatically
__device__ __forceinline__ void load_slot(const BundleRsrc& b, int64_t i, art::Ray& r, uint8_t& alive) {
  const unsigned o1 = (unsigned)i, o8 = o1 * 8u;
  alive = __builtin_amdgcn_raw_buffer_load_b8(b.alive, (int)o1, 0, ART_LD_AUX);
  r.ox = ld_f64(b.ox, o8); r.oy = ld_f64(b.oy, o8); r.oz = ld_f64(b.oz, o8);
  r.dx = ld_f64(b.dx, o8); r.dy = ld_f64(b.dy, o8); r.dz = ld_f64(b.dz, o8);
  r.path = ld_f64(b.path, o8);
}
// The same loads with the DEFAULT cache policy: for an input that other workgroups are about to read again (the shared
// input of a chain-interleaved scene launch) -- a non-temporal load does not leave its line in the caches.
__device__ __forceinline__ double ld_f64_keep(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  const v2i32 d = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0);
  double v;
  __builtin_memcpy(&v, &d, 8);
  return v;
}
__device__ __forceinline__ D2 ld_2f64_keep(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  const v4i32 d = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
  D2 v;
  __builtin_memcpy(&v, &d, 16);
  return v;
}
__device__ __forceinline__ void load_slot_keep(const BundleRsrc& b, int64_t i, art::Ray& r, uint8_t& alive) {
  const unsigned o1 = (unsigned)i, o8 = o1 * 8u;
  alive = __builtin_amdgcn_raw_buffer_load_b8(b.alive, (int)o1, 0, 0);
  r.ox = ld_f64_keep(b.ox, o8); r.oy = ld_f64_keep(b.oy, o8); r.oz = ld_f64_keep(b.oz, o8);
  r.dx = ld_f64_keep(b.dx, o8); r.dy = ld_f64_keep(b.dy, o8); r.dz = ld_f64_keep(b.dz, o8);
  r.path = ld_f64_keep(b.path, o8);
}
__device__ __forceinline__ void store_slot(const BundleRsrc& b, int64_t i, const art::Ray& r, bool ok) {
  const unsigned o1 = (unsigned)i;
#ifdef ART_DIAG_NOSTORE   // timing-only build: keep the compute, drop the 8 data stores (results are wrong)
  const unsigned o8 = (ok && r.path == -1.2345e300) ? o1 * 8u : kDropOffset;
#else
  const unsigned o8 = ok ? o1 * 8u : kDropOffset;  // dead rays: the range check drops the 8 stores
#endif
  st_f64(b.ox, o8, r.ox); st_f64(b.oy, o8, r.oy); st_f64(b.oz, o8, r.oz);
  st_f64(b.dx, o8, r.dx); st_f64(b.dy, o8, r.dy); st_f64(b.dz, o8, r.dz);
  st_f64(b.path, o8, r.path);
  st_f64(b.inc, o8, r.inc);
#ifdef ART_DIAG_NOALIVE   // timing-only build: slots >= 4096 get no alive store (results of large bundles are wrong)
  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(ok ? 1 : 0), b.alive, o1 < 4096u ? (int)o1 : (int)kDropOffset, 0, ART_ST_AUX);
#else
  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(ok ? 1 : 0), b.alive, (int)o1, 0, ART_ST_AUX);
#endif
}

// plain-pointer access for the small kernels (detector, sources)
__device__ __forceinline__ void load_ray(const ArtBundleView& v, int64_t i, art::Ray& r) {
  r.ox = v.ox[i]; r.oy = v.oy[i]; r.oz = v.oz[i];
  r.dx = v.dx[i]; r.dy = v.dy[i]; r.dz = v.dz[i];
  r.path = v.path[i];
}
__device__ __forceinline__ void store_ray(const ArtBundleView& v, int64_t i, const art::Ray& r) {
  v.ox[i] = r.ox; v.oy[i] = r.oy; v.oz[i] = r.oz;
  v.dx[i] = r.dx; v.dy[i] = r.dy; v.dz[i] = r.dz;
  v.path[i] = r.path;
  v.incidence[i] = r.inc;
}

// ---- masked streaming reads of the reduction kernels -------------------------------------------------------------------
// A reduction over the alive rays used to read `alive[i]`, branch, and only then load the slot's data: two dependent memory
// latencies per iteration and ONE iteration's loads in flight per lane (0.42-0.63 of the rate the trace kernels reach,
// profiles/r04_relay4.md).  Now every stream of kU grid-stride iterations is requested UNCONDITIONALLY and up front
// (non-temporal: each byte is used once), and `alive` is applied by SELECTS when the values are folded: 4 x 9 loads in
// flight per lane, no divergent skip.  A lane beyond the end re-reads slot n - 1 (a valid address, a cache hit) and folds
// nothing.  The values of a dead slot are unspecified by contract (possibly NaN): they are dropped by the select, never
// multiplied by 0.  The fold ORDER is unchanged: lane t of workgroup b still folds slots b*256 + t + k*stride for
// k = 0, 1, ... one after the other, so the results are the bits they were.
// MASKED bundles (a third of C3's slots are dead, in one contiguous range): these loops read the dead slots' streams too.
// The two kernels of the loop-list analysis, where that matters (k_analysis_sums, k_analysis_moments), request a slot's
// data at an out-of-range buffer offset when it is dead -- no traffic -- with the alive byte fetched one slot ahead.
// (the pointer is stated to be GLOBAL memory: one that was itself fetched from a table in memory -- a job's bundle view --
// would otherwise be a generic pointer and compile to flat_load, which also occupies the LDS counter)
template <typename T>
__device__ __forceinline__ T ld_nt(const T* p) {
  typedef const T __attribute__((address_space(1)))* gptr_t;
  return __builtin_nontemporal_load((gptr_t)p);
}
template <typename T>
__device__ __forceinline__ void st_nt(T* p, const T v) {
  typedef T __attribute__((address_space(1)))* gptr_t;
  __builtin_nontemporal_store(v, (gptr_t)p);
}
constexpr int kRedUnroll = 4;
// ------------------------------------------------------------------------------------------- reductions
// Deterministic: fixed grid, each lane accumulates its grid-stride slice, wave shuffle tree, LDS across the
// 4 waves, one partial per workgroup into `scratch`, then k_fold_partials: one workgroup per statistic folds the
// partials in a fixed order (fold_range).
constexpr int kRedBlocks = 1024;
inline int red_blocks(int64_t n) {   // workgroups of a reduction over n slots: one per 256, between 1 and kRedBlocks
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kRedBlocks ? kRedBlocks : b));
}
constexpr int kRedSlots = 16;       // art_detector_stats
constexpr int kReadoutSlots = 24;   // art_detector_readout / fused chain read-out statistics
constexpr int kUsedSlots = 22;      // slots 22, 23 are reserved (always 0): the fused tail writes no partials for them
constexpr int kSumSlots = 8;        // art_bundle_sums, art_detector_moments
constexpr int kScanSlots = 33;      // art_detector_scan_moments
constexpr int kMaxSlots = 2;        // the max pair: largest angle to the axis, largest distance from the origin

enum RedOp { RSUM = 0, RMIN = 1, RMAX = 2 };

__device__ __forceinline__ double fold_op(const double a, const double b, const int op_k) {
  return (op_k == RSUM) ? a + b : (op_k == RMIN ? fmin(a, b) : fmax(a, b));
}
constexpr double red_ident(const int op_k) { return (op_k == RSUM) ? 0.0 : (op_k == RMIN ? INFINITY : -INFINITY); }
// The operator of each slot of a layout: a function of the slot, computed where it is used (a run-time indexed local
// array of operators lives in scratch memory).  stat_op: the 24 read-out statistics (art_hip.h, art_detector_readout);
// the 16 of art_detector_stats are its first 16.  The analysis moments have ana_mom_op.
constexpr int stat_op(const int k) {   // minima in slots 2, 4, 12, maxima in 3, 5, 13 (a bit mask each: no branches)
  return ((0x1014 >> k) & 1) ? RMIN : (((0x2028 >> k) & 1) ? RMAX : RSUM);
}
constexpr int sum_op(int) { return RSUM; }   // kSumSlots, kScanSlots
constexpr int max_op(int) { return RMAX; }   // kMaxSlots

__device__ __forceinline__ double wave_reduce(double v, int op) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fold_op(v, __shfl_down(v, off, 64), op);
  return v;
}

// ---- 24 statistics x 64 lanes -> 24 wave totals, for the fused read-out tail (once per wave of 64 rays, so it has to
// be cheap: 24 shuffle trees through ds_bpermute cost more than tracing the rays, 24 DPP prefix trees still +50 %).
// Transpose through a wave-private LDS tile instead: in three passes of 8 statistics every lane parks its 8 values
// ([stat][lane], conflict-free), then lane l folds 8 of the 64 values of statistic l/8 (stride-8 reads) and the 8
// lanes of a statistic finish with a 3-step DPP butterfly (quad_perm xor 1, xor 2, row_half_mirror).  ~100
// instructions per lane instead of ~900; no barrier (same-wave LDS operations are ordered), no VMEM.
template <int CTRL>
__device__ __forceinline__ double dpp_xchg(const double v) {
  int2 s, r;
  __builtin_memcpy(&s, &v, 8);
  // every lane has a source under these controls: no "old" value to preserve (bound_ctrl), so no copy before the move
  r.x = __builtin_amdgcn_update_dpp(0, s.x, CTRL, 0xf, 0xf, true);
  r.y = __builtin_amdgcn_update_dpp(0, s.y, CTRL, 0xf, 0xf, true);
  double d;
  __builtin_memcpy(&d, &r, 8);
  return d;
}
// fmin() on values that come out of LDS compiles to v_max(x, x) (quieting a signalling NaN) + v_min: the bare
// instruction does the same fold in one
__device__ __forceinline__ double min_raw(const double a, const double b) {
  double d;
  asm("v_min_f64 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
constexpr int kTileStride = 72;   // doubles per statistic row of the tile (64 + padding against bank conflicts)
// Which statistic sits where: passes 0 and 1 carry the 16 sums, pass 2 the minima and -- negated, max(x) = -min(-x) --
// the maxima, so that every pass folds with ONE compile-time operator (a per-lane operator compiles to branches).
// Entries >= 24 are padding.
constexpr int kPassSlot[3][8] = {{0, 1, 6, 7, 8, 9, 10, 11}, {16, 17, 18, 19, 20, 21, 14, 15},
                                 {2, 4, 12, 3, 5, 13, 24, 24}};
// The per-wave partials go to the scratch area in THIS order (row = pass * 8 + j, rows 22 and 23 unused), so that the
// tail's three stores need no slot look-up; the fold kernels translate (row_of_slot).
constexpr int row_of_slot(const int slot) {
  for (int p = 0; p < 3; ++p)
    for (int j = 0; j < 8; ++j)
      if (kPassSlot[p][j] == slot) return p * 8 + j;
  return -1;
}

// tile: 8 * kTileStride doubles owned by this wave.  After the call, lanes with (lane & 7) == 0 hold in out[pass] the
// wave total of statistic kPassSlot[pass][lane >> 3] (= row pass * 8 + (lane >> 3) of the scratch area).
__device__ __forceinline__ void wave_reduce24(const double (&acc)[kReadoutSlots], double* tile, const int l,
                                              double (&out)[3]) {
  const int stat = l >> 3, part = l & 7;   // l = lane of the wave
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    // The lanes exchange data through the tile: wave-level barriers (no instruction, a scheduling fence for the compiler)
    // keep the stores of a pass in front of its row loads and the row loads in front of the next pass's stores.  The
    // hardware executes a wave's LDS operations in order; this pins the compiler to the same order.
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int g = kPassSlot[pass][j];
      tile[j * kTileStride + l] = (g >= kReadoutSlots) ? INFINITY : ((pass == 2 && j >= 3) ? -acc[g] : acc[g]);
    }
    __builtin_amdgcn_wave_barrier();
    const double* row = tile + stat * kTileStride + part;
    double v = row[0];
    if (pass < 2) {
#pragma unroll
      for (int k = 1; k < 8; ++k) v += row[8 * k];
      v += dpp_xchg<0xB1>(v);    // quad_perm:[1,0,3,2]  lane ^ 1
      v += dpp_xchg<0x4E>(v);    // quad_perm:[2,3,0,1]  lane ^ 2
      v += dpp_xchg<0x141>(v);   // row_half_mirror      lane i <-> 7 - i of its group of 8
    } else {
#pragma unroll
      for (int k = 1; k < 8; ++k) v = min_raw(v, row[8 * k]);
      v = min_raw(v, dpp_xchg<0xB1>(v));
      v = min_raw(v, dpp_xchg<0x4E>(v));
      v = min_raw(v, dpp_xchg<0x141>(v));
      v = (stat >= 3) ? -v : v;  // the maxima were folded as minima of their negatives
    }
    out[pass] = v;
  }
}

// The LITE tail's reduction: the two sums (rows 0, 1 of pass 0) and pass 2 (minima / maxima) of wave_reduce24; out[1] = 0
// and the lanes of pass 0's other rows hold 0, so that the partial statistics written behind it have the full layout.
__device__ __forceinline__ void wave_reduce_lite(const double (&acc)[kReadoutSlots], double* tile, const int l,
                                                 double (&out)[3]) {
  const int stat = l >> 3, part = l & 7;
  __builtin_amdgcn_wave_barrier();
  tile[0 * kTileStride + l] = acc[0];
  tile[1 * kTileStride + l] = acc[1];
  __builtin_amdgcn_wave_barrier();
  {
    const double* row = tile + (stat & 1) * kTileStride + part;
    double v = row[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += row[8 * k];
    v += dpp_xchg<0xB1>(v);
    v += dpp_xchg<0x4E>(v);
    v += dpp_xchg<0x141>(v);
    out[0] = (stat < 2) ? v : 0.0;
  }
  out[1] = 0.0;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int g = kPassSlot[2][j];
    tile[j * kTileStride + l] = (g >= kReadoutSlots) ? INFINITY : ((j >= 3) ? -acc[g] : acc[g]);
  }
  __builtin_amdgcn_wave_barrier();
  {
    const double* row = tile + stat * kTileStride + part;
    double v = row[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v = min_raw(v, row[8 * k]);
    v = min_raw(v, dpp_xchg<0xB1>(v));
    v = min_raw(v, dpp_xchg<0x4E>(v));
    v = min_raw(v, dpp_xchg<0x141>(v));
    out[2] = (stat >= 3) ? -v : v;
  }
}

// ---- the nine sums of the analysis' pass (1): count, sum point (3), sum vector (3), sum w, sum path ---------------------
// ONE canonical fold order, whoever forms them -- the tail of a tracing launch (the ray is still in registers: ArtChainReadout.sums),
// either kernel body, or k_analysis_sums re-reading a bundle: per TILE of 256 consecutive slots, four runs of 64 slots
// are folded by the LDS transpose below (lane l parks its 8 values, folds 8 of the 64 values of sum l/8, then a 3-step
// DPP butterfly), the four run totals are added in slot order, and the per-tile partials (row-major: scratch[row * ntiles
// + tile]) are folded by fold_range.  The count is a popcount of ballots (exact in any order).  So a bundle's sums -- and
// everything the analysis derives from them -- are the same bits whether they rode on the trace or were taken afterwards.
constexpr int kSumRows = 9;
// every lane has parked its values in `tile` rows 0..7 (row j = sum j + 1, column = slot of the run); returns, in all 8 lanes
// of group l >> 3, the run's total of sum (l >> 3) + 1
__device__ __forceinline__ double run_fold8(const double* tile, const int l) {
  const double* row = tile + (l >> 3) * kTileStride + (l & 7);
  double v = row[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) v += row[8 * k];
  v += dpp_xchg<0xB1>(v);
  v += dpp_xchg<0x4E>(v);
  v += dpp_xchg<0x141>(v);
  return v;
}
// one ray per lane, a wave = one run: -> the run's total of sum (l >> 3) + 1
__device__ __forceinline__ double run_sums8(const double (&v)[8], double* tile, const int l) {
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < 8; ++j) tile[j * kTileStride + l] = v[j];
  __builtin_amdgcn_wave_barrier();
  return run_fold8(tile, l);
}
// the masked values of one ray
__device__ __forceinline__ void sums_values(double (&v)[8], const bool live, const art::Ray& r, const double w) {
  v[0] = live ? r.ox : 0.0; v[1] = live ? r.oy : 0.0; v[2] = live ? r.oz : 0.0;
  v[3] = live ? r.dx : 0.0; v[4] = live ? r.dy : 0.0; v[5] = live ? r.dz : 0.0;
  v[6] = live ? w : 0.0; v[7] = live ? r.path : 0.0;
}
// a workgroup of 4 waves = one tile (one ray per lane): run totals -> the tile's partial, row-major in `rows`.
// s_run: 4 x kSumRows doubles of LDS.  Bare s_barrier: __syncthreads() would also wait for the stores in flight.
// Tiles beyond `ntiles` (a grid rounded up by the tile mapping) store nothing.
__device__ __forceinline__ void tile_sums_store(const double tot, const unsigned long long live_mask, double* s_run,
                                                const unsigned t, double* rows, const int64_t ntiles, const int64_t tile) {
  const int l = t & 63, w = t >> 6;
  if ((l & 7) == 0) s_run[w * kSumRows + 1 + (l >> 3)] = tot;
  if (l == 0) s_run[w * kSumRows] = (double)__popcll(live_mask);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (t < kSumRows && tile < ntiles)
    rows[(int64_t)t * ntiles + tile] = ((s_run[t] + s_run[kSumRows + t]) + s_run[2 * kSumRows + t]) + s_run[3 * kSumRows + t];
}
// Two NEIGHBOURING slots per lane (chain_body2): a wave's 128 slots are two runs -- lanes 0..31 hold run A, lanes 32..63
// run B -- and a workgroup's 512 slots two tiles (waves 0, 1 and waves 2, 3).  Same order as above: the values are parked
// in slot order, one run at a time.
__device__ __forceinline__ void run_sums8_pairs(const double (&v0)[8], const double (&v1)[8], double* tile, const int l,
                                                double& totA, double& totB) {
  const int col = 2 * (l & 31);
  __builtin_amdgcn_wave_barrier();
  if (l < 32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { tile[j * kTileStride + col] = v0[j]; tile[j * kTileStride + col + 1] = v1[j]; }
  }
  __builtin_amdgcn_wave_barrier();
  totA = run_fold8(tile, l);
  __builtin_amdgcn_wave_barrier();
  if (l >= 32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { tile[j * kTileStride + col] = v0[j]; tile[j * kTileStride + col + 1] = v1[j]; }
  }
  __builtin_amdgcn_wave_barrier();
  totB = run_fold8(tile, l);
}
// s_run: 8 x kSumRows doubles (the workgroup's eight runs); tiles 2 * pair_tile and 2 * pair_tile + 1
__device__ __forceinline__ void tile_sums_store_pairs(const double totA, const double totB, const unsigned long long m0,
                                                      const unsigned long long m1, double* s_run, const unsigned t,
                                                      double* rows, const int64_t ntiles, const int64_t pair_tile) {
  const int l = t & 63, w = t >> 6;
  if ((l & 7) == 0) {
    s_run[(2 * w) * kSumRows + 1 + (l >> 3)] = totA;
    s_run[(2 * w + 1) * kSumRows + 1 + (l >> 3)] = totB;
  }
  if (l == 0) {
    s_run[(2 * w) * kSumRows] = (double)(__popcll(m0 & 0xffffffffull) + __popcll(m1 & 0xffffffffull));
    s_run[(2 * w + 1) * kSumRows] = (double)(__popcll(m0 >> 32) + __popcll(m1 >> 32));
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  const int h = (int)(t >> 6);            // wave 0 stores the first tile, wave 1 the second
  const int row = (int)(t & 63);
  const int64_t tile = 2 * pair_tile + h;
  if (h < 2 && row < kSumRows && tile < ntiles) {
    const double* q = s_run + 4 * h * kSumRows + row;
    rows[(int64_t)row * ntiles + tile] = ((q[0] + q[kSumRows]) + q[2 * kSumRows]) + q[3 * kSumRows];
  }
}

// A workgroup's partial of each slot (operator op_of(k)) into dst[0 .. NS): wave shuffle trees, then the 4 waves in order
template <int NS, typename F>
__device__ __forceinline__ void block_reduce_store(double (&acc)[NS], F op_of, double* dst) {
  __shared__ double s[kBlock / 64][NS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double v = wave_reduce(acc[k], op_of(k));
    if (lane == 0) s[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int k = threadIdx.x;
    const int op = op_of(k);
    double v = s[0][k];
    for (int j = 1; j < kBlock / 64; ++j) v = fold_op(v, s[j][k], op);
    dst[k] = v;
  }
}

// THE fold of a sequence of partials, row[p * stride] for p in [lo, hi), in one fixed order: thread t takes p = lo + t,
// lo + t + B, lo + t + 2B, ... (B threads), then the wave shuffle tree, then the waves in order.  Every thread of the
// workgroup (a multiple of 64) calls this; thread 0 stores the result.  An empty range leaves the identity of op_k.
// kU: loads in flight per thread before the first is folded (a thread's ~40 values one load at a time are 40 memory
// latencies in a row: 17 us per 1e7 rays, measured); it does not change the order.  B: the workgroup size when the
// caller knows it (a table of per-workgroup partials: fewer than 2^31 of them, so 32-bit indices), 0 = blockDim.x.
// Constant B and stride leave one pointer with immediate offsets per thread instead of a 64-bit address per load.
constexpr int kFoldBlock = 1024;
template <int kU = 8, int B = 0>
__device__ __forceinline__ void fold_range(const double* row, const int64_t lo, const int64_t hi, const int op_k,
                                           double* out, const int64_t stride = 1) {
  using I = typename std::conditional<B == 0, int64_t, int>::type;
  __shared__ double s[(B ? B : kFoldBlock) / 64];
  const double ident = red_ident(op_k);
  double acc = ident;
  for (I p = (I)lo + threadIdx.x; p < (I)hi; p += (I)(B ? B : blockDim.x) * kU) {
    double v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const I q = p + (I)u * (B ? B : blockDim.x);
      v[u] = (q < (I)hi) ? row[(int64_t)q * stride] : ident;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) acc = fold_op(acc, v[u], op_k);
  }
  acc = wave_reduce(acc, op_k);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = s[0];
    for (int j = 1; j < (int)((B ? B : blockDim.x) >> 6); ++j) v = fold_op(v, s[j], op_k);
    *out = v;
  }
}

// Second pass of a standalone reduction: grid (NS), workgroup k folds slot k (operator OP(k)) of the nblocks partials
// [block][NS] in `scratch` into out[k], kU loads in flight per thread.  Zero partials leave the identities.
template <int NS, int kU, int (*OP)(int)>
__global__ __launch_bounds__(kBlock) void k_fold_partials(const double* scratch, const int nblocks, double* out) {
  fold_range<kU, kBlock>(scratch + blockIdx.x, 0, nblocks, OP(blockIdx.x), out + blockIdx.x, NS);
}

// The 24 read-out statistics (layout: art_hip.h, art_detector_readout) of one ray folded into `acc`; dead rays add the
// reduction identities through selects (no divergent skip).
__device__ __forceinline__ void readout_accumulate(double (&acc)[kReadoutSlots], const bool live, const double x,
                                                   const double y, const double o, const double wi, const bool has_w,
                                                   const double cx, const double cy, const double co) {
  const double ww = live ? (has_w ? wi : 1.0) : 0.0, one = live ? 1.0 : 0.0;
  const double xs = live ? x : 0.0, ys = live ? y : 0.0, os = live ? o : 0.0;
  acc[0] += one; acc[1] += os;
  acc[2] = fmin(acc[2], live ? x : INFINITY); acc[3] = fmax(acc[3], live ? x : -INFINITY);
  acc[4] = fmin(acc[4], live ? y : INFINITY); acc[5] = fmax(acc[5], live ? y : -INFINITY);
  acc[6] += xs; acc[7] += ys;
  acc[8] += ww; acc[9] = fma(ww, xs, acc[9]); acc[10] = fma(ww, ys, acc[10]); acc[11] = fma(ww, os, acc[11]);
  acc[12] = fmin(acc[12], live ? o : INFINITY); acc[13] = fmax(acc[13], live ? o : -INFINITY);
  const double ex = live ? x - cx : 0.0, ey = live ? y - cy : 0.0, eo = live ? o - co : 0.0;
  acc[16] = fma(ex, ex, acc[16]); acc[17] = fma(ey, ey, acc[17]); acc[18] = fma(eo, eo, acc[18]);
  acc[19] = fma(ww * ex, ex, acc[19]); acc[20] = fma(ww * ey, ey, acc[20]); acc[21] = fma(ww * eo, eo, acc[21]);
}
// The same for the fused tail, where a lane holds exactly ONE ray: the statistics are assigned, not added to their
// identities (0.0 + x is not x for the compiler: -0.0), which is 14 instructions less per ray.
__device__ __forceinline__ void readout_single(double (&acc)[kReadoutSlots], const bool live, const double x,
                                               const double y, const double o, const double wi, const bool has_w,
                                               const double cx, const double cy, const double co) {
  const double ww = live ? (has_w ? wi : 1.0) : 0.0;
  const double xs = live ? x : 0.0, ys = live ? y : 0.0, os = live ? o : 0.0;
  acc[0] = live ? 1.0 : 0.0; acc[1] = os;
  acc[2] = live ? x : INFINITY; acc[3] = live ? x : -INFINITY;
  acc[4] = live ? y : INFINITY; acc[5] = live ? y : -INFINITY;
  acc[6] = xs; acc[7] = ys;
  acc[8] = ww; acc[9] = ww * xs; acc[10] = ww * ys; acc[11] = ww * os;
  acc[12] = live ? o : INFINITY; acc[13] = live ? o : -INFINITY;
  acc[14] = 0.0; acc[15] = 0.0;
  const double ex = live ? x - cx : 0.0, ey = live ? y - cy : 0.0, eo = live ? o - co : 0.0;
  acc[16] = ex * ex; acc[17] = ey * ey; acc[18] = eo * eo;
  acc[19] = ww * ex * ex; acc[20] = ww * ey * ey; acc[21] = ww * eo * eo;
  acc[22] = 0.0; acc[23] = 0.0;
}
// LITE tail (ArtChainReadout.lite): count, sum of paths, bounding box and path range only -- 8 of the 22 statistics, no
// weights.  The other slots read 0.
__device__ __forceinline__ void readout_single_lite(double (&acc)[kReadoutSlots], const bool live, const double x,
                                                    const double y, const double o) {
  acc[0] = live ? 1.0 : 0.0; acc[1] = live ? o : 0.0;
  acc[2] = live ? x : INFINITY; acc[3] = live ? x : -INFINITY;
  acc[4] = live ? y : INFINITY; acc[5] = live ? y : -INFINITY;
  acc[12] = live ? o : INFINITY; acc[13] = live ? o : -INFINITY;
}
__device__ __forceinline__ void readout_accumulate_lite(double (&acc)[kReadoutSlots], const bool live, const double x,
                                                        const double y, const double o) {
  acc[0] += live ? 1.0 : 0.0; acc[1] += live ? o : 0.0;
  acc[2] = fmin(acc[2], live ? x : INFINITY); acc[3] = fmax(acc[3], live ? x : -INFINITY);
  acc[4] = fmin(acc[4], live ? y : INFINITY); acc[5] = fmax(acc[5], live ? y : -INFINITY);
  acc[12] = fmin(acc[12], live ? o : INFINITY); acc[13] = fmax(acc[13], live ? o : -INFINITY);
}

// ------------------------------------------------------------------------------------------- trace kernels
// The descriptor travels in a one-element array and is indexed with blockIdx.y (always 0): a dynamic index makes the
// compiler fetch descriptor fields with scalar loads where they are used instead of keeping all ~60 of them (plus
// 72 SGPRs of buffer descriptors) live across the ray loop, which overflowed the SGPR file into VGPR lanes (200
// v_readlane/v_writelane in the torus kernel).  The fused chain kernel indexes its descriptors by element anyway.
struct ElemArg {
  ArtElementDesc e[1];
};

#ifdef ART_ZERN_LDS
// Comparison build: the dense Zernike tables are staged in LDS once per workgroup and read by every
// lane from the same address, instead of travelling through the scalar cache.  To amortise the staging these kernels
// keep a persistent grid + loop, as in round 1.
constexpr bool kDefectLoop = true;
__device__ __forceinline__ void stage_tables(const double* src, double* dst, int doubles) {
  for (int j = threadIdx.x; j < doubles; j += kBlock) dst[j] = src[j];
}
#else
constexpr bool kDefectLoop = false;
#endif

// One ray per thread (grid_stream), no loop.  Slots beyond n fall outside every descriptor: their loads return 0
// (alive = 0) and their stores are dropped, so the tail needs no branch.
template <int KIND, bool DEFECT>
__global__ __launch_bounds__(kBlock) void k_trace_element(const ElemArg ea, const ArtBundleView in,
                                                          const ArtBundleView out, const int64_t n, const int xmap) {
  const ArtElementDesc& e = ea.e[blockIdx.y];
  const double* zern = e.zern;
#ifdef ART_ZERN_LDS
  __shared__ double s_zern[DEFECT ? 4 * ART_ZERN_STRIDE : 2];   // (comparison build: at most 4 tables per element)
  if (DEFECT) {
    stage_tables(e.zern, s_zern, e.n_defects * ART_ZERN_STRIDE);
    __syncthreads();
    zern = s_zern;
  }
#endif
  const BundleRsrc bi = make_rsrc(in, n), bo = make_rsrc(out, n);
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  int64_t i = tile_of(blockIdx.x, gridDim.x, xmap) * kBlock + threadIdx.x;
  do {
    art::Ray r;
    r.inc = 0.0;
    uint8_t a;
    load_slot(bi, i, r, a);
    bool ok = a != 0;
#ifdef ART_DIAG_NOCOMPUTE   // timing-only build: memory traffic without the intersection math (results are wrong)
    r.path += e.mp[0];
#else
    if (ok) ok = art::trace_ray<KIND, DEFECT>(e, zern, r);
#endif
    store_slot(bo, i, r, ok);
    i += stride;
  } while (DEFECT && kDefectLoop && i < n);
}

// Elements whose Zernike tables are in the recurrence layout (ART_FLAG_ZERN_RECURRENCE: orders above 16): the
// reference's recurrences per ray, three rotating rows of values and derivatives in per-lane arrays (private memory).
// A kernel of its own, so that the register-resident kernels above stay free of scratch; any optic kind (run-time
// switch), one ray per thread.
__global__ __launch_bounds__(kBlock) void k_trace_element_zrec(const ElemArg ea, const ArtBundleView in,
                                                               const ArtBundleView out, const int64_t n) {
  const ArtElementDesc& e = ea.e[blockIdx.y];
  const BundleRsrc bi = make_rsrc(in, n), bo = make_rsrc(out, n);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  art::Ray r;
  r.inc = 0.0;
  uint8_t a;
  load_slot(bi, i, r, a);
  bool ok = a != 0;
  if (ok) ok = art::trace_ray<ART_KIND_DYN, true, true>(e, e.zern, r);
  store_slot(bo, i, r, ok);
}

// Grating (ART_FLAG_GRATING, art_device.h grating_hit / grating_diffract): one ray per thread, any mirror kind (run-time
// switch, wave-uniform).  The input slot is read ONCE; frame change, intersection, support test and normal are formed
// once; then the thread loops over the nw wavelengths with the hit in registers and stores one diffracted ray each.
// The wavelengths and the output views are the same for every lane: read through the constant address space, i.e.
// scalar loads into SGPRs (one copy per wave).  Stores of lost rays and of slots >= n are dropped by the range check.
__global__ __launch_bounds__(kBlock) void k_trace_grating(const ElemArg ea, const ArtGratingDesc g, const ArtBundleView in,
                                                          const int64_t n) {
  const ArtElementDesc& e = ea.e[blockIdx.y];
  const BundleRsrc bi = make_rsrc(in, n);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned o8 = (unsigned)i * 8u, nb8 = (unsigned)(n * 8);
  art::Ray r;
  r.inc = 0.0;
  uint8_t a;
  load_slot(bi, i, r, a);
  const double g_in = ld_f64(rsrc_of(g.grooves_in, g.grooves_in ? nb8 : 0u), o8);     // NULL: every load reads 0
  art::GratingHit h = {};
  bool hit = a != 0;
  if (hit) hit = art::grating_hit<ART_KIND_DYN>(e, r, g.q[0], g.q[1], g.lines_per_mm, h);
  const double g_out = g_in + (double)g.order * h.G;
  const art::zuni_t wl = ART_ZUNI(g.wavelengths);
  typedef const uint64_t __attribute__((address_space(4)))* uview_t;
  const uview_t vp = (uview_t)(const void*)g.outs;
  static_assert(sizeof(ArtBundleView) == 9 * sizeof(uint64_t), "ArtBundleView is nine pointers");
  for (int j = 0; j < g.nw; ++j) {
    const double sc = (double)g.order * wl[j] * g.lines_per_mm;
    ArtBundleView v;
    v.ox = (double*)vp[9 * j + 0]; v.oy = (double*)vp[9 * j + 1]; v.oz = (double*)vp[9 * j + 2];
    v.dx = (double*)vp[9 * j + 3]; v.dy = (double*)vp[9 * j + 4]; v.dz = (double*)vp[9 * j + 5];
    v.path = (double*)vp[9 * j + 6]; v.incidence = (double*)vp[9 * j + 7]; v.alive = (uint8_t*)vp[9 * j + 8];
    art::Ray o;
    const bool ok = art::grating_diffract(e, h, sc * g.q[0], sc * g.q[1], r.path, o) && hit;
    store_slot(make_rsrc(v, n), i, o, ok);
    double* go = g.grooves_out ? g.grooves_out + (int64_t)j * n : nullptr;
    st_f64(rsrc_of(go, go ? nb8 : 0u), ok ? o8 : kDropOffset, g_out);
  }
}

// General quadric mirror (ART_FLAG_QUADRIC, art_device.h quadric_trace): one ray per thread, no loop, no LDS, no
// barrier.  The ten coefficients arrive in the kernel arguments: wave-uniform, i.e. scalar registers, and every product
// with them takes one as its scalar operand.
__global__ __launch_bounds__(kBlock) void k_trace_quadric(const ElemArg ea, const ArtQuadricDesc q, const ArtBundleView in,
                                                          const ArtBundleView out, const int64_t n) {
  const ArtElementDesc& e = ea.e[blockIdx.y];
  const BundleRsrc bi = make_rsrc(in, n), bo = make_rsrc(out, n);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  art::Ray r;
  r.inc = 0.0;
  uint8_t a;
  load_slot(bi, i, r, a);
  bool ok = a != 0;
  if (ok) ok = art::quadric_trace(e, q, r);
  store_slot(bo, i, r, ok);
}

// Freeform mirror (ART_FLAG_FREEFORM, art_device.h freeform_trace): k_trace_quadric's shape -- one ray per thread, the
// base's ten coefficients in the kernel arguments -- plus the figure's dense table, read through scalar loads inside a
// Newton loop that the whole wave leaves together.  No LDS, no barrier.
// Scalar registers: the loop keeps the ten coefficients, the support and the evaluators' coefficient loads in them; the
// frame map and the nine output addresses, which only the code behind the loop needs, would stay there across it (every
// kernel argument is loaded on entry) and push the allocation over the file.  They are read behind the loop instead,
// through an index (always blockIdx.y == 0) that the compiler cannot see through before the loop has produced t.
struct ViewArg {
  ArtBundleView v[1];
};
__global__ __launch_bounds__(kBlock) void k_trace_freeform(const ElemArg ea, const ArtQuadricDesc q, const double* __restrict__ fig,
                                                           const ArtBundleView in, const ViewArg outs, const int64_t n) {
  const ArtElementDesc& e = ea.e[blockIdx.y];
  const BundleRsrc bi = make_rsrc(in, n);
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  art::Ray r;
  r.inc = 0.0;
  uint8_t a;
  load_slot(bi, i, r, a);
  bool ok = a != 0;
  art::FreeformHit h = {};
  if (ok) ok = art::freeform_hit(e, q, ART_ZUNI(fig), r, h);
  unsigned late = blockIdx.y;
  asm volatile("" : "+s"(late) : "v"(h.t));
  if (ok) art::freeform_reflect(ea.e[late], h, r);
  const BundleRsrc bo = make_rsrc(outs.v[late], n);
  store_slot(bo, i, r, ok);
}

using art::ChainArgs;
using art::kChainMax;

#ifndef ART_STORE_DIRECT
// The 8 fp64 outputs of an element go through LDS so that every wave instruction stores 16 B per lane = 1 KiB of ONE
// stream (wave w owns streams 2w and 2w+1 of the workgroup's 256 rays) instead of 8 B per lane = 512 B: half the store
// instructions per element.  Mid-round, with the kernel bound by arithmetic, this bought nothing; with a quarter of the
// instructions gone it is 4-5 % on relay4 and 11 % on the 8-element C4 chain (tools/r02_exp22.sh; -DART_STORE_DIRECT is
// the 8-byte form).  A PAIR of slots is written when either ray is alive (the dead one's slot receives its last live
// state: unspecified by contract, its alive byte is 0); pairs of dead rays are dropped by the range check, so a masked
// bundle costs the bytes of its survivors, as before.  The two barriers order LDS only (no vmcnt wait: ISA checked).
__device__ __forceinline__ void store_tile_lds4(const ArtBundleView& v, const int64_t n, const int64_t first,
                                                const int64_t tile0, const unsigned t, const art::Ray& r, const bool ok,
                                                double (*s_out)[kBlock], uint8_t* s_al) {
  s_out[0][t] = r.ox; s_out[1][t] = r.oy; s_out[2][t] = r.oz;
  s_out[3][t] = r.dx; s_out[4][t] = r.dy; s_out[5][t] = r.dz;
  s_out[6][t] = r.path; s_out[7][t] = r.inc;
  s_al[t] = (uint8_t)(ok ? 1 : 0);
  const unsigned nb = (unsigned)(v.alive != nullptr ? n : 0);
  __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(ok ? 1 : 0), rsrc_of(v.alive + first, nb), (int)(unsigned)(tile0 + t), 0,
                                       ART_ST_AUX);
  __syncthreads();
  const int w = __builtin_amdgcn_readfirstlane((int)(t >> 6)), l = (int)(t & 63);
  double* const* rows = &v.ox;   // ox, oy, oz, dx, dy, dz, path, incidence are consecutive pointers
  bool keep[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) keep[h] = (s_al[h * 128 + 2 * l] | s_al[h * 128 + 2 * l + 1]) != 0;
#pragma unroll
  for (int js = 0; js < 2; ++js) {
    const int j = 2 * w + js;
    const __amdgpu_buffer_rsrc_t rs = rsrc_of(rows[j] + first, nb * 8u);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int s0 = h * 128 + 2 * l;
      st_2f64(rs, keep[h] ? (unsigned)(tile0 + s0) * 8u : kDropOffset, s_out[j][s0], s_out[j][s0 + 1]);
    }
  }
  __syncthreads();
}
#endif

// End of the fused read-out tail of both bodies.  One partial per WORKGROUP (round 3; per wave before): the four wave totals
// `tot` meet in LDS behind a bare s_barrier -- __syncthreads() would also wait for the acknowledgement of the stores in
// flight -- and threads 0..21 fold them in wave order and store row `thread` (= pass * 8 + stat, row_of_slot) of the scratch
// area.  A quarter of the partials: the fold that follows reads 7.5 MB instead of 30 MB per 1e7 rays and fits ONE launch
// (launch_fold).  `a` is passed by reference and ro.scratch read here: as a pointer argument its scalar load was hoisted
// and the scene kernel gained v_readlane moves.
__device__ __forceinline__ void tail_partial(const ChainArgs& a, const double tot[3], double (*s_part)[kReadoutSlots],
                                             const unsigned lane, const unsigned bx, const unsigned nbx) {
  if ((lane & 7) == 0) {
    const int stat = (lane & 63) >> 3, w = lane >> 6;
    s_part[w][stat] = tot[0];
    s_part[w][8 + stat] = tot[1];
    if (stat < 6) s_part[w][16 + stat] = tot[2];
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#ifdef ART_DIAG_RO_NOSCRATCH  // timing-only build: the fused tail without the partial-statistics stores
  if (tot[0] + tot[1] + tot[2] == -1.2345e300) {
#else
  if (lane < kUsedSlots) {
#endif
    double v = s_part[0][lane];
#pragma unroll
    for (int j = 1; j < kBlock / 64; ++j) {
      const double q = s_part[j][lane];
      v = (lane < 16) ? v + q : (lane < 19 ? fmin(v, q) : fmax(v, q));    // rows 16-18: minima, 19-21: maxima
    }
    a.ro.scratch[(int64_t)lane * nbx + bx] = v;
  }
}

__device__ __forceinline__ double or_bits(const double v, const uint64_t b) {
  return __longlong_as_double(__double_as_longlong(v) | (long long)b);
}

// Whole chain with the ray resident in registers; history written for every element whose view is non-null.
// `a` lives in kernel arguments (k_trace_chain) or in the device-resident scene table (k_trace_scene): either way
// its fields are wave-uniform and fetched by scalar loads where they are used.  Rays [first, first + n) of every view.
// `bx` / `nbx`: this workgroup's index among the launch's tile workgroups and their number -- blockIdx.x / gridDim.x in the
// tile-major launches, blockIdx.y / gridDim.y in the chain-interleaved scene launch (k_trace_scene, `transposed`).
// KIND1 >= 0: a chain of ONE element whose optic kind is known at compile time (the one-element defect chains: C5) -- no
// run-time switch on the kind, no element loop; ART_KIND_DYN: the general body.
// SUMMARY (the scene kernels): `sm` is NULL or this chain's row summary (art_scene.h RowSummary, formed by
// art_bundle_row_summary over a.in and a.ro.w).  A row it proves constant keeps its load instruction but gets a ZERO-LENGTH
// descriptor -- the range check answers 0 without touching memory, the mechanism the absent weight stream always used -- and
// its value is the summary's pattern (a select on wave-uniform conditions, see below): mask and patterns arrive by
// scalar loads.  41 of a point or plane source's 65 B per ray are not read.  A constant `alive` holds for slots below n
// only: the tail of the last tile and the padding workgroups of a rounded-up grid stay dead.
template <bool DEFECT, int KIND1 = ART_KIND_DYN, bool SUMMARY = false>
__device__ __forceinline__ void chain_body(const ChainArgs& a, const int64_t first, const int64_t n, const int xmap,
                                           double* s_zern, const unsigned bx, const unsigned nbx, const bool keep_in = false,
                                           const art::RowSummary* sm = nullptr) {
#ifdef ART_ZERN_LDS
  if (DEFECT) {
    int off = 0;
    for (int k = 0; k < a.n_elems; ++k) {
      stage_tables(a.e[k].zern, s_zern + off, a.e[k].n_defects * ART_ZERN_STRIDE);
      off += a.e[k].n_defects * ART_ZERN_STRIDE;
    }
    __syncthreads();
  }
#endif
  __shared__ double s_w[kBlock];   // per-lane parking slot (no barrier: a lane only reads what it wrote)
  __shared__ __attribute__((aligned(16))) double s_red[(kBlock / 64) * 8 * kTileStride];   // wave-private tiles of wave_reduce24 (18 KiB)
#ifndef ART_STORE_DIRECT
  // the staging tile of the 16-byte stores shares the tail's reduction tiles: the tail runs behind the last element's
  // closing barrier
  double (*s_out)[kBlock] = reinterpret_cast<double (*)[kBlock]>(s_red);
  static_assert(sizeof(double) * 8 * kBlock <= sizeof(double) * (kBlock / 64) * 8 * kTileStride, "staging tile fits");
  __shared__ uint8_t s_al[kBlock];
#endif
  __shared__ double s_part[kBlock / 64][kReadoutSlots];   // wave totals of the fused read-out, combined per workgroup
  const int64_t tile = tile_of(bx, nbx, xmap);
  BundleRsrc bi = make_rsrc(a.in, n, first);
  unsigned cm = 0;                                   // bit j: row j of the input is constant (wave-uniform)
  uint64_t cc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // ... and its pattern
  if (SUMMARY) {
    // Mask and patterns are read UNCONDITIONALLY, through the constant address space (scalar loads, like the table's):
    // loads behind `sm != NULL` came out as nine branches with a vector load each, behind the ray's own.  Without a
    // summary the words are read from the table entry itself -- any readable 88 bytes -- and cm = 0 discards them.
    typedef const art::RowSummary __attribute__((address_space(4)))* csum_t;
    const bool have = sm != nullptr;
    const csum_t q = (csum_t)(have ? (const void*)sm : (const void*)&a);
    if (have && q->n >= first + n) cm = ~q->differs & 0x1ffu;
#pragma unroll
    for (int j = 0; j < 9; ++j) cc[j] = (cm >> j & 1u) ? q->c[j] : 0;      // (0 for a row that is loaded)
    const unsigned b8 = (unsigned)(n * 8);
    bi.ox = rsrc_of(a.in.ox + first, (cm & 1u) ? 0u : b8); bi.oy = rsrc_of(a.in.oy + first, (cm & 2u) ? 0u : b8);
    bi.oz = rsrc_of(a.in.oz + first, (cm & 4u) ? 0u : b8); bi.dx = rsrc_of(a.in.dx + first, (cm & 8u) ? 0u : b8);
    bi.dy = rsrc_of(a.in.dy + first, (cm & 16u) ? 0u : b8); bi.dz = rsrc_of(a.in.dz + first, (cm & 32u) ? 0u : b8);
    bi.path = rsrc_of(a.in.path + first, (cm & 64u) ? 0u : b8);
    bi.alive = rsrc_of(a.in.alive + first, (cm & (1u << art::kRowAlive)) ? 0u : (unsigned)n);
  }
  const int64_t stride = (int64_t)nbx * kBlock;
  int64_t i0 = tile * kBlock + threadIdx.x;
  do {
    // One register identifies the lane from here on: the slot index, made opaque so that the compiler derives both the
    // buffer offsets and the lane's position in its workgroup (tile * 256 is a multiple of 256) from IT instead of
    // keeping threadIdx.x alive next to it -- at 80 registers (6 waves per SIMD) that second copy is spilled and its
    // reload in the tail is a VMEM load behind 32 stores.
    unsigned slot = (unsigned)i0;
    asm volatile("" : "+v"(slot));
    const int64_t i = slot;
    const unsigned lane = slot & (kBlock - 1);
    art::Ray r;
    r.inc = 0.0;
    uint8_t al;
    if (keep_in) load_slot_keep(bi, i, r, al);      // (wave-uniform: the launch's grid shape)
    else load_slot(bi, i, r, al);
    // Weight of the fused read-out: fetched with the ray (a zero-length descriptor without read-out or weights) and
    // parked in LDS until the tail needs it -- held in registers across the chain it costs the 2 VGPRs that push the
    // 5-wave build into scratch, and a scratch reload at the end is a VMEM load behind 36 stores (see the tail).
    double wl = ld_f64(rsrc_of(const_cast<double*>(a.ro.w) + first,
                               ((a.flags & art::kFlagReadout) && a.ro.w && !a.ro.lite &&
                                !(SUMMARY && (cm & (1u << art::kRowWeight)))) ? (unsigned)(n * 8) : 0u),
                       (unsigned)i * 8u);
    if (SUMMARY) {
      // The select `constant ? pattern : loaded`, bit for bit, in ONE instruction per dword: the range check answered a
      // constant row's load with 0 and cc[] holds 0 for a loaded row, so OR-ing the two IS the select, with the pattern as
      // the scalar operand.  (v_cndmask takes one scalar operand on gfx9 -- the lane mask -- so the patterns had to be
      // copied into VGPRs first: 16 more instructions per ray, which showed where the launch is VALU-bound -- C5, the
      // lazy-history step: DESIGN.md 5.)  No floating-point operation touches the value.
      r.ox = or_bits(r.ox, cc[0]); r.oy = or_bits(r.oy, cc[1]); r.oz = or_bits(r.oz, cc[2]);
      r.dx = or_bits(r.dx, cc[3]); r.dy = or_bits(r.dy, cc[4]); r.dz = or_bits(r.dz, cc[5]);
      r.path = or_bits(r.path, cc[6]);
      wl = or_bits(wl, cc[art::kRowWeight]);
      // (slot < n in 32 bits: a launch covers at most 2^28 slots and its grid fewer than 2^32 work-items)
      al |= (slot < (unsigned)n) ? (uint8_t)cc[art::kRowAlive] : (uint8_t)0;
    }
    s_w[lane] = wl;
    bool ok = al != 0;
    const double* zk = s_zern;
    // do-while (n_elems >= 1, checked on the host): with a zero-trip path the ray loads above would still be in
    // flight where that path joins the tail, and the ONE wait the compiler then places at the join makes the main
    // path wait for the acknowledgement of all its stores (vmcnt counts loads and stores in one in-order queue)
    int k = 0;
    do {
#ifdef ART_DIAG_NOCOMPUTE
      r.path += a.e[k].mp[0];
#else
#ifdef ART_ZERN_LDS
      if (ok) ok = art::trace_ray_dyn<DEFECT>(a.e[k], zk, r);
      zk += a.e[k].n_defects * ART_ZERN_STRIDE;
#else
      if (KIND1 != ART_KIND_DYN) {
        if (ok) ok = art::trace_ray<(KIND1 < 0 ? 0 : KIND1), DEFECT>(a.e[0], a.e[0].zern, r);
      } else {
        if (ok) ok = art::trace_ray_dyn<DEFECT>(a.e[k], a.e[k].zern, r);
      }
#endif
#endif
#ifndef ART_STORE_DIRECT
      store_tile_lds4(a.out[k], n, first, (int64_t)(slot - lane), lane, r, ok, s_out, s_al);
#else
      // no history view for this element -> zero-length descriptors: every store is dropped by the range check
      store_slot(make_rsrc(a.out[k], a.out[k].alive != nullptr ? n : 0, first), i, r, ok);
#endif
    } while (KIND1 == ART_KIND_DYN && ++k < a.n_elems);
    if (a.flags & art::kFlagReadout) {
      // Fused detector read-out of the last bundle (art_trace_chain_readout): the ray is still in registers.  X, Y, opl
      // of dead rays are dropped by the range check.  Statistics: per wave wave_reduce24, per workgroup one partial,
      // written row by row (row_of_slot) into ro.scratch -- no __syncthreads() and no load down here: either would make
      // every wave wait for the acknowledgement of its 36 outstanding stores (vmcnt counts loads and stores in one queue)
      // instead of retiring as soon as they are issued, which cost 35 %.
      if (a.ro.sums) {     // (wave-uniform) pass (1) of the analysis instead of a read-out: see run_sums8
        double v[8];
        sums_values(v, ok, r, a.ro.w ? s_w[lane ^ ((unsigned)a.flags >> 30)] : 1.0);
        const double tot = run_sums8(v, s_red + (lane >> 6) * (8 * kTileStride), lane & 63);
        tile_sums_store(tot, __ballot(ok), &s_part[0][0], lane, a.ro.scratch, (n + kBlock - 1) / kBlock, tile);
      } else {
      double acc[kReadoutSlots];
      double Ix, Iy, Iz, x = 0.0, y = 0.0, o = 0.0;
      if (ok) art::detector_ray(a.ro.det, r, Ix, Iy, Iz, x, y, o);
      const unsigned nb8 = (unsigned)(n * 8);
      const unsigned o8 = ok ? (unsigned)i * 8u : kDropOffset;
#ifndef ART_DIAG_RO_NOXYO    // timing-only builds of the fused tail: without its per-ray outputs, ...
      st_f64(rsrc_of(a.ro.X + first, a.ro.X ? nb8 : 0u), o8, x);
      st_f64(rsrc_of(a.ro.Y + first, a.ro.Y ? nb8 : 0u), o8, y);
      st_f64(rsrc_of(a.ro.opl + first, a.ro.opl ? nb8 : 0u), o8, o);
#endif
      // re-read the parked weight through an index the compiler cannot prove equal to the one it was stored with
      // (flags has no bit 30), so that the value is neither kept in a register nor spilled
      double tot[3];
      if (a.ro.lite) {     // (wave-uniform: the flag sits in the descriptor)
        readout_single_lite(acc, ok, x, y, o);
        wave_reduce_lite(acc, s_red + (lane >> 6) * (8 * kTileStride), lane & 63, tot);
      } else {
      readout_single(acc, ok, x, y, o, s_w[lane ^ ((unsigned)a.flags >> 30)], a.ro.w != nullptr, a.ro.cx, a.ro.cy,
                     a.ro.co);
#ifdef ART_DIAG_RO_NOREDUCE  // ... without the wave reduction (ART_DIAG_RO_NOSCRATCH: see tail_partial)
      tot[0] = acc[0] + acc[1] + acc[6] + acc[7] + acc[8] + acc[9] + acc[10] + acc[11];
      tot[1] = acc[16] + acc[17] + acc[18] + acc[19] + acc[20] + acc[21];
      tot[2] = acc[2] + acc[3] + acc[4] + acc[5] + acc[12] + acc[13];
#else
      wave_reduce24(acc, s_red + (lane >> 6) * (8 * kTileStride), lane & 63, tot);
#endif
      }
      tail_partial(a, tot, s_part, lane, bx, nbx);
      }
    }
    i0 += stride;
  } while (DEFECT && kDefectLoop && i0 < n);
}

// ---- two rays per lane (round-3 experiment, ART_CHAIN_RPL=2) -----------------------------------------------------------
// A lane owns the two NEIGHBOURING slots 2p, 2p + 1: every stream is then read and written with 16 bytes per lane (1 KiB
// per wave instruction) straight from registers -- no LDS staging tile, no workgroup barrier between the elements (the
// one-ray-per-lane body needs two per element to regroup its 8-byte values into 16-byte stores), per-row descriptors and
// hardware range checks as before (a pair of dead rays is dropped by its offset, the odd tail by the per-dword check).
// The two rays of a lane are traced one after the other; a wave carries 128 rays.
template <bool DEFECT>
__device__ __forceinline__ void chain_body2(const ChainArgs& a, const int64_t first, const int64_t n, const int xmap,
                                            const unsigned bx, const unsigned nbx, const bool keep_in = false) {
  __shared__ double s_w[2][kBlock];   // per-lane parking slots of the two weights (no barrier: a lane reads what it wrote)
  __shared__ __attribute__((aligned(16))) double s_red[(kBlock / 64) * 8 * kTileStride];   // wave-private tiles of wave_reduce24
  __shared__ double s_part[kBlock / 64][kReadoutSlots];
  const int64_t tile = tile_of(bx, nbx, xmap);
  const BundleRsrc bi = make_rsrc(a.in, n, first);
  unsigned pair = (unsigned)(tile * kBlock + threadIdx.x);
  asm volatile("" : "+v"(pair));                      // ONE register identifies the lane (see chain_body)
  const unsigned lane = pair & (kBlock - 1);
  const unsigned o16 = pair * 16u, o2 = pair * 2u;
  art::Ray r[2];
  bool ok[2];
  {
    D2 ox, oy, oz, dx, dy, dz, pa;
    if (keep_in) {       // the shared input of a chain-interleaved scene launch: default cache policy (see ld_f64_keep)
      ox = ld_2f64_keep(bi.ox, o16); oy = ld_2f64_keep(bi.oy, o16); oz = ld_2f64_keep(bi.oz, o16);
      dx = ld_2f64_keep(bi.dx, o16); dy = ld_2f64_keep(bi.dy, o16); dz = ld_2f64_keep(bi.dz, o16);
      pa = ld_2f64_keep(bi.path, o16);
    } else {
      ox = ld_2f64(bi.ox, o16); oy = ld_2f64(bi.oy, o16); oz = ld_2f64(bi.oz, o16);
      dx = ld_2f64(bi.dx, o16); dy = ld_2f64(bi.dy, o16); dz = ld_2f64(bi.dz, o16);
      pa = ld_2f64(bi.path, o16);
    }
    // The two alive bytes with ONE 16-bit load.  A 16-bit access straddling the end of an odd-length array is dropped as a
    // whole: for odd n (wave-uniform) the lane that holds the last slot fetches its byte separately.
    unsigned al2 = __builtin_amdgcn_raw_buffer_load_b16(bi.alive, (int)o2, 0, ART_LD_AUX);
    if (n & 1) al2 |= __builtin_amdgcn_raw_buffer_load_b8(bi.alive, (o2 + 1u == (unsigned)n) ? (int)o2 : (int)kDropOffset, 0, ART_LD_AUX);
    ok[0] = (al2 & 0xffu) != 0;
    ok[1] = (al2 & 0xff00u) != 0;
    const D2 wv = ld_2f64(rsrc_of(const_cast<double*>(a.ro.w) + first,
                                  ((a.flags & art::kFlagReadout) && a.ro.w && !a.ro.lite) ? (unsigned)(n * 8) : 0u), o16);
    s_w[0][lane] = wv.a; s_w[1][lane] = wv.b;
    r[0].ox = ox.a; r[0].oy = oy.a; r[0].oz = oz.a; r[0].dx = dx.a; r[0].dy = dy.a; r[0].dz = dz.a; r[0].path = pa.a;
    r[1].ox = ox.b; r[1].oy = oy.b; r[1].oz = oz.b; r[1].dx = dx.b; r[1].dy = dy.b; r[1].dz = dz.b; r[1].path = pa.b;
    r[0].inc = 0.0; r[1].inc = 0.0;
  }
  int k = 0;
  do {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (ok[h]) ok[h] = art::trace_ray_dyn<DEFECT>(a.e[k], a.e[k].zern, r[h]);
    const ArtBundleView& v = a.out[k];
    const unsigned nb = (unsigned)(v.alive != nullptr ? n : 0);     // no history view: every store is dropped
    const unsigned off = (ok[0] || ok[1]) ? o16 : kDropOffset;
    st_2f64(rsrc_of(v.ox + first, nb * 8u), off, r[0].ox, r[1].ox);
    st_2f64(rsrc_of(v.oy + first, nb * 8u), off, r[0].oy, r[1].oy);
    st_2f64(rsrc_of(v.oz + first, nb * 8u), off, r[0].oz, r[1].oz);
    st_2f64(rsrc_of(v.dx + first, nb * 8u), off, r[0].dx, r[1].dx);
    st_2f64(rsrc_of(v.dy + first, nb * 8u), off, r[0].dy, r[1].dy);
    st_2f64(rsrc_of(v.dz + first, nb * 8u), off, r[0].dz, r[1].dz);
    st_2f64(rsrc_of(v.path + first, nb * 8u), off, r[0].path, r[1].path);
    st_2f64(rsrc_of(v.incidence + first, nb * 8u), off, r[0].inc, r[1].inc);
    const __amdgpu_buffer_rsrc_t ra = rsrc_of(v.alive + first, nb);
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)((ok[0] ? 1u : 0u) | (ok[1] ? 0x100u : 0u)), ra, (int)o2, 0, ART_ST_AUX);
    if (n & 1)      // odd n: the 16-bit store of the pair that holds the last slot was dropped by the range check
      __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(ok[0] ? 1 : 0), ra, (o2 + 1u == (unsigned)n) ? (int)o2 : (int)kDropOffset, 0, ART_ST_AUX);
  } while (++k < a.n_elems);
  if ((a.flags & art::kFlagReadout) && a.ro.sums) {     // pass (1) of the analysis instead of a read-out: see run_sums8
    const unsigned li = lane ^ ((unsigned)a.flags >> 30);
    double v0[8], v1[8], totA, totB;
    sums_values(v0, ok[0], r[0], a.ro.w ? s_w[0][li] : 1.0);
    sums_values(v1, ok[1], r[1], a.ro.w ? s_w[1][li] : 1.0);
    run_sums8_pairs(v0, v1, s_red + (lane >> 6) * (8 * kTileStride), lane & 63, totA, totB);
    static_assert(sizeof(s_part) >= sizeof(double) * 8 * kSumRows, "eight runs fit the partial area");
    tile_sums_store_pairs(totA, totB, __ballot(ok[0]), __ballot(ok[1]), &s_part[0][0], lane, a.ro.scratch,
                          (n + kBlock - 1) / kBlock, tile);
  } else if (a.flags & art::kFlagReadout) {
    double acc[kReadoutSlots];
    double Ix, Iy, Iz, x[2] = {0.0, 0.0}, y[2] = {0.0, 0.0}, o[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (ok[h]) art::detector_ray(a.ro.det, r[h], Ix, Iy, Iz, x[h], y[h], o[h]);
    const unsigned nb8 = (unsigned)(n * 8);
    const unsigned off = (ok[0] || ok[1]) ? o16 : kDropOffset;
    st_2f64(rsrc_of(a.ro.X + first, a.ro.X ? nb8 : 0u), off, x[0], x[1]);
    st_2f64(rsrc_of(a.ro.Y + first, a.ro.Y ? nb8 : 0u), off, y[0], y[1]);
    st_2f64(rsrc_of(a.ro.opl + first, a.ro.opl ? nb8 : 0u), off, o[0], o[1]);
    const unsigned li = lane ^ ((unsigned)a.flags >> 30);     // an index the compiler cannot prove equal to the parking one
    double tot[3];
    if (a.ro.lite) {
      readout_single_lite(acc, ok[0], x[0], y[0], o[0]);
      readout_accumulate_lite(acc, ok[1], x[1], y[1], o[1]);
      wave_reduce_lite(acc, s_red + (lane >> 6) * (8 * kTileStride), lane & 63, tot);
    } else {
      readout_single(acc, ok[0], x[0], y[0], o[0], s_w[0][li], a.ro.w != nullptr, a.ro.cx, a.ro.cy, a.ro.co);
      readout_accumulate(acc, ok[1], x[1], y[1], o[1], s_w[1][li], a.ro.w != nullptr, a.ro.cx, a.ro.cy, a.ro.co);
      wave_reduce24(acc, s_red + (lane >> 6) * (8 * kTileStride), lane & 63, tot);
    }
    tail_partial(a, tot, s_part, lane, bx, nbx);
  }
}

// Fold of the fused read-out's per-WORKGROUP partials (row-major: scratch[row_of_slot(slot) * nparts + part], 39 063
// parts per 1e7 rays), always in a fixed order (deterministic).  ONE launch up to kFoldDirect partials (1.67e7 rays):
// a 1024-thread workgroup per statistic folds its whole row (312 KB at 1e7 rays: thread t takes parts t, t + 1024, ...,
// ~40 independent loads, then a shuffle tree and 16 wave totals through LDS).  Round 2 left one partial per WAVE and
// folded the four-times-longer rows in two launches (64 chunks per statistic, then one workgroup per statistic): 8 + 5 us
// behind every relay4 trace, 18 us behind C2's 11 chains; that two-stage form remains for longer rows.
// Grids: (24, 1, chains) direct; (24, chunks, chains) + (24, 1, chains) beyond.
constexpr int kFoldChunks = 64;
constexpr int64_t kFoldDirect = 65536;
__device__ __forceinline__ double* fold_mid(double* scratch, const int64_t nparts) {
  return scratch + (int64_t)kReadoutSlots * nparts;
}
__device__ __forceinline__ int fold_row_of(const int slot) {
  int row = 0;
#pragma unroll
  for (int k = 0; k < kUsedSlots; ++k) row = (slot == k) ? row_of_slot(k) : row;
  return row;
}
__device__ __forceinline__ void fold_stage1(double* scratch, const int64_t nparts) {
  if (blockIdx.x >= kUsedSlots) return;
  const int64_t per = (nparts + kFoldChunks - 1) / kFoldChunks;
  const int64_t lo = (int64_t)blockIdx.y * per, hi = (lo + per < nparts) ? lo + per : nparts;
  fold_range(scratch + (int64_t)fold_row_of(blockIdx.x) * nparts, lo, hi, stat_op(blockIdx.x),
             fold_mid(scratch, nparts) + blockIdx.x * kFoldChunks + blockIdx.y);
}
__device__ __forceinline__ void fold_stage2(double* scratch, const int64_t nparts, double* out24, const int direct) {
  if (blockIdx.x >= kUsedSlots) {
    if (threadIdx.x == 0) out24[blockIdx.x] = 0.0;
    return;
  }
  if (direct) {   // nparts == 0 (an empty bundle): the fold of nothing leaves the identities
    fold_range(scratch + (int64_t)fold_row_of(blockIdx.x) * nparts, 0, nparts, stat_op(blockIdx.x), out24 + blockIdx.x);
    return;
  }
  fold_range(fold_mid(scratch, nparts) + blockIdx.x * kFoldChunks, 0, kFoldChunks, stat_op(blockIdx.x), out24 + blockIdx.x);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_readout_fold1(const ChainArgs* __restrict__ tab, const int64_t nparts) {
  fold_stage1(tab[blockIdx.z].ro.scratch, nparts);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_readout_fold2(const ChainArgs* __restrict__ tab, const int64_t nparts,
                                                                    const int direct) {
  fold_stage2(tab[blockIdx.z].ro.scratch, nparts, tab[blockIdx.z].ro.out24, direct);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_readout_fold1_one(double* scratch, const int64_t nparts) {
  fold_stage1(scratch, nparts);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_readout_fold2_one(double* scratch, double* out24, const int64_t nparts,
                                                                        const int direct) {
  fold_stage2(scratch, nparts, out24, direct);
}

// threads per workgroup of a one-stage fold: a short row does not need 1024
inline int fold_threads(int64_t nparts) { return nparts <= 4096 ? kBlock : kFoldBlock; }

// Fold of the per-tile partial SUMS (kSumRows rows of `ntiles`, see run_sums8) into out[0 .. 8]: the same launch shape and
// fold_range for the tail of a tracing launch and for art_analyse_bundles' own pass (1) -- same bits either way.  Beyond
// kFoldDirect tiles two stages, with the chunk totals behind the rows (rows + kSumRows * ntiles, kSumRows x kFoldChunks).
__device__ __forceinline__ void sums_fold1(double* rows, const int64_t ntiles) {
  const int64_t per = (ntiles + kFoldChunks - 1) / kFoldChunks;
  const int64_t lo = (int64_t)blockIdx.y * per, hi = (lo + per < ntiles) ? lo + per : ntiles;
  fold_range(rows + (int64_t)blockIdx.x * ntiles, lo < hi ? lo : hi, hi, RSUM,
             rows + (int64_t)kSumRows * ntiles + blockIdx.x * kFoldChunks + blockIdx.y);
}
__device__ __forceinline__ void sums_fold2(double* rows, const int64_t ntiles, double* out, const int direct) {
  if (direct) fold_range(rows + (int64_t)blockIdx.x * ntiles, 0, ntiles, RSUM, out + blockIdx.x);
  else fold_range(rows + (int64_t)kSumRows * ntiles + blockIdx.x * kFoldChunks, 0, kFoldChunks, RSUM, out + blockIdx.x);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_sums_fold1(const ChainArgs* __restrict__ tab, const int64_t ntiles) {
  sums_fold1(tab[blockIdx.z].ro.scratch, ntiles);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_sums_fold2(const ChainArgs* __restrict__ tab, const int64_t ntiles,
                                                                 const int direct) {
  sums_fold2(tab[blockIdx.z].ro.scratch, ntiles, tab[blockIdx.z].ro.out24, direct);
  if (blockIdx.x == 0 && threadIdx.x < kReadoutSlots - kSumRows) tab[blockIdx.z].ro.out24[kSumRows + threadIdx.x] = 0.0;
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_sums_fold1_one(double* scratch, const int64_t ntiles) {
  sums_fold1(scratch, ntiles);
}
__global__ __launch_bounds__(kFoldBlock) void k_chain_sums_fold2_one(double* scratch, double* out24, const int64_t ntiles,
                                                                     const int direct) {
  sums_fold2(scratch, ntiles, out24, direct);
  if (blockIdx.x == 0 && threadIdx.x < kReadoutSlots - kSumRows) out24[kSumRows + threadIdx.x] = 0.0;
}
// Launch the fold behind a tail (host side): `sums` selects the sums kernels (kSumRows rows of `nparts` tiles) over the
// read-out ones (24 slots of `nparts` workgroups); `seg` != nullptr folds the tails of the n_chains chains of that table
// segment, else the one pair `scratch` / `out24`.  ONE launch up to kFoldDirect partials.
void launch_fold(const bool sums, const ChainArgs* seg, const int n_chains, double* scratch, double* out24,
                 const int64_t nparts, hipStream_t s) {
  const int direct = nparts <= kFoldDirect;
  const unsigned rows = sums ? kSumRows : kReadoutSlots, z = seg ? n_chains : 1;
  if (!direct) {
    if (seg) hipLaunchKernelGGL(sums ? k_chain_sums_fold1 : k_chain_readout_fold1, dim3(rows, kFoldChunks, z), dim3(kFoldBlock),
                                0, s, seg, nparts);
    else hipLaunchKernelGGL(sums ? k_chain_sums_fold1_one : k_chain_readout_fold1_one, dim3(rows, kFoldChunks), dim3(kFoldBlock),
                            0, s, scratch, nparts);
  }
  const dim3 g2(rows, 1, z), b2(direct ? fold_threads(nparts) : kBlock);
  if (seg) hipLaunchKernelGGL(sums ? k_chain_sums_fold2 : k_chain_readout_fold2, g2, b2, 0, s, seg, nparts, direct);
  else hipLaunchKernelGGL(sums ? k_chain_sums_fold2_one : k_chain_readout_fold2_one, g2, b2, 0, s, scratch, out24, nparts, direct);
}

template <bool DEFECT, int WAVES>
__global__ __launch_bounds__(kBlock, WAVES) void k_trace_chain(const ChainArgs, const int64_t n, const int xmap) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];   // used by the -DART_ZERN_LDS build only
  // The descriptors are read where the launch put them, in the kernel-argument segment (constant address space ->
  // scalar loads, first parameter = offset 0).  Through the by-value parameter itself that is only what the compiler
  // usually makes of it: the element index is a run-time value, and one build of the defect kernel came out with the
  // whole 3.3 KB copied to scratch at entry and 452 vector loads from there.
  typedef const ChainArgs __attribute__((address_space(4)))* kernarg_t;
  chain_body<DEFECT>(*(const ChainArgs*)(kernarg_t)__builtin_amdgcn_kernarg_segment_ptr(), 0, n, xmap, s_dyn, blockIdx.x,
                     gridDim.x);
}

template <bool DEFECT, int WAVES>
__global__ __launch_bounds__(kBlock, WAVES) void k_trace_chain2(const ChainArgs, const int64_t n, const int xmap) {
  typedef const ChainArgs __attribute__((address_space(4)))* kernarg_t;
  chain_body2<DEFECT>(*(const ChainArgs*)(kernarg_t)__builtin_amdgcn_kernarg_segment_ptr(), 0, n, xmap, blockIdx.x, gridDim.x);
}
// Which (chain, tile) a workgroup of a scene launch works on.  `shape`: 0 = tile-major grid (tiles, chains); bit 0 =
// chain-interleaved grid (chains, tiles); bit 2 = XCD-GROUPED: a 1-D grid of chains x tiles workgroups (tiles a multiple of
// 8, chain count in bits 8 and up) in which the C workgroups of one tile all run on ONE XCD.  The dispatcher hands
// consecutive workgroup ids to the 8 XCDs in turn (id mod 8) and every XCD has its own L2: in the plain interleaved grid
// the C workgroups that read the same input tile land on 8 different XCDs, so the tile crosses the fabric 8 times (from
// the memory-side cache after the first) and the L2s share nothing.  Here id = 8 k + xcd; inside an XCD consecutive k
// run through the chains of one tile (chain = k mod C), then the next tile of that XCD (tile = 8 (k / C) + xcd): the
// tile is fetched into that XCD's L2 once and the other C - 1 workgroups, dispatched right behind, hit it there.
// (bit 1 = the shared input is loaded with the default cache policy, see scene_keep.)
// The grid holds C x (tiles rounded up to a multiple of 8) workgroups; the launch's TRUE tile count arrives in the `xmap`
// parameter (the tile mapping of tile_of does not apply to this shape): workgroups of the padding leave at once, and the
// per-tile partials of a read-out keep the layout and fold order of the other shapes (same bits whatever the shape).
struct SceneWG { unsigned chain, bx, nbx; int xmap; bool idle; };
__device__ __forceinline__ SceneWG scene_wg(const int shape, const int xmap) {
  if (shape & 4) {
    const unsigned C = (unsigned)shape >> 8, id = blockIdx.x;
    const unsigned k = id >> 3, tq = k / C, bx = tq * 8u + (id & 7u);
    return {k - tq * C, bx, (unsigned)xmap, 0, bx >= (unsigned)xmap};
  }
  if (shape & 1) return {blockIdx.x, blockIdx.y, gridDim.y, xmap, false};
  return {blockIdx.y, blockIdx.x, gridDim.x, xmap, false};
}

template <bool DEFECT, int WAVES>
__global__ __launch_bounds__(kBlock, WAVES) void k_trace_scene2(const ChainArgs* __restrict__ tab, const int64_t first,
                                                                const int64_t n, const int xmap, const int transposed,
                                                                const art::RowSummary*) {   // (summaries: one-ray bodies only)
  const SceneWG w = scene_wg(transposed, xmap);
  if (w.idle) return;
  chain_body2<DEFECT>(tab[w.chain], first, n, w.xmap, w.bx, w.nbx, (transposed & 2) != 0);
}

// Many chains in one launch, descriptors in the device-resident scene table (art_scene.h).  Three grid shapes (scene_wg):
//   tile-major    grid (tiles, chains): blockIdx.y = chain -- the dispatcher works through one chain's tiles after the other;
//   interleaved   grid (chains, tiles): blockIdx.x = chain -- the workgroups of ONE tile of ALL chains are dispatched together;
//   XCD-grouped   1-D grid: ... and on the same XCD, so that they share the tile in that XCD's L2.
// The last two are for scenes whose chains all read the SAME input bundle (a loop list traced from one source or from its
// shared prefix, art_scene.h kFlagSharedIn): interleaved, the tile of the input that chain 0 fetches from HBM is still in the
// memory-side cache when chains 1 .. C-1 ask for it a few microseconds later, instead of being streamed from HBM once per
// chain; XCD-grouped (the default), it does not even leave the L2.
template <bool DEFECT, int WAVES>
__global__ __launch_bounds__(kBlock, WAVES) void k_trace_scene(const ChainArgs* __restrict__ tab, const int64_t first,
                                                               const int64_t n, const int xmap, const int transposed,
                                                               const art::RowSummary* __restrict__ sums) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const SceneWG w = scene_wg(transposed, xmap);   // (ONE copy of the body)
  if (w.idle) return;
  chain_body<DEFECT, ART_KIND_DYN, true>(tab[w.chain], first, n, w.xmap, s_dyn, w.bx, w.nbx, (transposed & 2) != 0,
                                         sums ? sums + w.chain : nullptr);
}

// One-element chains WITH defects, the optic's kind a template parameter (round 5, C5: a deformed parabola + read-out).
template <int KIND1, int WAVES>
__global__ __launch_bounds__(kBlock, WAVES) void k_trace_scene1(const ChainArgs* __restrict__ tab, const int64_t first,
                                                                const int64_t n, const int xmap, const int transposed,
                                                                const art::RowSummary* __restrict__ sums) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const SceneWG w = scene_wg(transposed, xmap);
  if (w.idle) return;
  chain_body<true, KIND1, true>(tab[w.chain], first, n, w.xmap, s_dyn, w.bx, w.nbx, (transposed & 2) != 0,
                                sums ? sums + w.chain : nullptr);
}
template <int KIND1, int WAVES>
__global__ __launch_bounds__(kBlock, WAVES) void k_trace_chain1(const ChainArgs, const int64_t n, const int xmap) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  typedef const ChainArgs __attribute__((address_space(4)))* kernarg_t;
  chain_body<true, KIND1>(*(const ChainArgs*)(kernarg_t)__builtin_amdgcn_kernarg_segment_ptr(), 0, n, xmap, s_dyn, blockIdx.x,
                          gridDim.x);
}

// ------------------------------------------------------------------------------------------- row summary
// art_bundle_row_summary: one streaming pass over the nine per-slot rows a fused trace reads of its input (7 fp64 rows,
// alive, the read-out's weights) that proves which of them repeat slot 0's BIT PATTERN in every slot (-0.0 differs from
// +0.0; a row of one NaN pattern is constant).  Every lane ORs the rows it saw differ into one word, the workgroup's word
// meets in LDS and goes out with ONE integer atomicOr (order-independent: the result is deterministic).  `out` was cleared
// by the caller's memset; a row without an array, or an empty bundle, is reported as differing.
__global__ __launch_bounds__(kBlock) void k_row_summary(const ArtBundleView in, const double* __restrict__ w, const int64_t n,
                                                        art::RowSummary* __restrict__ out) {
  __shared__ unsigned s_diff;
  if (threadIdx.x == 0) s_diff = 0;
  __syncthreads();
  const double* const rows[8] = {in.ox, in.oy, in.oz, in.dx, in.dy, in.dz, in.path, w};
  uint64_t c0[8];
  unsigned diff = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int bit = (j < 7) ? j : art::kRowWeight;
    const bool has = rows[j] != nullptr && n > 0;
    c0[j] = has ? (uint64_t)__double_as_longlong(rows[j][0]) : 0;
    if (!has) diff |= 1u << bit;
  }
  const bool has_a = in.alive != nullptr && n > 0;
  const uint8_t a0 = has_a ? in.alive[0] : (uint8_t)0;
  if (!has_a) diff |= 1u << art::kRowAlive;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int bit = (j < 7) ? j : art::kRowWeight;
      if (rows[j] != nullptr) diff |= ((uint64_t)__double_as_longlong(ld_nt(rows[j] + i)) != c0[j]) ? 1u << bit : 0u;
    }
    if (has_a) diff |= (ld_nt(in.alive + i) != a0) ? 1u << art::kRowAlive : 0u;
  }
  if (diff) atomicOr(&s_diff, diff);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_diff) atomicOr(&out->differs, s_diff);
    if (blockIdx.x == 0) {
      out->n = n;
#pragma unroll
      for (int j = 0; j < 7; ++j) out->c[j] = c0[j];
      out->c[art::kRowAlive] = a0;
      out->c[art::kRowWeight] = c0[7];
    }
  }
}

// ------------------------------------------------------------------------------------------- AoS -> SoA
__global__ __launch_bounds__(kBlock) void k_pack_rays(const double* __restrict__ points, const double* __restrict__ vectors,
                                                      const double* __restrict__ path0, const int64_t n,
                                                      const ArtBundleView out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    art::Ray r;
    r.ox = points[3 * i]; r.oy = points[3 * i + 1]; r.oz = points[3 * i + 2];
    const double vx = vectors[3 * i], vy = vectors[3 * i + 1], vz = vectors[3 * i + 2];
    const double inv = 1.0 / sqrt(art::dot3(vx, vy, vz, vx, vy, vz));
    r.dx = vx * inv; r.dy = vy * inv; r.dz = vz * inv;
    r.path = path0 ? path0[i] : 0.0;
    r.inc = NAN;
    store_ray(out, i, r);
    out.alive[i] = 1;
  }
}

// ------------------------------------------------------------------------------------------- affine map
__global__ __launch_bounds__(kBlock) void k_transform(const ArtDetectorDesc mt, const int rotate_points,
                                                      const ArtBundleView in, const ArtBundleView out, const int64_t n) {
  // mt.rot = M, mt.centre = T (ArtDetectorDesc reused as a POD carrier)
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    art::Ray r;
    load_ray(in, i, r);
    r.inc = in.incidence[i];
    const uint8_t a = in.alive[i];
    double px = r.ox, py = r.oy, pz = r.oz, vx, vy, vz;
    if (rotate_points) art::mat3_apply(mt.rot, r.ox, r.oy, r.oz, px, py, pz);
    art::mat3_apply(mt.rot, r.dx, r.dy, r.dz, vx, vy, vz);
    const double inv = 1.0 / sqrt(art::dot3(vx, vy, vz, vx, vy, vz));   // Ray.vector setter
    r.ox = px + mt.centre[0]; r.oy = py + mt.centre[1]; r.oz = pz + mt.centre[2];
    r.dx = vx * inv; r.dy = vy * inv; r.dz = vz * inv;
    store_ray(out, i, r);
    out.alive[i] = a;
  }
}

// ------------------------------------------------------------------------------------------- detector
__global__ __launch_bounds__(kBlock) void k_detector(const ArtDetectorDesc d, const ArtBundleView b, const int64_t n,
                                                     double* p3x, double* p3y, double* p3z, double* X, double* Y,
                                                     double* opl) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    if (b.alive[i] == 0) continue;
    art::Ray r;
    load_ray(b, i, r);
    double Ix, Iy, Iz, x, y, o;
    art::detector_ray(d, r, Ix, Iy, Iz, x, y, o);
    if (p3x) { p3x[i] = Ix; p3y[i] = Iy; p3z[i] = Iz; }
    if (X) { X[i] = x; Y[i] = y; }
    if (opl) opl[i] = o;
  }
}

template <bool HAS_W>
__global__ __launch_bounds__(kBlock) void k_stats_partial(const uint8_t* alive, const double* X, const double* Y,
                                                          const double* opl, const double* w, const int64_t n,
                                                          double* scratch) {
  double acc[kRedSlots];
#pragma unroll
  for (int k = 0; k < kRedSlots; ++k) acc[k] = red_ident(stat_op(k));
  const int64_t stride = (int64_t)gridDim.x * kBlock, last = n - 1;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kRedUnroll * stride) {
    double xv[kRedUnroll], yv[kRedUnroll], ov[kRedUnroll], wv[kRedUnroll];
    bool live[kRedUnroll];
#pragma unroll
    for (int u = 0; u < kRedUnroll; ++u) {
      const int64_t i = i0 + u * stride, c = i < n ? i : last;
      live[u] = (ld_nt(alive + c) != 0) & (i < n);
      xv[u] = X ? ld_nt(X + c) : 0.0;      // (wave-uniform: absent streams read 0)
      yv[u] = Y ? ld_nt(Y + c) : 0.0;
      ov[u] = opl ? ld_nt(opl + c) : 0.0;
      wv[u] = HAS_W ? ld_nt(w + c) : 1.0;
    }
#pragma unroll
    for (int u = 0; u < kRedUnroll; ++u) {
      const bool l = live[u];
      const double x = l ? xv[u] : 0.0, y = l ? yv[u] : 0.0, o = l ? ov[u] : 0.0, ww = l ? wv[u] : 0.0;
      acc[0] += l ? 1.0 : 0.0; acc[1] += o;
      acc[2] = fmin(acc[2], l ? xv[u] : INFINITY); acc[3] = fmax(acc[3], l ? xv[u] : -INFINITY);
      acc[4] = fmin(acc[4], l ? yv[u] : INFINITY); acc[5] = fmax(acc[5], l ? yv[u] : -INFINITY);
      acc[6] += x; acc[7] += y;
      acc[8] += ww; acc[9] = fma(ww, x, acc[9]); acc[10] = fma(ww, y, acc[10]); acc[11] = fma(ww, o, acc[11]);
      acc[12] = fmin(acc[12], l ? ov[u] : INFINITY); acc[13] = fmax(acc[13], l ? ov[u] : -INFINITY);
    }
  }
  block_reduce_store<kRedSlots>(acc, stat_op, scratch + (int64_t)blockIdx.x * kRedSlots);
}

// detector read-out fused with its reductions: one pass over the bundle, statistics accumulated in registers
__global__ __launch_bounds__(kBlock) void k_detector_readout(const ArtDetectorDesc d, const ArtBundleView b,
                                                             const double* w, const int64_t n, const double cx,
                                                             const double cy, const double co, double* p3x, double* p3y,
                                                             double* p3z, double* X, double* Y, double* opl,
                                                             double* scratch) {
  double acc[kReadoutSlots];
#pragma unroll
  for (int k = 0; k < kReadoutSlots; ++k) acc[k] = red_ident(stat_op(k));
  // Two consecutive slots per lane and iteration: every stream is read with one 16-byte access per lane (1 KiB per
  // wave instruction) and the three outputs are written the same way; per-dword range checking of the raw buffer
  // descriptors takes care of an odd tail.  Dead rays contribute nothing through selects (no divergent skip); their
  // output slots receive unspecified values.
  const BundleRsrc bi = make_rsrc(b, n);
  const unsigned nb8 = (unsigned)(n * 8);
  const __amdgpu_buffer_rsrc_t rw = rsrc_of(const_cast<double*>(w), w ? nb8 : 0u);
  const __amdgpu_buffer_rsrc_t r3x = rsrc_of(p3x, p3x ? nb8 : 0u), r3y = rsrc_of(p3y, p3y ? nb8 : 0u),
                               r3z = rsrc_of(p3z, p3z ? nb8 : 0u), rX = rsrc_of(X, X ? nb8 : 0u),
                               rY = rsrc_of(Y, Y ? nb8 : 0u), rO = rsrc_of(opl, opl ? nb8 : 0u);
  const int64_t npairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < npairs; j += stride) {
    const unsigned o16 = (unsigned)j * 16u, o2 = (unsigned)j * 2u;
    const D2 ox = ld_2f64(bi.ox, o16), oy = ld_2f64(bi.oy, o16), oz = ld_2f64(bi.oz, o16);
    const D2 dx = ld_2f64(bi.dx, o16), dy = ld_2f64(bi.dy, o16), dz = ld_2f64(bi.dz, o16);
    const D2 pa = ld_2f64(bi.path, o16), wv = ld_2f64(rw, o16);
    // two byte loads: a 16-bit load straddling the end of an odd-length array is dropped as a whole
    const unsigned char al[2] = {__builtin_amdgcn_raw_buffer_load_b8(bi.alive, (int)o2, 0, ART_LD_AUX),
                                 __builtin_amdgcn_raw_buffer_load_b8(bi.alive, (int)o2 + 1, 0, ART_LD_AUX)};
    double xo[2], yo[2], oo[2], p3[3][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      art::Ray r;
      r.ox = h ? ox.b : ox.a; r.oy = h ? oy.b : oy.a; r.oz = h ? oz.b : oz.a;
      r.dx = h ? dx.b : dx.a; r.dy = h ? dy.b : dy.a; r.dz = h ? dz.b : dz.a;
      r.path = h ? pa.b : pa.a;
      const bool live = al[h] != 0;
      double x, y, o;
      art::detector_ray(d, r, p3[0][h], p3[1][h], p3[2][h], x, y, o);
      xo[h] = x; yo[h] = y; oo[h] = o;
      readout_accumulate(acc, live, x, y, o, h ? wv.b : wv.a, w != nullptr, cx, cy, co);
    }
    st_2f64(r3x, o16, p3[0][0], p3[0][1]); st_2f64(r3y, o16, p3[1][0], p3[1][1]); st_2f64(r3z, o16, p3[2][0], p3[2][1]);
    st_2f64(rX, o16, xo[0], xo[1]); st_2f64(rY, o16, yo[0], yo[1]); st_2f64(rO, o16, oo[0], oo[1]);
  }
#ifdef ART_READOUT_SHUFFLE_REDUCE      // round-1 form: 24 shuffle trees per wave + __syncthreads()
  block_reduce_store<kReadoutSlots>(acc, stat_op, scratch + (int64_t)blockIdx.x * kReadoutSlots);
#else
  // One partial per WORKGROUP, [block][24] as k_fold_partials expects it.  Per wave the LDS transpose of the fused tail
  // (wave_reduce24, ~100 instructions instead of 24 shuffle trees), then the four waves meet in LDS behind a bare
  // s_barrier: __syncthreads() would also wait for the acknowledgement of every store this workgroup has in flight
  // (vmcnt).  174 -> 158 us per 1e7 rays (tools/r02_exp21.sh).
  __shared__ double s_tile[(kBlock / 64) * 8 * kTileStride];
  __shared__ double s_part[kBlock / 64][kReadoutSlots];
  const int lane = threadIdx.x & 63, wv_ = threadIdx.x >> 6;
  double tot[3];
  wave_reduce24(acc, s_tile + wv_ * (8 * kTileStride), lane, tot);
  if ((lane & 7) == 0) {
    const int stat = lane >> 3;
    int g0 = 0, g1 = 0, g2 = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      g0 = (stat == q) ? kPassSlot[0][q] : g0;
      g1 = (stat == q) ? kPassSlot[1][q] : g1;
      g2 = (stat == q) ? kPassSlot[2][q] : g2;
    }
    s_part[wv_][g0] = tot[0];
    s_part[wv_][g1] = tot[1];
    if (stat < 6) s_part[wv_][g2] = tot[2];
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (threadIdx.x < kUsedSlots) {
    const int k = threadIdx.x;
    double v = s_part[0][k];
#pragma unroll
    for (int j = 1; j < kBlock / 64; ++j) v = fold_op(v, s_part[j][k], stat_op(k));
    scratch[(int64_t)blockIdx.x * kReadoutSlots + k] = v;
  } else if (threadIdx.x < kReadoutSlots) {
    scratch[(int64_t)blockIdx.x * kReadoutSlots + threadIdx.x] = 0.0;    // reserved slots 22, 23
  }
#endif
}

// the slot's seven streams + weight of kU grid-stride iterations, requested up front (see ld_nt)
template <int kU>
struct SlotBatch {
  art::Ray r[kU];
  double w[kU];
  bool live[kU];
};
// every stream of the batch, unconditionally (a lane beyond the end re-reads slot n - 1 and is dead)
template <int kU, bool HAS_W>
__device__ __forceinline__ void load_batch_all(const ArtBundleView& b, const double* w, const int64_t i0, const int64_t stride,
                                               const int64_t n, SlotBatch<kU>& q) {
  const int64_t last = n - 1;
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t i = i0 + u * stride, c = i < n ? i : last;
    q.live[u] = (ld_nt(b.alive + c) != 0) & (i < n);
    q.r[u].ox = ld_nt(b.ox + c); q.r[u].oy = ld_nt(b.oy + c); q.r[u].oz = ld_nt(b.oz + c);
    q.r[u].dx = ld_nt(b.dx + c); q.r[u].dy = ld_nt(b.dy + c); q.r[u].dz = ld_nt(b.dz + c);
    q.r[u].path = ld_nt(b.path + c);
    q.w[u] = HAS_W ? ld_nt(w + c) : 1.0;
  }
}
template <bool HAS_W>
__global__ __launch_bounds__(kBlock) void k_scan_moments_partial(const ArtDetectorDesc d, const ArtBundleView b,
                                                                 const double* w, const int64_t n, const double co,
                                                                 const double span, double* scratch) {
  double acc[kScanSlots];
#pragma unroll
  for (int k = 0; k < kScanSlots; ++k) acc[k] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  constexpr int kU = 1;     // (two slots per iteration need 148 VGPRs = 3 waves per SIMD: 0.65 of peak; one: 4 waves)
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kU * stride) {
    SlotBatch<kU> q;
    load_batch_all<kU, HAS_W>(b, w, i0, stride, n, q);
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool l = q.live[u];
      double q0[3], sq[3];
      bool crosses;
      art::detector_ray_scan(d, q.r[u], span, q0[0], q0[1], q0[2], sq[0], sq[1], sq[2], crosses);
      acc[32] += (l && crosses) ? 1.0 : 0.0;
      q0[2] -= co;
      sq[2] -= 1.0;
      const double ww = l ? q.w[u] : 0.0;
      acc[0] += l ? 1.0 : 0.0;
      acc[16] += ww;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int o = 1 + 5 * k;
        const double a0 = l ? q0[k] : 0.0, s0 = l ? sq[k] : 0.0;       // (a dead slot's values are unspecified: selected away)
        acc[o] += a0; acc[o + 1] += s0;
        acc[o + 2] = fma(a0, a0, acc[o + 2]); acc[o + 3] = fma(a0, s0, acc[o + 3]);
        acc[o + 4] = fma(s0, s0, acc[o + 4]);
        const double wq = ww * a0, ws = ww * s0;
        acc[16 + o] += wq; acc[16 + o + 1] += ws;
        acc[16 + o + 2] = fma(wq, a0, acc[16 + o + 2]); acc[16 + o + 3] = fma(wq, s0, acc[16 + o + 3]);
        acc[16 + o + 4] = fma(ws, s0, acc[16 + o + 4]);
      }
    }
  }
  block_reduce_store<kScanSlots>(acc, sum_op, scratch + (int64_t)blockIdx.x * kScanSlots);
}

// ------------------------------------------------------------------------------------------- histogram
// art_histogram: every alive ray's bin is found in registers and counted with INTEGER atomics (a count and the
// fixed-point weight q), so the result is the same bytes whatever the order of arrival.  Two forms, chosen by the bin
// count: up to kHistLdsBins bins each workgroup bins into a private copy in LDS (ds_add_u32 / ds_add_u64) and adds its
// non-zero bins to the output at the end; a larger image (up to 2^24 bins) cannot sit in LDS, and there every ray adds
// to the output in global memory directly.  Reads like the fused read-out: two slots per lane through buffer
// descriptors; the FRAME source gives the direction and path streams descriptors of 0 bytes, so they cost no traffic.
constexpr int kHistBlocks = 512;      // persistent grid: 2 workgroups per CU, so that the LDS form flushes few copies
constexpr int kHistLdsBins = 4096;    // 4 B count + 8 B weight sum per bin: 48 KiB of LDS at most

struct HistArg {
  ArtDetectorDesc map;
  double lo[3], step[3], inv[3], hi[3];
  double delay_centre;
  int32_t bins[3], axis[3];
  int32_t source, wshift;
};

// bin of v among the edges i*step + lo (i < nb) and hi (numpy.linspace: two roundings, NO fused multiply-add), with
// numpy.histogramdd's rule: edge[j] <= v < edge[j+1], v == hi in the last bin; -1 outside (v < lo, v > hi, NaN).  The
// guess from the uniform formula is off by at most one bin unless the range is so narrow against lo that rounding
// makes several edges equal; the walks find the last bin whose edge is <= v in every case.
__device__ __forceinline__ int hist_bin(const double v, const double lo, const double hi, const double step,
                                        const double inv, const int nb) {
#pragma clang fp contract(off)
  if (!(v >= lo && v <= hi)) return -1;
  if (v == hi) return nb - 1;
  int j = (int)fmin(fmax((v - lo) * inv, 0.0), (double)(nb - 1));
  while (j > 0 && v < (double)j * step + lo) --j;
  while (j < nb - 1 && v >= (double)(j + 1) * step + lo) ++j;
  return j;
}

// row-major bin of one ray (axis 0 slowest), -1 if a coordinate is outside its range
__device__ __forceinline__ int hist_flat(const HistArg& a, const int ndim, const art::Ray& r) {
  double v[3];
  if (a.source == ART_HIST_DETECTOR) {
    double Ix, Iy, Iz, o;
    art::detector_ray(a.map, r, Ix, Iy, Iz, v[0], v[1], o);
    v[2] = ((o - a.delay_centre) / 299792458000.0) * 1e15;      // Detector.get_Delays (no multiply-add to contract)
  } else {
    art::mat3_apply(a.map.rot, r.ox - a.map.centre[0], r.oy - a.map.centre[1], r.oz - a.map.centre[2], v[0], v[1], v[2]);
  }
  int flat = 0;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < ndim) {
      const int ax = a.axis[k];
      const double c = ax == 0 ? v[0] : (ax == 1 ? v[1] : v[2]);      // v[2]: FRAME component 2 or the DELAY
      const int j = hist_bin(c, a.lo[k], a.hi[k], a.step[k], a.inv[k], a.bins[k]);
      in = in && j >= 0;
      flat = flat * a.bins[k] + j;
    }
  }
  return in ? flat : -1;
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_histogram(const HistArg a, const int ndim, const int nbins,
                                                      const ArtBundleView b, const double* w, const int64_t n,
                                                      unsigned long long* counts, unsigned long long* wsums,
                                                      unsigned long long* totals) {
  extern __shared__ unsigned long long s_wsum[];        // LDS form: [nbins] weight sums (with w), then [nbins] counts
  unsigned* const s_cnt = reinterpret_cast<unsigned*>(s_wsum + (w ? nbins : 0));
  if (LDS) {
    for (int i = threadIdx.x; i < nbins; i += kBlock) {
      s_cnt[i] = 0u;
      if (w) s_wsum[i] = 0ull;
    }
    __syncthreads();
  }
  const bool det = a.source == ART_HIST_DETECTOR;
  const unsigned nb8 = (unsigned)(n * 8), nd8 = det ? nb8 : 0u;
  const __amdgpu_buffer_rsrc_t rox = rsrc_of(b.ox, nb8), roy = rsrc_of(b.oy, nb8), roz = rsrc_of(b.oz, nb8),
                               rdx = rsrc_of(b.dx, nd8), rdy = rsrc_of(b.dy, nd8), rdz = rsrc_of(b.dz, nd8),
                               rpa = rsrc_of(b.path, nd8), ral = rsrc_of(b.alive, (unsigned)n),
                               rw = rsrc_of(const_cast<double*>(w), w ? nb8 : 0u);
  unsigned long long n_in = 0, n_out = 0, q_in = 0, q_out = 0;
  const int64_t npairs = (n + 1) / 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < npairs; j += stride) {
    const unsigned o16 = (unsigned)j * 16u, o2 = (unsigned)j * 2u;
    const D2 ox = ld_2f64(rox, o16), oy = ld_2f64(roy, o16), oz = ld_2f64(roz, o16);
    const D2 dx = ld_2f64(rdx, o16), dy = ld_2f64(rdy, o16), dz = ld_2f64(rdz, o16);
    const D2 pa = ld_2f64(rpa, o16), wv = ld_2f64(rw, o16);
    const unsigned char al[2] = {__builtin_amdgcn_raw_buffer_load_b8(ral, (int)o2, 0, ART_LD_AUX),
                                 __builtin_amdgcn_raw_buffer_load_b8(ral, (int)o2 + 1, 0, ART_LD_AUX)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      art::Ray r;
      r.ox = h ? ox.b : ox.a; r.oy = h ? oy.b : oy.a; r.oz = h ? oz.b : oz.a;
      r.dx = h ? dx.b : dx.a; r.dy = h ? dy.b : dy.a; r.dz = h ? dz.b : dz.a;
      r.path = h ? pa.b : pa.a;
      const bool live = al[h] != 0;
      const int flat = hist_flat(a, ndim, r);
      // a dead slot's weight is unspecified (possibly NaN): selected away before the conversion
      const double wl = live ? (h ? wv.b : wv.a) : 0.0;
      const unsigned long long q = (unsigned long long)(long long)rint(ldexp(wl, a.wshift));
      const bool in = live && flat >= 0, out = live && flat < 0;
      n_in += in ? 1ull : 0ull; q_in += in ? q : 0ull;
      n_out += out ? 1ull : 0ull; q_out += out ? q : 0ull;
      if (in) {
        if (LDS) {
          atomicAdd(&s_cnt[flat], 1u);
          if (w) atomicAdd(&s_wsum[flat], q);
        } else {
          atomicAdd(&counts[flat], 1ull);
          if (w) atomicAdd(&wsums[flat], q);
        }
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < nbins; i += kBlock) {
      const unsigned c = s_cnt[i];
      if (c) {
        atomicAdd(&counts[i], (unsigned long long)c);
        if (w) atomicAdd(&wsums[i], s_wsum[i]);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_in += __shfl_xor(n_in, off, 64); n_out += __shfl_xor(n_out, off, 64);
    q_in += __shfl_xor(q_in, off, 64); q_out += __shfl_xor(q_out, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_in) atomicAdd(&totals[0], n_in);
    if (n_out) atomicAdd(&totals[1], n_out);
    if (q_in) atomicAdd(&totals[2], q_in);
    if (q_out) atomicAdd(&totals[3], q_out);
  }
}

// ------------------------------------------------------------------------------------------- focal field
// art_focal_field: E_q = V^T diag(c_q) U, a complex GEMM over the rays in which U and V are never stored.
// k_focal_prep writes, per slot, the amplitude and the phase coefficients of the ray into kFocalRows rows of scratch (a
// dead slot gets amplitude 0).  k_focal_field: one workgroup per (64 x 64 pixel tile, plane, slice of the rays); per
// chunk of kFocalChunk rays it forms the chunk's column phasors U and row phasors c_q V in LDS -- fp64 sincos at every
// kFocalSeg-th pixel, rotations by the ray's one-pixel step in between (at most kFocalSeg - 1 of them: ~1e-15 rad) --
// and every lane accumulates a 4 x 4 block of pixels with fp64 FMAs.  k_focal_fold adds the slices' partials in slice
// order.  No float atomics: the same bytes on every call.
constexpr int kFocalRows = 9;         // amp, base, k d.e1, k d.e2, k d.n, exp(i k d.e1 dx) (2), exp(i k d.e2 dy) (2)
constexpr int kFocalTile = 64;        // pixels per tile side
constexpr int kFocalLanes = 16;       // lanes per tile side: lane (lx, ly) owns columns lx + 16u and rows ly + 16v
constexpr int kFocalMicro = kFocalTile / kFocalLanes;
constexpr int kFocalChunk = 32;       // rays per LDS stage: 2 x 32 KiB of phasors
constexpr int kFocalSeg = 16;         // phasors per sincos: kBlock / 2 lanes build 32 rays x 4 segments of each kind
constexpr int kFocalMaxSlices = 64;
constexpr int kFocalWantBlocks = 2048;   // 8 workgroups per CU when the grid has enough tiles x planes x slices
static_assert(kFocalChunk * (kFocalTile / kFocalSeg) * 2 == kBlock, "one phasor segment per lane");

struct FocalArg {
  double k, L_ref, x0, dx, y0, dy;
  double C[3], nrm[3], e1[3], e2[3];
  int64_t stride, per_slice, n;   // scratch row stride; rays per slice; slots
  int32_t nx, ny, planes, tiles_x;
  double shift[ART_FOCAL_MAX_PLANES];
};

inline int64_t focal_stride(int64_t n) { return (n + 63) / 64 * 64; }
inline int focal_tiles(int nx, int ny) { return ((nx + kFocalTile - 1) / kFocalTile) * ((ny + kFocalTile - 1) / kFocalTile); }

// slices of the rays: enough workgroups to fill the machine, at least 4 chunks of rays per slice
inline int focal_slices(int nx, int ny, int planes, int64_t n) {
  const int64_t wgs = (int64_t)focal_tiles(nx, ny) * planes;
  int64_t s = (kFocalWantBlocks + wgs - 1) / wgs;
  const int64_t by_rays = (n + 4 * kFocalChunk - 1) / (4 * kFocalChunk);
  if (s > by_rays) s = by_rays;
  if (s > kFocalMaxSlices) s = kFocalMaxSlices;
  return s < 1 ? 1 : (int)s;
}

__global__ __launch_bounds__(kBlock) void k_focal_prep(const FocalArg a, const ArtBundleView b, const double* w,
                                                       const int64_t m, double* rows) {
#pragma clang fp contract(off)
  const int64_t st = a.stride;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const bool live = b.alive[i] != 0;
    const double px = b.ox[i], py = b.oy[i], pz = b.oz[i], dx = b.dx[i], dy = b.dy[i], dz = b.dz[i];
    // a dead slot's values are unspecified (possibly NaN): selected away
    const double amp = live ? (w ? sqrt(w[i]) : 1.0) : 0.0;
    const double base = live ? a.k * ((b.path[i] - a.L_ref) + ((dx * (a.C[0] - px) + dy * (a.C[1] - py)) + dz * (a.C[2] - pz)))
                             : 0.0;
    const double ka = live ? a.k * ((dx * a.e1[0] + dy * a.e1[1]) + dz * a.e1[2]) : 0.0;
    const double kb = live ? a.k * ((dx * a.e2[0] + dy * a.e2[1]) + dz * a.e2[2]) : 0.0;
    const double kc = live ? a.k * ((dx * a.nrm[0] + dy * a.nrm[1]) + dz * a.nrm[2]) : 0.0;
    double sa, ca, sb, cb;
    sincos(ka * a.dx, &sa, &ca);
    sincos(kb * a.dy, &sb, &cb);
    rows[i] = amp; rows[st + i] = base; rows[2 * st + i] = ka; rows[3 * st + i] = kb; rows[4 * st + i] = kc;
    rows[5 * st + i] = ca; rows[6 * st + i] = sa; rows[7 * st + i] = cb; rows[8 * st + i] = sb;
  }
}

// ---- the pieces that k_focal_field, k_focal_image, k_focal_spectrum_field and k_vecspec_field are made of.  The
// rotation and the sums are explicit FMAs, so the four kernels round alike: from the same phase terms, the same bytes.

using FocalStage = double2[kFocalChunk][kFocalTile];      // one chunk's phasors in LDS
using FocalAcc = double[kFocalMicro][kFocalMicro];        // a lane's 4 x 4 block of sums

// a lane's two roles in its workgroup (blockIdx.x is the tile)
struct FocalLane {
  int tx0, ty0;      // first pixel of the tile
  int lx, ly;        // accumulating: columns tx0 + lx + 16 u and rows ty0 + ly + 16 v
  bool colw;         // staging: columns (U) or rows (W),
  int sr, sg;        //          ray sr of the chunk, segment sg of the tile
};

__device__ __forceinline__ FocalLane focal_lane(const int tiles_x) {
  const int t = threadIdx.x;
  FocalLane L;
  L.tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kFocalTile;
  L.ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kFocalTile;
  L.lx = t % kFocalLanes;
  L.ly = t / kFocalLanes;
  L.colw = t < kBlock / 2;
  L.sr = (t % (kBlock / 2)) / (kFocalTile / kFocalSeg);
  L.sg = t % (kFocalTile / kFocalSeg);
  return L;
}

// a product that is never contracted into an FMA: k_j * row rounds as k * (...) does in k_focal_prep
__device__ __forceinline__ double focal_mul(const double a, const double b) {
#pragma clang fp contract(off)
  return a * b;
}

// For slot r of the rows (in: it belongs to the workgroup's rays; else neutral values), the staging lane's phase at the
// first pixel of its segment (plane shift sh) and its one-pixel step phasor, read from k_focal_prep's rows ...
__device__ __forceinline__ void focal_phase_terms(const FocalArg& a, const double* __restrict__ rows, const FocalLane& L,
                                                  const int64_t r, const bool in, const double sh, double& ph,
                                                  double& s_re, double& s_im) {
  const int64_t st = a.stride;
  if (L.colw) {
    const int p0 = L.tx0 + L.sg * kFocalSeg;
    const double ka = in ? rows[2 * st + r] : 0.0;
    ph = ka * (a.x0 + (double)p0 * a.dx);
    s_re = in ? rows[5 * st + r] : 1.0; s_im = in ? rows[6 * st + r] : 0.0;
  } else {
    const int p0 = L.ty0 + L.sg * kFocalSeg;
    const double base = in ? rows[st + r] : 0.0, kb = in ? rows[3 * st + r] : 0.0, kc = in ? rows[4 * st + r] : 0.0;
    ph = (base + sh * kc) + kb * (a.y0 + (double)p0 * a.dy);
    s_re = in ? rows[7 * st + r] : 1.0; s_im = in ? rows[8 * st + r] : 0.0;
  }
}

// ... or formed at the wavenumber kj from k_focal_spectrum_prep's rows, with the operations and their order of
// k_focal_prep (one more sincos per lane and chunk): the same values as the rows of k_focal_prep at k = kj
__device__ __forceinline__ void focal_phase_terms_at(const double kj, const FocalArg& a, const double* __restrict__ rows,
                                                     const FocalLane& L, const int64_t r, const bool in, const double sh,
                                                     double& ph, double& s_re, double& s_im) {
  const int64_t st = a.stride;
  if (L.colw) {
    const int p0 = L.tx0 + L.sg * kFocalSeg;
    const double ka = focal_mul(kj, in ? rows[2 * st + r] : 0.0);
    ph = ka * (a.x0 + (double)p0 * a.dx);
    sincos(focal_mul(ka, a.dx), &s_im, &s_re);
  } else {
    const int p0 = L.ty0 + L.sg * kFocalSeg;
    const double base = focal_mul(kj, in ? rows[st + r] : 0.0), kb = focal_mul(kj, in ? rows[3 * st + r] : 0.0),
                 kc = focal_mul(kj, in ? rows[4 * st + r] : 0.0);
    ph = (base + sh * kc) + kb * (a.y0 + (double)p0 * a.dy);
    sincos(focal_mul(kb, a.dy), &s_im, &s_re);
  }
}

// the staging lane's kFocalSeg phasors of its ray: z at the segment's first pixel, then rotated by s pixel by pixel
__device__ __forceinline__ void focal_rotate_store(FocalStage& sU, FocalStage& sW, const FocalLane& L, double z_re,
                                                   double z_im, const double s_re, const double s_im) {
  double2* dst = L.colw ? &sU[L.sr][L.sg * kFocalSeg] : &sW[L.sr][L.sg * kFocalSeg];
#pragma unroll
  for (int m = 0; m < kFocalSeg; ++m) {
    dst[m] = make_double2(z_re, z_im);
    const double n_re = fma(z_re, s_re, -(z_im * s_im));
    z_im = fma(z_re, s_im, z_im * s_re);
    z_re = n_re;
  }
}

// acc += W U^T over the chunk's rays, for the lane's 4 x 4 pixels (between the kernel's two barriers)
__device__ __forceinline__ void focal_accumulate(const FocalStage& sU, const FocalStage& sW, const FocalLane& L,
                                                 FocalAcc& acc_re, FocalAcc& acc_im) {
#pragma unroll 2
  for (int rr = 0; rr < kFocalChunk; ++rr) {
    double2 uu[kFocalMicro], vv[kFocalMicro];
#pragma unroll
    for (int i = 0; i < kFocalMicro; ++i) {
      uu[i] = sU[rr][L.lx + kFocalLanes * i];
      vv[i] = sW[rr][L.ly + kFocalLanes * i];
    }
#pragma unroll
    for (int v = 0; v < kFocalMicro; ++v)
#pragma unroll
      for (int u = 0; u < kFocalMicro; ++u) {
        acc_re[v][u] = fma(vv[v].x, uu[u].x, acc_re[v][u]);
        acc_re[v][u] = fma(-vv[v].y, uu[u].y, acc_re[v][u]);
        acc_im[v][u] = fma(vv[v].x, uu[u].y, acc_im[v][u]);
        acc_im[v][u] = fma(vv[v].y, uu[u].x, acc_im[v][u]);
      }
  }
}

// the lane's 4 x 4 complex sums into the [ny][nx] plane at o, pixels beyond the grid left out
__device__ __forceinline__ void focal_store(double2* __restrict__ o, const FocalArg& a, const FocalLane& L,
                                            const FocalAcc& acc_re, const FocalAcc& acc_im) {
#pragma unroll
  for (int v = 0; v < kFocalMicro; ++v)
#pragma unroll
    for (int u = 0; u < kFocalMicro; ++u) {
      const int l = L.ty0 + L.ly + kFocalLanes * v, j = L.tx0 + L.lx + kFocalLanes * u;
      if (l < a.ny && j < a.nx) o[(int64_t)l * a.nx + j] = make_double2(acc_re[v][u], acc_im[v][u]);
    }
}

__global__ __launch_bounds__(kBlock) void k_focal_field(const FocalArg a, const double* __restrict__ rows,
                                                        double* __restrict__ out) {
  __shared__ FocalStage sU;                           // exp(i X_j k d.e1)
  __shared__ FocalStage sW;                           // amp exp(i (base + s_q k d.n + Y_l k d.e2))
  const int q = blockIdx.y, slice = blockIdx.z;
  const FocalLane L = focal_lane(a.tiles_x);
  const int64_t r0 = (int64_t)slice * a.per_slice;
  const int64_t r1 = (r0 + a.per_slice < a.n) ? r0 + a.per_slice : a.n;
  const double sh = a.shift[q];
  FocalAcc acc_re = {}, acc_im = {};

  for (int64_t c0 = r0; c0 < r1; c0 += kFocalChunk) {
    const int64_t r = c0 + L.sr;
    const bool in = r < r1;                       // beyond the slice: a zero row phasor, nothing is added
    double ph, s_re, s_im, sn, cs;
    focal_phase_terms(a, rows, L, r, in, sh, ph, s_re, s_im);
    const double amp = L.colw ? 1.0 : (in ? rows[r] : 0.0);
    sincos(ph, &sn, &cs);
    focal_rotate_store(sU, sW, L, amp * cs, amp * sn, s_re, s_im);
    __syncthreads();
    focal_accumulate(sU, sW, L, acc_re, acc_im);
    __syncthreads();
  }
  focal_store(reinterpret_cast<double2*>(out) + ((int64_t)slice * a.planes + q) * a.ny * a.nx, a, L, acc_re, acc_im);
}

// field[p] = sum over the slices in slice order of partial[slice][p]
__global__ __launch_bounds__(kBlock) void k_focal_fold(const double2* __restrict__ part, const int slices,
                                                       const int64_t pixels, double2* __restrict__ field) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * kBlock) {
    double re = 0.0, im = 0.0;
    for (int s = 0; s < slices; ++s) {
      const double2 v = part[(int64_t)s * pixels + p];
      re += v.x;
      im += v.y;
    }
    field[p] = make_double2(re, im);
  }
}

// ------------------------------------------------------------------------------------------- focal image
// art_focal_image: the partially coherent image of an extended source, I_q = sum_g |sum_{r in g} ...|^2 over groups g
// of slots [seg[g], seg[g+1]) (seg on the device, never read by the host).  k_focal_prep's rows, then k_focal_image:
// k_focal_field's loop run group by group -- a chunk never
// straddles two groups, the tail of a group's last chunk has amplitude 0 -- and at the end of a group every lane adds
// re^2 + im^2 of its 16 complex sums to 16 real ones and clears the complex ones.  Grid: (tile, plane x slice), a slice
// a contiguous range of `per` groups; partials [plane][slice][ny][nx] go through k_focal_image_fold in slice order.
// With so few groups that slices of them cannot fill the machine (split > 1) a workgroup instead takes one of `split`
// chunk-aligned pieces of ONE group and writes its complex sum [plane][group][piece][ny][nx]; k_focal_image_fold_split
// adds a group's pieces in order, squares, and adds the groups in order.  Offsets are clamped to [0, n] and
// seg[g+1] <= seg[g] is an empty group: safe for any contents of seg.  No float atomics: the same bytes on every call.
__global__ __launch_bounds__(kBlock) void k_focal_image(const FocalArg a, const double* __restrict__ rows,
                                                        const int64_t* __restrict__ seg, const int groups, const int per,
                                                        const int slices, const int split, double* __restrict__ out) {
  __shared__ FocalStage sU;                           // exp(i X_j k d.e1)
  __shared__ FocalStage sW;                           // amp exp(i (base + s_q k d.n + Y_l k d.e2))
  const int job = blockIdx.y;                         // split == 1: (plane, slice); else (plane, group, piece)
  const int q = split > 1 ? job / (groups * split) : job / slices;
  const int g0 = split > 1 ? (job / split) % groups : (job % slices) * per;
  const int g1 = split > 1 ? g0 + 1 : (g0 + per < groups ? g0 + per : groups);
  const int piece = job % split;
  const FocalLane L = focal_lane(a.tiles_x);
  const double sh = a.shift[q];
  FocalAcc acc_re = {}, acc_im = {}, acc_in = {};

  for (int g = g0; g < g1; ++g) {
    int64_t r0 = seg[g], r1 = seg[g + 1];
    r0 = r0 < 0 ? 0 : (r0 > a.n ? a.n : r0);
    r1 = r1 < 0 ? 0 : (r1 > a.n ? a.n : r1);
    if (split > 1 && r1 > r0) {                       // this piece of the group, a whole number of chunks
      const int64_t chunks = (r1 - r0 + kFocalChunk - 1) / kFocalChunk;
      const int64_t len = (chunks + split - 1) / split * kFocalChunk;
      r0 += piece * len;
      if (r0 + len < r1) r1 = r0 + len;
    }
    for (int64_t c0 = r0; c0 < r1; c0 += kFocalChunk) {
      const int64_t r = c0 + L.sr;
      const bool in = r < r1;                     // beyond the group: a zero row phasor, nothing is added
      double ph, s_re, s_im, sn, cs;
      focal_phase_terms(a, rows, L, r, in, sh, ph, s_re, s_im);
      const double amp = L.colw ? 1.0 : (in ? rows[r] : 0.0);
      sincos(ph, &sn, &cs);
      focal_rotate_store(sU, sW, L, amp * cs, amp * sn, s_re, s_im);
      __syncthreads();
      focal_accumulate(sU, sW, L, acc_re, acc_im);
      __syncthreads();
    }
    if (split > 1) break;                         // the piece's complex sum is the result
#pragma unroll
    for (int v = 0; v < kFocalMicro; ++v)
#pragma unroll
      for (int u = 0; u < kFocalMicro; ++u) {
        acc_in[v][u] = fma(acc_re[v][u], acc_re[v][u], fma(acc_im[v][u], acc_im[v][u], acc_in[v][u]));
        acc_re[v][u] = acc_im[v][u] = 0.0;
      }
  }
  const int64_t o = (int64_t)job * a.ny * a.nx;
  if (split > 1) {
    focal_store(reinterpret_cast<double2*>(out) + o, a, L, acc_re, acc_im);
    return;
  }
#pragma unroll
  for (int v = 0; v < kFocalMicro; ++v)
#pragma unroll
    for (int u = 0; u < kFocalMicro; ++u) {
      const int l = L.ty0 + L.ly + kFocalLanes * v, j = L.tx0 + L.lx + kFocalLanes * u;
      if (l < a.ny && j < a.nx) out[o + (int64_t)l * a.nx + j] = acc_in[v][u];
    }
}

// image[q][p] = sum over the slices in slice order of partial[q][slice][p]
__global__ __launch_bounds__(kBlock) void k_focal_image_fold(const double* __restrict__ part, const int slices,
                                                             const int64_t pixels, const int64_t total,
                                                             double* __restrict__ image) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < total; p += (int64_t)gridDim.x * kBlock) {
    const int64_t q = p / pixels, px = p - q * pixels;
    double v = 0.0;
    for (int s = 0; s < slices; ++s) v += part[(q * slices + s) * pixels + px];
    image[p] = v;
  }
}

// image[q][p] = sum over the groups in order of |sum over the pieces in order of partial[q][group][piece][p]|^2
__global__ __launch_bounds__(kBlock) void k_focal_image_fold_split(const double2* __restrict__ part, const int groups,
                                                                   const int split, const int64_t pixels,
                                                                   const int64_t total, double* __restrict__ image) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < total; p += (int64_t)gridDim.x * kBlock) {
    const int64_t q = p / pixels, px = p - q * pixels;
    double v = 0.0;
    for (int g = 0; g < groups; ++g) {
      double re = 0.0, im = 0.0;
      for (int s = 0; s < split; ++s) {
        const double2 z = part[((q * groups + g) * split + s) * pixels + px];
        re += z.x;
        im += z.y;
      }
      v = fma(re, re, fma(im, im, v));
    }
    image[p] = v;
  }
}

// ------------------------------------------------------------------------------------------- focal spectrum
// art_focal_spectrum: the focal field at nk wavenumbers k_j = k_0 + j dk from one bundle (mirrors are achromatic, so
// only the phase k (optical path) changes with k).  k_focal_spectrum_prep writes the k-independent rows of each slot
// (amp, base / k, d.e1, d.e2, d.n; a dead slot gets amplitude 0).  k_focal_spectrum_field is k_focal_field with
// (plane, wavenumber) on the grid's y dimension and focal_phase_terms_at in the staging lanes; everything after the
// phase terms is k_focal_field's code, so a slice equals art_focal_field's at k = k_j.  The slices' partials go
// through k_focal_fold.
constexpr int kFocalSpecRows = 5;     // amp, base / k, d.e1, d.e2, d.n

// k_j = k_0 + j * dk, unfused (k_0 exactly at j = 0); the host's validation forms it the same way
__host__ __device__ inline double focal_kj(const double k0, const int j, const double dk) {
#pragma clang fp contract(off)
  return k0 + (double)j * dk;
}

__global__ __launch_bounds__(kBlock) void k_focal_spectrum_prep(const FocalArg a, const ArtBundleView b,
                                                                const double* w, const int64_t m, double* rows) {
#pragma clang fp contract(off)
  const int64_t st = a.stride;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const bool live = b.alive[i] != 0;
    const double px = b.ox[i], py = b.oy[i], pz = b.oz[i], dx = b.dx[i], dy = b.dy[i], dz = b.dz[i];
    // a dead slot's values are unspecified (possibly NaN): selected away
    const double amp = live ? (w ? sqrt(w[i]) : 1.0) : 0.0;
    const double base = live ? (b.path[i] - a.L_ref) + ((dx * (a.C[0] - px) + dy * (a.C[1] - py)) + dz * (a.C[2] - pz))
                             : 0.0;
    const double da = live ? (dx * a.e1[0] + dy * a.e1[1]) + dz * a.e1[2] : 0.0;
    const double db = live ? (dx * a.e2[0] + dy * a.e2[1]) + dz * a.e2[2] : 0.0;
    const double dc = live ? (dx * a.nrm[0] + dy * a.nrm[1]) + dz * a.nrm[2] : 0.0;
    rows[i] = amp; rows[st + i] = base; rows[2 * st + i] = da; rows[3 * st + i] = db; rows[4 * st + i] = dc;
  }
}

// blockIdx.y = q * nk + j (plane q, wavenumber j): out is [slice][planes][nk][ny][nx]
__global__ __launch_bounds__(kBlock) void k_focal_spectrum_field(const FocalArg a, const double dk, const int nk,
                                                                 const double* __restrict__ rows,
                                                                 double* __restrict__ out) {
  __shared__ FocalStage sU;                           // exp(i X_j k d.e1)
  __shared__ FocalStage sW;                           // amp exp(i (base + s_q k d.n + Y_l k d.e2))
  const int qj = blockIdx.y, q = qj / nk, slice = blockIdx.z;
  const double kj = focal_kj(a.k, qj - q * nk, dk);
  const FocalLane L = focal_lane(a.tiles_x);
  const int64_t r0 = (int64_t)slice * a.per_slice;
  const int64_t r1 = (r0 + a.per_slice < a.n) ? r0 + a.per_slice : a.n;
  const double sh = a.shift[q];
  FocalAcc acc_re = {}, acc_im = {};

  for (int64_t c0 = r0; c0 < r1; c0 += kFocalChunk) {
    const int64_t r = c0 + L.sr;
    const bool in = r < r1;                       // beyond the slice: a zero row phasor, nothing is added
    double ph, s_re, s_im, sn, cs;
    focal_phase_terms_at(kj, a, rows, L, r, in, sh, ph, s_re, s_im);
    const double amp = L.colw ? 1.0 : (in ? rows[r] : 0.0);
    sincos(ph, &sn, &cs);
    focal_rotate_store(sU, sW, L, amp * cs, amp * sn, s_re, s_im);
    __syncthreads();
    focal_accumulate(sU, sW, L, acc_re, acc_im);
    __syncthreads();
  }
  focal_store(reinterpret_cast<double2*>(out) + ((int64_t)slice * gridDim.y + qj) * a.ny * a.nx, a, L, acc_re, acc_im);
}

// ------------------------------------------------------------------------------------------- focal chromatic
// art_focal_chromatic (include/art_hip.h): art_focal_spectrum's sum for a source whose divergence and apparent position
// along the unit axis a depend on the frequency.  Per slot r, from the slot-aligned SOURCE bundle's direction s_r,
//     u_r = 0.5 * (((s_x - a_x)^2 + (s_y - a_y)^2) + (s_z - a_z)^2)        (this order, no fma: 1 - cos theta_r)
// and per wavenumber j a table row (k_j, c_j, z_j, 0):
//     field[q][j] = sum_r sqrt(w_r) exp(-(u_r c_j)) exp(i [k_j * (base_r / k + z_j * u_r) + shift, X and Y terms])
// k_focal_chromatic_prep is k_focal_spectrum_prep with a sixth row u (a dead slot of the FINAL bundle gets u = 0,
// whatever the source slot holds).  k_focal_chromatic_field is k_focal_spectrum_field with k_j read from the table (one
// row per workgroup, uniform) and the two new terms in the row-phasor staging lanes: base_r / k + z_j * u_r before the
// product with k_j, and the amplitude times exp(-(u_r c_j)).  With c_j = z_j = 0 these add +0.0 and multiply by 1: the
// roundings, and so the bytes, of k_focal_spectrum_field at k = k_j.  Everything after the phase terms is the shared code.
constexpr int kFocalChromRows = 6;    // amp, base / k, d.e1, d.e2, d.n, u

__global__ __launch_bounds__(kBlock) void k_focal_chromatic_prep(const FocalArg a, const ArtBundleView b,
                                                                 const ArtBundleView src, const double ax,
                                                                 const double ay, const double az, const double* w,
                                                                 const int64_t m, double* rows) {
#pragma clang fp contract(off)
  const int64_t st = a.stride;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
    const bool live = b.alive[i] != 0;
    const double px = b.ox[i], py = b.oy[i], pz = b.oz[i], dx = b.dx[i], dy = b.dy[i], dz = b.dz[i];
    const double sx = src.dx[i] - ax, sy = src.dy[i] - ay, sz = src.dz[i] - az;
    // a dead slot's values are unspecified (possibly NaN), in either bundle: selected away
    const double amp = live ? (w ? sqrt(w[i]) : 1.0) : 0.0;
    const double base = live ? (b.path[i] - a.L_ref) + ((dx * (a.C[0] - px) + dy * (a.C[1] - py)) + dz * (a.C[2] - pz))
                             : 0.0;
    const double da = live ? (dx * a.e1[0] + dy * a.e1[1]) + dz * a.e1[2] : 0.0;
    const double db = live ? (dx * a.e2[0] + dy * a.e2[1]) + dz * a.e2[2] : 0.0;
    const double dc = live ? (dx * a.nrm[0] + dy * a.nrm[1]) + dz * a.nrm[2] : 0.0;
    const double u = live ? 0.5 * ((sx * sx + sy * sy) + sz * sz) : 0.0;
    rows[i] = amp; rows[st + i] = base; rows[2 * st + i] = da; rows[3 * st + i] = db; rows[4 * st + i] = dc;
    rows[5 * st + i] = u;
  }
}

// base / k + z_j * u, unfused: with z_j = 0 it is base / k itself
__device__ __forceinline__ double focal_chromatic_path(const double base, const double zj, const double u) {
#pragma clang fp contract(off)
  return base + zj * u;
}

// focal_phase_terms_at for a source moved by zj along the axis (u: the slot's row 5, 0 outside the workgroup's rays):
// the column lanes' terms are focal_phase_terms_at's own, the row lanes' have base / k + zj * u in place of base / k
__device__ __forceinline__ void focal_phase_terms_chromatic(const double kj, const double zj, const double u,
                                                            const FocalArg& a, const double* __restrict__ rows,
                                                            const FocalLane& L, const int64_t r, const bool in,
                                                            const double sh, double& ph, double& s_re, double& s_im) {
  if (L.colw) {
    focal_phase_terms_at(kj, a, rows, L, r, in, sh, ph, s_re, s_im);
    return;
  }
  const int64_t st = a.stride;
  const int p0 = L.ty0 + L.sg * kFocalSeg;
  const double base = focal_mul(kj, focal_chromatic_path(in ? rows[st + r] : 0.0, zj, u)),
               kb = focal_mul(kj, in ? rows[3 * st + r] : 0.0), kc = focal_mul(kj, in ? rows[4 * st + r] : 0.0);
  ph = (base + sh * kc) + kb * (a.y0 + (double)p0 * a.dy);
  sincos(focal_mul(kb, a.dy), &s_im, &s_re);
}

// blockIdx.y = q * nk + j (plane q, table row j): out is [slice][planes][nk][ny][nx]
__global__ __launch_bounds__(kBlock) void k_focal_chromatic_field(const FocalArg a, const double* __restrict__ table,
                                                                  const int nk, const double* __restrict__ rows,
                                                                  double* __restrict__ out) {
  __shared__ FocalStage sU;                           // exp(i X_j k d.e1)
  __shared__ FocalStage sW;                           // amp exp(-u c) exp(i (k (base / k + z u) + s_q k d.n + Y_l k d.e2))
  const int qj = blockIdx.y, q = qj / nk, slice = blockIdx.z;
  const double* row = table + 4 * (qj - q * nk);      // (k_j, c_j, z_j, 0): the same for every lane
  const double kj = row[0], cj = row[1], zj = row[2];
  const FocalLane L = focal_lane(a.tiles_x);
  const int64_t r0 = (int64_t)slice * a.per_slice;
  const int64_t r1 = (r0 + a.per_slice < a.n) ? r0 + a.per_slice : a.n;
  const double sh = a.shift[q];
  FocalAcc acc_re = {}, acc_im = {};

  for (int64_t c0 = r0; c0 < r1; c0 += kFocalChunk) {
    const int64_t r = c0 + L.sr;
    const bool in = r < r1;                       // beyond the slice: a zero row phasor, nothing is added
    double ph, s_re, s_im, sn, cs;
    const double u = (!L.colw && in) ? rows[5 * a.stride + r] : 0.0;
    focal_phase_terms_chromatic(kj, zj, u, a, rows, L, r, in, sh, ph, s_re, s_im);
    const double amp = L.colw ? 1.0 : (in ? rows[r] : 0.0) * exp(-focal_mul(u, cj));
    sincos(ph, &sn, &cs);
    focal_rotate_store(sU, sW, L, amp * cs, amp * sn, s_re, s_im);
    __syncthreads();
    focal_accumulate(sU, sW, L, acc_re, acc_im);
    __syncthreads();
  }
  focal_store(reinterpret_cast<double2*>(out) + ((int64_t)slice * gridDim.y + qj) * a.ny * a.nx, a, L, acc_re, acc_im);
}

// ------------------------------------------------------------------------------------------- wavefront
// art_wavefront: per job the Gram matrix G = sum_r w_r v_r v_r^T of the rows v_r = [Z_0 .. Z_{J-1}, d.n, W_r]
// (include/art_hip.h); the Zernike fit and the best reference point are small dense algebra on G, done by the caller.
// k_wavefront_prep: one pass per job over its slots into kWfRows rows of scratch (w, W, d.e1 - a1, d.e2 - a2, d.n; a
// slot that is not alive gets W = NaN and zeros elsewhere) and, per workgroup, the largest (d.e1 - a1)^2 + (d.e2 - a2)^2
// of its alive rays (the default pupil radius).  k_wavefront_gram<N>: grid = (ray slices, jobs of order N).  Per chunk
// of kWfChunk rays, kWfStage lanes of every wave stage one ray each -- pupil coordinates, all J polynomials by the
// recurrences (zernike_values), the K columns into LDS once scaled by w and once not -- then the lanes own 4 x 4 blocks
// of the K x K upper triangle (K padded to KP = 4 B) and accumulate them with fp64 FMAs, in kBlock / (B (B + 1) / 2)
// lane groups that take turns over the chunk's rays.  At the end of its slice a workgroup adds the groups' blocks in
// group order and writes the packed triangle and the slice's statistics.  k_wavefront_fold adds the slices of every job
// in slice order.  No float atomics; a job's slicing depends on its own n: the same bytes whichever jobs share the call.
constexpr int kWfRows = 5;
constexpr int kWfChunk = 64;          // rays per LDS stage
constexpr int kWfStage = 16;          // staging lanes per wave: the staging work is spread over the four SIMDs
constexpr int kWfPrepBlocks = 1024;   // workgroups per job of the prep at most (one radius partial each)
constexpr int kWfMaxSlices = 512;     // two workgroups per CU for one large job
constexpr int kWfStats = 8;           // per slice behind the triangle: used, outside, sum w, rho, min W, max W, 0, 0
static_assert(kWfStage * (kBlock / 64) == kWfChunk, "one staged ray per staging lane");

__host__ __device__ inline int wf_cols(const int order) { return (order + 1) * (order + 2) / 2 + 2; }
__host__ __device__ inline int64_t wf_stride(const int64_t n) { return (n + 63) / 64 * 64; }
// slices of a job: at least 4 chunks of rays each, kWfMaxSlices at most; whole chunks per slice
__host__ __device__ inline int wf_slices(const int64_t n) {
  const int64_t s = (n + 4 * kWfChunk - 1) / (4 * kWfChunk);
  return s < 1 ? 1 : (s > kWfMaxSlices ? kWfMaxSlices : (int)s);
}
__host__ __device__ inline int64_t wf_per_slice(const int64_t n, const int slices) {
  const int64_t p = (n + slices - 1) / slices;
  return p < 1 ? kWfChunk : (p + kWfChunk - 1) / kWfChunk * kWfChunk;
}
inline int64_t wf_per_job(const int64_t nmax, const int kmax) {
  return kWfRows * wf_stride(nmax) + kWfPrepBlocks + (int64_t)wf_slices(nmax) * (kmax * (kmax + 1) / 2 + kWfStats);
}

struct WfArg {
  int64_t per_job;      // scratch doubles per job: rows (kWfRows x stride), radius partials, slice partials
  int64_t stride;       // row stride of the prep rows
  int32_t prep_blocks;  // workgroups per job of the prep
  int32_t job0;         // first job of a gram launch
};

template <int N>
struct WfShape {
  static constexpr int J = (N + 1) * (N + 2) / 2, K = J + 2, T = K * (K + 1) / 2;
  static constexpr int KP = (K + 3) / 4 * 4, B = KP / 4, NB = B * (B + 1) / 2;
  static constexpr int G = kBlock / NB;            // lane groups
  static constexpr int HALF = KP / 2;              // doubles per ray in each half of a stage
  static constexpr int STAGE = 4 * kWfChunk * HALF;
  static constexpr int LDS = STAGE > G * NB * 16 ? STAGE : G * NB * 16;
  static_assert(G >= 1, "at most kBlock blocks");
};

__global__ __launch_bounds__(kBlock) void k_wavefront_prep(const ArtWavefrontJob* __restrict__ jobs, const WfArg a,
                                                           double* scratch) {
#pragma clang fp contract(off)
  __shared__ double red[kBlock];
  const ArtWavefrontJob& jb = jobs[blockIdx.y];
  const int t = threadIdx.x;
  const int64_t n = jb.n, st = a.stride;
  double* rows = scratch + (int64_t)blockIdx.y * a.per_job;
  const double* C = jb.det.centre;
  const double* e1 = jb.det.rot;
  const double* e2 = jb.det.rot + 3;
  const double* nr = jb.det.normal;
  const double R0 = ((C[0] + jb.ref[0] * e1[0]) + jb.ref[1] * e2[0]) - jb.ref[2] * nr[0];
  const double R1 = ((C[1] + jb.ref[0] * e1[1]) + jb.ref[1] * e2[1]) - jb.ref[2] * nr[1];
  const double R2 = ((C[2] + jb.ref[0] * e1[2]) + jb.ref[1] * e2[2]) - jb.ref[2] * nr[2];
  const double a1 = jb.pupil[0], a2 = jb.pupil[1], L = jb.L_ref;
  double m2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + t; i < n; i += (int64_t)gridDim.x * kBlock) {
    const bool live = jb.b.alive[i] != 0;
    const double px = jb.b.ox[i], py = jb.b.oy[i], pz = jb.b.oz[i], dx = jb.b.dx[i], dy = jb.b.dy[i], dz = jb.b.dz[i];
    // a dead slot's values are unspecified (possibly NaN): selected away
    const double W = (jb.b.path[i] - L) + ((dx * (R0 - px) + dy * (R1 - py)) + dz * (R2 - pz));
    const double xr = ((dx * e1[0] + dy * e1[1]) + dz * e1[2]) - a1;
    const double yr = ((dx * e2[0] + dy * e2[1]) + dz * e2[2]) - a2;
    const double dn = (dx * nr[0] + dy * nr[1]) + dz * nr[2];
    rows[i] = live ? (jb.w ? jb.w[i] : 1.0) : 0.0;
    rows[st + i] = live ? W : NAN;
    rows[2 * st + i] = live ? xr : 0.0;
    rows[3 * st + i] = live ? yr : 0.0;
    rows[4 * st + i] = live ? dn : 0.0;
    if (live) m2 = fmax(m2, xr * xr + yr * yr);
  }
  red[t] = m2;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (t < h) red[t] = fmax(red[t], red[t + h]);
    __syncthreads();
  }
  if (t == 0) rows[kWfRows * st + blockIdx.x] = red[0];
}

template <int N>
__global__ __launch_bounds__(kBlock) void k_wavefront_gram(const ArtWavefrontJob* __restrict__ jobs, const WfArg a,
                                                           double* scratch) {
#pragma clang fp contract(off)
  using S = WfShape<N>;
  __shared__ __attribute__((aligned(16))) double lds[S::LDS];
  __shared__ double red[kBlock];
  const int j = a.job0 + (int)blockIdx.y, slice = blockIdx.x, t = threadIdx.x;
  const ArtWavefrontJob& jb = jobs[j];
  const int64_t n = jb.n, st = a.stride;
  const int nslices = wf_slices(n);
  if (slice >= nslices) return;                         // (the launch covers the largest job of the run)
  const double* rows = scratch + (int64_t)j * a.per_job;
  double* part = scratch + (int64_t)j * a.per_job + kWfRows * st + kWfPrepBlocks + (int64_t)slice * (S::T + kWfStats);
  // the pupil radius: given, or the largest transverse distance over the prep's partials (a max: any order)
  double rho = jb.pupil[2];
  const bool given = rho > 0.0;
  if (!given) {
    double m = 0.0;
    for (int p = t; p < a.prep_blocks; p += kBlock) m = fmax(m, rows[kWfRows * st + p]);
    red[t] = m;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if (t < h) red[t] = fmax(red[t], red[t + h]);
      __syncthreads();
    }
    rho = red[0] > 0.0 ? sqrt(red[0]) : 1.0;
    __syncthreads();
  }
  const int64_t per = wf_per_slice(n, nslices), r0 = (int64_t)slice * per;
  const int64_t r1 = (r0 + per < n) ? r0 + per : n;
  // staging role: ray sr of the chunk
  const bool stager = (t & 63) < kWfStage;
  const int sr = (t >> 6) * kWfStage + (t & 63);
  // accumulating role: group g, block (bi, bj) of the upper triangle of blocks
  const int g = t / S::NB, blk = t % S::NB;
  const bool worker = g < S::G;
  int bi = 0, q = blk;
  while (q >= S::B - bi) { q -= S::B - bi; ++bi; }
  const int bj = bi + q;
  double* sA = lds;                          // w v, halves [2][kWfChunk][HALF]: columns 4b + {0, 1} | 4b + {2, 3}
  double* sB = lds + 2 * kWfChunk * S::HALF; // v
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  double used_n = 0.0, out_n = 0.0, wmin = INFINITY, wmax = -INFINITY;

  for (int64_t c0 = r0; c0 < r1; c0 += kWfChunk) {
    if (stager) {
      const int64_t r = c0 + sr;
      double w = 0.0, W = 0.0, x = 0.0, y = 0.0, dn = 0.0;
      bool used = false;
      if (r < r1) {
        W = rows[st + r];
        if (W == W) {                                   // alive
          x = rows[2 * st + r] / rho;
          y = rows[3 * st + r] / rho;
          used = !given || x * x + y * y <= 1.0;
          if (used) {
            w = rows[r];
            dn = rows[4 * st + r];
            used_n += 1.0;
            wmin = fmin(wmin, W);
            wmax = fmax(wmax, W);
          } else {
            out_n += 1.0;
          }
        }
        if (jb.opd) jb.opd[r] = used ? W : NAN;
        if (jb.pupil_x) jb.pupil_x[r] = used ? x : NAN;
        if (jb.pupil_y) jb.pupil_y[r] = used ? y : NAN;
      }
      if (!used) x = y = 0.0;
      auto put = [&](const int col, const double z) {
        const double v = used ? z : 0.0;
        const int off = (((col >> 1) & 1) * kWfChunk + sr) * S::HALF + (col >> 2) * 2 + (col & 1);
        sB[off] = v;
        sA[off] = w * v;
      };
      art::zernike_values<N>(x, y, put);
      put(S::J, dn);
      put(S::J + 1, W);
#pragma unroll
      for (int col = S::K; col < S::KP; ++col) put(col, 0.0);
    }
    __syncthreads();
    if (worker) {
#pragma unroll 2
      for (int rr = g; rr < kWfChunk; rr += S::G) {
        const double2 a0 = *reinterpret_cast<const double2*>(sA + rr * S::HALF + 2 * bi);
        const double2 a1 = *reinterpret_cast<const double2*>(sA + (kWfChunk + rr) * S::HALF + 2 * bi);
        const double2 b0 = *reinterpret_cast<const double2*>(sB + rr * S::HALF + 2 * bj);
        const double2 b1 = *reinterpret_cast<const double2*>(sB + (kWfChunk + rr) * S::HALF + 2 * bj);
        const double av[4] = {a0.x, a0.y, a1.x, a1.y}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] = fma(av[u], bv[v], acc[u][v]);
      }
    }
    __syncthreads();
  }
  // the groups' blocks, added in group order; the stagers' statistics in lane order
  if (worker) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) lds[(g * S::NB + blk) * 16 + u * 4 + v] = acc[u][v];
  }
  if (stager) {
    red[sr] = used_n;
    red[kWfChunk + sr] = out_n;
    red[2 * kWfChunk + sr] = wmin;
    red[3 * kWfChunk + sr] = wmax;
  }
  __syncthreads();
  for (int e = t; e < S::NB * 16; e += kBlock) {
    const int bb = e >> 4, k = e & 15;
    int i0 = 0, qq = bb;
    while (qq >= S::B - i0) { qq -= S::B - i0; ++i0; }
    const int i = 4 * i0 + (k >> 2), jj = 4 * (i0 + qq) + (k & 3);
    if (i <= jj && jj < S::K) {
      double s = 0.0;
      for (int gg = 0; gg < S::G; ++gg) s += lds[(gg * S::NB + bb) * 16 + k];
      part[i * (2 * S::K - i - 1) / 2 + jj] = s;
      if (e == 0) part[S::T + 2] = s;                 // sum w = G[0][0] (Z_0 = 1)
    }
  }
  if (t == 0) {
    double c = 0.0, o = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int l = 0; l < kWfChunk; ++l) {
      c += red[l];
      o += red[kWfChunk + l];
      lo = fmin(lo, red[2 * kWfChunk + l]);
      hi = fmax(hi, red[3 * kWfChunk + l]);
    }
    part[S::T] = c;
    part[S::T + 1] = o;
    part[S::T + 3] = rho;
    part[S::T + 4] = lo;
    part[S::T + 5] = hi;
    part[S::T + 6] = 0.0;
    part[S::T + 7] = 0.0;
  }
}

// out = [used, outside, sum w, rho, min W, max W, K, 0, G packed, zeros]: every job's slices added in slice order (the
// loads of a thread are independent, so they are unrolled ahead of its additions: the fold is latency-bound otherwise)
__global__ __launch_bounds__(kBlock) void k_wavefront_fold(const ArtWavefrontJob* __restrict__ jobs, const WfArg a,
                                                           const double* scratch) {
  const int j = blockIdx.y;
  const ArtWavefrontJob& jb = jobs[j];
  const int K = wf_cols(jb.order), T = K * (K + 1) / 2, S = wf_slices(jb.n);
  const int64_t ps = T + kWfStats;
  const double* part = scratch + (int64_t)j * a.per_job + kWfRows * a.stride + kWfPrepBlocks;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < ART_WAVEFRONT_DOUBLES; e += gridDim.x * kBlock) {
    double v = 0.0;
    if (e >= 8 && e < 8 + T) {
#pragma unroll 16
      for (int s = 0; s < S; ++s) v += part[s * ps + (e - 8)];
    } else if (e < 6) {
      double used = 0.0;
#pragma unroll 16
      for (int s = 0; s < S; ++s) used += part[s * ps + T];
      if (e == 0) {
        v = used;
      } else if (e == 3) {
        v = part[T + 3];
      } else if (e == 4) {
        v = INFINITY;
#pragma unroll 16
        for (int s = 0; s < S; ++s) v = fmin(v, part[s * ps + T + 4]);
      } else if (e == 5) {
        v = -INFINITY;
#pragma unroll 16
        for (int s = 0; s < S; ++s) v = fmax(v, part[s * ps + T + 5]);
      } else {
#pragma unroll 16
        for (int s = 0; s < S; ++s) v += part[s * ps + T + e];
      }
      if (used == 0.0 && e >= 2) v = 0.0;
    } else if (e == 6) {
      v = (double)K;
    }
    jb.out[e] = v;
  }
}

template <int N>
void launch_wf_gram(const dim3 grid, hipStream_t s, const ArtWavefrontJob* jobs, const WfArg a, double* scratch) {
  hipLaunchKernelGGL(k_wavefront_gram<N>, grid, dim3(kBlock), 0, s, jobs, a, scratch);
}
using WfGramLaunch = void (*)(dim3, hipStream_t, const ArtWavefrontJob*, WfArg, double*);
constexpr WfGramLaunch kWfGram[ART_WAVEFRONT_MAX_ORDER + 1] = {
    launch_wf_gram<0>, launch_wf_gram<1>, launch_wf_gram<2>, launch_wf_gram<3>, launch_wf_gram<4>, launch_wf_gram<5>,
    launch_wf_gram<6>, launch_wf_gram<7>, launch_wf_gram<8>, launch_wf_gram<9>, launch_wf_gram<10>};

// ------------------------------------------------------------------------------------------- polarisation
// art_polarisation: one pass over a traced chain's history per job (include/art_hip.h; the per-ray math is art_coating.h).
// k_polarisation: grid (tiles of 256 slots, jobs), one ray per lane.  The slot's alive bytes in the source and the final
// bundle are read first; every other stream of a slot that is dead at the end is requested at an out-of-range offset
// (no traffic, reads 0, selected away).
// Job, views and coating table are wave-uniform: scalar loads.  Per tile kPolStats partials (block_reduce_store), folded
// per job in tile order by k_polarisation_fold (fold_range).  A job's tiles depend on its own n: same bytes in any batch.
constexpr int kPolStats = 11;   // [0] alive [1] sum w0 [2] sum w_out [3] min T [4] max T [5..9] Stokes, |E.n|^2 [10] min |P_perp|
__host__ __device__ inline int64_t pol_tiles(const int64_t n) { return n < 1 ? 1 : (n + kBlock - 1) / kBlock; }
constexpr int pol_op(const int q) { return (q == 3 || q == 10) ? RMIN : (q == 4 ? RMAX : RSUM); }

// The views are read through the constant address space: scalar loads (a pointer fetched from the job table is a
// generic one, and a generic load of a descriptor's base would need a waterfall loop around every buffer access)
typedef const ArtBundleView __attribute__((address_space(4)))* pol_view_t;
__device__ __forceinline__ void pol_dirs(const ArtBundleView* views, const int e, const unsigned nb8, const unsigned o8,
                                         double* d) {
  const pol_view_t v = (pol_view_t)views + e;
  d[0] = ld_f64(rsrc_of(v->dx, nb8), o8);
  d[1] = ld_f64(rsrc_of(v->dy, nb8), o8);
  d[2] = ld_f64(rsrc_of(v->dz, nb8), o8);
}
__device__ __forceinline__ uint8_t* pol_alive(const ArtBundleView* views, const int e) { return ((pol_view_t)views + e)->alive; }

__global__ __launch_bounds__(kBlock, 4) void k_polarisation(const ArtPolarisationJob* __restrict__ jobs,
                                                         const ArtCoating* __restrict__ coats, const int64_t per_job,
                                                         double* scratch) {
  __shared__ artc::cplx s_kz[ART_COATING_MAX_MATERIALS * kBlock];   // kz / k per material, one column per lane
  __shared__ double s_dir[6 * kBlock];                                     // d_in, d_out, one column per lane
  const ArtPolarisationJob& jb = jobs[blockIdx.y];
  const int64_t n = jb.n;
  if ((int64_t)blockIdx.x >= pol_tiles(n)) return;     // (the grid covers the largest job)
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned nb8 = (unsigned)(n * 8), nb1 = (unsigned)n;   // n <= 2^28 (checked by the host)
  const int K = jb.n_elems;
  const ArtBundleView* views = jb.views;
  const bool live = __builtin_amdgcn_raw_buffer_load_b8(rsrc_of(pol_alive(views, K), nb1), (int)i, 0, ART_LD_AUX) != 0;
  const bool live0 = __builtin_amdgcn_raw_buffer_load_b8(rsrc_of(pol_alive(views, 0), nb1), (int)i, 0, ART_LD_AUX) != 0;
  const unsigned o8 = live ? i * 8u : kDropOffset, o8s = live0 ? i * 8u : kDropOffset;
  const double w = jb.w ? ld_f64(rsrc_of(const_cast<double*>(jb.w), nb8), o8) : 1.0;
  const double w0 = jb.w0 ? ld_f64(rsrc_of(const_cast<double*>(jb.w0), nb8), o8s) : 1.0;
  double din[3];
  pol_dirs(views, 0, nb8, o8, din);
  const bool pol = jb.polarised != 0;
  // the input state(s), transverse to the source direction
  double er0[3], ei0[3], er1[3], ei1[3];
  double pmin = INFINITY;
  if (pol) {
    const double* P = jb.pol;
    const double pr = P[0] * din[0] + P[2] * din[1] + P[4] * din[2], pi = P[1] * din[0] + P[3] * din[1] + P[5] * din[2];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      er0[q] = P[2 * q] - pr * din[q];
      ei0[q] = P[2 * q + 1] - pi * din[q];
    }
    const double m = sqrt(er0[0] * er0[0] + er0[1] * er0[1] + er0[2] * er0[2] + ei0[0] * ei0[0] + ei0[1] * ei0[1] +
                          ei0[2] * ei0[2]);
    pmin = m;
#pragma unroll
    for (int q = 0; q < 3; ++q) { er0[q] /= m; ei0[q] /= m; er1[q] = ei1[q] = 0.0; }
  } else {
    artc::perp_unit(din[0], din[1], din[2], er0[0], er0[1], er0[2]);
    er1[0] = din[1] * er0[2] - din[2] * er0[1];
    er1[1] = din[2] * er0[0] - din[0] * er0[2];
    er1[2] = din[0] * er0[1] - din[1] * er0[0];
#pragma unroll
    for (int q = 0; q < 3; ++q) ei0[q] = ei1[q] = 0.0;
  }
  for (int e = 0; e < K; ++e) {
    double dout[3];
    pol_dirs(views, e + 1, nb8, o8, dout);
    const int c = jb.coating[e];
    if (c >= 0) {                                         // (a mask leaves E unchanged)
      // the two directions wait in LDS while the coefficients are formed (the Parratt loop needs every register)
      double* sd = s_dir + threadIdx.x;
#pragma unroll
      for (int q = 0; q < 3; ++q) { sd[q * kBlock] = din[q]; sd[(3 + q) * kBlock] = dout[q]; }
      artc::cplx rs, rp;
      artc::coating_rs_rp(coats[c], artc::cos_incidence(din, dout), jb.k, s_kz + threadIdx.x, kBlock, rs, rp);
      asm volatile("" ::: "memory");                      // (read them back: do not keep them in registers)
#pragma unroll
      for (int q = 0; q < 3; ++q) { din[q] = sd[q * kBlock]; dout[q] = sd[(3 + q) * kBlock]; }
      artc::Frame f;                                      // (formed after the coefficients: fewer registers live)
      artc::reflection_frame(din, dout, f);
      artc::prt_step(f, rs, rp, er0, ei0);
      if (!pol) artc::prt_step(f, rs, rp, er1, ei1);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) din[q] = dout[q];
  }
  const double T0 = (er0[0] * er0[0] + er0[1] * er0[1] + er0[2] * er0[2]) + (ei0[0] * ei0[0] + ei0[1] * ei0[1] + ei0[2] * ei0[2]);
  const double T1 = (er1[0] * er1[0] + er1[1] * er1[1] + er1[2] * er1[2]) + (ei1[0] * ei1[0] + ei1[1] * ei1[1] + ei1[2] * ei1[2]);
  const double T = pol ? T0 : 0.5 * (T0 + T1);
  const double wout = live ? w * T : 0.0;
  st_f64(rsrc_of(jb.w_out, nb8), i * 8u, wout);           // (slots >= n fall outside the descriptor)
  if (jb.field && (int64_t)i < n) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      jb.field[2 * ((int64_t)q * n + i)] = live ? er0[q] : 0.0;
      jb.field[2 * ((int64_t)q * n + i) + 1] = live ? ei0[q] : 0.0;
    }
  }
  double acc[kPolStats];
  acc[0] = live ? 1.0 : 0.0;
  acc[1] = live0 ? w0 : 0.0;
  acc[2] = wout;
  acc[3] = live ? T : INFINITY;
  acc[4] = live ? T : -INFINITY;
  double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (jb.has_det) {
    const double* e1 = jb.det.rot;
    const double* e2 = jb.det.rot + 3;
    const double* nd = jb.det.normal;
    auto stokes = [&](const double* er, const double* ei, const double scale) {
      const double xr = er[0] * e1[0] + er[1] * e1[1] + er[2] * e1[2], xi = ei[0] * e1[0] + ei[1] * e1[1] + ei[2] * e1[2];
      const double yr = er[0] * e2[0] + er[1] * e2[1] + er[2] * e2[2], yi = ei[0] * e2[0] + ei[1] * e2[1] + ei[2] * e2[2];
      const double zr = er[0] * nd[0] + er[1] * nd[1] + er[2] * nd[2], zi = ei[0] * nd[0] + ei[1] * nd[1] + ei[2] * nd[2];
      const double ix = xr * xr + xi * xi, iy = yr * yr + yi * yi;
      st[0] += scale * (ix + iy);
      st[1] += scale * (ix - iy);
      st[2] += scale * (2.0 * (xr * yr + xi * yi));
      st[3] += scale * (2.0 * (xr * yi - xi * yr));
      st[4] += scale * (zr * zr + zi * zi);
    };
    const double ws = live ? w : 0.0;
    stokes(er0, ei0, pol ? ws : 0.5 * ws);
    if (!pol) stokes(er1, ei1, 0.5 * ws);
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) acc[5 + q] = (live && jb.has_det) ? st[q] : 0.0;
  acc[10] = (live && pol) ? pmin : INFINITY;
  block_reduce_store<kPolStats>(acc, pol_op, scratch + (int64_t)blockIdx.y * per_job + (int64_t)blockIdx.x * kPolStats);
}

// grid (ART_POLARISATION_DOUBLES, jobs): workgroup (q, j) folds statistic q of job j's tiles in tile order
__global__ __launch_bounds__(kFoldBlock) void k_polarisation_fold(const ArtPolarisationJob* __restrict__ jobs,
                                                                  const int64_t per_job, const double* scratch) {
  const int q = blockIdx.x;
  const ArtPolarisationJob& jb = jobs[blockIdx.y];
  if (q >= kPolStats) {
    if (threadIdx.x == 0) jb.out[q] = 0.0;
    return;
  }
  const double* part = scratch + (int64_t)blockIdx.y * per_job;
  const int64_t tiles = pol_tiles(jb.n);
  double v = 0.0, cnt = 1.0;
  fold_range(part + q, 0, tiles, pol_op(q), &v, kPolStats);
  if (q == 3 || q == 4 || q == 10) {                      // a minimum or maximum over no ray is 0
    __syncthreads();
    fold_range(part, 0, tiles, RSUM, &cnt, kPolStats);
  }
  if (threadIdx.x == 0) jb.out[q] = (cnt == 0.0 || (q == 10 && !jb.polarised)) ? 0.0 : v;
}

// ------------------------------------------------------------------------------------------- ray tubes
// art_ray_tubes: one pass over a traced chain's history per job (include/art_hip.h; the per-ray math is art_tubes.h).
// k_ray_tubes: k_polarisation's shape -- grid (tiles of 256 slots, jobs), one ray per lane, the loop over the elements
// inside.  The slot's alive bytes in all K + 1 views are read first; every other stream of a slot that does not count is
// requested at an out-of-range offset (no traffic, reads 0, selected away).  Job, views, elements and quadrics are
// wave-uniform: scalar loads through the constant address space.  Per tile kTubeStats partials (block_reduce_store),
// folded per job in tile order by k_ray_tubes_fold (fold_range).  A job's tiles depend on its own n: same bytes in any batch.
constexpr int kTubeStats = 11;  // [0] count [1] sum w [2] sum w |sa| [3] min [4] max |sa| [5] sum w |area| [6..7] sum w kappa
                                // [8] sum w, [9] count of the rays with finite kappa [10] max relative asymmetry
constexpr int tube_op(const int q) { return q == 3 ? RMIN : ((q == 4 || q == 10) ? RMAX : RSUM); }
typedef const ArtElementDesc __attribute__((address_space(4)))* tube_elem_t;
typedef const ArtQuadricDesc __attribute__((address_space(4)))* tube_quad_t;

__device__ __forceinline__ void tube_ray(const ArtBundleView* views, const int e, const unsigned nb8, const unsigned o8,
                                         double* P, double* D) {
  const pol_view_t v = (pol_view_t)views + e;
  P[0] = ld_f64(rsrc_of(v->ox, nb8), o8);
  P[1] = ld_f64(rsrc_of(v->oy, nb8), o8);
  P[2] = ld_f64(rsrc_of(v->oz, nb8), o8);
  D[0] = ld_f64(rsrc_of(v->dx, nb8), o8);
  D[1] = ld_f64(rsrc_of(v->dy, nb8), o8);
  D[2] = ld_f64(rsrc_of(v->dz, nb8), o8);
}

__global__ __launch_bounds__(kBlock) void k_ray_tubes(const ArtTubeJob* __restrict__ jobs, const int64_t per_job,
                                                      double* scratch) {
  const ArtTubeJob& jb = jobs[blockIdx.y];
  const int64_t n = jb.n;
  if ((int64_t)blockIdx.x >= pol_tiles(n)) return;     // (the grid covers the largest job)
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned nb8 = (unsigned)(n * 8), nb1 = (unsigned)n;   // n <= 2^28 (checked by the host)
  const int K = jb.n_elems;
  const ArtBundleView* views = jb.views;
  bool live = true;                                    // (slots >= n fall outside the descriptor: they read 0)
  for (int e = 0; e <= K; ++e)
    live = live && __builtin_amdgcn_raw_buffer_load_b8(rsrc_of(pol_alive(views, e), nb1), (int)i, 0, ART_LD_AUX) != 0;
  const unsigned o8 = live ? i * 8u : kDropOffset;
  const double w = jb.w ? ld_f64(rsrc_of(const_cast<double*>(jb.w), nb8), o8) : 1.0;
  double P[3], D[3];
  tube_ray(views, 0, nb8, o8, P, D);
  artt::Tube T;
  artt::seed(jb.seed, D, T);
  for (int e = 0; e < K; ++e) {
    double Pn[3], Dn[3];
    tube_ray(views, e + 1, nb8, o8, Pn, Dn);
    artt::Surface s;
    artt::load_surface((tube_elem_t)jb.elems + e, (tube_quad_t)jb.quadrics + e, s);
    artt::step(s, D, P, Pn, T);
#pragma unroll
    for (int q = 0; q < 3; ++q) { P[q] = Pn[q]; D[q] = Dn[q]; }
  }
  artt::Readout R;
  artt::readout(T, D, P, jb.has_detector != 0, jb.det.centre, jb.det.normal, R);
  const double sa = fabs(R.solid_angle);
  const double weight = live ? w * sa : 0.0;
  st_f64(rsrc_of(jb.weight, nb8), i * 8u, weight);     // (slots >= n fall outside the descriptor)
  // the optional arrays: a NULL one gets a descriptor of no bytes, which drops every store
  st_f64(rsrc_of(jb.solid_angle, jb.solid_angle ? nb8 : 0u), i * 8u, live ? R.solid_angle : NAN);
  st_f64(rsrc_of(jb.area, jb.area ? nb8 : 0u), i * 8u, live ? R.area : NAN);
  st_f64(rsrc_of(jb.kappa1, jb.kappa1 ? nb8 : 0u), i * 8u, live ? R.kappa1 : NAN);
  st_f64(rsrc_of(jb.kappa2, jb.kappa2 ? nb8 : 0u), i * 8u, live ? R.kappa2 : NAN);
#pragma unroll
  for (int q = 0; q < 3; ++q)
    st_f64(rsrc_of(jb.axis ? jb.axis + (int64_t)q * n : nullptr, jb.axis ? nb8 : 0u), i * 8u, live ? R.axis[q] : NAN);
  const bool fin = live && isfinite(R.kappa1) && isfinite(R.kappa2);
  const double den = fabs(R.kappa1) + fabs(R.kappa2);
  double acc[kTubeStats];
  acc[0] = live ? 1.0 : 0.0;
  acc[1] = live ? w : 0.0;
  acc[2] = weight;
  acc[3] = live ? sa : INFINITY;
  acc[4] = live ? sa : -INFINITY;
  acc[5] = live ? w * fabs(R.area) : 0.0;
  acc[6] = fin ? w * R.kappa1 : 0.0;
  acc[7] = fin ? w * R.kappa2 : 0.0;
  acc[8] = fin ? w : 0.0;
  acc[9] = fin ? 1.0 : 0.0;
  acc[10] = fin ? (den > 0.0 ? R.asymmetry / den : 0.0) : -INFINITY;
  block_reduce_store<kTubeStats>(acc, tube_op, scratch + (int64_t)blockIdx.y * per_job + (int64_t)blockIdx.x * kTubeStats);
}

// grid (ART_TUBE_DOUBLES, jobs): workgroup (q, j) folds statistic q of job j's tiles in tile order
__global__ __launch_bounds__(kFoldBlock) void k_ray_tubes_fold(const ArtTubeJob* __restrict__ jobs, const int64_t per_job,
                                                               const double* scratch, double* out) {
  const int q = blockIdx.x;
  double* row = out + (int64_t)blockIdx.y * ART_TUBE_DOUBLES;
  if (q >= kTubeStats) {
    if (threadIdx.x == 0) row[q] = 0.0;
    return;
  }
  const double* part = scratch + (int64_t)blockIdx.y * per_job;
  const int64_t tiles = pol_tiles(jobs[blockIdx.y].n);
  double v = 0.0, other = 1.0;
  fold_range(part + q, 0, tiles, tube_op(q), &v, kTubeStats);
  // a minimum or maximum over no ray is 0; a mean is the sum over the sum of the weights
  const int with = (q == 3 || q == 4) ? 0 : ((q == 6 || q == 7) ? 8 : (q == 10 ? 9 : -1));
  if (with >= 0) {
    __syncthreads();
    fold_range(part + with, 0, tiles, RSUM, &other, kTubeStats);
  }
  if (threadIdx.x == 0) row[q] = other == 0.0 ? 0.0 : ((q == 6 || q == 7) ? v / other : v);
}

// ------------------------------------------------------------------------------------------- alignment sensitivities
// art_sensitivities: the pose derivatives of a traced chain, one pass over its history per job and group (include/art_hip.h;
// the per-ray math is art_tubes.h).  k_sensitivities: k_ray_tubes' shape with the groups as a grid dimension -- grid (tiles
// of 256 slots, groups x parts, jobs), one ray per lane.  Group g (0: the source, g >= 1: element g - 1) starts at its own
// element, because its columns are zero before it, and reads the rays of the views from there on only; the alive bytes of
// all K + 1 views are read first.  A workgroup carries kSensPerWg of the group's six columns per lane (6 / kSensPerWg
// parts per group).  Per tile and part kSensRow0 + 12 kSensPerWg partial sums (block_sum_store) at
// scratch[job][group x part][tile]; k_sensitivities_fold folds them per entry of the table in tile order (fold_range).
// Row 0 is formed by every workgroup (its inputs are in registers anyway) and folded from group 0's partials.
#ifndef ART_SENS_PER_WG
#define ART_SENS_PER_WG 6          // 6: all columns of a group in one lane; 3: two workgroups per group
#endif
constexpr int kSensPerWg = ART_SENS_PER_WG, kSensParts = ART_SENS_COLS / kSensPerWg;
constexpr int kSensRow0 = 8, kSensPerCol = 12, kSensStats = kSensRow0 + kSensPerCol * kSensPerWg;
static_assert(kSensPerWg * kSensParts == ART_SENS_COLS && kSensStats <= kBlock, "columns per workgroup");

// A workgroup's SUM of each of NS slots into dst[0 .. NS): wave_reduce24's transpose through a wave-private LDS tile for
// any number of sums, eight per pass (NS shuffle trees cost more than the transport of the columns they sum: measured,
// DESIGN.md 5), then the 4 waves in order.  One fixed order: the same bytes on every run.
template <int NS>
__device__ __forceinline__ void block_sum_store(const double (&acc)[NS], double* dst) {
  constexpr int kPasses = (NS + 7) / 8;
  __shared__ double tile[kBlock / 64][8 * kTileStride];
  __shared__ double total[kBlock / 64][kPasses * 8];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, stat = l >> 3, part = l & 7;
#pragma unroll
  for (int pass = 0; pass < kPasses; ++pass) {
    // (wave-level barriers: scheduling fences that keep a pass's stores, its row loads and the next pass's stores in order)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 8; ++j) tile[w][j * kTileStride + l] = (pass * 8 + j < NS) ? acc[(pass * 8 + j < NS) ? pass * 8 + j : 0] : 0.0;
    __builtin_amdgcn_wave_barrier();
    const double* row = tile[w] + stat * kTileStride + part;
    double v = row[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += row[8 * k];
    v += dpp_xchg<0xB1>(v);    // quad_perm:[1,0,3,2]  lane ^ 1
    v += dpp_xchg<0x4E>(v);    // quad_perm:[2,3,0,1]  lane ^ 2
    v += dpp_xchg<0x141>(v);   // row_half_mirror      lane i <-> 7 - i of its group of 8
    if (part == 0) total[w][pass * 8 + stat] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int k = threadIdx.x;
    double v = total[0][k];
    for (int j = 1; j < kBlock / 64; ++j) v += total[j][k];
    dst[k] = v;
  }
}

// the tables of the jobs before job j, in rows of ART_SENS_DOUBLES
__device__ __forceinline__ int64_t sens_rows_before(const ArtSensitivityJob* jobs, const int j) {
  int64_t rows = 0;
  for (int k = 0; k < j; ++k) rows += 1 + ART_SENS_COLS * (jobs[k].n_elems + 1);
  return rows;
}

__global__ __launch_bounds__(kBlock) void k_sensitivities(const ArtSensitivityJob* __restrict__ jobs, const int64_t per_job,
                                                          const int64_t tiles_max, double* scratch) {
  const ArtSensitivityJob& jb = jobs[blockIdx.z];
  const int64_t n = jb.n;
  const int K = jb.n_elems;
  const int g = blockIdx.y / kSensParts, part = blockIdx.y % kSensParts;
  if ((int64_t)blockIdx.x >= pol_tiles(n) || g > K) return;     // (the grid covers the largest job)
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned nb8 = (unsigned)(n * 8), nb1 = (unsigned)n;    // n <= 2^28 (checked by the host)
  const ArtBundleView* views = jb.views;
  bool live = true;                                             // (slots >= n fall outside the descriptor: they read 0)
  for (int e = 0; e <= K; ++e)
    live = live && __builtin_amdgcn_raw_buffer_load_b8(rsrc_of(pol_alive(views, e), nb1), (int)i, 0, ART_LD_AUX) != 0;
  const unsigned o8 = live ? i * 8u : kDropOffset;
  const double w = jb.w ? ld_f64(rsrc_of(const_cast<double*>(jb.w), nb8), o8) : 1.0;
  const int first = g ? g - 1 : 0;
  double P[3], D[3];
  tube_ray(views, first, nb8, o8, P, D);
  artt::Column c[kSensPerWg];
#pragma unroll
  for (int k = 0; k < kSensPerWg; ++k) {
    if (g == 0) artt::seed_source(part * kSensPerWg + k, D, c[k]);
    else artt::clear(c[k]);
  }
  for (int e = first; e < K; ++e) {
    double Pn[3], Dn[3];
    tube_ray(views, e + 1, nb8, o8, Pn, Dn);
    artt::Surface s;
    artt::load_surface((tube_elem_t)jb.elems + e, (tube_quad_t)jb.quadrics + e, s);
    artt::Hit h;
    artt::hit_of(s, D, P, Pn, h);
    if (g == e + 1) {                                           // (wave-uniform: the group's own element)
#pragma unroll
      for (int k = 0; k < kSensPerWg; ++k) {
        double sv[3], th[3];
        artt::motion(s, part * kSensPerWg + k, Pn, sv, th);
        artt::step_moved(s, h, D, sv, th, c[k]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kSensPerWg; ++k) artt::step_path(s, h, D, c[k]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { P[q] = Pn[q]; D[q] = Dn[q]; }
  }
  const double path = ld_f64(rsrc_of(((pol_view_t)views + K)->path, nb8), o8);
  // the nominal read-out about the caller's origin
  const double toC[3] = {jb.det.centre[0] - P[0], jb.det.centre[1] - P[1], jb.det.centre[2] - P[2]};
  const double tdet = artt::dot(jb.det.normal, toC) / artt::dot(jb.det.normal, D);
  const double rel[3] = {fma(tdet, D[0], -toC[0]), fma(tdet, D[1], -toC[1]), fma(tdet, D[2], -toC[2])};
  double xy[3];
  artt::rot(jb.det.rot, rel, xy);
  const double X = xy[0] - jb.origin[0], Y = xy[1] - jb.origin[1], L = (path + tdet) - jb.origin[2];
  const double ww = live ? w : 0.0;
  double acc[kSensStats];
  acc[0] = live ? 1.0 : 0.0;
  acc[1] = ww;
  acc[2] = live ? w * X : 0.0;
  acc[3] = live ? w * Y : 0.0;
  acc[4] = live ? w * L : 0.0;
  acc[5] = live ? w * X * X : 0.0;
  acc[6] = live ? w * Y * Y : 0.0;
  acc[7] = live ? w * L * L : 0.0;
  const int64_t col0 = (int64_t)ART_SENS_COLS * g + part * kSensPerWg;
#pragma unroll
  for (int k = 0; k < kSensPerWg; ++k) {
    double dX, dY;
    artt::readout_column(D, P, jb.det.centre, jb.det.normal, jb.det.rot, c[k], dX, dY);
    const double dL = c[k].dL;
    // the optional arrays: a NULL one gets a descriptor of no bytes, which drops every store; slots >= n fall outside
    const int64_t at = (col0 + k) * n;
    st_f64(rsrc_of(jb.dX ? jb.dX + at : nullptr, jb.dX ? nb8 : 0u), i * 8u, live ? dX : NAN);
    st_f64(rsrc_of(jb.dY ? jb.dY + at : nullptr, jb.dY ? nb8 : 0u), i * 8u, live ? dY : NAN);
    st_f64(rsrc_of(jb.dL ? jb.dL + at : nullptr, jb.dL ? nb8 : 0u), i * 8u, live ? dL : NAN);
    double* a = acc + kSensRow0 + kSensPerCol * k;
    a[0] = live ? w * dX : 0.0;
    a[1] = live ? w * dY : 0.0;
    a[2] = live ? w * dL : 0.0;
    a[3] = live ? w * X * dX : 0.0;
    a[4] = live ? w * Y * dY : 0.0;
    a[5] = live ? w * L * dL : 0.0;
    a[6] = live ? w * dX * dX : 0.0;
    a[7] = live ? w * dY * dY : 0.0;
    a[8] = live ? w * dL * dL : 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) a[9 + q] = live ? w * c[k].dD[q] : 0.0;
  }
  block_sum_store<kSensStats>(acc, scratch + (int64_t)blockIdx.z * per_job +
                                       ((int64_t)blockIdx.y * tiles_max + blockIdx.x) * kSensStats);
}

// grid (ART_SENS_DOUBLES, 1 + the largest M, jobs): workgroup (q, r, j) folds entry q of row r of job j's table in tile order
__global__ __launch_bounds__(kFoldBlock) void k_sensitivities_fold(const ArtSensitivityJob* __restrict__ jobs,
                                                                   const int64_t per_job, const int64_t tiles_max,
                                                                   const double* scratch, double* out) {
  const int q = blockIdx.x, r = blockIdx.y, j = blockIdx.z;
  if (r > ART_SENS_COLS * (jobs[j].n_elems + 1)) return;
  double* dst = out + (sens_rows_before(jobs, j) + r) * ART_SENS_DOUBLES + q;
  if (q >= (r == 0 ? kSensRow0 : kSensPerCol)) {
    if (threadIdx.x == 0) *dst = 0.0;
    return;
  }
  const int col = r == 0 ? 0 : r - 1;
  const int y = (col / ART_SENS_COLS) * kSensParts + (col % ART_SENS_COLS) / kSensPerWg;   // (row 0: group 0, part 0)
  const int slot = r == 0 ? q : kSensRow0 + kSensPerCol * (col % kSensPerWg) + q;
  double v = 0.0;
  fold_range(scratch + (int64_t)j * per_job + (int64_t)y * tiles_max * kSensStats + slot, 0, pol_tiles(jobs[j].n), RSUM, &v,
             kSensStats);
  if (threadIdx.x == 0) *dst = v;
}

// ------------------------------------------------------------------------------------------- compensator sums
// art_alignment_sums (include/art_hip.h): the Gram matrix of a CHOSEN handful of the columns above, in k_sensitivities'
// shape -- grid (tiles of 256 slots, jobs), one ray per lane -- but with all C <= 8 columns of a job in ONE lane, because a
// product needs both of its columns there.  The kernels are compiled for NC = 2, 4, 6, 8 columns; a job runs in the one
// for NC = C rounded up to even, whichever jobs share its call (a workgroup of another NC returns at once), with its
// spare column idle.  Which column moves at which element comes from the job: wave-uniform branches on scalar loads
// around columns at fixed places (artt::step_selected).  k_alignment_pilot runs the same lane over the first
// min(n, ART_ALIGN_PILOT) slots (at most 4 tiles) and leaves per tile sum w and sum w dQ_a behind the scratch of the main
// pass; align_centre adds them in tile order and divides: the centres.  k_alignment_sums stages them in LDS, subtracts
// them and stores per tile 8 + 3 (2 NC + NC (NC + 1) / 2) partial sums (block_sum_store, a chunk per coordinate so that
// they are never live at once); k_alignment_fold folds them per entry in tile order and records the centres.
constexpr int kAlignIdle = 6 * 4096;      // the id of a spare column: a group no chain has
constexpr int align_bucket(const int c) { return (c + 1) / 2 * 2; }
constexpr int align_per_q(const int nc) { return 2 * nc + nc * (nc + 1) / 2; }
constexpr int align_stats(const int nc) { return kSensRow0 + 3 * align_per_q(nc); }

template <int NC>
struct AlignRay {
  bool live;
  double w, X, Y, L, d[3][NC];            // d[q][a]: dX, dY, dL of the column at place a
};

template <int NC>
__device__ __forceinline__ void align_ray(const ArtAlignmentJob& jb, const unsigned i, AlignRay<NC>& r) {
  const int64_t n = jb.n;
  const int K = jb.n_elems, C = jb.n_dofs;
  const unsigned nb8 = (unsigned)(n * 8), nb1 = (unsigned)n;    // n <= 2^28 (checked by the host)
  const ArtBundleView* views = jb.views;
  bool live = true;                                             // (slots >= n fall outside the descriptor: they read 0)
  for (int e = 0; e <= K; ++e)
    live = live && __builtin_amdgcn_raw_buffer_load_b8(rsrc_of(pol_alive(views, e), nb1), (int)i, 0, ART_LD_AUX) != 0;
  const unsigned o8 = live ? i * 8u : kDropOffset;
  r.live = live;
  r.w = jb.w ? ld_f64(rsrc_of(const_cast<double*>(jb.w), nb8), o8) : 1.0;
  int id[NC];
  int first = K;
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    id[a] = a < C ? jb.dofs[a] : kAlignIdle;
    const int f = a < C ? artt::dof_first(id[a], K) : K;
    first = f < first ? f : first;
  }
  double P[3], D[3];
  tube_ray(views, first, nb8, o8, P, D);
  artt::Column c[NC];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    artt::seed_selected(id[a], D, c[a]);                        // (a source column makes first 0)
    // a seed is the same in every lane (a unit vector, zeros), and 8 columns of them in scalar registers up to their own
    // elements would not fit: they start in vector registers
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      asm volatile("" : "+v"(c[a].dP[q]));
      asm volatile("" : "+v"(c[a].dD[q]));
    }
    asm volatile("" : "+v"(c[a].dL));
  }
  for (int e = first; e < K; ++e) {
    double Pn[3], Dn[3];
    tube_ray(views, e + 1, nb8, o8, Pn, Dn);
    artt::Surface s;
    artt::load_surface((tube_elem_t)jb.elems + e, (tube_quad_t)jb.quadrics + e, s);
    artt::Hit h;
    artt::hit_of(s, D, P, Pn, h);
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      int ida = id[a];                                          // (opaque: the branches' conditions are formed here, per
      asm volatile("" : "+s"(ida));                             //  element, not kept for all columns around the loop)
      artt::step_selected(s, h, D, Pn, ida, e, c[a]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { P[q] = Pn[q]; D[q] = Dn[q]; }
  }
  const double path = ld_f64(rsrc_of(((pol_view_t)views + K)->path, nb8), o8);
  // the nominal read-out about the caller's origin (k_sensitivities' lines)
  const double toC[3] = {jb.det.centre[0] - P[0], jb.det.centre[1] - P[1], jb.det.centre[2] - P[2]};
  const double tdet = artt::dot(jb.det.normal, toC) / artt::dot(jb.det.normal, D);
  const double rel[3] = {fma(tdet, D[0], -toC[0]), fma(tdet, D[1], -toC[1]), fma(tdet, D[2], -toC[2])};
  double xy[3];
  artt::rot(jb.det.rot, rel, xy);
  r.X = xy[0] - jb.origin[0];
  r.Y = xy[1] - jb.origin[1];
  r.L = (path + tdet) - jb.origin[2];
#pragma unroll
  for (int a = 0; a < NC; ++a) {
    artt::readout_selected(id[a], D, P, jb.det.centre, jb.det.normal, jb.det.rot, c[a], r.d[0][a], r.d[1][a]);
    r.d[2][a] = c[a].dL;
  }
}

// grid (tiles of the prefix, jobs): per tile sum w and the 3 NC sums w dQ_a of the first min(n, ART_ALIGN_PILOT) slots, at
// pilot[job][tile][kAlignPilotStats]
constexpr int kAlignPilotTiles = ART_ALIGN_PILOT / kBlock, kAlignPilotStats = 1 + 3 * ART_ALIGN_MAX_DOFS;
__host__ __device__ inline int64_t align_pilot_tiles(const int64_t n) { return pol_tiles(n < ART_ALIGN_PILOT ? n : ART_ALIGN_PILOT); }

template <int NC>
__global__ __launch_bounds__(kBlock) void k_alignment_pilot(const ArtAlignmentJob* __restrict__ jobs, double* pilot) {
  const ArtAlignmentJob& jb = jobs[blockIdx.y];
  if (align_bucket(jb.n_dofs) != NC || (int64_t)blockIdx.x >= align_pilot_tiles(jb.n)) return;
  AlignRay<NC> r;
  align_ray<NC>(jb, blockIdx.x * kBlock + threadIdx.x, r);     // (the last tile's slots >= n are not alive)
  double acc[1 + 3 * NC];
  acc[0] = r.live ? r.w : 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int a = 0; a < NC; ++a) acc[1 + q * NC + a] = r.live ? r.w * r.d[q][a] : 0.0;
  block_sum_store<1 + 3 * NC>(acc, pilot + ((int64_t)blockIdx.y * kAlignPilotTiles + blockIdx.x) * kAlignPilotStats);
}

// centre_a^Q of a job from its pilot partials (k_alignment_pilot<nc>'s), in tile order: 0 for a place >= C and when no ray of
// the prefix counts.  The main pass and the fold both call it: the table records exactly what was subtracted.
__device__ __forceinline__ double align_centre(const double* part, const int tiles, const int nc, const int C, const int q,
                                               const int a) {
  if (a >= C) return 0.0;
  double sw = 0.0, v = 0.0;
  for (int t = 0; t < tiles; ++t) {
    sw += part[t * kAlignPilotStats];
    v += part[t * kAlignPilotStats + 1 + q * nc + a];
  }
  return sw > 0.0 ? v / sw : 0.0;
}

template <int NC>
__global__ __launch_bounds__(kBlock) void k_alignment_sums(const ArtAlignmentJob* __restrict__ jobs, const int64_t per_job,
                                                           double* scratch, const double* pilot) {
  const ArtAlignmentJob& jb = jobs[blockIdx.y];
  if (align_bucket(jb.n_dofs) != NC || (int64_t)blockIdx.x >= pol_tiles(jb.n)) return;   // (the grid covers the largest job)
  __shared__ double cen[3 * ART_ALIGN_MAX_DOFS];            // (LDS, not 48 scalar registers)
  if (threadIdx.x < 3 * ART_ALIGN_MAX_DOFS)
    cen[threadIdx.x] = align_centre(pilot + (int64_t)blockIdx.y * kAlignPilotTiles * kAlignPilotStats, (int)align_pilot_tiles(jb.n),
                                    NC, jb.n_dofs, threadIdx.x / ART_ALIGN_MAX_DOFS, threadIdx.x % ART_ALIGN_MAX_DOFS);
  __syncthreads();
  AlignRay<NC> r;
  align_ray<NC>(jb, blockIdx.x * kBlock + threadIdx.x, r);
  const bool live = r.live;
  const double ww = live ? r.w : 0.0;
  double* dst = scratch + (int64_t)blockIdx.y * per_job + (int64_t)blockIdx.x * align_stats(NC);
  const double Q[3] = {live ? r.X : 0.0, live ? r.Y : 0.0, live ? r.L : 0.0};
  {
    double acc[kSensRow0];
    acc[0] = live ? 1.0 : 0.0;
    acc[1] = ww;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      acc[2 + q] = ww * Q[q];
      acc[5 + q] = ww * Q[q] * Q[q];
    }
    block_sum_store<kSensRow0>(acc, dst);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    constexpr int kPerQ = align_per_q(NC);
    double d[NC], acc[kPerQ];
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      d[a] = live ? r.d[q][a] - cen[ART_ALIGN_MAX_DOFS * q + a] : 0.0;
      acc[a] = ww * d[a];
      acc[NC + a] = ww * Q[q] * d[a];
    }
    int p = 2 * NC;
#pragma unroll
    for (int a = 0; a < NC; ++a)
#pragma unroll
      for (int b = a; b < NC; ++b) acc[p++] = ww * d[a] * d[b];
    if (q) __syncthreads();               // (the previous chunk's totals have been read)
    block_sum_store<kPerQ>(acc, dst + kSensRow0 + q * kPerQ);
  }
}

// grid (ART_ALIGN_DOUBLES, jobs): workgroup (x, j) folds entry x of job j's block in tile order
__global__ __launch_bounds__(kFoldBlock) void k_alignment_fold(const ArtAlignmentJob* __restrict__ jobs, const int64_t per_job,
                                                               const double* scratch, const double* pilot, double* out) {
  const int x = blockIdx.x, j = blockIdx.y;
  const int C = jobs[j].n_dofs, nc = align_bucket(C), per_q = align_per_q(nc);
  if (x >= ART_ALIGN_CENTRES && x < ART_ALIGN_MEANS) {
    const int k = x - ART_ALIGN_CENTRES;
    if (threadIdx.x == 0)
      out[(int64_t)j * ART_ALIGN_DOUBLES + x] = align_centre(pilot + (int64_t)j * kAlignPilotTiles * kAlignPilotStats,
                                                             (int)align_pilot_tiles(jobs[j].n), nc, C, k / ART_ALIGN_MAX_DOFS,
                                                             k % ART_ALIGN_MAX_DOFS);
    return;
  }
  int slot = -1;
  if (x < kSensRow0) {
    slot = x;
  } else if (x < ART_ALIGN_PAIRS) {
    const int k = x - ART_ALIGN_MEANS, kind = k / (3 * ART_ALIGN_MAX_DOFS), q = k / ART_ALIGN_MAX_DOFS % 3, a = k % ART_ALIGN_MAX_DOFS;
    if (a < C) slot = kSensRow0 + q * per_q + kind * nc + a;
  } else if (x < ART_ALIGN_PAIRS + 3 * 36) {
    const int k = x - ART_ALIGN_PAIRS, q = k / 36;
    int a = 0, p = k % 36;
    for (; p >= ART_ALIGN_MAX_DOFS - a; ++a) p -= ART_ALIGN_MAX_DOFS - a;   // row a of the table holds b = a .. 7
    if (a + p < C) slot = kSensRow0 + q * per_q + 2 * nc + a * (2 * nc + 1 - a) / 2 + p;
  }
  double v = 0.0;
  if (slot >= 0) fold_range(scratch + (int64_t)j * per_job + slot, 0, pol_tiles(jobs[j].n), RSUM, &v, align_stats(nc));
  if (threadIdx.x == 0) out[(int64_t)j * ART_ALIGN_DOUBLES + x] = v;
}

// the pilot or the main pass for NC columns, when bit NC / 2 - 1 of `buckets` says that a job of the call runs in it
template <int NC>
static void align_launch(const bool first, const unsigned buckets, const ArtAlignmentJob* jobs_dev, const int32_t n_jobs,
                         const int64_t tiles, const int64_t per_job, double* scratch, double* pilot, hipStream_t s) {
  if (!(buckets & (1u << (NC / 2 - 1)))) return;
  if (first)
    hipLaunchKernelGGL(k_alignment_pilot<NC>, dim3((unsigned)align_pilot_tiles(tiles * kBlock), n_jobs), dim3(kBlock), 0, s,
                       jobs_dev, pilot);
  else
    hipLaunchKernelGGL(k_alignment_sums<NC>, dim3((unsigned)tiles, n_jobs), dim3(kBlock), 0, s, jobs_dev, per_job, scratch,
                       (const double*)pilot);
}

// ------------------------------------------------------------------------------------------- vector focal spectrum
// art_focal_vector_spectrum (include/art_hip.h): art_focal_spectrum's sum with a complex amplitude per (ray, wavenumber,
// component), the field of art_polarisation carried through coatings whose optical constants depend on the wavenumber.
// k_vecspec_rays: grid (tiles of 256 slots, wavenumbers of the block), one ray per lane, k_polarisation's pass over the
// history for a polarised input at k_j with the material table of (j, coating); it writes sqrt(w) (E . u_c) for
// u = e1, e2, n of the detector as 6 rows of `amp` per wavenumber (re, im per component; 0 for a dead slot).  The frame
// and cos t of an element do not depend on k, but a lane that kept them for all K elements, or the fields of several
// wavenumbers, would not fit the 128 registers of four workgroups per CU: they are formed again per wavenumber, a few
// hundred operations beside the element's Parratt steps (~150 each).  Views, coatings and materials are wave-uniform:
// scalar loads.
// k_vecspec_field is k_focal_spectrum_field with (plane, wavenumber, component) on the grid's y dimension and the row
// phasor W = (a . u_c) exp(i ...); it reads k_focal_spectrum_prep's rows.  Partials are laid out
// [plane][slice][wavenumber of the block][component] so that k_focal_fold folds a plane's slices straight into its
// place in the field.
struct VecSpecArg {
  const ArtBundleView* views;
  const double* w;
  double pol[6], u[9];          // P; e1, e2, n of the detector
  double k0, dk;
  int64_t n, stride;
  int32_t n_elems, n_coatings, j0, nkb;
  int32_t coating[ART_POLARISATION_MAX_ELEMS];
};

// The body of k_vecspec_rays and of k_vecchrom_rays (art_focal_vector_chromatic, below).  TABLE: k_j is row j of `table`
// (k_j, c_j, z_j, 0) instead of focal_kj, and the amplitude sqrt(w) is multiplied by exp(-(u c_j)) with the slot's u read
// from `urow` (k_focal_chromatic_prep's row 5) after the element loop, so that it lives through no Parratt step.
template <bool TABLE>
__device__ __forceinline__ void vecspec_rays_body(const VecSpecArg& a, const ArtCoating* __restrict__ coats,
                                                  const ArtCoatingMaterial* __restrict__ mats,
                                                  const double* __restrict__ table, const double* __restrict__ urow,
                                                  double* __restrict__ amp) {
  __shared__ artc::cplx s_kz[ART_COATING_MAX_MATERIALS * kBlock];   // kz / k per material, one column per lane
  __shared__ double s_dir[6 * kBlock];                                     // d_in, d_out, one column per lane
  const int jj = blockIdx.y, j = a.j0 + jj;
  const double k = TABLE ? table[4 * j] : focal_kj(a.k0, j, a.dk);
  const int64_t n = a.n;
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  const unsigned nb8 = (unsigned)(n * 8), nb1 = (unsigned)n;   // n <= 2^28 (checked by the host)
  const int K = a.n_elems;
  const ArtBundleView* views = a.views;
  const bool live = __builtin_amdgcn_raw_buffer_load_b8(rsrc_of(pol_alive(views, K), nb1), (int)i, 0, ART_LD_AUX) != 0;
  const unsigned o8 = live ? i * 8u : kDropOffset;
  const double w = a.w ? ld_f64(rsrc_of(const_cast<double*>(a.w), nb8), o8) : 1.0;
  double din[3], er[3], ei[3];
  pol_dirs(views, 0, nb8, o8, din);
  artc::transverse_state(a.pol, din, er, ei);
  for (int e = 0; e < K; ++e) {
    double dout[3];
    pol_dirs(views, e + 1, nb8, o8, dout);
    const int c = a.coating[e];
    if (c >= 0) {                                         // (a mask leaves E unchanged)
      // the two directions wait in LDS while the coefficients are formed (the Parratt loop needs every register)
      double* sd = s_dir + threadIdx.x;
#pragma unroll
      for (int q = 0; q < 3; ++q) { sd[q * kBlock] = din[q]; sd[(3 + q) * kBlock] = dout[q]; }
      artc::cplx rs, rp;
      artc::coating_rs_rp_at(coats[c], mats + ((int64_t)j * a.n_coatings + c) * ART_COATING_MAX_MATERIALS,
                             artc::cos_incidence(din, dout), k, s_kz + threadIdx.x, kBlock, rs, rp);
      asm volatile("" ::: "memory");                      // (read them back: do not keep them in registers)
#pragma unroll
      for (int q = 0; q < 3; ++q) { din[q] = sd[q * kBlock]; dout[q] = sd[(3 + q) * kBlock]; }
      artc::Frame f;                                      // (formed after the coefficients: fewer registers live)
      artc::reflection_frame(din, dout, f);
      artc::prt_step(f, rs, rp, er, ei);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) din[q] = dout[q];
  }
  if ((int64_t)i >= n) return;
  double sw = live ? sqrt(w) : 0.0;                       // (k_focal_spectrum_prep's amplitude)
  if (TABLE) sw *= exp(-focal_mul(urow[i], table[4 * j + 1]));   // (a dead slot's u is 0; c_j = 0: times exp(-0) = 1)
  double* row = amp + (int64_t)jj * 6 * a.stride + i;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double* u = a.u + 3 * c;
    const double re = er[0] * u[0] + er[1] * u[1] + er[2] * u[2], im = ei[0] * u[0] + ei[1] * u[1] + ei[2] * u[2];
    row[(2 * c) * a.stride] = live ? sw * re : 0.0;       // a dead slot's values are unspecified: selected away
    row[(2 * c + 1) * a.stride] = live ? sw * im : 0.0;
  }
}

__global__ __launch_bounds__(kBlock, 4) void k_vecspec_rays(const VecSpecArg a, const ArtCoating* __restrict__ coats,
                                                         const ArtCoatingMaterial* __restrict__ mats,
                                                         double* __restrict__ amp) {
  vecspec_rays_body<false>(a, coats, mats, nullptr, nullptr, amp);
}

// blockIdx.y = ((q * nkb + jj) * 3 + c) (plane q, wavenumber j0 + jj of the block, component c); amps: the rows of
// k_vecspec_rays; out (double2): plane q at q * plane_stride, slice at slice * slice_stride, then [jj][c][ny][nx]
__global__ __launch_bounds__(kBlock) void k_vecspec_field(const FocalArg a, const double dk, const int j0, const int nkb,
                                                          const double* __restrict__ rows,
                                                          const double* __restrict__ amps, const int64_t plane_stride,
                                                          const int64_t slice_stride, double* __restrict__ out) {
  __shared__ FocalStage sU;                           // exp(i X_j k d.e1)
  __shared__ FocalStage sW;                           // (a . u_c) exp(i (base + s_q k d.n + Y_l k d.e2))
  const int qjc = blockIdx.y, qj = qjc / 3, comp = qjc - 3 * qj, q = qj / nkb, jj = qj - q * nkb, slice = blockIdx.z;
  const double kj = focal_kj(a.k, j0 + jj, dk);
  const FocalLane L = focal_lane(a.tiles_x);
  const int64_t st = a.stride, r0 = (int64_t)slice * a.per_slice;
  const int64_t r1 = (r0 + a.per_slice < a.n) ? r0 + a.per_slice : a.n;
  const double sh = a.shift[q];
  const double* am = amps + ((int64_t)jj * 6 + 2 * comp) * st;
  FocalAcc acc_re = {}, acc_im = {};

  for (int64_t c0 = r0; c0 < r1; c0 += kFocalChunk) {
    const int64_t r = c0 + L.sr;
    const bool in = r < r1;                       // beyond the slice: a zero row phasor, nothing is added
    double ph, s_re, s_im, sn, cs;
    focal_phase_terms_at(kj, a, rows, L, r, in, sh, ph, s_re, s_im);
    const double a_re = L.colw ? 1.0 : (in ? am[r] : 0.0), a_im = L.colw || !in ? 0.0 : am[st + r];
    sincos(ph, &sn, &cs);
    focal_rotate_store(sU, sW, L, a_re * cs - a_im * sn, a_re * sn + a_im * cs, s_re, s_im);
    __syncthreads();
    focal_accumulate(sU, sW, L, acc_re, acc_im);
    __syncthreads();
  }
  focal_store(reinterpret_cast<double2*>(out) + (int64_t)q * plane_stride + (int64_t)slice * slice_stride +
                  (int64_t)(jj * 3 + comp) * a.ny * a.nx,
              a, L, acc_re, acc_im);
}

// ------------------------------------------------------------------------------------------- vector focal chromatic
// art_focal_vector_chromatic (include/art_hip.h): art_focal_vector_spectrum for art_focal_chromatic's source.  The rows
// are k_focal_chromatic_prep's (src = views[0]; u in row 5), the wavenumbers the table's.  k_vecchrom_rays is
// k_vecspec_rays' body with k_j from the table and the amplitude sqrt(w) exp(-(u c_j)); k_vecchrom_field is
// k_vecspec_field with focal_phase_terms_chromatic in place of focal_phase_terms_at.  With c_j = z_j = 0 both round as
// the kernels they come from: art_focal_vector_spectrum's bytes at the same k_j.
__global__ __launch_bounds__(kBlock, 4) void k_vecchrom_rays(const VecSpecArg a, const ArtCoating* __restrict__ coats,
                                                          const ArtCoatingMaterial* __restrict__ mats,
                                                          const double* __restrict__ table,
                                                          const double* __restrict__ urow, double* __restrict__ amp) {
  vecspec_rays_body<true>(a, coats, mats, table, urow, amp);
}

// k_vecspec_field's grid, arguments and layout of out; table: the call's rows (k_j, c_j, z_j, 0), row j0 + jj the
// workgroup's (uniform); rows: k_focal_chromatic_prep's
__global__ __launch_bounds__(kBlock) void k_vecchrom_field(const FocalArg a, const double* __restrict__ table, const int j0,
                                                           const int nkb, const double* __restrict__ rows,
                                                           const double* __restrict__ amps, const int64_t plane_stride,
                                                           const int64_t slice_stride, double* __restrict__ out) {
  __shared__ FocalStage sU;                           // exp(i X_j k d.e1)
  __shared__ FocalStage sW;                           // (a . u_c) exp(i (k (base / k + z u) + s_q k d.n + Y_l k d.e2))
  const int qjc = blockIdx.y, qj = qjc / 3, comp = qjc - 3 * qj, q = qj / nkb, jj = qj - q * nkb, slice = blockIdx.z;
  const double* row = table + 4 * (j0 + jj);
  const double kj = row[0], zj = row[2];
  const FocalLane L = focal_lane(a.tiles_x);
  const int64_t st = a.stride, r0 = (int64_t)slice * a.per_slice;
  const int64_t r1 = (r0 + a.per_slice < a.n) ? r0 + a.per_slice : a.n;
  const double sh = a.shift[q];
  const double* am = amps + ((int64_t)jj * 6 + 2 * comp) * st;
  FocalAcc acc_re = {}, acc_im = {};

  for (int64_t c0 = r0; c0 < r1; c0 += kFocalChunk) {
    const int64_t r = c0 + L.sr;
    const bool in = r < r1;                       // beyond the slice: a zero row phasor, nothing is added
    double ph, s_re, s_im, sn, cs;
    const double u = (!L.colw && in) ? rows[5 * st + r] : 0.0;
    focal_phase_terms_chromatic(kj, zj, u, a, rows, L, r, in, sh, ph, s_re, s_im);
    const double a_re = L.colw ? 1.0 : (in ? am[r] : 0.0), a_im = L.colw || !in ? 0.0 : am[st + r];
    sincos(ph, &sn, &cs);
    focal_rotate_store(sU, sW, L, a_re * cs - a_im * sn, a_re * sn + a_im * cs, s_re, s_im);
    __syncthreads();
    focal_accumulate(sU, sW, L, acc_re, acc_im);
    __syncthreads();
  }
  focal_store(reinterpret_cast<double2*>(out) + (int64_t)q * plane_stride + (int64_t)slice * slice_stride +
                  (int64_t)(jj * 3 + comp) * a.ny * a.nx,
              a, L, acc_re, acc_im);
}

template <bool HAS_W>
__global__ __launch_bounds__(kBlock) void k_moments_partial(const uint8_t* alive, const double* X, const double* Y,
                                                            const double* opl, const double* w, const int64_t n,
                                                            const double cx, const double cy, const double co,
                                                            double* scratch) {
  double acc[kSumSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t stride = (int64_t)gridDim.x * kBlock, last = n - 1;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kRedUnroll * stride) {
    double xv[kRedUnroll], yv[kRedUnroll], ov[kRedUnroll], wv[kRedUnroll];
    bool live[kRedUnroll];
#pragma unroll
    for (int u = 0; u < kRedUnroll; ++u) {
      const int64_t i = i0 + u * stride, c = i < n ? i : last;
      live[u] = (ld_nt(alive + c) != 0) & (i < n);
      xv[u] = X ? ld_nt(X + c) : cx;       // (wave-uniform: an absent stream sits on its centre)
      yv[u] = Y ? ld_nt(Y + c) : cy;
      ov[u] = opl ? ld_nt(opl + c) : co;
      wv[u] = HAS_W ? ld_nt(w + c) : 1.0;
    }
#pragma unroll
    for (int u = 0; u < kRedUnroll; ++u) {
      const bool l = live[u];
      const double ww = l ? wv[u] : 0.0;
      const double ex = (l && X) ? xv[u] - cx : 0.0, ey = (l && Y) ? yv[u] - cy : 0.0, eo = (l && opl) ? ov[u] - co : 0.0;
      acc[0] += ww;
      acc[1] = fma(ww * ex, ex, acc[1]);
      acc[2] = fma(ww * ey, ey, acc[2]);
      acc[3] = fma(ww * eo, eo, acc[3]);
      acc[4] += l ? 1.0 : 0.0;
    }
  }
  block_reduce_store<kSumSlots>(acc, sum_op, scratch + (int64_t)blockIdx.x * kSumSlots);
}

template <bool HAS_W>
__global__ __launch_bounds__(kBlock) void k_bundle_sums_partial(const ArtBundleView b, const double* w,
                                                                const int64_t n, double* scratch) {
  double acc[kSumSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t stride = (int64_t)gridDim.x * kBlock, last = n - 1;
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kRedUnroll * stride) {
    double v[kRedUnroll][7];
    bool live[kRedUnroll];
#pragma unroll
    for (int u = 0; u < kRedUnroll; ++u) {
      const int64_t i = i0 + u * stride, c = i < n ? i : last;
      live[u] = (ld_nt(b.alive + c) != 0) & (i < n);
      v[u][0] = ld_nt(b.ox + c); v[u][1] = ld_nt(b.oy + c); v[u][2] = ld_nt(b.oz + c);
      v[u][3] = ld_nt(b.dx + c); v[u][4] = ld_nt(b.dy + c); v[u][5] = ld_nt(b.dz + c);
      v[u][6] = HAS_W ? ld_nt(w + c) : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kRedUnroll; ++u) {
      acc[0] += live[u] ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < 7; ++k) acc[1 + k] += live[u] ? v[u][k] : 0.0;
    }
  }
  block_reduce_store<kSumSlots>(acc, sum_op, scratch + (int64_t)blockIdx.x * kSumSlots);
}

// ------------------------------------------------------------------------------------------- source weights
struct Axis3 { double x, y, z; };

__device__ __forceinline__ double angle_to_axis(const Axis3 ax, double vx, double vy, double vz) {
  // AngleBetweenTwoVectors(Axis, vector), ART/ModuleGeometry.py:40-44, with the norms as the reference applies them
  const double u = sqrt(art::dot3(ax.x, ax.y, ax.z, ax.x, ax.y, ax.z)), v = sqrt(art::dot3(vx, vy, vz, vx, vy, vz));
  const double ax_ = ax.x * v - vx * u, ay_ = ax.y * v - vy * u, az_ = ax.z * v - vz * u;
  const double bx_ = ax.x * v + vx * u, by_ = ax.y * v + vy * u, bz_ = ax.z * v + vz * u;
  return 2.0 * atan2(sqrt(art::dot3(ax_, ay_, az_, ax_, ay_, az_)), sqrt(art::dot3(bx_, by_, bz_, bx_, by_, bz_)));
}

// tan^2(angle / 2) of the same Kahan pair, |a v - v' u|^2 / |a v + v' u|^2: monotone in the angle, one reciprocal instead of
// two square roots and an atan2 per ray -- for a MAXIMUM over rays the angle itself is formed once, from the largest ratio
// (k_analysis_fold: 2 atan(sqrt(.))).
__device__ __forceinline__ double tan2_half_angle_to_axis(const Axis3 ax, const double u, double vx, double vy, double vz,
                                                          const double v) {     // u = |axis|, v = |vector|
  const double ax_ = ax.x * v - vx * u, ay_ = ax.y * v - vy * u, az_ = ax.z * v - vz * u;
  const double bx_ = ax.x * v + vx * u, by_ = ax.y * v + vy * u, bz_ = ax.z * v + vz * u;
  // (the denominator is ~4 |u|^2 |v|^2 for the small angles this is about: a refined reciprocal, not an IEEE division)
  return art::dot3(ax_, ay_, az_, ax_, ay_, az_) * art::rcp_full(art::dot3(bx_, by_, bz_, bx_, by_, bz_));
}

// `axis_sums` (or NULL): DEVICE, the 8 sums of art_bundle_sums -- the axis is then the bundle's own central ray, mean vector
// normalised (FindCentralRay + the Ray.vector setter, ART/ModuleProcessing.py:464-482, ART/ModuleOpticalRay.py:85-90), formed
// here instead of on the host: no round trip between the sums and the weights
__device__ __forceinline__ Axis3 axis_of(const Axis3 given, const double* axis_sums) {
  if (axis_sums == nullptr) return given;
  const double c = axis_sums[0];
  const double x = axis_sums[4] / c, y = axis_sums[5] / c, z = axis_sums[6] / c;
  const double nrm = sqrt(art::dot3(x, y, z, x, y, z));
  return Axis3{x / nrm, y / nrm, z / nrm};
}

__global__ __launch_bounds__(kBlock) void k_gauss_max_partial(const ArtBundleView b, const Axis3 ax_in, const double* axis_sums,
                                                              const int64_t n, double* scratch) {
  const Axis3 ax = axis_of(ax_in, axis_sums);
  double acc[kMaxSlots] = {0, 0};    // (the largest of nothing is 0)
  const int64_t stride = (int64_t)gridDim.x * kBlock, last = n - 1;
  constexpr int kU = 2;     // (an atan2 and three square roots per ray: the arithmetic hides the rest of the latency)
  for (int64_t i0 = (int64_t)blockIdx.x * kBlock + threadIdx.x; i0 < n; i0 += kU * stride) {
    double v[kU][6];
    bool live[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int64_t i = i0 + u * stride, c = i < n ? i : last;
      live[u] = (ld_nt(b.alive + c) != 0) & (i < n);
      v[u][0] = ld_nt(b.ox + c); v[u][1] = ld_nt(b.oy + c); v[u][2] = ld_nt(b.oz + c);
      v[u][3] = ld_nt(b.dx + c); v[u][4] = ld_nt(b.dy + c); v[u][5] = ld_nt(b.dz + c);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      // a dead slot holds unspecified values: it takes part as the axis itself at the origin (angle 0, distance 0)
      const double dx = live[u] ? v[u][3] : ax.x, dy = live[u] ? v[u][4] : ax.y, dz = live[u] ? v[u][5] : ax.z;
      const double px = live[u] ? v[u][0] : 0.0, py = live[u] ? v[u][1] : 0.0, pz = live[u] ? v[u][2] : 0.0;
      const double ang = angle_to_axis(ax, dx, dy, dz);
      acc[0] = fmax(acc[0], live[u] ? ang : 0.0);
      acc[1] = fmax(acc[1], sqrt(art::dot3(px, py, pz, px, py, pz)));
    }
  }
  block_reduce_store<kMaxSlots>(acc, max_op, scratch + (int64_t)blockIdx.x * kMaxSlots);
}

__global__ __launch_bounds__(kBlock) void k_gauss_weights(const ArtBundleView b, const Axis3 ax_in, const double* axis_sums,
                                                          const double kexp, const double* maxima, const int64_t n, double* w) {
  const Axis3 ax = axis_of(ax_in, axis_sums);
  const double div = maxima[0], maxdist = maxima[1];
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    double q;
    if (div > 1e-12) {   // diverging bundle: profile in angle (ModuleSource.py:247-251)
      q = tan(angle_to_axis(ax, b.dx[i], b.dy[i], b.dz[i])) / div;
    } else {             // collimated: profile in distance from the origin (:252-259)
      q = sqrt(art::dot3(b.ox[i], b.oy[i], b.oz[i], b.ox[i], b.oy[i], b.oz[i])) / maxdist;
    }
    w[i] = exp(-2.0 * q * q * kexp);
  }
}

// ------------------------------------------------------------------------------------------- guide rays
// One guide ray per thread, each through ITS OWN element (art_trace_guides): the 1-ray alignment traces of OEPlacement for
// up to 8 chains in one launch.  The descriptors are kernel arguments, indexed per lane (vector loads from the constant
// argument segment: this kernel is launch-latency, not throughput).
struct GuideArgs {
  ArtElementDesc e[ART_GUIDES_MAX];
};
template <bool DEFECT>
__global__ __launch_bounds__(64) void k_trace_guides(const GuideArgs ga, double* rays, uint8_t* alive, const int count) {
  const int t = threadIdx.x;
  if (t >= count) return;
  art::Ray r;
  double* q = rays + 8 * t;
  r.ox = q[0]; r.oy = q[1]; r.oz = q[2]; r.dx = q[3]; r.dy = q[4]; r.dz = q[5]; r.path = q[6]; r.inc = q[7];
  bool ok = alive[t] != 0;
  if (ok) {
    // one lane at a time: the torus solver's Newton loop votes across the wave and the descriptor must be wave-uniform
    for (int j = 0; j < count; ++j) {
      if (t == j) ok = art::trace_ray_dyn<DEFECT>(ga.e[j], ga.e[j].zern, r);
    }
  }
  if (ok) { q[0] = r.ox; q[1] = r.oy; q[2] = r.oz; q[3] = r.dx; q[4] = r.dy; q[5] = r.dz; q[6] = r.path; q[7] = r.inc; }
  alive[t] = (uint8_t)(ok ? 1 : 0);
}

// ------------------------------------------------------------------------------------------- batched analysis
// art_analyse_bundles: blockIdx.y = job.  Partials per job and workgroup, folded in a fixed order.
constexpr int kAnaMom = 42;      // 32 moment sums, kink shifts (2), max angle, bounding box + path range (6), pad
constexpr int kAnaPlace = 24;    // per job: ArtDetectorDesc (15 doubles), axis (3), co, cx, cy, pad
constexpr int kAnaBlocks = 1024; // workgroups per job of the moments pass at most
constexpr int kAnaSumsPad = 16;  // doubles per job of the folded sums (9 used)
// Workgroups per job of the moments pass: a function of the ray count ALONE, so that a bundle's moments are folded in the
// same order whether it is analysed alone or as one of a list (same bits either way).
inline int analysis_blocks(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (int)(b < 1 ? 1 : (b > kAnaBlocks ? kAnaBlocks : b));
}
inline int64_t analysis_tiles(int64_t n) { return n < 1 ? 1 : (n + kBlock - 1) / kBlock; }
// ART_ANALYSIS_ORDER=job: the moments pass in job-major order instead of XCD-grouped (read per call: in-process A/B)
inline int analysis_job_major() {
  const char* e = getenv("ART_ANALYSIS_ORDER");
  return (e && e[0] == 'j') ? 1 : 0;
}
__device__ __forceinline__ int ana_mom_op(const int q) {   // operator of moment-pass partial q
  return (q < 32) ? RSUM : ((q == 33 || q == 35 || q == 37 || q == 39) ? RMIN : ((q == 41) ? RSUM : RMAX));
}
__device__ __forceinline__ int ana_mom_slot(const int q) { // where partial q lands in a job's output row
  return (q < 32) ? 20 + q : ((q < 35) ? 53 + (q - 32) : 56 + (q - 35));
}

// Pass (1) for the jobs that do not bring their sums along (ArtAnalysisJob.sums): one workgroup per tile of 256 slots, one
// ray per lane, the canonical order of run_sums8.  rows: [job][kSumRows][ntiles] (+ the chunk totals of a two-stage fold).
// (launched per RUN of consecutive jobs that need it -- job = job0 + blockIdx.y: a grid over all jobs would dispatch 39 063
// workgroups per 1e7-ray job only to let them return)
__global__ __launch_bounds__(kBlock) void k_analysis_sums(const ArtAnalysisJob* __restrict__ jobs, const int job0,
                                                          const int64_t n, double* rows, const int64_t job_stride) {
  const int job = job0 + (int)blockIdx.y;
  const ArtAnalysisJob& jb = jobs[job];
  if (jb.sums != nullptr) return;      // (workgroup-uniform) formed by the tracing launch already
  __shared__ __attribute__((aligned(16))) double s_tile[(kBlock / 64) * 8 * kTileStride];
  __shared__ double s_run[(kBlock / 64) * kSumRows];
  const unsigned t = threadIdx.x;
  // buffer descriptors (n <= 2^28, checked by the host): slots beyond the end read alive = 0, and a dead slot's data is
  // requested at an out-of-range offset, i.e. not at all (a workgroup of dead slots -- the shadow of a mask -- moves 256 bytes)
  const unsigned i = blockIdx.x * kBlock + t;
  const BundleRsrc rb = make_rsrc(jb.b, n);
  const bool live = __builtin_amdgcn_raw_buffer_load_b8(rb.alive, (int)i, 0, ART_LD_AUX) != 0;
  const unsigned o8 = live ? i * 8u : kDropOffset;
  art::Ray r;
  r.ox = ld_f64(rb.ox, o8); r.oy = ld_f64(rb.oy, o8); r.oz = ld_f64(rb.oz, o8);
  r.dx = ld_f64(rb.dx, o8); r.dy = ld_f64(rb.dy, o8); r.dz = ld_f64(rb.dz, o8);
  r.path = ld_f64(rb.path, o8);
  const double w = jb.w ? ld_f64(rsrc_of(const_cast<double*>(jb.w), (unsigned)(n * 8)), o8) : 1.0;
  double v[8];
  sums_values(v, live, r, w);
  const double tot = run_sums8(v, s_tile + (t >> 6) * (8 * kTileStride), t & 63);
  tile_sums_store(tot, __ballot(live), s_run, t, rows + (int64_t)job * job_stride, gridDim.x, blockIdx.x);
}
// grids (kSumRows, kFoldChunks, jobs) and (kSumRows, 1, jobs): the sums folds of launch_fold, or a copy of the sums a job
// brought along
__global__ __launch_bounds__(kFoldBlock) void k_analysis_sums_fold1(const ArtAnalysisJob* __restrict__ jobs, const int job0,
                                                                    double* rows, const int64_t job_stride,
                                                                    const int64_t ntiles) {
  const int job = job0 + (int)blockIdx.z;
  if (jobs[job].sums != nullptr) return;
  sums_fold1(rows + (int64_t)job * job_stride, ntiles);
}
__global__ __launch_bounds__(kFoldBlock) void k_analysis_sums_fold2(const ArtAnalysisJob* __restrict__ jobs, double* rows,
                                                                    const int64_t job_stride, const int64_t ntiles,
                                                                    const int direct, double* sums) {
  double* out = sums + (int64_t)blockIdx.z * kAnaSumsPad;
  const double* given = jobs[blockIdx.z].sums;
  if (given != nullptr) {
    if (threadIdx.x == 0) out[blockIdx.x] = given[blockIdx.x];
    return;
  }
  sums_fold2(rows + (int64_t)blockIdx.z * job_stride, ntiles, out, direct);
}

// one thread per job: the sums are folded; place the detector
__global__ __launch_bounds__(64) void k_analysis_place(const ArtAnalysisJob* __restrict__ jobs, const int n_jobs,
                                                       const double* sums, double* place, double* out) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_jobs) return;
  const double* s_sum = sums + (int64_t)j * kAnaSumsPad;
  const ArtAnalysisJob& jb = jobs[j];
  double* o = out + (int64_t)j * ART_ANALYSIS_DOUBLES;
  double* pl = place + (int64_t)j * kAnaPlace;
  for (int k = 0; k < ART_ANALYSIS_DOUBLES; ++k) o[k] = 0.0;
  for (int k = 0; k < kSumRows; ++k) o[k] = s_sum[k];
  o[53] = -INFINITY; o[54] = INFINITY;
  o[56] = INFINITY; o[57] = -INFINITY; o[58] = INFINITY; o[59] = -INFINITY; o[60] = INFINITY; o[61] = -INFINITY;
  if (jb.mode == ART_JOB_SUMS) return;
  ArtDetectorDesc d;
  double ref[3], axis[3], co, cxy[2] = {0.0, 0.0};
  if (s_sum[0] > 0.0) {
    art::analysis_place_centred(s_sum, jb.mode, jb.distance, jb.centre, jb.normal, jb.refpoint, d, ref, axis, co, cxy);
  } else {
    for (int k = 0; k < 3; ++k) { d.centre[k] = NAN; d.normal[k] = NAN; ref[k] = NAN; axis[k] = NAN; }
    for (int k = 0; k < 9; ++k) d.rot[k] = NAN;
    co = NAN;
  }
  for (int k = 0; k < 3; ++k) { o[10 + k] = d.centre[k]; o[13 + k] = d.normal[k]; o[16 + k] = ref[k]; }
  o[19] = co;
  o[62] = cxy[0]; o[63] = cxy[1];
  for (int k = 0; k < 3; ++k) { pl[k] = d.centre[k]; pl[3 + k] = d.normal[k]; pl[15 + k] = axis[k]; }
  for (int k = 0; k < 9; ++k) pl[6 + k] = d.rot[k];
  pl[18] = co;
  pl[19] = cxy[0]; pl[20] = cxy[1];
}

// The moments pass keeps 42 accumulators (84 VGPRs) beside the ray: 128 VGPRs = 4 waves per SIMD, which is also all the
// fixed grid of 1024 workgroups offers.  What it gained in round 5: the next slot's nine streams are requested
// UNCONDITIONALLY (ld_nt, selects instead of the alive-guarded skip) while the current slot is worked on.
template <bool HAS_W>
__device__ __forceinline__ void moments_body(const ArtAnalysisJob& jb, const int64_t n, const double* pl, double (&acc)[kAnaMom],
                                             const unsigned blk, const unsigned nblk) {
  ArtDetectorDesc d;
#pragma unroll
  for (int k = 0; k < 3; ++k) { d.centre[k] = pl[k]; d.normal[k] = pl[3 + k]; }
#pragma unroll
  for (int k = 0; k < 9; ++k) d.rot[k] = pl[6 + k];
  const Axis3 ax = {pl[15], pl[16], pl[17]};
  const double au = sqrt(art::dot3(ax.x, ax.y, ax.z, ax.x, ax.y, ax.z));      // |axis|: once, not per ray
  const double inv_nn = 1.0 / art::dot3(d.normal[0], d.normal[1], d.normal[2], d.normal[0], d.normal[1], d.normal[2]);
  const double co = pl[18], cx = pl[19], cy = pl[20];      // (workgroup-uniform: scalar registers)
  const ArtBundleView b = jb.b;
  const double* w = jb.w;
  const int64_t stride = (int64_t)nblk * kBlock;
  // Every stream of the slot is requested UNCONDITIONALLY at the top of its iteration (alive is applied by selects: no
  // load waits for another load); buffer descriptors: one 32-bit offset register serves all nine streams (nine 64-bit
  // addresses would not fit beside the accumulators), slots beyond the end read 0 = dead.  A software pipeline (the next
  // slot's loads in flight behind this slot's arithmetic) does NOT fit: 41 fp64 accumulators + two slots' state exceed
  // the 128 registers of 4 waves per SIMD and the compiler parks the prefetched values in scratch (tried, round 5).
  // n <= 2^28 (checked by the host).
  const BundleRsrc rb = make_rsrc(b, n);
  const __amdgpu_buffer_rsrc_t rw = rsrc_of(const_cast<double*>(w), HAS_W ? (unsigned)(n * 8) : 0u);
  const unsigned ustride = (unsigned)stride, un_ = (unsigned)n;
  int cnt = 0;
  unsigned i = blk * kBlock + threadIdx.x;
  bool l = __builtin_amdgcn_raw_buffer_load_b8(rb.alive, (int)i, 0, ART_LD_AUX) != 0;
  for (; i < un_; i += ustride) {
    // the data of an ALIVE slot only (a dead one is requested out of range: no traffic; its fields read 0 and are selected
    // away below), and the NEXT slot's alive byte in flight behind it
    const unsigned o8 = l ? i * 8u : kDropOffset;
    const unsigned char nl_raw = __builtin_amdgcn_raw_buffer_load_b8(rb.alive, (int)(i + ustride), 0, ART_LD_AUX);
    const double cox = ld_f64(rb.ox, o8), coy = ld_f64(rb.oy, o8), coz = ld_f64(rb.oz, o8);
    const double cdx = ld_f64(rb.dx, o8), cdy = ld_f64(rb.dy, o8), cdz = ld_f64(rb.dz, o8);
    const double pth = ld_f64(rb.path, o8);
    const double wv = HAS_W ? ld_f64(rw, o8) : 1.0;
    art::Ray r;
    r.ox = cox; r.oy = coy; r.oz = coz; r.dx = cdx; r.dy = cdy; r.dz = cdz; r.path = pth; r.inc = 0.0;
    double q0[3], sq[3], sk, un;
    art::detector_ray_scan_kink(d, r, inv_nn, q0[0], q0[1], q0[2], sq[0], sq[1], sq[2], sk, un);
    acc[35] = fmin(acc[35], l ? q0[0] : INFINITY); acc[36] = fmax(acc[36], l ? q0[0] : -INFINITY);
    acc[37] = fmin(acc[37], l ? q0[1] : INFINITY); acc[38] = fmax(acc[38], l ? q0[1] : -INFINITY);
    acc[39] = fmin(acc[39], l ? q0[2] : INFINITY); acc[40] = fmax(acc[40], l ? q0[2] : -INFINITY);
    acc[32] = fmax(acc[32], (l && sk <= 0.0) ? sk : -INFINITY);
    acc[33] = fmin(acc[33], (l && sk > 0.0) ? sk : INFINITY);
    const double t2 = tan2_half_angle_to_axis(ax, au, r.dx, r.dy, r.dz, un);
    acc[34] = fmax(acc[34], l ? t2 : 0.0);
    // the moments about the mean ray's hit, not about Detector.centre (the bounding box above stays about the centre)
    q0[0] -= cx; q0[1] -= cy;
    q0[2] -= co;
    sq[2] -= 1.0;
    const double ww = l ? wv : 0.0;
    cnt += l ? 1 : 0;
    acc[16] += ww;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int o = 1 + 5 * k;
      const double a0 = l ? q0[k] : 0.0, s0 = l ? sq[k] : 0.0;       // (a dead slot's values are unspecified: selected away)
      acc[o] += a0; acc[o + 1] += s0;
      acc[o + 2] = fma(a0, a0, acc[o + 2]); acc[o + 3] = fma(a0, s0, acc[o + 3]);
      acc[o + 4] = fma(s0, s0, acc[o + 4]);
      const double wq = ww * a0, ws = ww * s0;
      acc[16 + o] += wq; acc[16 + o + 1] += ws;
      acc[16 + o + 2] = fma(wq, a0, acc[16 + o + 2]); acc[16 + o + 3] = fma(wq, s0, acc[16 + o + 3]);
      acc[16 + o + 4] = fma(ws, s0, acc[16 + o + 4]);
    }
    l = nl_raw != 0;
  }
  acc[0] = (double)cnt;      // (a lane folds < 2^31 slots: the integer count is exact, as the sum of 1.0s was)
}

// 1-D grid of (P rounded up to a multiple of 8) x J workgroups, XCD-grouped like the scene launches (scene_wg): id = 8 k + xcd,
// job = k mod J, block = 8 (k / J) + xcd -- the J workgroups that walk the SAME slots of J bundles run on one XCD, so the
// weights the jobs of a loop list share (one source: one intensity array) are fetched into its L2 once, not J times.
// Which slots a block folds, and the fold order, do not depend on the mapping.
__global__ __launch_bounds__(kBlock, 4) void k_analysis_moments(const ArtAnalysisJob* __restrict__ jobs, const int64_t n,
                                                             const double* place, const double* out, double* scratch,
                                                             const int P, const int job0, const int J, const int job_major) {
  const unsigned id = blockIdx.x, P8 = gridDim.x / (unsigned)J;     // (jobs job0 .. job0 + J - 1 in this launch)
  unsigned blk;
  int j;
  if (job_major) {                           // (ART_ANALYSIS_ORDER=job: one job's workgroups after the other, for the A/B)
    j = (int)(id / P8);
    blk = id - (unsigned)j * P8;
  } else {
    const unsigned k = id >> 3, kq = k / (unsigned)J;
    blk = kq * 8u + (id & 7u);
    j = (int)(k - kq * (unsigned)J);
  }
  if (blk >= (unsigned)P) return;            // (padding)
  j += job0;
  const ArtAnalysisJob& jb = jobs[j];
  double acc[kAnaMom];
#pragma unroll
  for (int k = 0; k < kAnaMom; ++k) acc[k] = red_ident(ana_mom_op(k));
  acc[34] = 0.0;    // the largest angle of an empty set is 0 (ReturnNumericalAperture's max over nothing never happens)
  const bool active = jb.mode != ART_JOB_SUMS && out[(int64_t)j * ART_ANALYSIS_DOUBLES] > 0.0;
  if (active) {
    if (jb.w) moments_body<true>(jb, n, place + (int64_t)j * kAnaPlace, acc, blk, (unsigned)P);
    else moments_body<false>(jb, n, place + (int64_t)j * kAnaPlace, acc, blk, (unsigned)P);
  }
  block_reduce_store<kAnaMom>(acc, ana_mom_op, scratch + ((int64_t)j * P + blk) * kAnaMom);
}

// grid (kAnaMom - 1, n_jobs): workgroup (q, j) folds partial q of job j into its output slot
__global__ __launch_bounds__(kBlock) void k_analysis_fold(const ArtAnalysisJob* __restrict__ jobs, const int nblocks,
                                                          const double* scratch, double* out) {
  const int q = blockIdx.x, j = blockIdx.y;
  if (jobs[j].mode == ART_JOB_SUMS) return;
  double v;
  fold_range<4, kBlock>(scratch + (int64_t)j * nblocks * kAnaMom + q, 0, nblocks, ana_mom_op(q), &v, kAnaMom);
  // partial 34 carries tan^2(angle / 2) of the ray farthest from the mean direction: the angle is formed here, once
  if (threadIdx.x == 0) out[(int64_t)j * ART_ANALYSIS_DOUBLES + ana_mom_slot(q)] = (q == 34) ? 2.0 * atan(sqrt(v)) : v;
}

// ------------------------------------------------------------------------------------------- compaction
// Stable stream compaction of the alive mask in three passes: per-tile counts, exclusive scan of the tile
// counts by one workgroup, scatter with an intra-wave ballot/popcount rank.
constexpr int kTile = 2048;  // slots per workgroup: 8 per lane

// number of non-zero bytes of a 64-bit word
__device__ __forceinline__ int nonzero_bytes(const unsigned long long x) {
  const unsigned long long lo7 = 0x7f7f7f7f7f7f7f7full;
  return __popcll(((x & lo7) + lo7 | x) & ~lo7);
}
// A tile's 2048 alive bytes as ONE 8-byte load per lane (the count needs no order); the last, partial tile and a mask that
// does not start on an 8-byte boundary take the byte path.  10 MB per 1e7 rays: the kernel is a few microseconds of launch
// and latency, not bandwidth (it was 14.6 us with eight dependent byte loads per lane).
__global__ __launch_bounds__(kBlock) void k_compact_count(const uint8_t* alive, const int64_t n, int32_t* counts) {
  __shared__ int s[kBlock / 64];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  int c = 0;
  if (base + kTile <= n && (reinterpret_cast<uintptr_t>(alive) & 7u) == 0) {     // (workgroup-uniform)
    c = nonzero_bytes(reinterpret_cast<const unsigned long long*>(alive + base)[threadIdx.x]);   // (default policy: the scatter pass reads the mask again)
  } else {
    uint8_t a[kTile / kBlock];
#pragma unroll
    for (int j = 0; j < kTile / kBlock; ++j) {
      const int64_t i = base + j * kBlock + threadIdx.x;
      a[j] = (i < n) ? alive[i] : 0;
    }
#pragma unroll
    for (int j = 0; j < kTile / kBlock; ++j) c += a[j] != 0 ? 1 : 0;
  }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

__global__ __launch_bounds__(1024) void k_compact_scan(int32_t* counts, const int64_t ntiles, int64_t* total,
                                                       int64_t* tile_offsets) {
  // single workgroup; each lane owns a contiguous chunk -> local sums -> LDS scan -> write back
  __shared__ int64_t s[1024];
  const int64_t per = (ntiles + 1023) / 1024;
  const int64_t lo = (int64_t)threadIdx.x * per;
  const int64_t hi = (lo + per < ntiles) ? lo + per : ntiles;
  int64_t sum = 0;
  for (int64_t k = lo; k < hi; ++k) sum += counts[k];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    int64_t v = (threadIdx.x >= (unsigned)off) ? s[threadIdx.x - off] : 0;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
  int64_t run = s[threadIdx.x] - sum;  // exclusive prefix of this chunk
  for (int64_t k = lo; k < hi; ++k) {
    tile_offsets[k] = run;
    run += counts[k];
  }
  if (threadIdx.x == 1023) *total = s[1023];
}

// Ranks of a tile's alive slots, all eight passes at once: the eight alive bytes of a lane (slots base + j*256 + t) are
// requested together, every wave ballots its eight passes and parks the popcounts, ONE barrier, and each lane adds up what
// lies in front of it (passes before its own in full, earlier waves of its own pass, its rank inside the ballot).  Round 4
// did this pass by pass: eight dependent byte loads and sixteen barriers per tile.
struct TileRanks {
  bool a[kTile / kBlock];
  int pos[kTile / kBlock];     // position of slot j among the tile's alive slots (valid where a[j])
};
__device__ __forceinline__ void tile_ranks(const uint8_t* alive, const int64_t n, const int64_t base, int (*s_cnt)[kBlock / 64],
                                           TileRanks& q) {
  constexpr int P = kTile / kBlock;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint8_t raw[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int64_t i = base + j * kBlock + threadIdx.x;
    raw[j] = (i < n) ? alive[i] : 0;      // (default policy: the count pass has just read these lines)
  }
  int rank[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    q.a[j] = raw[j] != 0;
    const unsigned long long m = __ballot(q.a[j]);
    rank[j] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[j][wv] = __popcll(m);
  }
  __syncthreads();
  int run = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    int before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kBlock / 64; ++k) {
      const int c = s_cnt[j][k];
      before += (k < wv) ? c : 0;
      tot += c;
    }
    q.pos[j] = run + before + rank[j];
    run += tot;
  }
}

__global__ __launch_bounds__(kBlock) void k_compact_scatter(const uint8_t* alive, const int64_t n,
                                                            const int64_t* tile_offsets, int64_t* idx_out) {
  __shared__ int s_cnt[kTile / kBlock][kBlock / 64];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int64_t run = tile_offsets[blockIdx.x];
  TileRanks q;
  tile_ranks(alive, n, base, s_cnt, q);
#pragma unroll
  for (int j = 0; j < kTile / kBlock; ++j)
    if (q.a[j]) idx_out[run + q.pos[j]] = base + j * kBlock + threadIdx.x;
}

// ------------------------------------------------------------------------------------------- survivor records
// Send buffer of the multi-GPU gather (art_pack_survivors, include/art_hip.h): a 16-byte header (count, flags) followed
// by the sections X[count], Y[count], path[count] (fp64) and number[count] (int32) of the SURVIVING rays in slot order.
// Pass 1 + 2 are the compaction's (per-tile counts, one-workgroup scan); the header is written from the scan's total,
// and pass 3 scatters the records instead of slot indices.
constexpr int64_t kSurvHeader = 16;
constexpr int64_t kSurvDense = 1;   // header flag: every slot alive and numbers implicit -> no number section

__global__ void k_survivor_header(const int64_t* total, const int64_t n, const int implicit_numbers, int64_t* header) {
  if (threadIdx.x == 0) {
    header[0] = *total;
    header[1] = (implicit_numbers && *total == n) ? kSurvDense : 0;
  }
}

__global__ __launch_bounds__(kBlock) void k_survivor_scatter(const uint8_t* alive, const int64_t n,
                                                             const int64_t* tile_offsets, const double* X,
                                                             const double* Y, const double* opl, const int64_t* number,
                                                             const int64_t first, const int64_t step,
                                                             unsigned char* send) {
  __shared__ int s_cnt[kTile / kBlock][kBlock / 64];
  const int64_t* header = reinterpret_cast<const int64_t*>(send);
  const int64_t count = header[0];
  const bool dense = (header[1] & kSurvDense) != 0;
  double* sx = reinterpret_cast<double*>(send + kSurvHeader);
  double* sy = sx + count;
  double* so = sy + count;
  int32_t* sn = reinterpret_cast<int32_t*>(so + count);
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int64_t run = tile_offsets[blockIdx.x];
  TileRanks q;
  tile_ranks(alive, n, base, s_cnt, q);
  // four passes at a time: their records are requested together (12-16 loads in flight per lane) and then stored -- with
  // the default cache policy: the records of a masked shard land at unaligned positions, and non-temporal partial-line
  // stores measured 8 % slower (98.5 -> 106.5 us per 1e7 dense slots, profiles/r05_experiments.md)
  constexpr int P = kTile / kBlock, H = 4;
#pragma unroll
  for (int j0 = 0; j0 < P; j0 += H) {
    double xv[H], yv[H], ov[H];
    int64_t nv[H];
#pragma unroll
    for (int u = 0; u < H; ++u) {
      const int64_t i = base + (j0 + u) * kBlock + threadIdx.x;
      if (q.a[j0 + u]) {
        xv[u] = ld_nt(X + i); yv[u] = ld_nt(Y + i); ov[u] = ld_nt(opl + i);
        nv[u] = (number && !dense) ? ld_nt(number + i) : first + i * step;
      }
    }
#pragma unroll
    for (int u = 0; u < H; ++u) {
      if (q.a[j0 + u]) {
        const int64_t p = run + q.pos[j0 + u];
        sx[p] = xv[u]; sy[p] = yv[u]; so[p] = ov[u];
        if (!dense) sn[p] = (int32_t)nv[u];
      }
    }
  }
}

// Zero-copy form of the send buffer (art_survivor_finish): the read-out wrote X, Y, path of ALL n slots straight into the
// dense layout's sections; if every slot is alive the buffer is complete once its header says so.  Otherwise the header
// says "unpacked" (flags bit 1): the sections hold slot-indexed values with holes, and the caller packs them elsewhere.
constexpr int64_t kSurvUnpacked = 2;
// xhdr (optional): the rank's contribution to the per-step header exchange of a sharded run -- [0], [1] = count, flags as
// int64 bit patterns, [2 .. 25] = the shard's 24 read-out statistics (zeros if none are given)
constexpr int kXhdrDoubles = 26;
__device__ __forceinline__ void xheader_store(const int64_t count, const int64_t flags, const double* stats24, double* xhdr) {
  const int t = threadIdx.x;
  if (t == 0) { reinterpret_cast<int64_t*>(xhdr)[0] = count; reinterpret_cast<int64_t*>(xhdr)[1] = flags; }
  if (t < kReadoutSlots) xhdr[2 + t] = stats24 ? stats24[t] : 0.0;
}
__global__ void k_survivor_finish(const double* stats24, const int64_t n, int64_t* header, double* xhdr) {
  const int64_t count = (int64_t)stats24[0];
  const int64_t flags = (count == n) ? kSurvDense : kSurvUnpacked;
  if (threadIdx.x == 0) { header[0] = count; header[1] = flags; }
  if (xhdr) xheader_store(count, flags, stats24, xhdr);
}
__global__ void k_survivor_xheader(const int64_t* header, const double* stats24, double* xhdr) {
  xheader_store(header[0], header[1], stats24, xhdr);
}

// ------------------------------------------------------------------------------------------- sources
__global__ __launch_bounds__(kBlock) void k_make_source(const int32_t kind, const double size, const ArtDetectorDesc rs,
                                                        const int64_t first, const int64_t step, const int64_t n,
                                                        const int64_t n_total, const ArtBundleView out) {
  // rs.rot = rotation ez -> axis, rs.centre = S (ArtDetectorDesc reused as a POD carrier); slot i = global ray
  // first + i * step (step 1: a contiguous shard; step = world size: a strided one)
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    art::Ray r;
    art::source_ray(kind, size, rs.rot, rs.centre, first + i * step, n_total, r);
    store_ray(out, i, r);
    out.alive[i] = 1;
  }
}

__global__ __launch_bounds__(kBlock) void k_make_extended_source(const double radius, const double divergence,
                                                                 const int64_t n_points, const int64_t per,
                                                                 const ArtDetectorDesc rs, const int64_t first,
                                                                 const int64_t n, const ArtBundleView out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    art::Ray r;
    art::source_ray_extended(radius, divergence, n_points, per, rs.rot, rs.centre, first + i, r);
    store_ray(out, i, r);
    out.alive[i] = 1;
  }
}

// multi-GPU exchange (include/art_hip.h): pack statistics + a sample of the read-out; fold the gathered statistics
__global__ __launch_bounds__(kBlock) void k_exchange_pack(const double* stats, const double* X, const double* Y,
                                                          const double* opl, const uint8_t* alive, const int64_t* slots,
                                                          const int64_t k, double* send) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j < kReadoutSlots) send[j] = stats[j];
  if (j < k) {
    const int64_t s = slots[j];
    double* o = send + kReadoutSlots + 4 * j;
    o[0] = X[s]; o[1] = Y[s]; o[2] = opl[s]; o[3] = alive[s] ? 1.0 : 0.0;
  }
}

__global__ void k_exchange_fold(const double* recv, const int world, const int64_t stride, double* out) {
  const int s = threadIdx.x;
  if (s >= kReadoutSlots) return;
  const int op = stat_op(s);
  double v = recv[s];
  for (int r = 1; r < world; ++r) v = fold_op(v, recv[(int64_t)r * stride + s], op);   // rank order: deterministic
  out[s] = v;
}

// rays per launch: the hardware limit, or less when ART_MAX_RAYS_PER_LAUNCH is set (lets tests cover the chunking)
int64_t max_rays_per_launch() {
  const char* v = getenv("ART_MAX_RAYS_PER_LAUNCH");
  if (v) {
    const long long x = atoll(v);
    if (x >= 64 && x < kMaxRaysPerLaunchHw) return (int64_t)x;
  }
  return kMaxRaysPerLaunchHw;
}

// slot-offset copy of a view (launch chunking: one launch addresses at most max_rays_per_launch() slots)
ArtBundleView view_at(const ArtBundleView& v, int64_t off) {
  ArtBundleView r = v;
  if (v.alive == nullptr) return r;  // absent history view stays absent
  r.ox += off; r.oy += off; r.oz += off; r.dx += off; r.dy += off; r.dz += off;
  r.path += off; r.incidence += off; r.alive += off;
  return r;
}

bool view_ok(const ArtBundleView* v) {
  return v && v->ox && v->oy && v->oz && v->dx && v->dy && v->dz && v->path && v->incidence && v->alive;
}

int check_elem(const ArtElementDesc* e) {
  if (!e) return fail(ART_ERR_BAD_ARG, "element descriptor is NULL");
  if (e->kind < 0 || e->kind >= ART_NUM_KINDS) return fail(ART_ERR_BAD_ARG, "unknown optic kind");
  if (e->support_kind < 0 || e->support_kind > ART_SUP_RECTRECTHOLE) return fail(ART_ERR_BAD_ARG, "unknown support kind");
  if (e->n_defects < 0 || e->n_defects > ART_MAX_DEFECTS) return fail(ART_ERR_UNSUPPORTED, "too many defects on one mirror");
#ifdef ART_ZERN_LDS
  if (e->n_defects > 4) return fail(ART_ERR_UNSUPPORTED, "ART_ZERN_LDS comparison build: at most 4 Zernike tables per element");
#endif
  if (e->n_defects > 0 && e->kind == ART_MASK) return fail(ART_ERR_BAD_ARG, "a mask cannot carry defects");
  if (e->n_defects > 0 && !e->zern) return fail(ART_ERR_BAD_ARG, "n_defects > 0 but zern table is NULL");
  if (e->n_grid < 0 || e->n_grid > ART_MAX_DEFECTS) return fail(ART_ERR_UNSUPPORTED, "too many gridded defects on one mirror");
  if (e->n_grid > 0 && e->kind == ART_MASK) return fail(ART_ERR_BAD_ARG, "a mask cannot carry defects");
  if (e->n_grid > 0 && !e->grid) return fail(ART_ERR_BAD_ARG, "n_grid > 0 but grid table is NULL");
  if ((e->flags & ART_FLAG_ZERN_RECURRENCE) && e->n_defects == 0) return fail(ART_ERR_BAD_ARG, "recurrence flag without Zernike tables");
  return ART_OK;
}

const char* const kGratingRefusal = "an element is a grating: trace it with art_trace_grating";
const char* const kQuadricRefusal = "an element is a general quadric: trace it with art_trace_quadric";
const char* const kFreeformRefusal = "an element is a freeform mirror: trace it with art_trace_freeform";

template <int KIND>
void launch_element(const ArtElementDesc& e, const ArtBundleView& in, const ArtBundleView& out, int64_t n,
                    hipStream_t s) {
  ElemArg ea;
  ea.e[0] = e;
  const int xm = xcd_map();
  if (e.n_defects > 0 || e.n_grid > 0)
    hipLaunchKernelGGL((k_trace_element<KIND, true>), dim3(kDefectLoop ? grid_for(n) : grid_stream_mapped(n, xm)),
                       dim3(kBlock), 0, s, ea, in, out, n, kDefectLoop ? 0 : xm);
  else
    hipLaunchKernelGGL((k_trace_element<KIND, false>), dim3(grid_stream_mapped(n, xm)), dim3(kBlock), 0, s, ea, in, out, n,
                       xm);
}

// The launches of an n-ray call: f(off, m) for the slots [off, off + m), m <= max_rays_per_launch() (32-bit buffer
// offsets); stops at the first error code f returns.
template <typename F>
int per_launch(const int64_t n, F&& f) {
  const int64_t chunk = max_rays_per_launch();
  for (int64_t off = 0; off < n; off += chunk) {
    const int rc = f(off, (n - off < chunk) ? n - off : chunk);
    if (rc) return rc;
  }
  return ART_OK;
}

// the entry points' epilogue: a launch that failed in this call (hipGetLastError) -> ART_ERR_HIP
int launched(const char* what) {
  const hipError_t err = hipGetLastError();
  return (err != hipSuccess) ? fail_hip(err, what) : ART_OK;
}

// the epilogue of a standalone reduction: fold the nb partials [block][NS] in `scratch` into out[0 .. NS)
template <int NS, int (*OP)(int)>
int fold_partials(const double* scratch, const int nb, double* out, hipStream_t s, const char* what) {
  hipLaunchKernelGGL((k_fold_partials<NS, 8, OP>), dim3(NS), dim3(kBlock), 0, s, scratch, nb, out);
  return launched(what);
}

#ifdef ART_ZERN_LDS
inline size_t zern_lds_bytes(const ChainArgs& a) {
  size_t d = 0;
  for (int k = 0; k < a.n_elems; ++k) d += (size_t)a.e[k].n_defects;
  return d * ART_ZERN_STRIDE * sizeof(double);
}
#endif
// Workgroups per launch of the separate read-out: a persistent grid of kReadoutBlocks (2048).  The scratch area has room
// for 8 x that; ART_READOUT_BLOCKS=<n> uses it (measured at 1e7 rays, tools/r02_exp21.sh: 2048 -> 157-160 us, 4096 ->
// 161, 8192 -> 161, 16384 -> 170-177: here the per-workgroup reduction outweighs what shorter-lived workgroups gain).
inline int64_t readout_block_cap(int64_t launches) {
  static const int64_t env = [] {
    const char* e = getenv("ART_READOUT_BLOCKS");
    const long x = e ? atol(e) : 0;
    return (int64_t)(x < 1 ? 0 : x);
  }();
  const int64_t room = (int64_t)8 * kReadoutBlocks / (launches < 1 ? 1 : launches);
  return (env > 0) ? (env < room ? env : room) : (kReadoutBlocks < room ? kReadoutBlocks : room);
}
// register budget of the fused kernel in waves per SIMD: 5 (91 VGPRs with the LDS store path).  A 6-wave build (80
// VGPRs) is kept as ART_CHAIN_WAVES=6 for experiments: with 8-byte stores it fitted without spills and measured 3 %
// faster on relay4 without the read-out tail, the same with it, C2 +1 %, C4 13 % slower (tools/r02_exp16.sh); with the
// LDS store path it spills 5 dwords.
inline int chain_waves() {
  const char* wv = getenv("ART_CHAIN_WAVES");
  return wv ? atoi(wv) : 5;
}
// Which body traces a chain without defects: chain_body (one ray per lane, outputs regrouped through LDS) or chain_body2
// (two rays per lane, no staging).  Measured A/B inside one process (tools/ab_kernel.py, profiles/r03_experiments.md): the
// two-ray body is 4-7 % faster on chains behind a MASK (C2, C3: a third to a half of the slots are dead -- it skips a
// dead pair with one branch and two dropped offsets, where the one-ray body still stages, synchronises and issues the
// workgroup's stores) and -3 ... +9 % elsewhere, box-dependent; so it is the default exactly where a mask is part of the
// launch -- and in a one-segment scene whose chains share their input (XCD-grouped grid, scene_wg): -8 % without a mask,
// -9 % behind one, where a lone chain (relay4) is 7 % SLOWER with it (profiles/r05_experiments.md batch s).
// ART_CHAIN_RPL=1|2 overrides (read at every call: the A/B tool alternates the variants inside one process).
// (One getenv + atoi per launch, ~0.1 us, on purpose: a cached value could not be alternated by the A/B tool.)
inline int chain_rpl(const bool has_mask) {
  const char* e = getenv("ART_CHAIN_RPL");
  const int v = e ? atoi(e) : 0;
  return (v == 1 || v == 2) ? v : (has_mask ? 2 : 1);
}
// Grid shape of a scene launch whose chains share their input: XCD-grouped by default (scene_wg).  -> 0 tile-major, 1
// chain-interleaved 2-D grid, 4 XCD-grouped.  ART_SCENE_ORDER=tile|chain|xcd forces one shape for every scene (read per
// launch: the A/B tools alternate them inside one process).
inline int scene_order(const bool shared_in) {
  const char* e = getenv("ART_SCENE_ORDER");
  if (e && e[0] == 't') return 0;
  if (e && e[0] == 'c') return 1;
  if (e && e[0] == 'x') return 4;
  return shared_in ? 4 : 0;
}
// ART_ROW_SUMMARY=0: scene launches ignore the row summaries attached to their image (art_scene_set_row_summaries) and load
// every row, as without them (read per launch: the A/B tools alternate the two inside one process).
inline bool row_summaries_on() {
  const char* e = getenv("ART_ROW_SUMMARY");
  return !(e && e[0] == '0');
}
// ... and whether that shared input is loaded with the default cache policy instead of non-temporal loads.  XCD-grouped:
// always -- the C - 1 re-reads of a tile follow within microseconds in the same L2 (profiles/r05_experiments.md batch r: 10
// chains x 1e7 rays 3.167 against 3.280 ms, 11 x 1e6 0.299 against 0.314).  In the interleaved 2-D grid the re-reads come
// from the memory-side cache: worth it while the input (57 B per slot) fits its 256 MB -- 11 chains x 1e6 rays -10 %, 10
// chains x 4e6 rays (228 MB) -15 %, but 10 chains x 1e7 rays (570 MB) +6 ... +8 % (profiles/r04_experiments.md, batch 8).
// ART_SCENE_KEEP=0|1 overrides (A/B).
inline bool scene_keep(const int64_t n, const bool xcd_grouped) {
  const char* e = getenv("ART_SCENE_KEEP");
  if (e && (e[0] == '0' || e[0] == '1')) return e[0] == '1';
  return xcd_grouped || n * 57 <= ((int64_t)256 << 20);
}
// ART_CHAIN_DYN_LDS=<bytes>: unused dynamic LDS per workgroup of the fused kernel, i.e. FEWER resident workgroups per CU
// (20 KB static + 20480 -> 4, + 33000 -> 3).  An experiment knob: the bare access pattern gains 3-7 % of bandwidth with 2-3
// instead of 8 workgroups per CU (tools/stream_floor.hip); the kernel needs its waves to hide latency.
inline size_t chain_dyn_lds() {
  static const size_t v = [] {
    const char* e = getenv("ART_CHAIN_DYN_LDS");
    const long x = e ? atol(e) : 0;
    return (size_t)(x < 0 ? 0 : (x > 100000 ? 100000 : x));
  }();
  return v;
}

// One-element chains with defects whose optic is a plane, a sphere or a parabola (what a deformed mirror usually is: C5)
// run a body compiled for that kind (k_trace_*1): no run-time switch, no torus state -- 98 VGPRs instead of 118.
// ART_CHAIN_SPECIAL=0 switches it off, ART_CHAIN_SPECIAL_WAVES=5 selects the 5-wave build (96 VGPRs, one 8-byte spill per
// ray in front of the stores); read per launch: the A/B tool alternates them inside one process.
inline int special_waves() {
  const char* e = getenv("ART_CHAIN_SPECIAL");
  if (e && e[0] == '0') return 0;
  const char* w = getenv("ART_CHAIN_SPECIAL_WAVES");
  return (w && atoi(w) == 5) ? 5 : 4;
}
inline bool special_kind(const int kind) { return kind == ART_PLANE || kind == ART_SPHERE || kind == ART_PARABOLA; }
static_assert(ART_PLANE == 0 && ART_SPHERE == 1 && ART_PARABOLA == 2, "special kinds index the dispatchers' tables");

// The body of a fused launch: kSpecial k_trace_*1<kind, waves>, kDefect k_trace_*<true, 4>, kTwoRay k_trace_*2<false, 4>,
// kOneRay k_trace_*<false, waves>.
enum class Body { kSpecial, kDefect, kTwoRay, kOneRay };
struct BodyChoice {
  Body body;
  int waves;   // waves per SIMD of the build (__launch_bounds__)
  int kind;    // kSpecial: the optic kind the body is compiled for
};
// The one rule of both entry points: art_trace_chain* (descriptors in kernel arguments, launch_chain_body) and
// art_trace_scene (table segments, launch_scene_body).  Where the two paths differ they do so on purpose, as measured:
//   * has_mask -- chain path: a MASK element in this segment; scene path: kFlagMask, or kFlagSharedIn && n_chains > 1 &&
//     S == 1 (one segment of chains that share their input: the XCD-grouped grid, where the two-ray body gains too);
//   * kind1, the kind a special body would be compiled for (ART_KIND_DYN: none) -- chain path: m == 1, !kDefectLoop and special_kind;
//     scene path: n_elems == 1 and the same kind in every chain;
//   * dynamic LDS -- chain path: chain_dyn_lds() for the bodies without defects, zern_lds_bytes() (ART_ZERN_LDS) for the
//     defect body, 0 for the special one; scene path: 0;
//   * kDefectLoop builds (ART_ZERN_LDS) -- chain path: the defect body runs the persistent grid_for(n) with xmap 0; scene
//     path: scenes with defects are refused;
//   * a chain of ONE element without a read-out never gets here: trace_chain_impl hands it to art_trace_element.
// The knobs are read at every call (chain_rpl, chain_waves, special_waves): the A/B tools and the GPU tests switch them
// inside one process.
BodyChoice choose_body(const bool defects, const bool has_mask, const int kind1) {
  if (defects) {
    const int sw = special_kind(kind1) ? special_waves() : 0;
    if (sw) return {Body::kSpecial, sw, kind1};
    // (the fused kernel WITH defects stays at 4 waves: 112 VGPRs without spills; at 5 waves it spills 15 dwords and
    // measured 0.335 instead of 0.31 ms per 1e7 rays on C5, tools/r02_exp17.sh.  It keeps the one-ray body: the two-ray
    // one needs 133 VGPRs = 3 waves per SIMD there and measured +1.6 % on C5 with the read-out, the same without;
    // profiles/r03_experiments.md)
    return {Body::kDefect, 4, ART_KIND_DYN};
  }
  // two rays per lane: 107 VGPRs, 4 waves per SIMD (3 and 5 measured the same or worse, tools/ab_kernel.py)
  if (chain_rpl(has_mask) == 2) return {Body::kTwoRay, 4, ART_KIND_DYN};
  return {Body::kOneRay, chain_waves() == 6 ? 6 : 5, ART_KIND_DYN};
}

// The choice -> its kernel, and the launch.  Descriptors in kernel arguments (one chain, `n` rays of one launch):
void launch_chain_body(const BodyChoice& c, const ChainArgs& a, const int64_t n, const int tiles, const int xm,
                       const size_t zern_lds, hipStream_t s) {
  typedef void (*K)(const ChainArgs, const int64_t, const int);
  const K special[2][3] = {{k_trace_chain1<ART_PLANE, 4>, k_trace_chain1<ART_SPHERE, 4>, k_trace_chain1<ART_PARABOLA, 4>},
                           {k_trace_chain1<ART_PLANE, 5>, k_trace_chain1<ART_SPHERE, 5>, k_trace_chain1<ART_PARABOLA, 5>}};
  const K k = (c.body == Body::kSpecial) ? special[c.waves - 4][c.kind]
              : (c.body == Body::kDefect) ? k_trace_chain<true, 4>
              : (c.body == Body::kTwoRay) ? k_trace_chain2<false, 4>
              : (c.waves == 6) ? k_trace_chain<false, 6> : k_trace_chain<false, 5>;
  const bool loop = kDefectLoop && c.body == Body::kDefect;
  const size_t lds = (c.body == Body::kSpecial) ? 0 : (c.body == Body::kDefect ? zern_lds : chain_dyn_lds());
  hipLaunchKernelGGL(k, dim3(loop ? grid_for(n) : tiles), dim3(kBlock), lds, s, a, n, loop ? 0 : xm);
}
// ... in a segment of the scene table (rays [first, first + n) of every chain, grid and shape from art_trace_scene):
void launch_scene_body(const BodyChoice& c, const dim3 g, const ChainArgs* seg, const int64_t first, const int64_t n,
                       const int xarg, const int shape, const art::RowSummary* sums, hipStream_t s) {
  typedef void (*K)(const ChainArgs*, const int64_t, const int64_t, const int, const int, const art::RowSummary*);
  const K special[2][3] = {{k_trace_scene1<ART_PLANE, 4>, k_trace_scene1<ART_SPHERE, 4>, k_trace_scene1<ART_PARABOLA, 4>},
                           {k_trace_scene1<ART_PLANE, 5>, k_trace_scene1<ART_SPHERE, 5>, k_trace_scene1<ART_PARABOLA, 5>}};
  const K k = (c.body == Body::kSpecial) ? special[c.waves - 4][c.kind]
              : (c.body == Body::kDefect) ? k_trace_scene<true, 4>
              : (c.body == Body::kTwoRay) ? k_trace_scene2<false, 4>
              : (c.waves == 6) ? k_trace_scene<false, 6> : k_trace_scene<false, 5>;
  hipLaunchKernelGGL(k, g, dim3(kBlock), 0, s, seg, first, n, xarg, shape, sums);
}

}  // namespace

// =================================================================================================== C ABI
extern "C" {

int art_abi_version(void) { return ART_ABI_VERSION; }

const char* art_last_error(void) { return g_err; }

int art_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail_hip(e, "hipGetDeviceCount");
  }
  int good = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  return good;
}

int art_trace_element(const ArtElementDesc* e, const ArtBundleView* in, const ArtBundleView* out, int64_t n,
                      void* stream) {
  int rc = check_elem(e);
  if (rc) return rc;
  if (e->flags & ART_FLAG_GRATING) return fail(ART_ERR_UNSUPPORTED, kGratingRefusal);
  if (e->flags & ART_FLAG_QUADRIC) return fail(ART_ERR_UNSUPPORTED, kQuadricRefusal);
  if (e->flags & ART_FLAG_FREEFORM) return fail(ART_ERR_UNSUPPORTED, kFreeformRefusal);
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n == 0) return ART_OK;  // an empty bundle has no arrays to point to
  if (!view_ok(in) || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  hipStream_t s = (hipStream_t)stream;
  ArtElementDesc ec = *e;
  art::prepare_element(ec);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    const ArtBundleView vi = view_at(*in, off), vo = view_at(*out, off);
    if (ec.flags & ART_FLAG_ZERN_RECURRENCE) {
      ElemArg ea;
      ea.e[0] = ec;
      hipLaunchKernelGGL(k_trace_element_zrec, dim3(grid_stream(m)), dim3(kBlock), 0, s, ea, vi, vo, m);
      return ART_OK;
    }
    switch (ec.kind) {
      case ART_PLANE: launch_element<ART_PLANE>(ec, vi, vo, m, s); break;
      case ART_SPHERE: launch_element<ART_SPHERE>(ec, vi, vo, m, s); break;
      case ART_PARABOLA: launch_element<ART_PARABOLA>(ec, vi, vo, m, s); break;
      case ART_TORUS: launch_element<ART_TORUS>(ec, vi, vo, m, s); break;
      case ART_ELLIPSOID: launch_element<ART_ELLIPSOID>(ec, vi, vo, m, s); break;
      case ART_CYLINDER: launch_element<ART_CYLINDER>(ec, vi, vo, m, s); break;
      default: launch_element<ART_MASK>(ec, vi, vo, m, s); break;
    }
    return ART_OK;
  });
  return launched("art_trace_element launch");
}

int art_trace_grating(const ArtElementDesc* e, const ArtGratingDesc* g, const double* wavelengths_host,
                      const ArtBundleView* outs_host, const ArtBundleView* in, int64_t n, void* stream) {
  int rc = check_elem(e);
  if (rc) return rc;
  if (e->flags & ART_FLAG_QUADRIC) return fail(ART_ERR_UNSUPPORTED, kQuadricRefusal);
  if (e->flags & ART_FLAG_FREEFORM) return fail(ART_ERR_UNSUPPORTED, kFreeformRefusal);
  if (e->kind == ART_MASK) return fail(ART_ERR_BAD_ARG, "art_trace_grating: a mask cannot be a grating");
  if (e->n_defects > 0 || e->n_grid > 0) return fail(ART_ERR_BAD_ARG, "art_trace_grating: mirrors with defects are not supported as substrates");
  if (!g || !wavelengths_host || !outs_host) return fail(ART_ERR_BAD_ARG, "art_trace_grating: NULL argument");
  if (!(fabs(g->q[0] * g->q[0] + g->q[1] * g->q[1] - 1.0) <= 1e-12)) return fail(ART_ERR_BAD_ARG, "art_trace_grating: q must be a unit vector");
  if (!(isfinite(g->lines_per_mm) && g->lines_per_mm >= 0.0)) return fail(ART_ERR_BAD_ARG, "art_trace_grating: lines_per_mm must be finite and >= 0");
  if (g->nw < 1 || g->nw > ART_GRATING_MAX_WAVELENGTHS) return fail(ART_ERR_BAD_ARG, "art_trace_grating: nw must be in 1..ART_GRATING_MAX_WAVELENGTHS");
  for (int j = 0; j < g->nw; ++j)
    if (!(isfinite(wavelengths_host[j]) && wavelengths_host[j] > 0.0)) return fail(ART_ERR_BAD_ARG, "art_trace_grating: every wavelength must be finite and > 0");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "art_trace_grating: more rays than one launch covers");
  if (n == 0) return ART_OK;  // an empty bundle has no arrays to point to
  if (!g->wavelengths || !g->outs) return fail(ART_ERR_BAD_ARG, "art_trace_grating: device arrays of wavelengths / views missing");
  if (!view_ok(in)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  for (int j = 0; j < g->nw; ++j) {
    if (!view_ok(&outs_host[j])) return fail(ART_ERR_BAD_ARG, "an output view has a NULL array");
    if (g->nw > 1 && (outs_host[j].ox == in->ox || outs_host[j].alive == in->alive))
      return fail(ART_ERR_BAD_ARG, "art_trace_grating: an output may alias the input only when nw == 1");
  }
  ElemArg ea;
  ea.e[0] = *e;
  art::prepare_element(ea.e[0]);
  hipLaunchKernelGGL(k_trace_grating, dim3(grid_stream(n)), dim3(kBlock), 0, (hipStream_t)stream, ea, *g, *in, n);
  return launched("art_trace_grating launch");
}

int art_trace_quadric(const ArtElementDesc* e, const ArtQuadricDesc* q, const ArtBundleView* in, const ArtBundleView* out,
                      int64_t n, void* stream) {
  int rc = check_elem(e);
  if (rc) return rc;
  if (e->flags & ART_FLAG_FREEFORM) return fail(ART_ERR_UNSUPPORTED, kFreeformRefusal);
  if (!q || !in || !out) return fail(ART_ERR_BAD_ARG, "art_trace_quadric: NULL argument");
  if (e->n_defects > 0 || e->n_grid > 0) return fail(ART_ERR_BAD_ARG, "art_trace_quadric: mirrors with defects are not supported");
  bool finite = isfinite(q->c), any = false;
  for (int k = 0; k < 6; ++k) { finite = finite && isfinite(q->q[k]); any = any || q->q[k] != 0.0; }
  for (int k = 0; k < 3; ++k) { finite = finite && isfinite(q->b[k]); any = any || q->b[k] != 0.0; }
  if (!finite) return fail(ART_ERR_BAD_ARG, "art_trace_quadric: every coefficient must be finite");
  if (!any) return fail(ART_ERR_BAD_ARG, "art_trace_quadric: q and b are all zero: no surface");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n == 0) return ART_OK;  // an empty bundle has no arrays to point to
  if (!view_ok(in) || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  ElemArg ea;
  ea.e[0] = *e;
  art::prepare_element(ea.e[0]);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    hipLaunchKernelGGL(k_trace_quadric, dim3(grid_stream(m)), dim3(kBlock), 0, (hipStream_t)stream, ea, *q, view_at(*in, off),
                       view_at(*out, off), m);
    return ART_OK;
  });
  return launched("art_trace_quadric launch");
}

int art_trace_freeform(const ArtElementDesc* e, const ArtQuadricDesc* q, const ArtFigureDesc* figure, const ArtBundleView* in,
                       const ArtBundleView* out, int64_t n, void* stream) {
  int rc = check_elem(e);
  if (rc) return rc;
  if (!q || !figure || !in || !out) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: NULL argument");
  if (e->n_defects > 0 || e->n_grid > 0) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: defects on the element are not supported (they belong into the figure)");
  if (e->flags & (ART_FLAG_GRATING | ART_FLAG_QUADRIC)) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: the element is flagged as a grating or as a plain quadric");
  bool finite = isfinite(q->c), any = false;
  for (int k = 0; k < 6; ++k) { finite = finite && isfinite(q->q[k]); any = any || q->q[k] != 0.0; }
  for (int k = 0; k < 3; ++k) { finite = finite && isfinite(q->b[k]); any = any || q->b[k] != 0.0; }
  if (!finite) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: every coefficient must be finite");
  if (!any) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: q and b are all zero: no surface");
  if (!figure->table) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: the figure table is NULL");
  if (figure->order < 0 || figure->order > ART_ZERN_MAX_ORDER) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: figure order outside [0, 16]");
  if (!(isfinite(figure->radius) && figure->radius > 0.0)) return fail(ART_ERR_BAD_ARG, "art_trace_freeform: the figure's radius must be finite and positive");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n == 0) return ART_OK;  // an empty bundle has no arrays to point to
  if (!view_ok(in) || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  ElemArg ea;
  ea.e[0] = *e;
  art::prepare_element(ea.e[0]);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    hipLaunchKernelGGL(k_trace_freeform, dim3(grid_stream(m)), dim3(kBlock), 0, (hipStream_t)stream, ea, *q, figure->table,
                       view_at(*in, off), ViewArg{{view_at(*out, off)}}, m);
    return ART_OK;
  });
  return launched("art_trace_freeform launch");
}

static int trace_chain_impl(const ArtElementDesc* elems, int32_t n_elems, const ArtBundleView* in,
                            const ArtBundleView* outs, const ArtChainReadout* ro, int64_t n, void* stream) {
  if (!elems || !outs || n_elems <= 0) return fail(ART_ERR_BAD_ARG, "empty chain");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  for (int k = 0; k < n_elems; ++k) {
    int rc = check_elem(&elems[k]);
    if (rc) return rc;
    if (elems[k].flags & ART_FLAG_ZERN_RECURRENCE)
      return fail(ART_ERR_UNSUPPORTED, "an element carries Zernike tables in the recurrence layout: trace it with art_trace_element");
    if (elems[k].flags & ART_FLAG_GRATING) return fail(ART_ERR_UNSUPPORTED, kGratingRefusal);
    if (elems[k].flags & ART_FLAG_QUADRIC) return fail(ART_ERR_UNSUPPORTED, kQuadricRefusal);
    if (elems[k].flags & ART_FLAG_FREEFORM) return fail(ART_ERR_UNSUPPORTED, kFreeformRefusal);
  }
  hipStream_t s = (hipStream_t)stream;
  if (ro) {
    if (!art::readout_ok(*ro)) return fail(ART_ERR_BAD_ARG, "read-out: scratch/out24 missing, X/Y/opl partially NULL, or outputs / lite with sums");
    if (n > max_rays_per_launch()) return fail(ART_ERR_UNSUPPORTED, "fused read-out: more rays than one launch covers");
#ifdef ART_ZERN_LDS
    return fail(ART_ERR_UNSUPPORTED, "ART_ZERN_LDS comparison build: no fused read-out");
#endif
  }
  if (n == 0) {
    if (ro) {   // nothing to trace: the statistics are the reduction identities
      launch_fold(ro->sums, nullptr, 1, ro->scratch, ro->out24, 0, s);
      return launched("art_trace_chain_readout launch");
    }
    return ART_OK;  // an empty bundle has no arrays to point to
  }
  if (!view_ok(in)) return fail(ART_ERR_BAD_ARG, "input bundle view has a NULL array");
  for (int k = 0; k < n_elems; ++k)
    if (outs[k].alive != nullptr && !view_ok(&outs[k])) return fail(ART_ERR_BAD_ARG, "history view partially NULL");
  if (!view_ok(&outs[n_elems - 1])) return fail(ART_ERR_BAD_ARG, "the last output view is mandatory");
  // a chain of ONE element is the per-element kernel's job: compiled for the optic's kind, it needs fewer registers
  // than the fused kernel's run-time dispatch (5 instead of 4 waves per SIMD with defects) -- same results
  if (n_elems == 1 && !ro) return art_trace_element(&elems[0], in, &outs[0], n, stream);
  for (int k0 = 0; k0 < n_elems; k0 += kChainMax) {
    const int m = (n_elems - k0 < kChainMax) ? n_elems - k0 : kChainMax;
    // the chunk's last bundle is the next chunk's input: it must exist
    if (!view_ok(&outs[k0 + m - 1])) return fail(ART_ERR_BAD_ARG, "chains longer than 8 need a view every 8th element");
  }
  const int rc = per_launch(n, [&](const int64_t off, const int64_t cnt) {
    ArtBundleView cur = view_at(*in, off);
    for (int k0 = 0; k0 < n_elems; k0 += kChainMax) {
      ChainArgs a;
      memset(&a, 0, sizeof(a));
      const int m = (n_elems - k0 < kChainMax) ? n_elems - k0 : kChainMax;
      a.n_elems = m;
      a.in = cur;
      bool has_mask = false;
      for (int k = 0; k < m; ++k) {
        a.e[k] = elems[k0 + k];
        art::prepare_element(a.e[k]);
        a.out[k] = view_at(outs[k0 + k], off);
        if (a.e[k].n_defects > 0 || a.e[k].n_grid > 0) a.flags |= art::kFlagDefects;
        has_mask = has_mask || a.e[k].kind == ART_MASK;
      }
      const bool tail = ro && k0 + m == n_elems;       // the read-out rides on the chain's last fused launch
      if (tail) {
        a.ro = *ro;
        a.flags |= art::kFlagReadout;
      }
      size_t lds = 0;
#ifdef ART_ZERN_LDS
      lds = zern_lds_bytes(a);
      if (lds > 64 * 1024) return fail(ART_ERR_UNSUPPORTED, "ART_ZERN_LDS build: Zernike tables of one fused launch exceed 64 KiB");
#endif
      const BodyChoice c = choose_body((a.flags & art::kFlagDefects) != 0, has_mask,
                                       (!kDefectLoop && m == 1) ? a.e[0].kind : ART_KIND_DYN);
      const int xm = xcd_map();
      const int tiles = grid_stream_mapped(c.body == Body::kTwoRay ? (cnt + 1) / 2 : cnt, xm);
      launch_chain_body(c, a, cnt, tiles, xm, lds, s);
      if (tail) launch_fold(ro->sums, nullptr, 1, ro->scratch, ro->out24, ro->sums ? analysis_tiles(cnt) : tiles, s);
      cur = a.out[m - 1];
    }
    return ART_OK;
  });
  return rc ? rc : launched("art_trace_chain launch");
}

int art_trace_chain(const ArtElementDesc* elems, int32_t n_elems, const ArtBundleView* in, const ArtBundleView* outs,
                    int64_t n, void* stream) {
  return trace_chain_impl(elems, n_elems, in, outs, nullptr, n, stream);
}

int64_t art_chain_readout_scratch_doubles(int64_t n) {
  if (n < 0) n = 0;
  if (n > kMaxRaysPerLaunchHw) n = kMaxRaysPerLaunchHw;
  // one 24-slot partial per WORKGROUP of the fused launch (its grid may be rounded up by the tile mapping) + the chunk
  // totals of the two-stage fold behind them
  return (((n + kBlock - 1) / kBlock + 1024) + kFoldChunks) * kReadoutSlots;
}

int art_trace_chain_readout(const ArtElementDesc* elems, int32_t n_elems, const ArtBundleView* in,
                            const ArtBundleView* outs, const ArtChainReadout* readout, int64_t n, void* stream) {
  if (!readout) return fail(ART_ERR_BAD_ARG, "read-out descriptor is NULL");
  return trace_chain_impl(elems, n_elems, in, outs, readout, n, stream);
}

int64_t art_scene_bytes(int32_t n_chains, int32_t n_elems) {
  if (n_chains <= 0 || n_elems <= 0) return 0;
  return art::scene_bytes(n_chains, n_elems);
}

int art_scene_pack(const ArtElementDesc* elems, int32_t n_chains, int32_t n_elems, const ArtBundleView* ins,
                   const ArtBundleView* outs, const ArtChainReadout* readouts, void* image) {
  const char* msg = "";
  const int rc = art::scene_pack(elems, n_chains, n_elems, ins, outs, readouts, image, &msg);
  if (rc < 0) return fail(rc, msg);
  return rc;
}

int art_trace_scene(const void* image_dev, const void* image_host, int64_t n, void* stream) {
  if (!image_dev || !image_host) return fail(ART_ERR_BAD_ARG, "scene image is NULL");
  // Counts and flags are read from the header art_scene_pack wrote, not taken from the caller: a read-out bit without
  // read-out descriptors in the table would make the tail dereference NULL on the device, a wrong defect bit select the
  // wrong kernel body.
  art::SceneHeader h;
  memcpy(&h, image_host, sizeof(h));
  if (h.magic != art::kSceneMagic) return fail(ART_ERR_BAD_ARG, "host image was not written by art_scene_pack");
  const int32_t n_chains = h.n_chains, n_elems = h.n_elems, flags = h.flags;
  if (n_chains <= 0 || n_chains > 65535 || n_elems <= 0 || h.n_segments != art::scene_segments(n_elems) ||
      (flags & ~(art::kFlagDefects | art::kFlagReadout | art::kFlagMask | art::kFlagSharedIn | art::kFlagSums)))
    return fail(ART_ERR_BAD_ARG, "scene header is corrupt");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
#ifdef ART_ZERN_LDS
  if (flags & 1) return fail(ART_ERR_UNSUPPORTED, "ART_ZERN_LDS build: scenes with defects go through art_trace_chain");
#endif
  if ((flags & art::kFlagReadout) && n > max_rays_per_launch())
    return fail(ART_ERR_UNSUPPORTED, "fused read-out: more rays than one launch covers");
  hipStream_t s = (hipStream_t)stream;
  const ChainArgs* tab = art::scene_table(image_dev);
  const int S = art::scene_segments(n_elems);
  const bool sums = (flags & art::kFlagSums) != 0, tails = sums || (flags & art::kFlagReadout);
  if (n == 0) {
    if (tails) launch_fold(sums, tab + (int64_t)(S - 1) * n_chains, n_chains, nullptr, nullptr, 0, s);
    return ART_OK;
  }
  // one-element scenes with defects whose chains all carry the same simple optic: the body compiled for that kind
  int kind1 = ART_KIND_DYN;
  if ((flags & 1) && n_elems == 1) {
    const ChainArgs* ht = art::scene_table(image_host);
    kind1 = ht[0].e[0].kind;
    for (int c = 1; c < n_chains; ++c) kind1 = (ht[c].e[0].kind == kind1) ? kind1 : ART_KIND_DYN;
  }
  const BodyChoice c = choose_body((flags & 1) != 0, (flags & art::kFlagMask) != 0 ||
                                   ((flags & art::kFlagSharedIn) != 0 && n_chains > 1 && S == 1), kind1);
  const art::RowSummary* rowsum = row_summaries_on() ? art::scene_row_summaries(h) : nullptr;
  per_launch(n, [&](const int64_t off, const int64_t cnt) {
    const int xm = xcd_map();
    const int tiles = grid_stream_mapped(c.body == Body::kTwoRay ? (cnt + 1) / 2 : cnt, xm);
    for (int sg = 0; sg < S; ++sg) {
      const ChainArgs* seg = tab + (int64_t)sg * n_chains;
      // chains that share their input (first segment only: later segments read their own hand-over bundles) are
      // interleaved tile by tile (see k_trace_scene); ART_SCENE_ORDER=tile|chain overrides (A/B)
      // bit 0: interleaved grid; bit 1: the shared input is loaded with the default cache policy (scene_keep)
      int tr = scene_order((flags & art::kFlagSharedIn) != 0 && sg == 0 && n_chains > 1);
      const int tiles8 = (tiles + 7) / 8 * 8;       // (the padding workgroups leave at once: scene_wg)
      // (a grid dimension holds fewer than 2^32 work-items: 2^24 workgroups of 256)
      if (tr == 4 && (int64_t)tiles8 * n_chains >= ((int64_t)1 << 24)) tr = 1;
      if (tr == 1 && tiles > 65535) tr = 0;
      if (tr && scene_keep(cnt, (tr & 4) != 0)) tr |= 2;
      if (tr & 4) tr |= n_chains << 8;
      const dim3 g = (tr & 4) ? dim3((unsigned)(tiles8 * n_chains)) : ((tr & 1) ? dim3(n_chains, tiles) : dim3(tiles, n_chains));
      const int xarg = (tr & 4) ? tiles : xm;      // (XCD-grouped: the true tile count travels in the mapping's parameter)
      // the summaries describe the scene's inputs: the first segment's (later ones read their own hand-over bundles)
      launch_scene_body(c, g, seg, off, cnt, xarg, tr, sg == 0 ? rowsum : nullptr, s);
      if (tails && sg == S - 1) launch_fold(sums, seg, n_chains, nullptr, nullptr, sums ? analysis_tiles(cnt) : tiles, s);
    }
    return ART_OK;
  });
  return launched("art_trace_scene launch");
}

int64_t art_row_summary_bytes(void) { return (int64_t)sizeof(art::RowSummary); }

int art_bundle_row_summary(const ArtBundleView* in, const double* w, int64_t n, void* summary_dev, void* stream) {
  if (!summary_dev) return fail(ART_ERR_BAD_ARG, "row summary buffer is NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  ArtBundleView v;
  memset(&v, 0, sizeof(v));
  if (in) v = *in;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(summary_dev, 0, sizeof(art::RowSummary), s);
  if (e != hipSuccess) return fail_hip(e, "art_bundle_row_summary memset");
  hipLaunchKernelGGL(k_row_summary, dim3(grid_for(n)), dim3(kBlock), 0, s, v, w, n, (art::RowSummary*)summary_dev);
  return launched("art_bundle_row_summary launch");
}

int art_scene_set_row_summaries(void* image_host, const void* summaries_dev) {
  if (!image_host) return fail(ART_ERR_BAD_ARG, "scene image is NULL");
  art::SceneHeader h;
  memcpy(&h, image_host, sizeof(h));
  if (h.magic != art::kSceneMagic) return fail(ART_ERR_BAD_ARG, "host image was not written by art_scene_pack");
  art::scene_set_row_summaries(h, (const art::RowSummary*)summaries_dev);
  memcpy(image_host, &h, sizeof(h));
  return ART_OK;
}

int art_pack_rays(const double* points, const double* vectors, const double* path0, int64_t n, const ArtBundleView* out,
                  void* stream) {
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n == 0) return ART_OK;
  if (!points || !vectors || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "NULL argument");
  hipLaunchKernelGGL(k_pack_rays, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, points, vectors, path0, n,
                     *out);
  return launched("art_pack_rays launch");
}

int art_transform_bundle(const double M[9], const double T[3], int32_t rotate_points, const ArtBundleView* in,
                         const ArtBundleView* out, int64_t n, void* stream) {
  if (!M || !T) return fail(ART_ERR_BAD_ARG, "NULL matrix or translation");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n == 0) return ART_OK;
  if (!view_ok(in) || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  ArtDetectorDesc mt;
  memset(&mt, 0, sizeof(mt));
  memcpy(mt.rot, M, 9 * sizeof(double));
  memcpy(mt.centre, T, 3 * sizeof(double));
  hipLaunchKernelGGL(k_transform, dim3(grid_stream(n)), dim3(kBlock), 0, (hipStream_t)stream, mt, (int)rotate_points, *in,
                     *out, n);
  return launched("art_transform_bundle launch");
}

int art_detector(const ArtDetectorDesc* d, const ArtBundleView* b, int64_t n, double* p3x, double* p3y, double* p3z,
                 double* X, double* Y, double* opl, void* stream) {
  if (!d) return fail(ART_ERR_BAD_ARG, "detector descriptor is NULL");
  if (n == 0) return ART_OK;
  if (!view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  if ((p3x || p3y || p3z) && !(p3x && p3y && p3z)) return fail(ART_ERR_BAD_ARG, "p3x/p3y/p3z must be all set or all NULL");
  if ((X || Y) && !(X && Y)) return fail(ART_ERR_BAD_ARG, "X/Y must be both set or both NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n == 0) return ART_OK;
  hipLaunchKernelGGL(k_detector, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, *d, *b, n, p3x, p3y, p3z, X,
                     Y, opl);
  return launched("art_detector launch");
}

int art_detector_readout(const ArtDetectorDesc* d, const ArtBundleView* b, const double* w, int64_t n, double cx,
                         double cy, double co, double* p3x, double* p3y, double* p3z, double* X, double* Y,
                         double* opl, double* scratch, double* out24, void* stream) {
  if (!d || !scratch || !out24) return fail(ART_ERR_BAD_ARG, "descriptor/scratch/out24 must not be NULL");
  if ((p3x || p3y || p3z) && !(p3x && p3y && p3z)) return fail(ART_ERR_BAD_ARG, "p3x/p3y/p3z must be all set or all NULL");
  if ((X || Y) && !(X && Y)) return fail(ART_ERR_BAD_ARG, "X/Y must be both set or both NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    // an empty shard must not pollute a cross-rank fold: the fold of zero partials writes the reduction identities
    // (0 for sums, +inf / -inf for the min / max slots 2-5 and 12-13)
    return fold_partials<kReadoutSlots, stat_op>(scratch, 0, out24, s, "art_detector_readout launch");
  }
  if (!view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  // one launch per <= 2^28 rays (32-bit buffer offsets); every launch leaves one partial per workgroup, all of
  // them folded by k_fold_partials: scratch holds up to 8 launches x kReadoutBlocks workgroups x 24 doubles
  const int64_t chunk = max_rays_per_launch();
  const int64_t launches = (n + chunk - 1) / chunk;
  if (launches > 8) return fail(ART_ERR_UNSUPPORTED, "more than 2^31 rays in one read-out");
  int nb_total = 0;
  per_launch(n, [&](const int64_t off, const int64_t m) {
    const int64_t want = ((m + 1) / 2 + kBlock - 1) / kBlock;      // two slots per thread
    const int64_t cap = readout_block_cap(launches);
    const int nb = (int)(want < 1 ? 1 : (want > cap ? cap : want));
    const ArtBundleView v = view_at(*b, off);
    hipLaunchKernelGGL(k_detector_readout, dim3(nb), dim3(kBlock), 0, s, *d, v, w ? w + off : nullptr, m, cx, cy, co,
                       p3x ? p3x + off : nullptr, p3y ? p3y + off : nullptr, p3z ? p3z + off : nullptr,
                       X ? X + off : nullptr, Y ? Y + off : nullptr, opl ? opl + off : nullptr,
                       scratch + (int64_t)nb_total * kReadoutSlots);
    nb_total += nb;
    return ART_OK;
  });
  return fold_partials<kReadoutSlots, stat_op>(scratch, nb_total, out24, s, "art_detector_readout launch");
}

int art_detector_scan_moments(const ArtDetectorDesc* d, const ArtBundleView* b, const double* w, int64_t n, double co,
                              double span, double* scratch, double* out32, void* stream) {
  if (!d || !scratch || !out32) return fail(ART_ERR_BAD_ARG, "descriptor/scratch/out32 must not be NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    hipError_t e0 = hipMemsetAsync(out32, 0, kScanSlots * sizeof(double), s);
    if (e0 != hipSuccess) return fail_hip(e0, "hipMemsetAsync");
    return ART_OK;
  }
  if (!view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  const int nb = red_blocks(n);
  if (w) hipLaunchKernelGGL(k_scan_moments_partial<true>, dim3(nb), dim3(kBlock), 0, s, *d, *b, w, n, co, span, scratch);
  else hipLaunchKernelGGL(k_scan_moments_partial<false>, dim3(nb), dim3(kBlock), 0, s, *d, *b, w, n, co, span, scratch);
  return fold_partials<kScanSlots, sum_op>(scratch, nb, out32, s, "art_detector_scan_moments launch");
}

int art_histogram(const ArtHistogramDesc* h, const ArtBundleView* b, const double* w, int64_t n, int32_t accumulate,
                  int64_t* counts, int64_t* wsums, int64_t* totals4, void* stream) {
#pragma clang fp contract(off)
  if (!h) return fail(ART_ERR_BAD_ARG, "histogram descriptor is NULL");
  if (h->source != ART_HIST_DETECTOR && h->source != ART_HIST_FRAME) return fail(ART_ERR_BAD_ARG, "unknown histogram source");
  if (h->ndim < 1 || h->ndim > 3) return fail(ART_ERR_BAD_ARG, "histogram ndim must be 1, 2 or 3");
  HistArg a;
  memset(&a, 0, sizeof(a));
  a.map = h->map;
  a.delay_centre = h->delay_centre;
  a.source = h->source;
  a.wshift = h->wshift;
  int64_t nbins = 1;
  for (int k = 0; k < 3; ++k) {
    a.bins[k] = 1;
    if (k >= h->ndim) continue;
    const int ax = h->axis[k];
    if (ax < 0 || ax > 3 || (ax == 2 && h->source == ART_HIST_DETECTOR)) return fail(ART_ERR_BAD_ARG, "unknown histogram axis");
    if (h->bins[k] < 1) return fail(ART_ERR_BAD_ARG, "histogram bins must be >= 1");
    nbins *= h->bins[k];
    if (nbins > ART_HIST_MAX_BINS) return fail(ART_ERR_UNSUPPORTED, "more than 2^24 histogram bins");
    const double lo = h->lo[k], hi = h->hi[k], delta = hi - lo, step = delta / (double)h->bins[k];   // numpy.linspace
    if (!(isfinite(lo) && isfinite(hi) && lo < hi && isfinite(delta) && step > 0.0))
      return fail(ART_ERR_BAD_ARG, "histogram range: lo < hi must be finite, with a finite non-zero bin width");
    if (ax == ART_HAXIS_DELAY && h->source == ART_HIST_FRAME)
      return fail(ART_ERR_BAD_ARG, "a DELAY axis needs the DETECTOR source");
    a.axis[k] = ax;
    a.bins[k] = h->bins[k];
    a.lo[k] = lo; a.hi[k] = hi; a.step[k] = step;
    a.inv[k] = (double)h->bins[k] / delta;
  }
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (!counts || !totals4) return fail(ART_ERR_BAD_ARG, "counts/totals4 must not be NULL");
  if (w && !wsums) return fail(ART_ERR_BAD_ARG, "weights given but wsums is NULL");
  if (h->wshift < -1074 || h->wshift > 1074) return fail(ART_ERR_BAD_ARG, "wshift outside [-1074, 1074]");
  if (n > 0 && !view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  hipStream_t s = (hipStream_t)stream;
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)nbins * sizeof(int64_t), s);
    if (e == hipSuccess && wsums) e = hipMemsetAsync(wsums, 0, (size_t)nbins * sizeof(int64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(totals4, 0, 4 * sizeof(int64_t), s);
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync");
  }
  if (n == 0) return ART_OK;
  const bool lds = nbins <= kHistLdsBins;
  const size_t shmem = lds ? (size_t)nbins * (w ? 12 : 4) : 0;
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  auto* ws = reinterpret_cast<unsigned long long*>(wsums);
  auto* t = reinterpret_cast<unsigned long long*>(totals4);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    const int64_t want = ((m + 1) / 2 + kBlock - 1) / kBlock;      // two slots per thread
    const int nb = (int)(want < 1 ? 1 : (want > kHistBlocks ? kHistBlocks : want));
    const ArtBundleView v = view_at(*b, off);
    const double* wo = w ? w + off : nullptr;
    if (lds) hipLaunchKernelGGL(k_histogram<true>, dim3(nb), dim3(kBlock), shmem, s, a, h->ndim, (int)nbins, v, wo, m, c, ws, t);
    else hipLaunchKernelGGL(k_histogram<false>, dim3(nb), dim3(kBlock), 0, s, a, h->ndim, (int)nbins, v, wo, m, c, ws, t);
    return ART_OK;
  });
  return launched("art_histogram launch");
}

// ------------------------------------------------------------------------------------------- quantiles
// The scratch of art_quantiles, in doubles: what the whole call keeps, then what one block of pb planes needs.
namespace {
struct QuantileLayout {
  int64_t state, counts, centres, partials;          // offsets of the call's areas
  int64_t hist, rank, keys;                          // offsets of the block's areas
  int64_t total;
  int pb;                                            // planes per block
};

int quantile_check(const ArtQuantileDesc* d, int64_t n) {
  if (!d) return fail(ART_ERR_BAD_ARG, "quantile descriptor is NULL");
  if (d->key < ART_QKEY_GIVEN || d->key > ART_QKEY_DELAY) return fail(ART_ERR_BAD_ARG, "unknown quantile key source");
  if (d->planes < 1 || d->planes > ART_FOCAL_MAX_PLANES) return fail(ART_ERR_BAD_ARG, "planes must be in 1..ART_FOCAL_MAX_PLANES");
  if (d->n_fractions < 1 || d->n_fractions > ART_QUANTILE_MAX_FRACTIONS)
    return fail(ART_ERR_BAD_ARG, "n_fractions must be in 1..ART_QUANTILE_MAX_FRACTIONS");
  if (d->n_thresholds < 0 || d->n_thresholds > ART_QUANTILE_MAX_THRESHOLDS)
    return fail(ART_ERR_BAD_ARG, "n_thresholds must be in 0..ART_QUANTILE_MAX_THRESHOLDS");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "art_quantiles: more than 2^28 slots");
  if (d->scratch_bound < 0) return fail(ART_ERR_BAD_ARG, "negative scratch bound");
  if (d->wshift < -1074 || d->wshift > 1074) return fail(ART_ERR_BAD_ARG, "wshift outside [-1074, 1074]");
  return ART_OK;
}

QuantileLayout quantile_layout(const ArtQuantileDesc* d, int64_t n) {
  QuantileLayout L;
  const int64_t P = d->planes, K = d->n_fractions, R = d->n_thresholds;
  const bool metric = d->key != ART_QKEY_GIVEN;
  int64_t o = 0;
  L.state = o; o += P * K * (int64_t)(sizeof(artq::SelState) / 8);
  L.counts = o; o += 2 * P;
  L.centres = o; o += 4 * P;
  L.partials = o; o += metric ? P * artq::kMomBlocks * artq::kMomSlots : 0;
  const int64_t per_plane = K * artq::kBins + 2 * (R + 1) + (metric ? n : 0);
  const int64_t bound = d->scratch_bound > 0 ? d->scratch_bound : ART_QUANTILE_SCRATCH_DEFAULT;
  int64_t pb = (bound - o) / per_plane;
  pb = pb < 1 ? 1 : (pb > P ? P : pb);
  L.pb = (int)pb;
  L.hist = o; o += pb * K * artq::kBins;
  L.rank = o; o += pb * 2 * (R + 1);
  L.keys = o; o += metric ? pb * n : 0;
  L.total = o;
  return L;
}
}  // namespace

int64_t art_quantile_scratch_doubles(const ArtQuantileDesc* d, int64_t n) {
  const int rc = quantile_check(d, n);
  if (rc) return rc;
  return quantile_layout(d, n).total;
}

int art_quantiles(const ArtQuantileDesc* d, const ArtBundleView* b, const double* w, int64_t n, double* scratch,
                  void* stream) {
#pragma clang fp contract(off)
  const int rc = quantile_check(d, n);
  if (rc) return rc;
  const int P = d->planes, K = d->n_fractions, R = d->n_thresholds;
  const bool metric = d->key != ART_QKEY_GIVEN;
  if (!scratch || !d->totals) return fail(ART_ERR_BAD_ARG, "art_quantiles: scratch and totals must not be NULL");
  if (!d->values || !d->below || !d->upto) return fail(ART_ERR_BAD_ARG, "art_quantiles: values/below/upto missing");
  for (int k = 0; k < K; ++k)
    if (!(d->fraction[k] >= 0.0 && d->fraction[k] <= 1.0)) return fail(ART_ERR_BAD_ARG, "art_quantiles: a fraction is outside [0, 1]");
  if (R > 0) {
    if (!d->rank_sums || !d->rank_counts || !d->thresholds_dev || !d->thresholds_host)
      return fail(ART_ERR_BAD_ARG, "art_quantiles: thresholds or rank outputs missing");
    for (int p = 0; p < P; ++p)
      for (int r = 0; r < R; ++r) {
        const double t = d->thresholds_host[(int64_t)p * R + r];
        if (t != t || (r > 0 && t < d->thresholds_host[(int64_t)p * R + r - 1]))
          return fail(ART_ERR_BAD_ARG, "art_quantiles: thresholds must be sorted per plane and not NaN");
      }
  }
  artq::PlaneArg pa;
  artq::CentreArg ca;
  memset(&pa, 0, sizeof(pa));
  memset(&ca, 0, sizeof(ca));
  if (metric) {
    const double nn = d->det.normal[0] * d->det.normal[0] + d->det.normal[1] * d->det.normal[1] + d->det.normal[2] * d->det.normal[2];
    if (!(fabs(nn - 1.0) <= 1e-9)) return fail(ART_ERR_BAD_ARG, "art_quantiles: the detector normal must be a unit vector");
    pa.det = d->det;
    for (int p = 0; p < P; ++p) {
      if (!isfinite(d->shift[p])) return fail(ART_ERR_BAD_ARG, "art_quantiles: a shift is not finite");
      for (int k = 0; k < 3; ++k) {
        pa.pc[p][k] = d->det.centre[k] + d->shift[p] * d->det.normal[k];       // (two roundings: the moved detector's centre)
        if (d->centre_given && !isfinite(d->centre[p][k])) return fail(ART_ERR_BAD_ARG, "art_quantiles: a centre is not finite");
        ca.c[p][k] = d->centre[p][k];
      }
    }
    if (n > 0 && !view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  } else if (n > 0 && !d->keys) {
    return fail(ART_ERR_BAD_ARG, "art_quantiles: keys is NULL");
  }
  hipStream_t s = (hipStream_t)stream;
  const QuantileLayout L = quantile_layout(d, n);
  auto* state = reinterpret_cast<artq::SelState*>(scratch + L.state);
  auto* counts = reinterpret_cast<artq::u64*>(scratch + L.counts);
  double* centres = scratch + L.centres;
  auto* hist = reinterpret_cast<artq::u64*>(scratch + L.hist);
  auto* rank = reinterpret_cast<artq::u64*>(scratch + L.rank);
  double* staged = scratch + L.keys;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)2 * P * sizeof(double), s);
  if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync");
  hipLaunchKernelGGL(artq::k_select_init, dim3((P * K + artq::kBlock - 1) / artq::kBlock), dim3(artq::kBlock), 0, s, state, P * K);
  const int64_t tiles = (n + (int64_t)artq::kBlock * artq::kUnroll - 1) / ((int64_t)artq::kBlock * artq::kUnroll);
  const int gx = (int)(tiles < 1 ? 1 : (tiles > artq::kSelBlocks ? artq::kSelBlocks : tiles));
  if (metric) {
    const bool sums = !d->centre_given || d->key == ART_QKEY_DELAY;
    const ArtBundleView bv = n > 0 ? *b : ArtBundleView{};
    if (sums) {
      const int64_t want = (n + artq::kBlock - 1) / artq::kBlock;
      const int nb = (int)(want < 1 ? 1 : (want > artq::kMomBlocks ? artq::kMomBlocks : want));
      const dim3 grid(nb, (P + artq::kMomPlanes - 1) / artq::kMomPlanes);
      double* partials = scratch + L.partials;
      hipLaunchKernelGGL(artq::k_metric_moments, grid, dim3(artq::kBlock), 0, s, pa, P, 0, bv, w, n, centres, partials);
      hipLaunchKernelGGL(artq::k_metric_centres, dim3(P), dim3(64), 0, s, partials, nb, 0, (int)d->centre_given, ca, centres);
      if (d->key == ART_QKEY_DELAY && !d->centre_given) {
        hipLaunchKernelGGL(artq::k_metric_moments, grid, dim3(artq::kBlock), 0, s, pa, P, 1, bv, w, n, centres, partials);
        hipLaunchKernelGGL(artq::k_metric_centres, dim3(P), dim3(64), 0, s, partials, nb, 1, 0, ca, centres);
      }
    } else {
      hipLaunchKernelGGL(artq::k_metric_centres_given, dim3(1), dim3(64), 0, s, ca, P, centres);
    }
    if (d->centres_out) {
      e = hipMemcpyAsync(d->centres_out, centres, (size_t)4 * P * sizeof(double), hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) return fail_hip(e, "hipMemcpyAsync");
    }
  }
  const int root = d->key == ART_QKEY_RADIUS;
  artq::PickArg fr;
  for (int k = 0; k < ART_QUANTILE_MAX_FRACTIONS; ++k) fr.fraction[k] = k < K ? d->fraction[k] : 0.0;
  for (int p0 = 0; p0 < P; p0 += L.pb) {
    const int pb = (P - p0) < L.pb ? (P - p0) : L.pb;
    const size_t clear = (size_t)((int64_t)L.pb * K * artq::kBins + (int64_t)L.pb * 2 * (R + 1)) * sizeof(double);
    e = hipMemsetAsync(hist, 0, clear, s);                               // (hist and rank are adjacent)
    if (e != hipSuccess) return fail_hip(e, "hipMemsetAsync");
    const double* keys = metric ? staged : d->keys + (int64_t)p0 * n;
    const uint8_t* alive = metric ? (n > 0 ? b->alive : nullptr) : d->alive;
    if (metric && n > 0) {
      const int64_t want = (n + artq::kBlock - 1) / artq::kBlock;
      const int nb = (int)(want > 4096 ? 4096 : want);
      hipLaunchKernelGGL(artq::k_stage_keys, dim3(nb), dim3(artq::kBlock), 0, s, pa, (int)d->key, p0, pb, *b, n, centres, staged);
    }
    const dim3 grid(gx, pb);
    for (int pass = 0; pass < artq::kPasses; ++pass) {
      for (int k0 = 0; k0 < K; k0 += artq::kGroups) {
        const int G = (K - k0) < artq::kGroups ? (K - k0) : artq::kGroups;
        const size_t lds = (size_t)G * artq::kBins * sizeof(artq::u64);
        if (pass == 0) {
          if (k0 == 0)
            hipLaunchKernelGGL(artq::k_select_hist<true>, grid, dim3(artq::kBlock), lds, s, keys, alive, w, n, (int)d->wshift, pass,
                               K, k0, state + (int64_t)p0 * K, hist, counts + 2 * p0);
        } else {
          hipLaunchKernelGGL(artq::k_select_hist<false>, grid, dim3(artq::kBlock), lds, s, keys, alive, w, n, (int)d->wshift, pass,
                             K, k0, state + (int64_t)p0 * K, hist, counts + 2 * p0);
        }
      }
      hipLaunchKernelGGL(artq::k_select_pick, dim3(pb), dim3(artq::kBlock), 0, s, state + (int64_t)p0 * K, hist, counts + 2 * p0, K,
                         pass, fr, root, d->values + (int64_t)p0 * K, reinterpret_cast<long long*>(d->below) + (int64_t)p0 * K,
                         reinterpret_cast<long long*>(d->upto) + (int64_t)p0 * K,
                         reinterpret_cast<long long*>(d->totals) + 3 * p0);
    }
    if (R > 0) {
      hipLaunchKernelGGL(artq::k_rank_bins, grid, dim3(artq::kBlock), 0, s, keys, alive, w, n, (int)d->wshift, R, root,
                         d->thresholds_dev + (int64_t)p0 * R, rank);
      hipLaunchKernelGGL(artq::k_rank_finish, dim3(pb), dim3(64), 0, s, rank, R,
                         reinterpret_cast<long long*>(d->rank_sums) + (int64_t)p0 * R,
                         reinterpret_cast<long long*>(d->rank_counts) + (int64_t)p0 * R);
    }
  }
  return launched("art_quantiles launch");
}

// the ranges of a focal grid and its planes
static bool focal_shape_ok(int32_t nx, int32_t ny, int32_t planes) {
  return nx >= 1 && ny >= 1 && nx <= ART_FOCAL_MAX_PIXELS && ny <= ART_FOCAL_MAX_PIXELS && planes >= 1 &&
         planes <= ART_FOCAL_MAX_PLANES;
}

int64_t art_focal_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int64_t n) {
  if (!focal_shape_ok(nx, ny, planes) || n < 0)
    return fail(ART_ERR_BAD_ARG, "focal scratch: nx, ny in [1, 2048], planes in [1, 64], n >= 0");
  const int S = focal_slices(nx, ny, planes, n);
  return (int64_t)kFocalRows * focal_stride(n) + (S > 1 ? (int64_t)S * planes * ny * nx * 2 : 0);
}

// the checks of an ArtFocalDesc that do not depend on the call's other arguments
static int focal_desc_check(const ArtFocalDesc* f) {
  if (!focal_shape_ok(f->nx, f->ny, 1)) return fail(ART_ERR_BAD_ARG, "focal grid: nx and ny must be in [1, 2048]");
  if (!focal_shape_ok(f->nx, f->ny, f->planes)) return fail(ART_ERR_BAD_ARG, "focal planes must be in [1, 64]");
  if (!(isfinite(f->k) && f->k > 0.0)) return fail(ART_ERR_BAD_ARG, "focal k must be finite and > 0");
  if (!(isfinite(f->dx) && isfinite(f->dy))) return fail(ART_ERR_BAD_ARG, "focal pixel pitch must be finite");
  for (int q = 0; q < f->planes; ++q)
    if (!isfinite(f->shift[q])) return fail(ART_ERR_BAD_ARG, "focal plane shifts must be finite");
  return ART_OK;
}

// the checks of the rays and buffers, and the zeros of an empty call (*done = true then)
static int focal_call_check(const ArtBundleView* b, int64_t n, const double* scratch, double* field, int64_t pixels,
                            hipStream_t s, bool* done) {
  *done = true;
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n > 0 && (!field || !scratch)) return fail(ART_ERR_BAD_ARG, "focal field/scratch must not be NULL");
  if (n > 0 && !view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  if (n == 0) {
    if (!field) return ART_OK;
    const hipError_t e = hipMemsetAsync(field, 0, (size_t)pixels * 2 * sizeof(double), s);
    return e == hipSuccess ? ART_OK : fail_hip(e, "hipMemsetAsync");
  }
  *done = false;
  return ART_OK;
}

// the kernels' argument for n > 0 rays in S slices
static FocalArg focal_arg(const ArtFocalDesc* f, int64_t n, int S) {
  FocalArg a;
  memset(&a, 0, sizeof(a));
  a.k = f->k; a.L_ref = f->L_ref; a.x0 = f->x0; a.dx = f->dx; a.y0 = f->y0; a.dy = f->dy;
  for (int c = 0; c < 3; ++c) {
    a.C[c] = f->det.centre[c]; a.nrm[c] = f->det.normal[c];
    a.e1[c] = f->det.rot[c]; a.e2[c] = f->det.rot[3 + c];
  }
  a.stride = focal_stride(n);
  a.per_slice = (n + S - 1) / S;
  a.n = n;
  a.nx = f->nx; a.ny = f->ny; a.planes = f->planes;
  a.tiles_x = (f->nx + kFocalTile - 1) / kFocalTile;
  for (int q = 0; q < f->planes; ++q) a.shift[q] = f->shift[q];
  return a;
}

// field[p] = the sum of the S slices' partials at part, for p < pixels
static void focal_fold_launch(const double* part, int S, int64_t pixels, double* field, hipStream_t s) {
  const int64_t want = (pixels + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_focal_fold, dim3((int)(want > kMaxBlocks ? kMaxBlocks : want)), dim3(kBlock), 0, s,
                     (const double2*)part, S, pixels, reinterpret_cast<double2*>(field));
}

int art_focal_field(const ArtFocalDesc* f, const ArtBundleView* b, const double* w, int64_t n, double* scratch,
                    double* field, void* stream) {
  if (!f) return fail(ART_ERR_BAD_ARG, "focal descriptor is NULL");
  if (const int e = focal_desc_check(f)) return e;
  hipStream_t s = (hipStream_t)stream;
  const int64_t pixels = (int64_t)f->planes * f->ny * f->nx;
  bool done;
  if (const int e = focal_call_check(b, n, scratch, field, pixels, s, &done); e || done) return e;
  const int S = focal_slices(f->nx, f->ny, f->planes, n);
  const FocalArg a = focal_arg(f, n, S);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    hipLaunchKernelGGL(k_focal_prep, dim3(grid_for(m)), dim3(kBlock), 0, s, a, view_at(*b, off), w ? w + off : nullptr,
                       m, scratch + off);
    return ART_OK;
  });
  double* part = S > 1 ? scratch + (int64_t)kFocalRows * a.stride : field;
  hipLaunchKernelGGL(k_focal_field, dim3(focal_tiles(f->nx, f->ny), f->planes, S), dim3(kBlock), 0, s, a,
                     (const double*)scratch, part);
  if (S > 1) focal_fold_launch(part, S, pixels, field, s);
  return launched("art_focal_field launch");
}

// the launch shape of art_focal_image, from the sizes alone (seg stays on the device): S slices of `per` groups, or,
// when all the groups' workgroups fill less than half of kFocalWantBlocks, `split` pieces of every group (S = 1 then)
struct FocalImagePlan { int S, per, split; };
static FocalImagePlan focal_image_plan(int nx, int ny, int planes, int groups, int64_t n) {
  FocalImagePlan p;
  int s = focal_slices(nx, ny, planes, n);
  if (s > groups) s = groups;
  p.per = (groups + s - 1) / s;
  p.S = (groups + p.per - 1) / p.per;            // no empty slice
  const int64_t wgs = (int64_t)focal_tiles(nx, ny) * planes * groups;
  int64_t k = kFocalWantBlocks / wgs;
  const int64_t by_rays = (n / groups + 4 * kFocalChunk - 1) / (4 * kFocalChunk);   // 4 chunks of a mean group per piece
  if (k > by_rays) k = by_rays;
  if (k > kFocalMaxSlices) k = kFocalMaxSlices;
  p.split = k < 2 ? 1 : (int)k;
  if (p.split > 1) { p.S = 1; p.per = groups; }
  return p;
}

int64_t art_focal_image_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int32_t groups, int64_t n) {
  if (!focal_shape_ok(nx, ny, planes) || groups < 1 || groups > ART_FOCAL_MAX_GROUPS || n < 0)
    return fail(ART_ERR_BAD_ARG, "focal image scratch: nx, ny in [1, 2048], planes in [1, 64], groups in [1, 2^20], n >= 0");
  const FocalImagePlan p = focal_image_plan(nx, ny, planes, groups, n);
  const int64_t pixels = (int64_t)planes * ny * nx;
  const int64_t part = p.split > 1 ? (int64_t)groups * p.split * pixels * 2 : (p.S > 1 ? (int64_t)p.S * pixels : 0);
  return (int64_t)kFocalRows * focal_stride(n) + part;
}

int art_focal_image(const ArtFocalImageDesc* d, const ArtBundleView* b, const double* w, int64_t n, double* scratch,
                    double* image, void* stream) {
  if (!d) return fail(ART_ERR_BAD_ARG, "focal image descriptor is NULL");
  const ArtFocalDesc* f = &d->f;
  if (const int e = focal_desc_check(f)) return e;
  if (d->groups < 1 || d->groups > ART_FOCAL_MAX_GROUPS) return fail(ART_ERR_BAD_ARG, "focal image: groups must be in [1, 2^20]");
  if (!d->seg) return fail(ART_ERR_BAD_ARG, "focal image: seg must not be NULL");
  if (!image) return fail(ART_ERR_BAD_ARG, "focal image: image must not be NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n > 0 && !scratch) return fail(ART_ERR_BAD_ARG, "focal image: scratch must not be NULL");
  if (n > 0 && !view_ok(b)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  hipStream_t s = (hipStream_t)stream;
  const int64_t pixels = (int64_t)f->ny * f->nx, total = pixels * f->planes;
  if (n == 0) {
    const hipError_t e = hipMemsetAsync(image, 0, (size_t)total * sizeof(double), s);
    return e == hipSuccess ? ART_OK : fail_hip(e, "hipMemsetAsync");
  }
  const FocalImagePlan p = focal_image_plan(f->nx, f->ny, f->planes, d->groups, n);
  const FocalArg a = focal_arg(f, n, 1);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    hipLaunchKernelGGL(k_focal_prep, dim3(grid_for(m)), dim3(kBlock), 0, s, a, view_at(*b, off), w ? w + off : nullptr,
                       m, scratch + off);
    return ART_OK;
  });
  const bool direct = p.S == 1 && p.split == 1;
  double* part = direct ? image : scratch + (int64_t)kFocalRows * a.stride;
  const int jobs = p.split > 1 ? f->planes * d->groups * p.split : f->planes * p.S;   // <= 2048 or <= 64 * 64
  hipLaunchKernelGGL(k_focal_image, dim3(focal_tiles(f->nx, f->ny), jobs), dim3(kBlock), 0, s, a, (const double*)scratch,
                     d->seg, (int)d->groups, p.per, p.S, p.split, part);
  if (!direct) {
    const int64_t want = (total + kBlock - 1) / kBlock;
    const dim3 grid((int)(want > kMaxBlocks ? kMaxBlocks : want));
    if (p.split > 1)
      hipLaunchKernelGGL(k_focal_image_fold_split, grid, dim3(kBlock), 0, s, (const double2*)part, (int)d->groups, p.split,
                         pixels, total, image);
    else
      hipLaunchKernelGGL(k_focal_image_fold, grid, dim3(kBlock), 0, s, (const double*)part, p.S, pixels, total, image);
  }
  return launched("art_focal_image launch");
}

// the checks an ArtFocalSpectrumDesc adds to focal_desc_check
static int focal_spectrum_check(const ArtFocalSpectrumDesc* d) {
  if (d->nk < 1 || d->nk > ART_FOCAL_MAX_WAVENUMBERS) return fail(ART_ERR_BAD_ARG, "focal spectrum: nk must be in [1, 1024]");
  if (!isfinite(d->dk)) return fail(ART_ERR_BAD_ARG, "focal spectrum: dk must be finite");
  const double k_last = focal_kj(d->f.k, d->nk - 1, d->dk);   // k_j is linear in j: its ends bound it
  if (!(isfinite(k_last) && k_last > 0.0)) return fail(ART_ERR_BAD_ARG, "focal spectrum: every k_j must be finite and > 0");
  if ((int64_t)d->f.planes * d->nk > 65535) return fail(ART_ERR_BAD_ARG, "focal spectrum: planes * nk must be <= 65535");
  return ART_OK;
}

int64_t art_focal_spectrum_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int32_t nk, int64_t n) {
  if (!focal_shape_ok(nx, ny, planes) || nk < 1 || nk > ART_FOCAL_MAX_WAVENUMBERS || n < 0)
    return fail(ART_ERR_BAD_ARG, "focal spectrum scratch: nx, ny in [1, 2048], planes in [1, 64], nk in [1, 1024], n >= 0");
  const int S = focal_slices(nx, ny, planes * nk, n);
  return (int64_t)kFocalSpecRows * focal_stride(n) + (S > 1 ? (int64_t)S * planes * nk * ny * nx * 2 : 0);
}

int art_focal_spectrum(const ArtFocalSpectrumDesc* d, const ArtBundleView* b, const double* w, int64_t n,
                       double* scratch, double* field, void* stream) {
  if (!d) return fail(ART_ERR_BAD_ARG, "focal spectrum descriptor is NULL");
  const ArtFocalDesc* f = &d->f;
  if (const int e = focal_desc_check(f)) return e;
  if (const int e = focal_spectrum_check(d)) return e;
  hipStream_t s = (hipStream_t)stream;
  const int planes = f->planes * d->nk;      // (plane, wavenumber) pairs
  const int64_t pixels = (int64_t)planes * f->ny * f->nx;
  bool done;
  if (const int e = focal_call_check(b, n, scratch, field, pixels, s, &done); e || done) return e;
  // the slices of art_focal_field at nk = 1: the same partial sums, so the same bytes
  const int S = focal_slices(f->nx, f->ny, planes, n);
  const FocalArg a = focal_arg(f, n, S);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    hipLaunchKernelGGL(k_focal_spectrum_prep, dim3(grid_for(m)), dim3(kBlock), 0, s, a, view_at(*b, off),
                       w ? w + off : nullptr, m, scratch + off);
    return ART_OK;
  });
  double* part = S > 1 ? scratch + (int64_t)kFocalSpecRows * a.stride : field;
  hipLaunchKernelGGL(k_focal_spectrum_field, dim3(focal_tiles(f->nx, f->ny), planes, S), dim3(kBlock), 0, s, a, d->dk,
                     (int)d->nk, (const double*)scratch, part);
  if (S > 1) focal_fold_launch(part, S, pixels, field, s);
  return launched("art_focal_spectrum launch");
}

int64_t art_focal_chromatic_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int32_t nk, int64_t n) {
  if (!focal_shape_ok(nx, ny, planes) || nk < 1 || nk > ART_FOCAL_MAX_WAVENUMBERS || n < 0)
    return fail(ART_ERR_BAD_ARG, "focal chromatic scratch: nx, ny in [1, 2048], planes in [1, 64], nk in [1, 1024], n >= 0");
  const int S = focal_slices(nx, ny, planes * nk, n);
  return (int64_t)kFocalChromRows * focal_stride(n) + (S > 1 ? (int64_t)S * planes * nk * ny * nx * 2 : 0);
}

// the checks of art_focal_chromatic's axis and of the host copy of its table of nk rows
static int focal_chromatic_table_check(const double* axis, const int nk, const double* table_host) {
  const double a2 = (axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2];
  if (!(isfinite(a2) && fabs(sqrt(a2) - 1.0) <= 1e-12)) return fail(ART_ERR_BAD_ARG, "focal chromatic: axis must be a unit vector");
  if (!table_host) return fail(ART_ERR_BAD_ARG, "focal chromatic: the host copy of the table must not be NULL");
  for (int j = 0; j < nk; ++j) {
    const double k = table_host[4 * j], c = table_host[4 * j + 1], z = table_host[4 * j + 2];
    if (!(isfinite(k) && k > 0.0)) return fail(ART_ERR_BAD_ARG, "focal chromatic: every k_j must be finite and > 0");
    if (!(isfinite(c) && c >= 0.0)) return fail(ART_ERR_BAD_ARG, "focal chromatic: every c_j must be finite and >= 0");
    if (!isfinite(z)) return fail(ART_ERR_BAD_ARG, "focal chromatic: every z_j must be finite");
  }
  return ART_OK;
}

// the checks an ArtFocalChromaticDesc and the host copy of its table add to focal_desc_check
static int focal_chromatic_check(const ArtFocalChromaticDesc* d, const double* table_host) {
  if (d->nk < 1 || d->nk > ART_FOCAL_MAX_WAVENUMBERS) return fail(ART_ERR_BAD_ARG, "focal chromatic: nk must be in [1, 1024]");
  if ((int64_t)d->f.planes * d->nk > 65535) return fail(ART_ERR_BAD_ARG, "focal chromatic: planes * nk must be <= 65535");
  return focal_chromatic_table_check(d->axis, d->nk, table_host);
}

int art_focal_chromatic(const ArtFocalChromaticDesc* d, const ArtBundleView* b, const ArtBundleView* src, const double* w,
                        int64_t n, const double* table_dev, const double* table_host, double* scratch, double* field,
                        void* stream) {
  if (!d) return fail(ART_ERR_BAD_ARG, "focal chromatic descriptor is NULL");
  const ArtFocalDesc* f = &d->f;
  if (const int e = focal_desc_check(f)) return e;
  if (const int e = focal_chromatic_check(d, table_host)) return e;
  if (n > 0 && !table_dev) return fail(ART_ERR_BAD_ARG, "focal chromatic: the device table must not be NULL");
  if (n > 0 && !view_ok(src)) return fail(ART_ERR_BAD_ARG, "source bundle view has a NULL array");
  hipStream_t s = (hipStream_t)stream;
  const int planes = f->planes * d->nk;      // (plane, wavenumber) pairs
  const int64_t pixels = (int64_t)planes * f->ny * f->nx;
  bool done;
  if (const int e = focal_call_check(b, n, scratch, field, pixels, s, &done); e || done) return e;
  // the slices of art_focal_spectrum at the same nk: the same partial sums, so a neutral table gives its bytes
  const int S = focal_slices(f->nx, f->ny, planes, n);
  const FocalArg a = focal_arg(f, n, S);
  per_launch(n, [&](const int64_t off, const int64_t m) {
    hipLaunchKernelGGL(k_focal_chromatic_prep, dim3(grid_for(m)), dim3(kBlock), 0, s, a, view_at(*b, off),
                       view_at(*src, off), d->axis[0], d->axis[1], d->axis[2], w ? w + off : nullptr, m, scratch + off);
    return ART_OK;
  });
  double* part = S > 1 ? scratch + (int64_t)kFocalChromRows * a.stride : field;
  hipLaunchKernelGGL(k_focal_chromatic_field, dim3(focal_tiles(f->nx, f->ny), planes, S), dim3(kBlock), 0, s, a,
                     table_dev, (int)d->nk, (const double*)scratch, part);
  if (S > 1) focal_fold_launch(part, S, pixels, field, s);
  return launched("art_focal_chromatic launch");
}

// validates a job table; *nmax, *kmax: the largest slot count and column count
static int wf_check(const ArtWavefrontJob* jobs, int32_t n_jobs, int64_t* nmax, int* kmax) {
  if (!jobs) return fail(ART_ERR_BAD_ARG, "wavefront job table is NULL");
  if (n_jobs < 1 || n_jobs > 65535) return fail(ART_ERR_BAD_ARG, "n_jobs must be in 1..65535");
  *nmax = 0;
  *kmax = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtWavefrontJob& jb = jobs[j];
    if (jb.n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
    if (jb.n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays per bundle in one wavefront call");
    if (jb.order < 0 || jb.order > ART_WAVEFRONT_MAX_ORDER) return fail(ART_ERR_BAD_ARG, "wavefront order must be in [0, 10]");
    *nmax = jb.n > *nmax ? jb.n : *nmax;
    *kmax = wf_cols(jb.order) > *kmax ? wf_cols(jb.order) : *kmax;
  }
  return ART_OK;
}

int64_t art_wavefront_scratch_doubles(const ArtWavefrontJob* jobs_host, int32_t n_jobs) {
  int64_t nmax;
  int kmax;
  const int rc = wf_check(jobs_host, n_jobs, &nmax, &kmax);
  return rc ? rc : (int64_t)n_jobs * wf_per_job(nmax, kmax);
}

int art_wavefront(const ArtWavefrontJob* jobs_dev, const ArtWavefrontJob* jobs_host, int32_t n_jobs, double* scratch,
                  void* stream) {
  if (!jobs_dev || !scratch) return fail(ART_ERR_BAD_ARG, "NULL argument");
  int64_t nmax;
  int kmax;
  const int rc = wf_check(jobs_host, n_jobs, &nmax, &kmax);
  if (rc) return rc;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtWavefrontJob& jb = jobs_host[j];
    if (!jb.out) return fail(ART_ERR_BAD_ARG, "a wavefront job's output row is NULL");
    if (jb.n > 0 && !view_ok(&jb.b)) return fail(ART_ERR_BAD_ARG, "a job's bundle view has a NULL array");
    bool finite = isfinite(jb.L_ref);
    for (int c = 0; c < 3; ++c) finite = finite && isfinite(jb.ref[c]) && isfinite(jb.pupil[c]);
    if (!finite) return fail(ART_ERR_BAD_ARG, "a wavefront job's reference point, L_ref or pupil is not finite");
    if (jb.pupil[2] < 0.0) return fail(ART_ERR_BAD_ARG, "a wavefront job's pupil radius is negative");
  }
  hipStream_t s = (hipStream_t)stream;
  WfArg a;
  a.stride = wf_stride(nmax);
  a.per_job = wf_per_job(nmax, kmax);
  const int64_t pb = (nmax + kBlock - 1) / kBlock;
  a.prep_blocks = pb < 1 ? 1 : (pb > kWfPrepBlocks ? kWfPrepBlocks : (int)pb);
  a.job0 = 0;
  hipLaunchKernelGGL(k_wavefront_prep, dim3(a.prep_blocks, n_jobs), dim3(kBlock), 0, s, jobs_dev, a, scratch);
  for (int j0 = 0; j0 < n_jobs;) {        // one launch per run of consecutive jobs of one order
    const int order = jobs_host[j0].order;
    int j1 = j0, slices = 1;
    for (; j1 < n_jobs && jobs_host[j1].order == order; ++j1)
      slices = wf_slices(jobs_host[j1].n) > slices ? wf_slices(jobs_host[j1].n) : slices;
    a.job0 = j0;
    kWfGram[order](dim3(slices, j1 - j0), s, jobs_dev, a, scratch);
    j0 = j1;
  }
  a.job0 = 0;
  hipLaunchKernelGGL(k_wavefront_fold, dim3((ART_WAVEFRONT_DOUBLES + kBlock - 1) / kBlock, n_jobs), dim3(kBlock), 0, s,
                     jobs_dev, a, (const double*)scratch);
  return launched("art_wavefront launch");
}

// validates a polarisation job table (not its coatings); *nmax: the largest slot count
static int pol_check_jobs(const ArtPolarisationJob* jobs, int32_t n_jobs, int64_t* nmax) {
  if (!jobs) return fail(ART_ERR_BAD_ARG, "polarisation job table is NULL");
  if (n_jobs < 1 || n_jobs > 65535) return fail(ART_ERR_BAD_ARG, "n_jobs must be in 1..65535");
  *nmax = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtPolarisationJob& jb = jobs[j];
    if (jb.n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
    if (jb.n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays per chain in one polarisation call");
    if (jb.n_elems < 1 || jb.n_elems > ART_POLARISATION_MAX_ELEMS)
      return fail(ART_ERR_BAD_ARG, "a polarisation job must have 1..ART_POLARISATION_MAX_ELEMS elements");
    *nmax = jb.n > *nmax ? jb.n : *nmax;
  }
  return ART_OK;
}

static int coating_check(const ArtCoating& c) {
  if (c.ideal) return ART_OK;
  if (c.n_materials < 1 || c.n_materials > ART_COATING_MAX_MATERIALS)
    return fail(ART_ERR_BAD_ARG, "a coating must name 1..ART_COATING_MAX_MATERIALS materials");
  if (c.n_layers < 0 || c.n_layers > ART_COATING_MAX_LAYERS)
    return fail(ART_ERR_BAD_ARG, "a coating must have 0..ART_COATING_MAX_LAYERS layers");
  if (c.substrate < 0 || c.substrate >= c.n_materials) return fail(ART_ERR_BAD_ARG, "coating substrate index out of range");
  if (!(isfinite(c.roughness) && c.roughness >= 0.0)) return fail(ART_ERR_BAD_ARG, "coating roughness must be finite and >= 0");
  for (int m = 0; m < c.n_materials; ++m)
    if (!(isfinite(c.materials[m].n) && isfinite(c.materials[m].kappa) && c.materials[m].kappa >= 0.0))
      return fail(ART_ERR_BAD_ARG, "a coating material must have finite n and finite kappa >= 0");
  for (int l = 0; l < c.n_layers; ++l) {
    const ArtCoatingLayer& ly = c.layers[l];
    if (ly.material < 0 || ly.material >= c.n_materials) return fail(ART_ERR_BAD_ARG, "coating layer material out of range");
    if (!(isfinite(ly.thickness) && ly.thickness >= 0.0 && isfinite(ly.roughness) && ly.roughness >= 0.0))
      return fail(ART_ERR_BAD_ARG, "coating layer thickness and roughness must be finite and >= 0");
  }
  return ART_OK;
}

int64_t art_polarisation_scratch_doubles(const ArtPolarisationJob* jobs_host, int32_t n_jobs) {
  int64_t nmax;
  const int rc = pol_check_jobs(jobs_host, n_jobs, &nmax);
  return rc ? rc : (int64_t)n_jobs * kPolStats * pol_tiles(nmax);
}

int art_polarisation(const ArtPolarisationJob* jobs_dev, const ArtPolarisationJob* jobs_host, int32_t n_jobs,
                     const ArtCoating* coatings_dev, const ArtCoating* coatings_host, int32_t n_coatings, double* scratch,
                     void* stream) {
  if (!jobs_dev || !scratch) return fail(ART_ERR_BAD_ARG, "NULL argument");
  int64_t nmax;
  const int rc = pol_check_jobs(jobs_host, n_jobs, &nmax);
  if (rc) return rc;
  if (n_coatings < 0 || n_coatings > 65535) return fail(ART_ERR_BAD_ARG, "n_coatings must be in 0..65535");
  if (n_coatings > 0 && (!coatings_dev || !coatings_host)) return fail(ART_ERR_BAD_ARG, "coating table is NULL");
  for (int c = 0; c < n_coatings; ++c) {
    const int cr = coating_check(coatings_host[c]);
    if (cr) return cr;
  }
  for (int j = 0; j < n_jobs; ++j) {
    const ArtPolarisationJob& jb = jobs_host[j];
    if (!jb.out || !jb.w_out || !jb.views) return fail(ART_ERR_BAD_ARG, "a polarisation job's views, w_out or out is NULL");
    if (!(isfinite(jb.k) && jb.k > 0.0)) return fail(ART_ERR_BAD_ARG, "a polarisation job's wave number must be finite and > 0");
    bool finite = true;
    for (int q = 0; q < 6; ++q) finite = finite && isfinite(jb.pol[q]);
    if (!finite) return fail(ART_ERR_BAD_ARG, "a polarisation job's input state is not finite");
    if (jb.field && !jb.polarised) return fail(ART_ERR_BAD_ARG, "the per-ray field needs a polarised input");
    for (int e = 0; e < jb.n_elems; ++e)
      if (jb.coating[e] < -1 || jb.coating[e] >= n_coatings) return fail(ART_ERR_BAD_ARG, "coating index out of range");
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t per_job = kPolStats * pol_tiles(nmax);
  hipLaunchKernelGGL(k_polarisation, dim3((unsigned)pol_tiles(nmax), n_jobs), dim3(kBlock), 0, s, jobs_dev, coatings_dev,
                     per_job, scratch);
  hipLaunchKernelGGL(k_polarisation_fold, dim3(ART_POLARISATION_DOUBLES, n_jobs), dim3(kFoldBlock), 0, s, jobs_dev, per_job,
                     (const double*)scratch);
  return launched("art_polarisation launch");
}

// the elements of a ray-tube or sensitivity job (host copies): kinds the transport of art_tubes.h covers; `who` opens the message
static int tube_check_elems(const char* who, const ArtElementDesc* elems, const ArtQuadricDesc* quadrics, const int n_elems) {
  for (int e = 0; e < n_elems; ++e) {
    const ArtElementDesc& el = elems[e];
    char msg[96];
    if (el.kind < 0 || el.kind >= ART_NUM_KINDS) return fail(ART_ERR_BAD_ARG, "unknown optic kind");
    const char* why = (el.flags & ART_FLAG_GRATING)    ? "is a grating"
                      : (el.flags & ART_FLAG_FREEFORM) ? "is a freeform"
                      : (el.n_defects > 0 || el.n_grid > 0 || (el.flags & (ART_FLAG_PERTURBED_NORMAL | ART_FLAG_ZERN_RECURRENCE)))
                          ? "has defects"
                          : nullptr;
    if (why) {
      snprintf(msg, sizeof msg, "%s: element %d %s", who, e, why);
      return fail(ART_ERR_UNSUPPORTED, msg);
    }
    if ((el.flags & ART_FLAG_QUADRIC) && !quadrics) return fail(ART_ERR_BAD_ARG, "a quadric element without the quadrics table");
  }
  return ART_OK;
}

// validates a ray-tube job table (host copies of the elements included); *nmax: the largest slot count
static int tube_check_jobs(const ArtTubeJob* jobs, int32_t n_jobs, int64_t* nmax) {
  if (!jobs) return fail(ART_ERR_BAD_ARG, "ray-tube job table is NULL");
  if (n_jobs < 1 || n_jobs > ART_TUBE_MAX_JOBS) return fail(ART_ERR_BAD_ARG, "n_jobs must be in 1..ART_TUBE_MAX_JOBS");
  *nmax = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtTubeJob& jb = jobs[j];
    if (jb.n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
    if (jb.n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays per chain in one ray-tube call");
    if (jb.n_elems < 1 || jb.n_elems > ART_TUBE_MAX_ELEMS)
      return fail(ART_ERR_BAD_ARG, "a ray-tube job must have 1..ART_TUBE_MAX_ELEMS elements");
    if (jb.seed != ART_TUBE_POINT && jb.seed != ART_TUBE_PLANE) return fail(ART_ERR_BAD_ARG, "unknown ray-tube seed");
    if (!jb.views || !jb.elems || !jb.weight) return fail(ART_ERR_BAD_ARG, "a ray-tube job's views, elems or weight is NULL");
    if (jb.has_detector) {
      double nn = 0.0;
      bool finite = true;
      for (int q = 0; q < 3; ++q) {
        nn += jb.det.normal[q] * jb.det.normal[q];
        finite = finite && isfinite(jb.det.centre[q]) && isfinite(jb.det.normal[q]);
      }
      if (!finite || !(fabs(nn - 1.0) <= 1e-12)) return fail(ART_ERR_BAD_ARG, "a ray-tube job's detector needs a finite centre and a unit normal");
    }
    const int bad = tube_check_elems("ray tubes", jb.elems, jb.quadrics, jb.n_elems);
    if (bad) return bad;
    *nmax = jb.n > *nmax ? jb.n : *nmax;
  }
  return ART_OK;
}

int64_t art_ray_tubes_scratch_doubles(const ArtTubeJob* jobs_host, int32_t n_jobs) {
  int64_t nmax;
  const int rc = tube_check_jobs(jobs_host, n_jobs, &nmax);
  return rc ? rc : (int64_t)n_jobs * kTubeStats * pol_tiles(nmax);
}

int art_ray_tubes(const ArtTubeJob* jobs_dev, const ArtTubeJob* jobs_host, int32_t n_jobs, double* scratch, double* out,
                  void* stream) {
  if (!jobs_dev || !scratch || !out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  int64_t nmax;
  const int rc = tube_check_jobs(jobs_host, n_jobs, &nmax);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t per_job = kTubeStats * pol_tiles(nmax);
  hipLaunchKernelGGL(k_ray_tubes, dim3((unsigned)pol_tiles(nmax), n_jobs), dim3(kBlock), 0, s, jobs_dev, per_job, scratch);
  hipLaunchKernelGGL(k_ray_tubes_fold, dim3(ART_TUBE_DOUBLES, n_jobs), dim3(kFoldBlock), 0, s, jobs_dev, per_job,
                     (const double*)scratch, out);
  return launched("art_ray_tubes launch");
}

// validates a sensitivity job table (host copies of the elements included); *nmax, *kmax: the largest slot and element
// counts, *rows: the rows of all tables
static int sens_check_jobs(const ArtSensitivityJob* jobs, int32_t n_jobs, int64_t* nmax, int* kmax, int64_t* rows) {
  if (!jobs) return fail(ART_ERR_BAD_ARG, "sensitivity job table is NULL");
  if (n_jobs < 1 || n_jobs > ART_TUBE_MAX_JOBS) return fail(ART_ERR_BAD_ARG, "n_jobs must be in 1..ART_TUBE_MAX_JOBS");
  *nmax = 0;
  *kmax = 0;
  *rows = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtSensitivityJob& jb = jobs[j];
    if (jb.n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
    if (jb.n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays per chain in one sensitivity call");
    if (jb.n_elems < 1 || jb.n_elems > ART_TUBE_MAX_ELEMS)
      return fail(ART_ERR_BAD_ARG, "a sensitivity job must have 1..ART_TUBE_MAX_ELEMS elements");
    if (!jb.views || !jb.elems) return fail(ART_ERR_BAD_ARG, "a sensitivity job's views or elems is NULL");
    double nn = 0.0;
    bool finite = true;
    for (int q = 0; q < 3; ++q) {
      nn += jb.det.normal[q] * jb.det.normal[q];
      finite = finite && isfinite(jb.det.centre[q]) && isfinite(jb.det.normal[q]) && isfinite(jb.origin[q]);
    }
    for (int q = 0; q < 9; ++q) finite = finite && isfinite(jb.det.rot[q]);
    if (!finite || !(fabs(nn - 1.0) <= 1e-12))
      return fail(ART_ERR_BAD_ARG, "a sensitivity job needs a detector (finite centre and rot, unit normal) and a finite origin");
    const int bad = tube_check_elems("sensitivities", jb.elems, jb.quadrics, jb.n_elems);
    if (bad) return bad;
    *nmax = jb.n > *nmax ? jb.n : *nmax;
    *kmax = jb.n_elems > *kmax ? jb.n_elems : *kmax;
    *rows += 1 + ART_SENS_COLS * (jb.n_elems + 1);
  }
  return ART_OK;
}

int64_t art_sensitivities_scratch_doubles(const ArtSensitivityJob* jobs_host, int32_t n_jobs) {
  int64_t nmax, rows;
  int kmax;
  const int rc = sens_check_jobs(jobs_host, n_jobs, &nmax, &kmax, &rows);
  return rc ? rc : (int64_t)n_jobs * (kmax + 1) * kSensParts * pol_tiles(nmax) * kSensStats;
}

int art_sensitivities(const ArtSensitivityJob* jobs_dev, const ArtSensitivityJob* jobs_host, int32_t n_jobs, double* scratch,
                      double* out, void* stream) {
  if (!jobs_dev || !scratch || !out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  int64_t nmax, rows;
  int kmax;
  const int rc = sens_check_jobs(jobs_host, n_jobs, &nmax, &kmax, &rows);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = pol_tiles(nmax);
  const int groups = (kmax + 1) * kSensParts;
  const int64_t per_job = (int64_t)groups * tiles * kSensStats;
  hipLaunchKernelGGL(k_sensitivities, dim3((unsigned)tiles, groups, n_jobs), dim3(kBlock), 0, s, jobs_dev, per_job, tiles,
                     scratch);
  hipLaunchKernelGGL(k_sensitivities_fold, dim3(ART_SENS_DOUBLES, 1 + ART_SENS_COLS * (kmax + 1), n_jobs), dim3(kFoldBlock), 0,
                     s, jobs_dev, per_job, tiles, (const double*)scratch, out);
  return launched("art_sensitivities launch");
}

// validates a compensator job table (host copies of the elements included); *nmax: the largest slot count, *buckets: bit
// NC / 2 - 1 is set when a job runs in the kernels for NC columns
static int align_check_jobs(const ArtAlignmentJob* jobs, int32_t n_jobs, int64_t* nmax, unsigned* buckets) {
  if (!jobs) return fail(ART_ERR_BAD_ARG, "alignment job table is NULL");
  if (n_jobs < 1 || n_jobs > ART_TUBE_MAX_JOBS) return fail(ART_ERR_BAD_ARG, "n_jobs must be in 1..ART_TUBE_MAX_JOBS");
  *nmax = 0;
  *buckets = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtAlignmentJob& jb = jobs[j];
    if (jb.n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
    if (jb.n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays per chain in one alignment call");
    if (jb.n_elems < 1 || jb.n_elems > ART_TUBE_MAX_ELEMS)
      return fail(ART_ERR_BAD_ARG, "an alignment job must have 1..ART_TUBE_MAX_ELEMS elements");
    if (jb.n_dofs < 1 || jb.n_dofs > ART_ALIGN_MAX_DOFS)
      return fail(ART_ERR_BAD_ARG, "an alignment job must have 1..ART_ALIGN_MAX_DOFS degrees of freedom");
    for (int a = 0; a < jb.n_dofs; ++a) {
      if (jb.dofs[a] < ART_ALIGN_DOF_DETECTOR || jb.dofs[a] >= ART_SENS_COLS * (jb.n_elems + 1))
        return fail(ART_ERR_BAD_ARG, "an alignment job's degree of freedom is out of range: -1 or 0 .. 6 (K + 1) - 1");
      for (int b = 0; b < a; ++b)
        if (jb.dofs[b] == jb.dofs[a]) return fail(ART_ERR_BAD_ARG, "an alignment job names a degree of freedom twice (duplicate id)");
    }
    if (!jb.views || !jb.elems) return fail(ART_ERR_BAD_ARG, "an alignment job's views or elems is NULL");
    double nn = 0.0;
    bool finite = true;
    for (int q = 0; q < 3; ++q) {
      nn += jb.det.normal[q] * jb.det.normal[q];
      finite = finite && isfinite(jb.det.centre[q]) && isfinite(jb.det.normal[q]) && isfinite(jb.origin[q]);
    }
    for (int q = 0; q < 9; ++q) finite = finite && isfinite(jb.det.rot[q]);
    if (!finite || !(fabs(nn - 1.0) <= 1e-12))
      return fail(ART_ERR_BAD_ARG, "an alignment job needs a detector (finite centre and rot, unit normal) and a finite origin");
    const int bad = tube_check_elems("alignment sums", jb.elems, jb.quadrics, jb.n_elems);
    if (bad) return bad;
    *nmax = jb.n > *nmax ? jb.n : *nmax;
    *buckets |= 1u << (align_bucket(jb.n_dofs) / 2 - 1);
  }
  return ART_OK;
}

// the partial sums per tile of the call's widest kernel
static int align_stride(const unsigned buckets) {
  return align_stats(buckets & 8 ? 8 : (buckets & 4 ? 6 : (buckets & 2 ? 4 : 2)));
}

int64_t art_alignment_sums_scratch_doubles(const ArtAlignmentJob* jobs_host, int32_t n_jobs) {
  int64_t nmax;
  unsigned buckets;
  const int rc = align_check_jobs(jobs_host, n_jobs, &nmax, &buckets);
  return rc ? rc : (int64_t)n_jobs * (pol_tiles(nmax) * align_stride(buckets) + kAlignPilotTiles * kAlignPilotStats);
}

int art_alignment_sums(const ArtAlignmentJob* jobs_dev, const ArtAlignmentJob* jobs_host, int32_t n_jobs, double* scratch,
                       double* out, void* stream) {
  if (!jobs_dev || !scratch || !out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  int64_t nmax;
  unsigned buckets;
  const int rc = align_check_jobs(jobs_host, n_jobs, &nmax, &buckets);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = pol_tiles(nmax), per_job = tiles * align_stride(buckets);
  double* pilot = scratch + (int64_t)n_jobs * per_job;         // (behind the tiles' partial sums)
  for (int pass = 0; pass < 2; ++pass) {                       // every job's pilot sums, then the sums about their means
    const bool first = pass == 0;
    align_launch<2>(first, buckets, jobs_dev, n_jobs, tiles, per_job, scratch, pilot, s);
    align_launch<4>(first, buckets, jobs_dev, n_jobs, tiles, per_job, scratch, pilot, s);
    align_launch<6>(first, buckets, jobs_dev, n_jobs, tiles, per_job, scratch, pilot, s);
    align_launch<8>(first, buckets, jobs_dev, n_jobs, tiles, per_job, scratch, pilot, s);
  }
  hipLaunchKernelGGL(k_alignment_fold, dim3(ART_ALIGN_DOUBLES, n_jobs), dim3(kFoldBlock), 0, s, jobs_dev, per_job,
                     (const double*)scratch, (const double*)pilot, out);
  return launched("art_alignment_sums launch");
}

// the wavenumber blocks of art_focal_vector_spectrum: slices S of the rays (never from the block: the same bytes for any),
// wavenumbers per block nkb, doubles of scratch
struct VecSpecPlan {
  int S, nkb;
  int64_t stride, total;
};
static VecSpecPlan vecspec_plan(const ArtFocalVectorSpectrumDesc* d, const int prep_rows = kFocalSpecRows) {
  const ArtFocalDesc& f = d->s.f;
  VecSpecPlan p;
  // (the grid rows of ONE wavenumber: a block may hold no more, and a count taken from all nk leaves a launch of a
  // block with about as many workgroups as the machine has places for, so that a few stragglers run a round alone)
  p.S = focal_slices(f.nx, f.ny, f.planes * 3, d->n);
  p.stride = focal_stride(d->n);
  p.nkb = 1;
  p.total = 0;
  if (d->n == 0) return p;
  const int64_t rows = (int64_t)prep_rows * p.stride;
  const int64_t per_k = 6 * p.stride + (p.S > 1 ? (int64_t)p.S * f.planes * 3 * f.ny * f.nx * 2 : 0);
  const int64_t bound = d->scratch_bound ? d->scratch_bound : ART_FOCAL_VECTOR_SCRATCH_DEFAULT;
  const int64_t fit = (bound - rows) / per_k;
  p.nkb = fit < 1 ? 1 : (fit > d->s.nk ? d->s.nk : (int)fit);
  p.total = rows + p.nkb * per_k;
  return p;
}

// the checks of the descriptor that need neither the coatings nor the buffers
static int vecspec_check(const ArtFocalVectorSpectrumDesc* d) {
  if (!d) return fail(ART_ERR_BAD_ARG, "focal vector spectrum descriptor is NULL");
  if (const int e = focal_desc_check(&d->s.f)) return e;
  if (const int e = focal_spectrum_check(&d->s)) return e;
  if ((int64_t)d->s.f.planes * d->s.nk * 3 > 65535)
    return fail(ART_ERR_BAD_ARG, "focal vector spectrum: planes * nk * 3 must be <= 65535");
  if (d->n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (d->n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays in one focal vector spectrum call");
  if (d->n_elems < 1 || d->n_elems > ART_POLARISATION_MAX_ELEMS)
    return fail(ART_ERR_BAD_ARG, "a focal vector spectrum needs 1..ART_POLARISATION_MAX_ELEMS elements");
  if (d->n_coatings < 0 || d->n_coatings > 65535) return fail(ART_ERR_BAD_ARG, "n_coatings must be in 0..65535");
  if (d->scratch_bound < 0) return fail(ART_ERR_BAD_ARG, "focal vector spectrum: scratch_bound must be >= 0");
  for (int e = 0; e < d->n_elems; ++e)
    if (d->coating[e] < -1 || d->coating[e] >= d->n_coatings) return fail(ART_ERR_BAD_ARG, "coating index out of range");
  for (int q = 0; q < 6; ++q)
    if (!isfinite(d->pol[q])) return fail(ART_ERR_BAD_ARG, "focal vector spectrum: the input state is not finite");
  return ART_OK;
}

int64_t art_focal_vector_spectrum_scratch_doubles(const ArtFocalVectorSpectrumDesc* d) {
  if (const int e = vecspec_check(d)) return e;
  return vecspec_plan(d).total;
}

// what art_focal_vector_chromatic adds to art_focal_vector_spectrum's call: the source view, the axis and the table
struct VecChromArg {
  const ArtBundleView* src;
  const double* axis;
  const double* table_dev;
};

// art_focal_vector_spectrum (ch NULL) and art_focal_vector_chromatic after the checks of the descriptor: the checks of
// the tables and buffers, then the launches
static int vecspec_run(const ArtFocalVectorSpectrumDesc* d, const VecChromArg* ch, const ArtBundleView* b,
                       const ArtCoating* coatings_dev, const ArtCoating* coatings_host,
                       const ArtCoatingMaterial* materials_host, double* scratch, double* field, void* stream) {
  const ArtFocalDesc* f = &d->s.f;
  const int nk = d->s.nk, nc = d->n_coatings;
  if (nc > 0 && (!coatings_dev || !coatings_host || !materials_host || !d->materials))
    return fail(ART_ERR_BAD_ARG, "coating or material table is NULL");
  for (int c = 0; c < nc; ++c) {
    if (const int cr = coating_check(coatings_host[c])) return cr;
    if (coatings_host[c].ideal) continue;
    for (int j = 0; j < nk; ++j)
      for (int m = 0; m < coatings_host[c].n_materials; ++m) {
        const ArtCoatingMaterial& mt = materials_host[((int64_t)j * nc + c) * ART_COATING_MAX_MATERIALS + m];
        if (!(isfinite(mt.n) && isfinite(mt.kappa) && mt.kappa >= 0.0))
          return fail(ART_ERR_BAD_ARG, "a material of the per-wavenumber table must have finite n and finite kappa >= 0");
      }
  }
  if (d->n > 0 && !d->views) return fail(ART_ERR_BAD_ARG, "focal vector spectrum: views is NULL");
  if (ch && d->n > 0 && !ch->table_dev) return fail(ART_ERR_BAD_ARG, "focal vector chromatic: the device table must not be NULL");
  if (ch && d->n > 0 && !view_ok(ch->src)) return fail(ART_ERR_BAD_ARG, "source bundle view has a NULL array");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = d->n, pix = (int64_t)f->ny * f->nx;
  bool done;
  if (const int e = focal_call_check(b, n, scratch, field, (int64_t)f->planes * nk * 3 * pix, s, &done); e || done) return e;
  const int prep_rows = ch ? kFocalChromRows : kFocalSpecRows;
  const VecSpecPlan p = vecspec_plan(d, prep_rows);
  const int S = p.S;
  const FocalArg a = focal_arg(f, n, S);
  const int tiles = focal_tiles(f->nx, f->ny);
  VecSpecArg va;
  memset(&va, 0, sizeof(va));
  va.views = d->views; va.w = d->w;
  for (int q = 0; q < 6; ++q) va.pol[q] = d->pol[q];
  for (int c = 0; c < 3; ++c) { va.u[c] = a.e1[c]; va.u[3 + c] = a.e2[c]; va.u[6 + c] = a.nrm[c]; }
  va.k0 = f->k; va.dk = d->s.dk;
  va.n = n; va.stride = a.stride;
  va.n_elems = d->n_elems; va.n_coatings = nc;
  for (int e = 0; e < d->n_elems; ++e) va.coating[e] = d->coating[e];
  per_launch(n, [&](const int64_t off, const int64_t m) {       // (one launch: n <= 2^28)
    if (ch)
      hipLaunchKernelGGL(k_focal_chromatic_prep, dim3(grid_for(m)), dim3(kBlock), 0, s, a, view_at(*b, off),
                         view_at(*ch->src, off), ch->axis[0], ch->axis[1], ch->axis[2], d->w ? d->w + off : nullptr, m,
                         scratch + off);
    else
      hipLaunchKernelGGL(k_focal_spectrum_prep, dim3(grid_for(m)), dim3(kBlock), 0, s, a, view_at(*b, off),
                         d->w ? d->w + off : nullptr, m, scratch + off);
    return ART_OK;
  });
  double* amps = scratch + (int64_t)prep_rows * a.stride;
  double* part = amps + (int64_t)p.nkb * 6 * a.stride;
  // the field kernel of a block of m wavenumbers from j0: planes (and slices) strided as given, into out
  const auto field_launch = [&](const int j0, const int m, const int slices, const int64_t plane_stride,
                                const int64_t slice_stride, double* out) {
    const dim3 grid(tiles, f->planes * m * 3, slices);
    if (ch)
      hipLaunchKernelGGL(k_vecchrom_field, grid, dim3(kBlock), 0, s, a, ch->table_dev, j0, m, (const double*)scratch,
                         (const double*)amps, plane_stride, slice_stride, out);
    else
      hipLaunchKernelGGL(k_vecspec_field, grid, dim3(kBlock), 0, s, a, d->s.dk, j0, m, (const double*)scratch,
                         (const double*)amps, plane_stride, slice_stride, out);
  };
  for (int j0 = 0; j0 < nk; j0 += p.nkb) {
    const int m = nk - j0 < p.nkb ? nk - j0 : p.nkb;
    va.j0 = j0; va.nkb = m;
    const dim3 rays_grid((unsigned)pol_tiles(n), m);
    if (ch)
      hipLaunchKernelGGL(k_vecchrom_rays, rays_grid, dim3(kBlock), 0, s, va, coatings_dev, d->materials, ch->table_dev,
                         (const double*)scratch + 5 * a.stride, amps);
    else
      hipLaunchKernelGGL(k_vecspec_rays, rays_grid, dim3(kBlock), 0, s, va, coatings_dev, d->materials, amps);
    double* dst = field + (int64_t)j0 * 3 * pix * 2;          // plane 0's place of this block in the field
    if (S == 1) {
      field_launch(j0, m, 1, (int64_t)nk * 3 * pix, 0, dst);
      continue;
    }
    const int64_t block = (int64_t)m * 3 * pix;               // a plane's pixels of this block
    field_launch(j0, m, S, (int64_t)S * block, block, part);
    for (int q = 0; q < f->planes; ++q)
      focal_fold_launch(part + (int64_t)q * S * block * 2, S, block, dst + (int64_t)q * nk * 3 * pix * 2, s);
  }
  return launched(ch ? "art_focal_vector_chromatic launch" : "art_focal_vector_spectrum launch");
}

int art_focal_vector_spectrum(const ArtFocalVectorSpectrumDesc* d, const ArtBundleView* b, const ArtCoating* coatings_dev,
                              const ArtCoating* coatings_host, const ArtCoatingMaterial* materials_host, double* scratch,
                              double* field, void* stream) {
  if (const int e = vecspec_check(d)) return e;
  return vecspec_run(d, nullptr, b, coatings_dev, coatings_host, materials_host, scratch, field, stream);
}

int64_t art_focal_vector_chromatic_scratch_doubles(const ArtFocalVectorChromaticDesc* d) {
  if (!d) return fail(ART_ERR_BAD_ARG, "focal vector chromatic descriptor is NULL");
  if (const int e = vecspec_check(&d->v)) return e;
  return vecspec_plan(&d->v, kFocalChromRows).total;
}

int art_focal_vector_chromatic(const ArtFocalVectorChromaticDesc* d, const ArtBundleView* b, const ArtBundleView* src,
                               const ArtCoating* coatings_dev, const ArtCoating* coatings_host,
                               const ArtCoatingMaterial* materials_host, const double* table_dev,
                               const double* table_host, double* scratch, double* field, void* stream) {
  if (!d) return fail(ART_ERR_BAD_ARG, "focal vector chromatic descriptor is NULL");
  if (const int e = vecspec_check(&d->v)) return e;
  if (const int e = focal_chromatic_table_check(d->axis, d->v.s.nk, table_host)) return e;
  const VecChromArg ch = {src, d->axis, table_dev};
  return vecspec_run(&d->v, &ch, b, coatings_dev, coatings_host, materials_host, scratch, field, stream);
}

int64_t art_reduce_scratch_doubles(void) { return (int64_t)8 * kReadoutBlocks * kReadoutSlots + 64; }

int art_detector_stats(const uint8_t* alive, const double* X, const double* Y, const double* opl, const double* w,
                       int64_t n, double* scratch, double* out16, void* stream) {
  if (!alive || !scratch || !out16) return fail(ART_ERR_BAD_ARG, "alive/scratch/out16 must not be NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  const int nb = red_blocks(n);
  if (w) hipLaunchKernelGGL(k_stats_partial<true>, dim3(nb), dim3(kBlock), 0, s, alive, X, Y, opl, w, n, scratch);
  else hipLaunchKernelGGL(k_stats_partial<false>, dim3(nb), dim3(kBlock), 0, s, alive, X, Y, opl, w, n, scratch);
  return fold_partials<kRedSlots, stat_op>(scratch, nb, out16, s, "art_detector_stats launch");
}

int art_detector_moments(const uint8_t* alive, const double* X, const double* Y, const double* opl, const double* w,
                         int64_t n, double cx, double cy, double co, double* scratch, double* out8, void* stream) {
  if (!alive || !scratch || !out8) return fail(ART_ERR_BAD_ARG, "alive/scratch/out8 must not be NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  const int nb = red_blocks(n);
  if (w) hipLaunchKernelGGL(k_moments_partial<true>, dim3(nb), dim3(kBlock), 0, s, alive, X, Y, opl, w, n, cx, cy, co, scratch);
  else hipLaunchKernelGGL(k_moments_partial<false>, dim3(nb), dim3(kBlock), 0, s, alive, X, Y, opl, w, n, cx, cy, co, scratch);
  return fold_partials<kSumSlots, sum_op>(scratch, nb, out8, s, "art_detector_moments launch");
}

int art_bundle_sums(const ArtBundleView* bv, const double* w, int64_t n, double* scratch, double* out8, void* stream) {
  if (!view_ok(bv) || !scratch || !out8) return fail(ART_ERR_BAD_ARG, "bundle/scratch/out8 must not be NULL");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  const int nb = red_blocks(n);
  if (w) hipLaunchKernelGGL(k_bundle_sums_partial<true>, dim3(nb), dim3(kBlock), 0, s, *bv, w, n, scratch);
  else hipLaunchKernelGGL(k_bundle_sums_partial<false>, dim3(nb), dim3(kBlock), 0, s, *bv, w, n, scratch);
  return fold_partials<kSumSlots, sum_op>(scratch, nb, out8, s, "art_bundle_sums launch");
}

static int gaussian_impl(const ArtBundleView* bv, const double axis[3], const double* axis_sums, double fraction, int64_t n,
                         double* scratch, double* w_out, void* stream);

// the max pair of n > 0 rays (largest angle to the axis, largest distance from the origin) into max2[0 .. 1]; the
// partials take scratch[0 .. kRedBlocks * kMaxSlots)
static void max_pass(const ArtBundleView& b, const Axis3 ax, const double* axis_sums, int64_t n, double* scratch, double* max2,
                     hipStream_t s) {
  const int nb = red_blocks(n);
  hipLaunchKernelGGL(k_gauss_max_partial, dim3(nb), dim3(kBlock), 0, s, b, ax, axis_sums, n, scratch);
  // (at most 4 partials per thread: folded one load at a time)
  hipLaunchKernelGGL((k_fold_partials<kMaxSlots, 1, max_op>), dim3(kMaxSlots), dim3(kBlock), 0, s, scratch, nb, max2);
}

int art_gaussian_intensity(const ArtBundleView* bv, const double axis[3], double fraction, int64_t n, double* scratch,
                           double* w_out, void* stream) {
  if (!axis) return fail(ART_ERR_BAD_ARG, "NULL argument");
  return gaussian_impl(bv, axis, nullptr, fraction, n, scratch, w_out, stream);
}

int art_gaussian_intensity_central(const ArtBundleView* bv, double fraction, int64_t n, double* scratch, double* sums8,
                                   double* w_out, void* stream) {
  if (!view_ok(bv) || !scratch || !sums8 || !w_out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n <= 0) return (n == 0) ? ART_OK : fail(ART_ERR_BAD_ARG, "negative ray count");
  const int rc = art_bundle_sums(bv, nullptr, n, scratch, sums8, stream);       // the central ray's sums, left on the device
  if (rc) return rc;
  const double none[3] = {0.0, 0.0, 0.0};
  return gaussian_impl(bv, none, sums8, fraction, n, scratch, w_out, stream);
}

static int gaussian_impl(const ArtBundleView* bv, const double axis[3], const double* axis_sums, double fraction, int64_t n,
                         double* scratch, double* w_out, void* stream) {
  if (!view_ok(bv) || !axis || !scratch || !w_out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (!(fraction > 0.0 && fraction < 1.0)) return fail(ART_ERR_BAD_ARG, "fraction must be in (0, 1)");
  if (n == 0) return ART_OK;
  hipStream_t s = (hipStream_t)stream;
  const Axis3 ax = {axis[0], axis[1], axis[2]};
  double* maxima = scratch + (int64_t)kRedBlocks * kMaxSlots;   // right behind the partials
  max_pass(*bv, ax, axis_sums, n, scratch, maxima, s);
  hipLaunchKernelGGL(k_gauss_weights, dim3(grid_for(n)), dim3(kBlock), 0, s, *bv, ax, axis_sums, -0.5 * log(fraction), maxima, n,
                     w_out);
  return launched("art_gaussian_intensity launch");
}

int art_bundle_max_angle(const ArtBundleView* bv, const double axis[3], int64_t n, double* scratch, double* out2,
                         void* stream) {
  if (!axis || !scratch || !out2) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    hipError_t e0 = hipMemsetAsync(out2, 0, 2 * sizeof(double), s);
    if (e0 != hipSuccess) return fail_hip(e0, "hipMemsetAsync");
    return ART_OK;
  }
  if (!view_ok(bv)) return fail(ART_ERR_BAD_ARG, "bundle view has a NULL array");
  max_pass(*bv, Axis3{axis[0], axis[1], axis[2]}, nullptr, n, scratch, out2, s);
  return launched("art_bundle_max_angle launch");
}

int64_t art_compact_scratch_ints(int64_t n) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  // int32 counts [tiles] followed by int64 offsets [tiles] (8-byte aligned: round counts up to even)
  const int64_t c = (tiles + 1) & ~1ll;
  return c + 2 * tiles + 2;
}

int art_compact(const uint8_t* alive, int64_t n, int32_t* block_counts, int64_t* idx_out, int64_t* count_out,
                void* stream) {
  if (!alive || !block_counts || !idx_out || !count_out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    hipError_t e0 = hipMemsetAsync(count_out, 0, sizeof(int64_t), s);
    if (e0 != hipSuccess) return fail_hip(e0, "hipMemsetAsync");
    return ART_OK;
  }
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t c = (tiles + 1) & ~1ll;
  int64_t* offsets = reinterpret_cast<int64_t*>(block_counts + c);
  hipLaunchKernelGGL(k_compact_count, dim3((unsigned)tiles), dim3(kBlock), 0, s, alive, n, block_counts);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, s, block_counts, tiles, count_out, offsets);
  hipLaunchKernelGGL(k_compact_scatter, dim3((unsigned)tiles), dim3(kBlock), 0, s, alive, n, offsets, idx_out);
  return launched("art_compact launch");
}

int64_t art_survivor_bytes(int64_t count, int32_t dense) {
  if (count < 0) count = 0;
  const int64_t b = kSurvHeader + count * (dense ? 24 : 28);
  return (b + 15) / 16 * 16;
}

int art_pack_survivors(const uint8_t* alive, int64_t n, const double* X, const double* Y, const double* opl,
                       const int64_t* number, int64_t first, int64_t step, int32_t* scratch_ints, void* send,
                       int64_t send_bytes, void* stream) {
  if (!scratch_ints || !send) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (send_bytes < art_survivor_bytes(n, 0)) return fail(ART_ERR_BAD_ARG, "send buffer smaller than art_survivor_bytes(n, 0)");
  if (((uintptr_t)send & 7u) != 0) return fail(ART_ERR_BAD_ARG, "send buffer must be 8-byte aligned");
  if (!number && (first < 0 || step < 1 || (n > 0 && first + (n - 1) * step > INT32_MAX)))
    return fail(ART_ERR_UNSUPPORTED, "ray numbers do not fit int32");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    hipError_t e0 = hipMemsetAsync(send, 0, kSurvHeader, s);
    if (e0 != hipSuccess) return fail_hip(e0, "hipMemsetAsync");
    return ART_OK;
  }
  if (!alive || !X || !Y || !opl) return fail(ART_ERR_BAD_ARG, "NULL argument");
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int64_t c = (tiles + 1) & ~1ll;
  int64_t* offsets = reinterpret_cast<int64_t*>(scratch_ints + c);
  int64_t* total = offsets + tiles;    // art_compact_scratch_ints() leaves two ints behind the offsets
  hipLaunchKernelGGL(k_compact_count, dim3((unsigned)tiles), dim3(kBlock), 0, s, alive, n, scratch_ints);
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, s, scratch_ints, tiles, total, offsets);
  hipLaunchKernelGGL(k_survivor_header, dim3(1), dim3(64), 0, s, total, n, number ? 0 : 1, reinterpret_cast<int64_t*>(send));
  hipLaunchKernelGGL(k_survivor_scatter, dim3((unsigned)tiles), dim3(kBlock), 0, s, alive, n, offsets, X, Y, opl, number,
                     first, step, reinterpret_cast<unsigned char*>(send));
  return launched("art_pack_survivors launch");
}

int art_make_source(int32_t kind, double size, const double rot[9], const double S[3], int64_t first, int64_t n,
                    int64_t n_total, const ArtBundleView* out, void* stream) {
  return art_make_source_strided(kind, size, rot, S, first, 1, n, n_total, out, stream);
}

int art_make_source_strided(int32_t kind, double size, const double rot[9], const double S[3], int64_t first,
                            int64_t step, int64_t n, int64_t n_total, const ArtBundleView* out, void* stream) {
  if (kind != 0 && kind != 1) return fail(ART_ERR_BAD_ARG, "source kind must be 0 (point) or 1 (plane-wave disk)");
  if (!rot || !S || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n < 0 || first < 0 || step < 1 || n_total <= 0 || (n > 0 && first + (n - 1) * step >= n_total))
    return fail(ART_ERR_BAD_ARG, "bad index range");
  if (n == 0) return ART_OK;
  ArtDetectorDesc rs;
  memset(&rs, 0, sizeof(rs));
  memcpy(rs.rot, rot, 9 * sizeof(double));
  memcpy(rs.centre, S, 3 * sizeof(double));
  hipLaunchKernelGGL(k_make_source, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, kind, size, rs, first, step,
                     n, n_total, *out);
  return launched("art_make_source launch");
}

int art_exchange_pack(const double* stats24, const double* X, const double* Y, const double* opl, const uint8_t* alive,
                      const int64_t* slots, int64_t k, double* send, void* stream) {
  if (!stats24 || !send) return fail(ART_ERR_BAD_ARG, "stats24/send must not be NULL");
  if (k < 0 || (k > 0 && (!X || !Y || !opl || !alive || !slots))) return fail(ART_ERR_BAD_ARG, "bad sample arguments");
  const int64_t work = k > kReadoutSlots ? k : kReadoutSlots;
  hipLaunchKernelGGL(k_exchange_pack, dim3((unsigned)((work + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     stats24, X, Y, opl, alive, slots, k, send);
  return launched("art_exchange_pack launch");
}

int art_exchange_fold(const double* recv, int32_t world, int64_t stride_doubles, double* stats_out24, void* stream) {
  if (!recv || !stats_out24) return fail(ART_ERR_BAD_ARG, "recv/stats_out24 must not be NULL");
  if (world < 1 || stride_doubles < kReadoutSlots) return fail(ART_ERR_BAD_ARG, "bad world size or stride");
  hipLaunchKernelGGL(k_exchange_fold, dim3(1), dim3(64), 0, (hipStream_t)stream, recv, world, stride_doubles, stats_out24);
  return launched("art_exchange_fold launch");
}

int art_make_extended_source(double radius, double divergence, int64_t n_points, int64_t rays_per_point,
                             const double rot[9], const double S[3], int64_t first, int64_t n,
                             const ArtBundleView* out, void* stream) {
  if (!rot || !S || !view_ok(out)) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n_points <= 0 || rays_per_point <= 0) return fail(ART_ERR_BAD_ARG, "n_points and rays_per_point must be > 0");
  if (n < 0 || first < 0 || first + n > n_points * rays_per_point) return fail(ART_ERR_BAD_ARG, "bad index range");
  if (n == 0) return ART_OK;
  ArtDetectorDesc rs;
  memset(&rs, 0, sizeof(rs));
  memcpy(rs.rot, rot, 9 * sizeof(double));
  memcpy(rs.centre, S, 3 * sizeof(double));
  hipLaunchKernelGGL(k_make_extended_source, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, radius,
                     divergence, n_points, rays_per_point, rs, first, n, *out);
  return launched("art_make_extended_source launch");
}

int art_trace_guides(const ArtElementDesc* elems, int32_t count, double* rays, uint8_t* alive, void* stream) {
  if (!elems || !rays || !alive) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (count < 0 || count > ART_GUIDES_MAX) return fail(ART_ERR_BAD_ARG, "art_trace_guides: count must be in 0..8");
  if (count == 0) return ART_OK;
  GuideArgs ga;
  memset(&ga, 0, sizeof(ga));
  bool defects = false;
  for (int k = 0; k < count; ++k) {
    int rc = check_elem(&elems[k]);
    if (rc) return rc;
    if (elems[k].flags & ART_FLAG_ZERN_RECURRENCE)
      return fail(ART_ERR_UNSUPPORTED, "an element carries Zernike tables in the recurrence layout: trace it with art_trace_element");
    if (elems[k].flags & ART_FLAG_GRATING) return fail(ART_ERR_UNSUPPORTED, kGratingRefusal);
    if (elems[k].flags & ART_FLAG_QUADRIC) return fail(ART_ERR_UNSUPPORTED, kQuadricRefusal);
    if (elems[k].flags & ART_FLAG_FREEFORM) return fail(ART_ERR_UNSUPPORTED, kFreeformRefusal);
    ga.e[k] = elems[k];
    art::prepare_element(ga.e[k]);
    defects = defects || ga.e[k].n_defects > 0 || ga.e[k].n_grid > 0;
  }
  hipStream_t s = (hipStream_t)stream;
  if (defects) hipLaunchKernelGGL(k_trace_guides<true>, dim3(1), dim3(64), 0, s, ga, rays, alive, (int)count);
  else hipLaunchKernelGGL(k_trace_guides<false>, dim3(1), dim3(64), 0, s, ga, rays, alive, (int)count);
  return launched("art_trace_guides launch");
}

// scratch layout of art_analyse_bundles: [job][kSumRows rows x ntiles + chunk totals] | [job][kAnaSumsPad] | [job][P][kAnaMom] | [job][kAnaPlace]
static int64_t analysis_rows_stride(int64_t n) { return (int64_t)kSumRows * (analysis_tiles(n) + kFoldChunks); }
int64_t art_analysis_scratch_doubles(int32_t n_jobs, int64_t n) {
  if (n_jobs < 1) n_jobs = 1;
  if (n < 0) n = 0;
  return (int64_t)n_jobs * (analysis_rows_stride(n) + kAnaSumsPad + (int64_t)kAnaBlocks * kAnaMom + kAnaPlace);
}

int art_analyse_bundles(const ArtAnalysisJob* jobs_dev, const ArtAnalysisJob* jobs_host, int32_t n_jobs, int64_t n,
                        double* scratch, double* out, void* stream) {
  if (!jobs_dev || !jobs_host || !scratch || !out) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n_jobs <= 0 || n_jobs > 65535) return fail(ART_ERR_BAD_ARG, "n_jobs must be in 1..65535");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (n > kMaxRaysPerLaunchHw) return fail(ART_ERR_UNSUPPORTED, "more than 2^28 rays per bundle in one analysis");
  bool all_given = true;
  for (int j = 0; j < n_jobs; ++j) {
    const ArtAnalysisJob& jb = jobs_host[j];
    if (jb.mode < ART_JOB_AUTOPLACE || jb.mode > ART_JOB_SUMS) return fail(ART_ERR_BAD_ARG, "unknown job mode");
    if (n > 0 && !view_ok(&jb.b)) return fail(ART_ERR_BAD_ARG, "a job's bundle view has a NULL array");
    if (jb.mode == ART_JOB_MANUAL) {
      // the manual detector's normal is used bit for bit (rotation_to_ez and the Kahan angle assume a unit vector)
      const double nn = jb.normal[0] * jb.normal[0] + jb.normal[1] * jb.normal[1] + jb.normal[2] * jb.normal[2];
      if (!(fabs(nn - 1.0) <= 1e-12)) return fail(ART_ERR_BAD_ARG, "a manual job's detector normal is not a unit vector");
    }
    all_given = all_given && jb.sums != nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  const int P = analysis_blocks(n);
  const int64_t ntiles = analysis_tiles(n), rstride = analysis_rows_stride(n);
  double* rows = scratch;
  double* sums = rows + (int64_t)n_jobs * rstride;
  double* mom = sums + (int64_t)n_jobs * kAnaSumsPad;
  double* place = mom + (int64_t)n_jobs * P * kAnaMom;
  const int direct = ntiles <= kFoldDirect;
  if (!all_given && n > 0) {
    for (int j0 = 0; j0 < n_jobs;) {       // one launch per run of consecutive jobs without sums of their own
      if (jobs_host[j0].sums != nullptr) { ++j0; continue; }
      int j1 = j0;
      while (j1 < n_jobs && jobs_host[j1].sums == nullptr) ++j1;
      hipLaunchKernelGGL(k_analysis_sums, dim3((unsigned)ntiles, j1 - j0), dim3(kBlock), 0, s, jobs_dev, j0, n, rows, rstride);
      if (!direct)
        hipLaunchKernelGGL(k_analysis_sums_fold1, dim3(kSumRows, kFoldChunks, j1 - j0), dim3(kFoldBlock), 0, s, jobs_dev, j0, rows,
                           rstride, ntiles);
      j0 = j1;
    }
  }
  // (n == 0: no tiles were written; a fold over zero tiles leaves the sums' identities -- all zero)
  hipLaunchKernelGGL(k_analysis_sums_fold2, dim3(kSumRows, 1, n_jobs), dim3(direct ? fold_threads(n > 0 ? ntiles : 0) : kBlock), 0, s,
                     jobs_dev, rows, rstride, n > 0 ? ntiles : 0, direct, sums);
  hipLaunchKernelGGL(k_analysis_place, dim3((n_jobs + 63) / 64), dim3(64), 0, s, jobs_dev, (int)n_jobs, sums, place, out);
  {
    // (a grid dimension holds fewer than 2^32 work-items = 2^24 workgroups: more than 16 383 jobs go in several launches)
    const int P8 = (P + 7) / 8 * 8, jmax = ((1 << 24) - 1) / P8, jm = analysis_job_major();
    for (int j0 = 0; j0 < n_jobs; j0 += jmax) {
      const int J = (n_jobs - j0 < jmax) ? n_jobs - j0 : jmax;
      hipLaunchKernelGGL(k_analysis_moments, dim3((unsigned)P8 * (unsigned)J), dim3(kBlock), 0, s, jobs_dev, n, place, out, mom, P,
                         j0, J, jm);
    }
  }
  hipLaunchKernelGGL(k_analysis_fold, dim3(kAnaMom - 1, n_jobs), dim3(kBlock), 0, s, jobs_dev, P, mom, out);
  return launched("art_analyse_bundles launch");
}

int art_survivor_finish(const double* stats24, int64_t n, void* send, double* xhdr, void* stream) {
  if (!stats24 || !send) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (n < 0) return fail(ART_ERR_BAD_ARG, "negative ray count");
  if (((uintptr_t)send & 15u) != 0) return fail(ART_ERR_BAD_ARG, "send buffer must be 16-byte aligned");
  hipLaunchKernelGGL(k_survivor_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, stats24, n, reinterpret_cast<int64_t*>(send), xhdr);
  return launched("art_survivor_finish launch");
}

int art_survivor_xheader(const void* send, const double* stats24, double* xhdr, void* stream) {
  if (!send || !xhdr) return fail(ART_ERR_BAD_ARG, "NULL argument");
  if (((uintptr_t)send & 7u) != 0) return fail(ART_ERR_BAD_ARG, "send buffer must be 8-byte aligned");
  hipLaunchKernelGGL(k_survivor_xheader, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const int64_t*>(send), stats24, xhdr);
  return launched("art_survivor_xheader launch");
}

}  // extern "C"

/*
 * art_hip.h -- C ABI of libart_hip.so: MI355X (gfx950) ray-bundle propagation for ART.
 *
 * The reference (mightymightys/AttosecondRaytracing, pure Python) has no FFI layer; its boundary for
 * this path is the Python call
 *     ModuleProcessing.RayTracingCalculation(source_rays, optical_elements, IgnoreDefects)
 *         ART/ModuleProcessing.py:250-313, sole call site ART/ModuleOpticalChain.py:194
 * plus the Detector read-out methods ART/ModuleDetector.py:191-279.  The entry points below are what a
 * ctypes binding on the reference side would call instead of those Python loops (INTEGRATION.md shows
 * the stub).  Conventions:
 *   - plain C: pointers, sizes, POD structs; no C++/torch types cross the boundary;
 *   - every ray array is a DEVICE pointer owned by the caller (fp64 SoA, one entry per source ray, fixed
 *     length n for the whole chain; rays that missed an element keep their slot with alive = 0);
 *   - descriptors (ArtElementDesc, ArtDetectorDesc) are HOST structs, copied into kernel arguments;
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default);
 *   - return value 0 = ART_OK, negative = error; art_last_error() gives a thread-local message;
 *   - no mutable global state, re-entrant, current HIP device is used.
 */
#ifndef ART_HIP_H
#define ART_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ART_ABI_VERSION 14

/* error codes */
#define ART_OK 0
#define ART_ERR_BAD_ARG (-1)      /* null pointer, negative size, unknown kind                      */
#define ART_ERR_UNSUPPORTED (-2)  /* e.g. Zernike order above ART_ZERN_MAX_ORDER                    */
#define ART_ERR_HIP (-3)          /* a HIP runtime call failed (message holds hipGetErrorString)     */
#define ART_ERR_NO_DEVICE (-4)    /* no gfx950 device visible                                        */

/* optic kinds: ART/ModuleMirror.py classes + ART/ModuleMask.py                                       */
enum ArtOpticKind {
  ART_PLANE = 0,      /* MirrorPlane        ModuleMirror.py:42-113   */
  ART_SPHERE = 1,     /* MirrorSpherical    ModuleMirror.py:117-208  mp[0]=|R|                        */
  ART_PARABOLA = 2,   /* MirrorParabolic    ModuleMirror.py:212-387  mp[0]=p (semi latus rectum)      */
  ART_TORUS = 3,      /* MirrorToroidal     ModuleMirror.py:391-527  mp[0]=R major, mp[1]=r minor     */
  ART_ELLIPSOID = 4,  /* MirrorEllipsoidal  ModuleMirror.py:565-751  mp[0]=a, mp[1]=b                 */
  ART_CYLINDER = 5,   /* MirrorCylindrical  ModuleMirror.py:781-874  mp[0]=|R|                        */
  ART_MASK = 6,       /* Mask               ModuleMask.py:24-136                                      */
  ART_NUM_KINDS = 7
};

/* aperture kinds: ART/ModuleSupport.py `_IncludeSupport` predicates                                  */
enum ArtSupportKind {
  ART_SUP_ROUND = 0,        /* :68-70    sp = {R}                         */
  ART_SUP_ROUNDHOLE = 1,    /* :151-155  sp = {R, Rhole, cx, cy}          */
  ART_SUP_RECT = 2,         /* :228-230  sp = {X, Y}                      */
  ART_SUP_RECTHOLE = 3,     /* :322-326  sp = {X, Y, Rhole, cx, cy}       */
  ART_SUP_RECTRECTHOLE = 4  /* :431-435  sp = {X, Y, hx, hy, cx, cy}      */
};

/* element flags */
#define ART_FLAG_PERTURBED_NORMAL 1u /* IgnoreDefects=False: reflect off the defect-perturbed normal (ModuleMirror.py:933-936) */
#define ART_FLAG_ZERN_RECURRENCE 2u  /* the element's Zernike tables are in the RECURRENCE layout (any order, below)      */
#define ART_FLAG_GRATING 4u          /* this element is a grating: only art_trace_grating traces it                        */
#define ART_FLAG_QUADRIC 8u          /* this element is a general quadric mirror: only art_trace_quadric traces it         */
#define ART_FLAG_FREEFORM 16u        /* this element is a freeform mirror (quadric + figure): only art_trace_freeform does */

/* Zernike defect table (ART/ModuleDefects.py:149-174), a DEVICE array of doubles per element.  The polynomials
 * of ART/recursive_zernike_generator.py have integer monomial coefficients; the host expands
 *     h(x,y) = sum_nm c_nm Z_nm(x,y) = sum_pq A[p][q] x^p y^q        (x, y = (P - centre) / R)
 * exactly and stores A and its two partial derivatives, so that the kernels evaluate three bivariate Horner
 * schemes instead of carrying the recurrence rows in registers (the coefficients are wave-uniform: they reach the
 * lanes through scalar loads, one copy per wave; entries of total degree > N must be zero).  Layout, for defect d:
 *   base = d * ART_ZERN_STRIDE
 *   [base+0] = R (Support._CircumCirc()),  [base+1] = max total degree N (2..ART_ZERN_MAX_ORDER)
 *   [base+2            + p*ART_ZERN_DIM + q] = A[p][q]        coefficient of x^p y^q of h
 *   [base+2 +   DIM^2  + p*ART_ZERN_DIM + q] = dA/dx [p][q]   = (p+1) A[p+1][q]
 *   [base+2 + 2*DIM^2  + p*ART_ZERN_DIM + q] = dA/dy [p][q]   = (q+1) A[p][q+1]                        */
/* Orders above ART_ZERN_MAX_ORDER (and any order, if the caller prefers): set ART_FLAG_ZERN_RECURRENCE and hand over, per
 * defect, the coefficients themselves -- [R, N, c(0,0), c(1,0), c(1,1), c(2,0), ...], c(n,m) at 2 + n(n+1)/2 + m, absent
 * terms 0, every table of one element padded to the same N <= ART_ZERN_RECURRENCE_MAX_ORDER (stride 2 + (N+1)(N+2)/2).
 * The kernels then run the reference's recurrences per ray (the monomial form is exact but loses 4e-10 of the polynomial
 * to cancellation at order 20 and everything at order 40; the recurrences stay at 1e-15).  Such elements are traced by
 * art_trace_element only (a kernel of its own, with per-lane row storage); art_trace_chain / art_scene_pack return
 * ART_ERR_UNSUPPORTED for them.                                                                                          */
#define ART_ZERN_RECURRENCE_MAX_ORDER 64
#define ART_ZERN_MAX_ORDER 16
#define ART_ZERN_DIM (ART_ZERN_MAX_ORDER + 1)                      /* 17 */
#define ART_ZERN_STRIDE (2 + 3 * ART_ZERN_DIM * ART_ZERN_DIM)      /* 869 */
#define ART_MAX_DEFECTS 16   /* tables (Zernike: one per normalisation radius) / height maps per mirror; the kernels loop */

/* Gridded height-map defect (ART/ModuleDefects.py `Fourrier` :69-146; offset lookup :131-137 through SciPy's
 * RegularGridInterpolator(method="linear")): h[ix * ny + iy] on the regular grid x = x0 + ix*dx, y = y0 + iy*dy,
 * bilinear interpolation, evaluated at (P - centre).  An array of these structs lives in DEVICE memory.
 * Points outside the grid are clamped to the edge cell (SciPy raises there; hits are inside the support, which
 * the grid covers).  Only the offset is used: the reference's Fourrier.get_normal raises under NumPy >= 1.24. */
typedef struct ArtGridDefect {
  const double* h;       /* DEVICE, nx * ny doubles */
  int32_t nx, ny;
  double x0, y0, dx, dy;
} ArtGridDefect;

/* One optical element = optic + pose.  Replaces the per-ray frame changes of
 * ART/ModuleProcessing.py:289-295, :306-309 by two constant 3x3 maps built on the host with the
 * reference's own RotationPoint special cases (ART/ModuleGeometry.py:333-343):
 *     P_optic = fwd * (P_lab - pos) + centre        u_optic = fwd * u_lab
 *     P_lab   = bwd * (P_optic - centre) + pos      u_lab   = bwd * u_optic
 * Callers fill every field except mp[2..3].  Each entry point works on its own copy of the descriptors, in which it
 * replaces bwd, pos and (torus) mp[2..3] by constants derived from the other fields (the two translations folded
 * into one offset per direction, squared radii, ...: csrc/art_device.h prepare_element()); the caller's structs are
 * never written.                                                                                       */
typedef struct ArtElementDesc {
  int32_t kind;          /* ArtOpticKind                                    */
  int32_t support_kind;  /* ArtSupportKind                                  */
  int32_t n_defects;     /* 0..ART_MAX_DEFECTS Zernike defects on a mirror  */
  uint32_t flags;        /* ART_FLAG_*                                      */
  double fwd[9];         /* row-major                                       */
  double bwd[9];         /* informational: the kernels go back through the transpose of fwd (see below) */
  double pos[3];         /* OpticalElement.position                         */
  double centre[3];      /* optic.get_centre() in the optic frame           */
  double sp[6];          /* support parameters                              */
  double mp[4];          /* mirror parameters                               */
  const double* zern;    /* DEVICE pointer, n_defects * ART_ZERN_STRIDE doubles, or NULL */
  const ArtGridDefect* grid; /* DEVICE pointer to n_grid structs, or NULL           */
  int32_t n_grid;        /* 0..ART_MAX_DEFECTS gridded height-map defects           */
  int32_t reserved;
} ArtElementDesc;

/* SoA view of one ray bundle (all DEVICE pointers, length n).  `path` is the running optical path
 * (sum of the reference's Ray.path tuple); `incidence` the incidence angle on the element the ray
 * comes from (Ray.incidence).  Ray.number / intensity / wavelength never change along a chain and are
 * therefore not part of the per-element state (slot i of every bundle is source ray i).
 * Alignment: 8 bytes are enough for correctness; for full throughput every array should start on a cache-line
 * boundary (the package pitches its rows to 512 bytes): rows that start 8 bytes off a line cost about a third of
 * the bandwidth.                                                                                             */
typedef struct ArtBundleView {
  double* ox; double* oy; double* oz;   /* Ray.point  */
  double* dx; double* dy; double* dz;   /* Ray.vector */
  double* path;
  double* incidence;
  uint8_t* alive;                       /* 1 = ray still propagating */
} ArtBundleView;

/* Plane detector (ART/ModuleDetector.py:25-62).  rot = RotationPoint(., normal, ez) as a 3x3 map
 * (ModuleDetector.py:231), built on the host like fwd/bwd.                                            */
typedef struct ArtDetectorDesc {
  double centre[3];
  double normal[3];
  double rot[9];
} ArtDetectorDesc;

int art_abi_version(void);
const char* art_last_error(void);
/* number of visible HIP devices whose architecture is gfx950 (>= 0), or a negative error code */
int art_device_count(void);

/* One element of RayTracingCalculation (ART/ModuleProcessing.py:277-311): frame change, intersection
 * (`_get_intersection` of the optic's class incl. DeformedMirror, ModuleMirror.py:969-980), support test,
 * reflection / mask transmission (ModuleMirror.py:878-939, ModuleMask.py:93-136), frame change back.
 * Reads bundle `in`, writes bundle `out` (may alias `in`).  Slots with in->alive == 0 and rays that
 * miss get out->alive = 0 and their other outputs are left untouched.                                  */
int art_trace_element(const ArtElementDesc* e, const ArtBundleView* in, const ArtBundleView* out,
                      int64_t n, void* stream);

/* Diffraction grating ruled on any undeformed mirror (added under ABI 14: ART_FLAG_GRATING, ArtGratingDesc,
 * art_trace_grating).  The grooves are the intersections of the surface with equally spaced parallel planes: groove
 * number G(P) = N q0.(P - centre) at the hit point P (optic frame), q0 = (q[0], q[1], 0).  Per ray and wavelength, with
 * the unit normal n at P, the incident unit direction u and g = m lambda N q0 (lambda in mm, N in lines per mm):
 *     g_t = g - (g.n) n,  v_t = (u - (u.n) n) + g_t,  s = 1 - |v_t|^2,  v = v_t - sign(u.n) sqrt(s) n
 * s <= 0: the order is evanescent and the ray is lost.  path += the geometric length of the leg, incidence as for a
 * mirror, grooves_out[j][r] = grooves_in[r] + m G(P): the phase of a ray in a coherent analysis is
 * k path + 2 pi grooves (derivation: csrc/art_device.h).  g = 0 (N = 0 or m = 0) is the mirror.
 * ONE launch, one thread per ray: intersection, support test and normal are formed once, then the thread loops over the
 * nw wavelengths and stores one diffracted ray per wavelength into outs[j]: the input is read once, not nw times.
 * Slots dead on input, rays that miss and evanescent orders get alive = 0 in the affected outputs, whose other arrays
 * (and grooves_out) are left untouched there.  outs[j] may alias `in` only when nw == 1.
 * wavelengths_host / outs_host: HOST copies of the DEVICE arrays g->wavelengths / g->outs, read for validation only.
 * Limits: e valid by art_trace_element's rules, without defects, not a mask; | |q|^2 - 1 | <= 1e-12; N finite, >= 0;
 * 1 <= nw <= ART_GRATING_MAX_WAVELENGTHS; every wavelength finite and > 0; views complete when n > 0:
 * ART_ERR_BAD_ARG otherwise; 0 <= n <= 2^28 (ART_ERR_UNSUPPORTED beyond); nothing is launched on failure.
 * art_trace_element, art_trace_chain(_readout), art_scene_pack and art_trace_guides return ART_ERR_UNSUPPORTED for an
 * element with ART_FLAG_GRATING set.                                                                                  */
#define ART_GRATING_MAX_WAVELENGTHS 1024
typedef struct ArtGratingDesc {
  double q[2];                  /* q0: unit vector in the optic's xy plane, the direction of dispersion   */
  double lines_per_mm;          /* N >= 0, finite                                                         */
  int32_t order;                /* m                                                                      */
  int32_t nw;                   /* 1 .. ART_GRATING_MAX_WAVELENGTHS                                       */
  const double* wavelengths;    /* DEVICE, nw doubles (mm)                                                */
  const ArtBundleView* outs;    /* DEVICE, nw views: the diffracted bundle per wavelength                 */
  double* grooves_in;           /* DEVICE, n doubles, or NULL (= 0): the groove count each ray arrives with */
  double* grooves_out;          /* DEVICE, [nw][n] doubles, or NULL                                       */
} ArtGratingDesc;
int art_trace_grating(const ArtElementDesc* e, const ArtGratingDesc* g, const double* wavelengths_host,
                      const ArtBundleView* outs_host, const ArtBundleView* in, int64_t n, void* stream);

/* General quadric mirror (added under ABI 14: ART_FLAG_QUADRIC, ArtQuadricDesc, art_trace_quadric): the conics the six
 * kinds above lack -- plane-elliptical, parabolic and hyperbolic cylinders (Kirkpatrick-Baez pairs), hyperboloids
 * (Wolter pairs, Cassegrain secondaries) -- and any other surface of second degree.  In the optic frame
 *     F(P) = q[0] x^2 + q[1] y^2 + q[2] z^2 + 2 q[3] xy + 2 q[4] xz + 2 q[5] yz + 2 b.P + c = 0 .
 * Per ray, with P = A + t u: the roots of (u^T Q u) t^2 + 2 u.(Q A + b) t + F(A) by the cancellation-free quadratic of
 * the other kinds (a vanishing leading coefficient -- a ray parallel to a parabola's axis -- gives the one root -c/b).
 * A root counts when t > 1e-12, dF/dz < 0 at the hit (the sheet that faces +z) and the support contains
 * (x - centre[0], y - centre[1]); one candidate: it; two: the closer, the later one on a tie; none: the ray is lost.
 * Normal n = -grad F / |grad F|, reflection v = u - 2 (u.n) n, path += t, incidence as for every mirror.  No defects.
 * Write the surface in the mirror's own pole frame -- origin on the surface (c = 0), grad F(0) = 2 b = (0, 0, -1) -- as
 * ModuleMirror.MirrorConic does: F(A) then does not cancel, and |grad F| is of order 1, which the kernel's reciprocal
 * square root assumes (ordinary magnitudes: no scaling against overflow or denormals).
 * e->kind is ART_PLANE by convention and ignored; e->mp is unused.  Reads `in`, writes `out` (may alias `in`); slots
 * dead on input and rays that miss get alive = 0 and their other outputs are left untouched.  Any n >= 0 (chunked like
 * art_trace_element).  ART_ERR_BAD_ARG: NULL pointers, an invalid element (art_trace_element's rules), defects on the
 * element, a non-finite coefficient, q and b all zero, n < 0, an incomplete view with n > 0.
 * art_trace_element, art_trace_grating, art_trace_chain(_readout), art_scene_pack and art_trace_guides return
 * ART_ERR_UNSUPPORTED for an element with ART_FLAG_QUADRIC set.                                                       */
typedef struct ArtQuadricDesc {
  double q[6];                  /* xx, yy, zz, xy, xz, yz (the off-diagonal entries of the symmetric matrix, not doubled) */
  double b[3];
  double c;
} ArtQuadricDesc;
int art_trace_quadric(const ArtElementDesc* e, const ArtQuadricDesc* q, const ArtBundleView* in,
                      const ArtBundleView* out, int64_t n, void* stream);

/* Freeform and aspheric mirrors (added under ABI 14: ART_FLAG_FREEFORM, ArtFigureDesc, art_trace_freeform): a quadric base
 * in its pole frame (ArtQuadricDesc as above: origin on the surface, +z its normal there) plus a polynomial height figure
 *     z = sag_base(x, y) + h(x, y),    h = sum_{p+q<=N} a_pq (x/R)^p (y/R)^q  in mm,  N <= ART_ZERN_MAX_ORDER ,
 * implicitly Phi(P) = F(x, y, z - h(x, y)) = 0.  Positive h is a bump towards the incoming light.  Figure errors of
 * nanometres on a KB or Wolter mirror and aspheric departures of millimetres (an even asphere, a corrector plate) are the
 * same code: the ray is intersected with Phi exactly, by Newton's iteration, not by a first-order slide.
 * The figure is ONE table in the dense layout of the Zernike defects above (ART_ZERN_STRIDE doubles in DEVICE memory:
 * [R, N, A, dA/dx, dA/dy], evaluated at the pole-frame (x, y), no centre subtracted), which holds any polynomial of total
 * degree <= 16; ArtFigureDesc carries its device address and host copies of R and N for the validation.
 * Per ray, with P = A + t u: the candidates are the base's roots with t > 1e-12 and dF/dz < 0 (art_trace_quadric's tests
 * other than the support), in increasing t.  Each is refined by Newton on phi(t) = Phi(A + t u): dt = -phi / phi',
 * phi' = grad Phi . u, grad Phi = (F_x - F_z h_x, F_y - F_z h_y, F_z) at P' = (x, y, z - h), with F evaluated at P'.
 * Convergence: |dt| <= 1e-13 * max(1, |t|) within at most 12 steps (tau = 1e-13, K = 12; Newton converges quadratically,
 * so the accepted t is exact to rounding: typical figures take 2 to 5 steps).  A converged candidate is the hit when its
 * t is still > 1e-12, Phi_z < 0 there and the support contains the REFINED (x - centre[0], y - centre[1]); otherwise the
 * other candidate, if any, is refined and tested the same way; a candidate that does not converge is given up; no hit:
 * the ray is lost.  Normal n = -grad Phi / |grad Phi|; reflection, incidence, path += t as for art_trace_quadric, whose
 * outcome a zero figure reproduces.
 * e->kind is ART_PLANE by convention and ignored; e->mp is unused.  Reads `in`, writes `out` (may alias `in`); slots dead
 * on input and lost rays get alive = 0 and their other outputs are left untouched.  Any n >= 0 (chunked like
 * art_trace_element).  ART_ERR_BAD_ARG, before any device work: NULL pointers, an invalid element (art_trace_element's
 * rules), an element that also carries defects, ART_FLAG_GRATING or ART_FLAG_QUADRIC, a non-finite coefficient, q and b all
 * zero, a NULL table, an order outside [0, 16], a radius that is not finite and positive, n < 0, an incomplete view with
 * n > 0.  art_trace_element, art_trace_grating, art_trace_quadric, art_trace_chain(_readout), art_scene_pack and
 * art_trace_guides return ART_ERR_UNSUPPORTED for an element with ART_FLAG_FREEFORM set.                              */
typedef struct ArtFigureDesc {
  const double* table;          /* DEVICE: ART_ZERN_STRIDE doubles, dense layout; table[0] = radius, table[1] = order        */
  double radius;                /* host copy of table[0]: R > 0                                                              */
  int32_t order;                /* host copy of table[1]: N in [0, ART_ZERN_MAX_ORDER]; entries of degree > N are zero       */
  int32_t reserved;
} ArtFigureDesc;
int art_trace_freeform(const ArtElementDesc* e, const ArtQuadricDesc* q, const ArtFigureDesc* figure, const ArtBundleView* in,
                       const ArtBundleView* out, int64_t n, void* stream);

/* Whole chain in ONE launch: the ray stays in registers from element to element.  outs[k] receives the
 * bundle after element k for every k with outs[k].alive != NULL (pass zeroed views to skip history);
 * outs[n_elems-1] is mandatory.  Same results as n_elems calls of art_trace_element for every slot that is alive in
 * the respective bundle; the other outputs of a DEAD slot are unspecified (untouched, or the ray's last live state:
 * the fused kernels store pairs of neighbouring slots with one 16-byte access).                          */
int art_trace_chain(const ArtElementDesc* elems, int32_t n_elems, const ArtBundleView* in,
                    const ArtBundleView* outs, int64_t n, void* stream);

/* The same launch with the detector read-out of the LAST bundle fused behind it (art_detector_readout's outputs and
 * statistics, ART/ModuleDetector.py:191-279): the ray is still in registers when it reaches the detector, so the
 * read-out costs its 24 B/ray of outputs instead of a second pass that re-reads 57 B/ray.  For a detector that is known
 * before the trace (manual placement, a re-trace, a scan).  Per-workgroup partial statistics go to `scratch`
 * (art_chain_readout_scratch_doubles(n) doubles, DEVICE) and are folded into out24 by a second tiny launch; the fold
 * order differs from art_detector_readout's, so sums agree with it to rounding (minima, maxima and counts exactly).
 * One launch's limit applies: n <= 2^28 (ART_ERR_UNSUPPORTED beyond; use the two separate calls).                   */
typedef struct ArtChainReadout {
  ArtDetectorDesc det;
  const double* w;       /* DEVICE weights (Ray.intensity) or NULL (w = 1)                          */
  double cx, cy, co;     /* provisional centres of the second moments, as in art_detector_readout   */
  double* X;             /* DEVICE, n doubles each, or all three NULL (statistics only)              */
  double* Y;
  double* opl;
  double* scratch;       /* DEVICE, art_chain_readout_scratch_doubles(n) doubles                    */
  double* out24;         /* DEVICE, 24 doubles: slot layout of art_detector_readout                 */
  int32_t lite;          /* 1: only count [0], sum opl [1], bounding box [2..5] and path range [12..13] are formed -- what
                            Detector.get_Delays / get_PointList2DCentre consume (ART/ModuleDetector.py:236-279); the sums
                            [6..11] and the second moments [16..21] read 0 and the weights `w` are not touched.  The tail
                            then costs 8 instead of 22 statistics per ray.  0: all 22 (default)     */
  int32_t sums;          /* 1: NO read-out -- the tail forms pass (1) of art_analyse_bundles for the last bundle instead, while the
                            ray is still in registers: out24[0..8] = count, sum point (3), sum vector (3), sum w (= count if w is
                            NULL), sum path; out24[9..23] = 0.  `det`, cx, cy, co are ignored, X / Y / opl must be NULL and lite 0.
                            For a detector that is NOT known before the trace (Detector.autoplace needs exactly these sums,
                            ART/ModuleDetector.py:109-137): hand out24 to ArtAnalysisJob.sums and the analysis of the bundle is
                            placement + ONE pass.  Same bits as the sums art_analyse_bundles forms itself (one canonical fold
                            order: tiles of 256 slots).  0 (default): a read-out                    */
} ArtChainReadout;
int64_t art_chain_readout_scratch_doubles(int64_t n);
int art_trace_chain_readout(const ArtElementDesc* elems, int32_t n_elems, const ArtBundleView* in,
                            const ArtBundleView* outs, const ArtChainReadout* readout, int64_t n, void* stream);

/* MANY chains in ONE launch (ART/ModuleProcessing.py:203-239: OEPlacement with a list-valued argument returns 10-11
 * chains that differ only in poses, which ARTmain.py:304-342 traces one after the other; the misalignment loop lists of
 * ART/ModuleOpticalChain.py:371-657 likewise).  All chains have n_elems elements and bundles of n slots.  The
 * descriptors do not fit kernel arguments, so they travel as a SCENE IMAGE in device memory:
 *   1. art_scene_bytes(n_chains, n_elems)      size of the image;
 *   2. art_scene_pack(...)                     fills a HOST buffer of that size -- pure host code, no HIP call;
 *                                              elems[c * n_elems + k], ins[c], outs[c * n_elems + k] (rules of
 *                                              art_trace_chain: outs[..].alive == NULL skips that history bundle, the
 *                                              last view of a chain and every 8th are mandatory); readouts = NULL or
 *                                              one ArtChainReadout per chain (fused read-out of each chain's last
 *                                              bundle, see art_trace_chain_readout).  Returns the scene's flags >= 0
 *                                              (bit 0: defects, bit 1: read-outs; informational -- they are also in
 *                                              the image's header), or a negative error code;
 *   3. the caller copies the image to DEVICE memory (its own allocation and memcpy);
 *   4. art_trace_scene(image_dev, image_host, n, stream)
 *                                              ONE kernel launch per 8 elements: grid.y = chain, grid.x = 256-ray tile.
 *                                              Chain count, element count and flags are read from the header of
 *                                              `image_host` (the packed host buffer image_dev is a copy of; it must stay
 *                                              valid until the call returns), never taken from the caller.
 * A launch reads nothing but the device image and the bundles: re-packing new poses into the same device buffer and
 * replaying a captured HIP graph re-traces a modified scene without host-side launch work.  Same per-ray results as
 * art_trace_chain, bit for bit.                                                                                      */
int64_t art_scene_bytes(int32_t n_chains, int32_t n_elems);
int art_scene_pack(const ArtElementDesc* elems, int32_t n_chains, int32_t n_elems, const ArtBundleView* ins,
                   const ArtBundleView* outs, const ArtChainReadout* readouts, void* image_host);
int art_trace_scene(const void* image_dev, const void* image_host, int64_t n, void* stream);

/* ROW SUMMARIES: a scene launch need not read the rows of its input that hold ONE value in every slot.  A generated
 * source repeats a value n times in most of the nine per-slot rows a fused trace reads (a point source: ox, oy, oz,
 * path, alive and a uniform intensity; a plane source: dx, dy, dz, path, alive, intensity -- 41 of 65 bytes per ray).
 *   art_row_summary_bytes                      size of one summary (a small device-only record: a mask, the slot count it
 *                                              was formed over, nine 8-byte patterns);
 *   art_bundle_row_summary                     one memset + ONE streaming kernel over in's ox..dz, path, alive and w (the
 *                                              weights the chain's read-out will use, or NULL) that writes the summary
 *                                              to summary_dev (DEVICE).  A row is constant iff every slot's BIT PATTERN
 *                                              equals slot 0's: -0.0 differs from +0.0, a row of one NaN pattern is
 *                                              constant.  n == 0 or a NULL row: not constant.  Deterministic (one
 *                                              integer atomic OR per workgroup); nothing returns to the host.
 *   art_scene_set_row_summaries                stores the DEVICE pointer to an array of n_chains summaries -- entry c
 *                                              formed over ins[c] and readouts[c].w -- in the HOST image's header
 *                                              (spare words: no layout changes, art_scene_bytes is what it was);
 *                                              NULL detaches.  art_scene_pack clears it: attach after packing.
 * art_trace_scene hands the pointer to its one-ray kernels, which give a constant row a zero-length buffer descriptor
 * (no memory traffic) and take its value from the summary: same results, bit for bit.  A summary is used only if the
 * slot count it was formed over covers the launch; the two-rays-per-lane bodies (masked chains, shared inputs) and
 * art_trace_chain ignore summaries.  The caller keeps a summary in step with its bundle: whenever the arrays or the
 * weights change, art_bundle_row_summary runs again into the same buffer, on the stream, ahead of the next launch (a
 * captured graph keeps the buffer's address).  ART_ROW_SUMMARY=0 in the environment, read at every launch, makes
 * art_trace_scene ignore attached summaries.                                                                          */
int64_t art_row_summary_bytes(void);
int art_bundle_row_summary(const ArtBundleView* in, const double* w, int64_t n, void* summary_dev, void* stream);
int art_scene_set_row_summaries(void* image_host, const void* summaries_dev);

/* Bundle from array-of-structs input (the layout a caller holding ART Ray lists / (n,3) NumPy arrays has):
 * points[n][3], vectors[n][3] (DEVICE, row-major) -> SoA view; directions normalised like the Ray.vector setter
 * (ART/ModuleOpticalRay.py:85-90), path = path0[i] (or 0 if NULL), incidence = NaN, alive = 1.                      */
int art_pack_rays(const double* points, const double* vectors, const double* path0, int64_t n,
                  const ArtBundleView* out, void* stream);

/* Rigid / affine map of a whole bundle: TranslationRayList, RotationRayList, RotationAroundAxisRayList
 * (ART/ModuleGeometry.py:308-314, :372-391) -- used by the source (mis-)alignment helpers, not by tracing:
 *   point' = (rotate_points ? M * point : point) + T,   vector' = normalize(M * vector);
 * path, incidence and alive are copied.  M row-major.  `out` may alias `in`.                                        */
int art_transform_bundle(const double M[9], const double T[3], int32_t rotate_points, const ArtBundleView* in,
                         const ArtBundleView* out, int64_t n, void* stream);

/* Detector read-out (ART/ModuleDetector.py:191-234, :272-275): for every alive ray
 *   I = IntersectionLinePlane (ModuleGeometry.py:48-57);  (X,Y) = first two components of rot*(I-centre);
 *   opl = |A - I| + path.  Any of p3x..p3z / X,Y / opl may be NULL to skip that output.               */
int art_detector(const ArtDetectorDesc* d, const ArtBundleView* b, int64_t n,
                 double* p3x, double* p3y, double* p3z, double* X, double* Y, double* opl, void* stream);

/* Read-out and statistics in ONE pass over the bundle (what Detector.readout uses): the outputs of art_detector
 * plus, accumulated while the values are still in registers, the statistics of art_detector_stats in out24[0..15]
 * and second moments about provisional centres (cx, cy, co) in out24[16..23]:
 *   [16] sum (X-cx)^2  [17] sum (Y-cy)^2  [18] sum (opl-co)^2
 *   [19] sum w (X-cx)^2 [20] sum w (Y-cy)^2 [21] sum w (opl-co)^2  [22..23] 0
 * Variances follow as E[(x-c)^2] - (E[x]-c)^2; with c within a few standard deviations of the mean (cx = cy = 0 is
 * the detector centre, co an estimate of the mean path) the cancellation is harmless.  w = weights or NULL (w = 1).
 * out24: DEVICE, 24 doubles.  scratch: DEVICE, art_reduce_scratch_doubles() doubles.                              */
int art_detector_readout(const ArtDetectorDesc* d, const ArtBundleView* b, const double* w, int64_t n, double cx,
                         double cy, double co, double* p3x, double* p3y, double* p3z, double* X, double* Y,
                         double* opl, double* scratch, double* out24, void* stream);

/* Moments for a detector SCAN along its normal (autofocus, ART/ModuleProcessing.py:317-460).  For a detector shifted
 * by s along -normal (Detector.shiftByDistance(s)) every ray's read-out is exactly linear in s:
 *     X(s) = X0 + s*sx,  Y(s) = Y0 + s*sy,  opl(s) = opl0 + s*so,   so = -1/(u.normal), (sx, sy) = rot*(so*u + normal)
 * so the spot-size and duration variances at ANY s follow from global sums of per-ray products: one pass over the
 * bundle replaces one pass per scan position.  The path is centred for conditioning: O = opl0 - co, sO = so - 1.
 * out33 (DEVICE, 33 doubles), first block with weight 1, second block (+16) with weight w (= 1 if w is NULL):
 *   [0] sum 1   then for q in (X, Y, O), base = 1 + 5*k:  [base] sum q0  [base+1] sum sq  [base+2] sum q0^2
 *   [base+3] sum q0*sq  [base+4] sum sq^2
 *   [32] number of alive rays whose hit point changes side of the ray origin (t changes sign) for some shift in
 *        [0, span] (span may be negative): the reference's path |I - A| + sum(path) (ModuleDetector.py:272-275) has a
 *        kink there, so if [32] > 0 the moments describe shift 0 exactly but not the whole scan -- the caller
 *        then evaluates the scan positions one by one (a detector scanned through the last optic).            */
int art_detector_scan_moments(const ArtDetectorDesc* d, const ArtBundleView* b, const double* w, int64_t n, double co,
                              double span, double* scratch, double* out33, void* stream);

/* N-D histogram (N = 1..3) of the ALIVE rays of one bundle, deterministic: integer accumulation only.
 * Coordinates, by source:
 *   ART_HIST_DETECTOR: axis ART_HAXIS_X / _Y = (X, Y) of art_detector on `map`; ART_HAXIS_DELAY =
 *                      ((opl - delay_centre) / 299792458000.0) * 1e15 (fs, Detector.get_Delays' expression);
 *   ART_HIST_FRAME:    axis k = component k of map.rot * (P - map.centre), P the ray's point (art_transform_bundle).
 * Bins: edges_k = numpy.linspace(lo_k, hi_k, bins_k + 1) exactly (edge i = i*step + lo, step = (hi - lo)/bins, the
 * last edge hi); v is in bin j iff edge[j] <= v < edge[j+1], v == hi in the last bin; v < lo, v > hi or NaN is
 * OUTSIDE.  counts / wsums are row-major, axis 0 slowest (numpy.histogramdd's layout).
 * Weights: q_i = (int64) rint(ldexp(w_i, wshift)) (half to even); w = NULL: q_i = 0.  The caller picks wshift so that
 * no sum overflows int64 (e.g. wshift = 62 - ceil(log2(n_total + 1)) - E with max|w| < 2^E) and w must be finite.
 * Outputs (DEVICE, int64): counts[prod bins], wsums[prod bins] (may be NULL when w is NULL),
 *   totals4: [0] binned alive rays [1] alive rays outside (or with a non-finite coordinate) [2] sum q binned
 *            [3] sum q outside.
 * accumulate = 0: the outputs are zeroed on the stream first; 1: the call adds to them (integers: exact across calls).
 * Limits: ndim 1..3, bins_k >= 1, prod bins <= 2^24 (ART_ERR_UNSUPPORTED), lo < hi finite with a finite, non-zero
 * step, no DELAY axis on the FRAME source, wshift in [-1074, 1074]: ART_ERR_BAD_ARG otherwise, with nothing launched. */
enum ArtHistSource { ART_HIST_DETECTOR = 0, ART_HIST_FRAME = 1 };
enum ArtHistAxis { ART_HAXIS_X = 0, ART_HAXIS_Y = 1, ART_HAXIS_DELAY = 3 };   /* DETECTOR axes (2 is not one) */
#define ART_HIST_MAX_BINS (1 << 24)
typedef struct ArtHistogramDesc {
  int32_t source, ndim;
  int32_t axis[3];        /* DETECTOR: ArtHistAxis;  FRAME: component 0/1/2 of rot * (P - centre)          */
  int32_t bins[3];
  int32_t wshift;         /* the fixed-point shift of the weights                                          */
  int32_t reserved;
  double lo[3], hi[3];
  double delay_centre;    /* the optical path the DELAY axis is measured from                              */
  ArtDetectorDesc map;    /* DETECTOR: the detector;  FRAME: rot = M, centre = T                           */
} ArtHistogramDesc;
int art_histogram(const ArtHistogramDesc* h, const ArtBundleView* b, const double* w, int64_t n, int32_t accumulate,
                  int64_t* counts, int64_t* wsums, int64_t* totals4, void* stream);

/* Coherent focal field of the ALIVE rays of one bundle on a pixel grid of up to 64 planes (the Debye / angular-spectrum
 * picture: every ray is a local plane wave).  With e1, e2 = rows 0 and 1 of det.rot, n = det.normal, C = det.centre:
 *     x_qjl    = C + shift[q] n + X_j e1 + Y_l e2,     X_j = x0 + j*dx,  Y_l = y0 + l*dy
 *     E_q[l,j] = sum_r sqrt(w_r) exp(i k [(path_r - L_ref) + d_r . (x_qjl - p_r)])
 * p_r, d_r, path_r the ray's point, direction and path; w_r = w[r] (w = NULL: 1); dead slots contribute nothing.  At
 * a ray's own hit point the phase is k (opl_r - L_ref), opl_r the value of art_detector.  The phase is separated as
 *     base_r = k * ((path_r - L_ref) + ((d_x (C_x - p_x) + d_y (C_y - p_y)) + d_z (C_z - p_z)))   (this order, no fma)
 *     phase  = base_r + shift[q] * k (d.n) + X_j * k (d.e1) + Y_l * k (d.e2)
 * field (DEVICE, complex128 = (re, im) doubles, [planes][ny][nx]) is written, not added to; n = 0 writes zeros.  The
 * sum runs in a fixed order (no float atomics): the same bytes on every call with the same arguments.
 * scratch: DEVICE, art_focal_scratch_doubles(nx, ny, planes, n) doubles.
 * Limits: 1 <= nx, ny <= ART_FOCAL_MAX_PIXELS, 1 <= planes <= ART_FOCAL_MAX_PLANES, k > 0 finite, dx, dy and the
 * shifts finite, field and scratch non-NULL when n > 0: ART_ERR_BAD_ARG otherwise, with nothing launched and field
 * untouched. */
#define ART_FOCAL_MAX_PIXELS 2048
#define ART_FOCAL_MAX_PLANES 64
typedef struct ArtFocalDesc {
  ArtDetectorDesc det;
  double k;               /* 2 pi / wavelength, 1/mm                                                       */
  double L_ref;           /* the optical path of phase 0                                                   */
  double x0, dx;          /* pixel centres X_j = x0 + j*dx, detector coordinates (mm)                      */
  double y0, dy;
  int32_t nx, ny;
  int32_t planes;
  int32_t reserved;
  double shift[ART_FOCAL_MAX_PLANES];   /* plane q lies at C + shift[q] * det.normal                      */
} ArtFocalDesc;
int64_t art_focal_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int64_t n);
int art_focal_field(const ArtFocalDesc* f, const ArtBundleView* b, const double* w, int64_t n, double* scratch,
                    double* field, void* stream);

/* Focal fields of one bundle at nk wavenumbers (v14): the space-time field of a broadband pulse follows from them by a
 * Fourier sum (attosecondraytracing_amd/pulse.py).  The optics are mirrors, achromatic, so one traced bundle serves
 * every wavenumber; only the phase changes.  With k_j = f.k + j * dk (formed so, unfused: k_0 == f.k exactly):
 *     field[q][j] = E_q of art_focal_field with k replaced by k_j,   j = 0 .. nk-1
 * in the same phase separation and operation order:
 *     base_r / k = (path_r - L_ref) + ((d_x (C_x - p_x) + d_y (C_y - p_y)) + d_z (C_z - p_z))   (this order, no fma)
 *     base_r     = k_j * (base_r / k),   k (d.e1) = k_j * (d.e1), ...  (each one rounding, as art_focal_field's k * (...))
 * so that nk = 1 gives art_focal_field's bytes and slice j equals art_focal_field at f.k = k_j to rounding.
 * field (DEVICE, complex128, [planes][nk][ny][nx]) is written, not added to; n = 0 writes zeros.  Fixed summation
 * order (no float atomics): the same bytes on every call with the same arguments.
 * scratch: DEVICE, art_focal_spectrum_scratch_doubles(nx, ny, planes, nk, n) doubles.
 * Limits: all of art_focal_field's, and 1 <= nk <= ART_FOCAL_MAX_WAVENUMBERS, dk finite, every k_j finite and > 0,
 * planes * nk <= 65535: ART_ERR_BAD_ARG otherwise, with nothing launched and field untouched. */
#define ART_FOCAL_MAX_WAVENUMBERS 1024
typedef struct ArtFocalSpectrumDesc {
  ArtFocalDesc f;         /* grid, planes, detector, L_ref; f.k = k_0, the wavenumber of slice 0             */
  double dk;              /* k_j = f.k + j * dk (1/mm)                                                     */
  int32_t nk;
  int32_t reserved;
} ArtFocalSpectrumDesc;
int64_t art_focal_spectrum_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int32_t nk, int64_t n);
int art_focal_spectrum(const ArtFocalSpectrumDesc* s, const ArtBundleView* b, const double* w, int64_t n,
                       double* scratch, double* field, void* stream);

/* Focal fields of one bundle from a CHROMATIC source (added under ABI 14: ArtFocalChromaticDesc, art_focal_chromatic,
 * art_focal_chromatic_scratch_doubles): art_focal_spectrum's sum with an amplitude and a phase per ray AND wavenumber,
 * for sources (high harmonics) whose divergence and apparent position along the axis depend on the frequency.
 * b is the bundle at focus, src the SOURCE bundle it was traced from, slot-aligned (slot r of src became slot r of b);
 * only src's directions s_r are read.  With the unit vector `axis` = a, per slot
 *     u_r = 0.5 * (((s_x - a_x)^2 + (s_y - a_y)^2) + (s_z - a_z)^2)       (this order, no fma)
 * which is 1 - cos(angle between s_r and a) without cancellation, and per wavenumber j a table row of four doubles
 *     (k_j, c_j, z_j, 0):  k_j > 0 the wavenumber (1/mm; ANY list, not a progression), c_j >= 0 the apodisation,
 *                          z_j (mm) the offset of that wavenumber's apparent source along a, positive downstream,
 *     field[q][j][l][i] = sum_r sqrt(w_r) exp(-(u_r c_j)) exp(i [k_j * (base_r / k + z_j * u_r) + shift, X and Y terms])
 * base_r / k and the shift, X and Y terms exactly art_focal_spectrum's, in its operation order; z_j * u_r and the sum
 * base_r / k + z_j * u_r are each one rounding (no fma), and the amplitude is sqrt(w_r) * exp(-(u_r * c_j)).
 * k_j z_j u_r is the phase of a spherical wave centred at S + z_j a relative to one centred at the source point S, its
 * on-axis constant dropped; exp(-u c_j) with c_j = 2 / Theta_j^2 is a Gaussian beam whose intensity falls to 1/e^2 at
 * the half-angle Theta_j.  The rays are NOT re-traced: the model is first order in z_j over the distance to the first
 * optic, has one axis, Gaussian apodisation only, and sums the scalar field only.
 * A row with c_j = 0 and z_j = 0 adds +0.0 and multiplies by exp(-0) = 1: with k_j = f.k + j * dk formed as
 * art_focal_spectrum forms them, the table gives that function's bytes.
 * A dead slot of b contributes nothing, whatever it or the slot of src holds (NaN included).
 * table_dev: DEVICE, 4 * nk doubles; table_host: the same values on the HOST, which the validation reads (the device
 * copy is never read back).  field (DEVICE, complex128, [planes][nk][ny][nx]) is written, not added to; n = 0 writes
 * zeros.  Fixed summation order (no float atomics): the same bytes on every call with the same arguments.
 * scratch: DEVICE, art_focal_chromatic_scratch_doubles(nx, ny, planes, nk, n) doubles (-1 on arguments out of range).
 * Limits: all of art_focal_field's on f (f.k is checked but not used: the table holds the wavenumbers),
 * 1 <= nk <= ART_FOCAL_MAX_WAVENUMBERS, planes * nk <= 65535, | |axis| - 1 | <= 1e-12, table_host non-NULL, every k_j
 * finite and > 0, every c_j finite and >= 0, every z_j finite, table_dev and src's arrays non-NULL when n > 0:
 * ART_ERR_BAD_ARG otherwise, with nothing launched and field untouched. */
typedef struct ArtFocalChromaticDesc {
  ArtFocalDesc f;         /* grid, planes, detector, L_ref: art_focal_field's; f.k only checked                    */
  double axis[3];         /* a: the unit axis of the source                                                        */
  int32_t nk;             /* rows of the table                                                                     */
  int32_t reserved;
} ArtFocalChromaticDesc;
int64_t art_focal_chromatic_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int32_t nk, int64_t n);
int art_focal_chromatic(const ArtFocalChromaticDesc* d, const ArtBundleView* b, const ArtBundleView* src, const double* w,
                        int64_t n, const double* table_dev, const double* table_host, double* scratch, double* field,
                        void* stream);

/* Wavefront aberrations of MANY bundles in one call (added under ABI 14: ArtWavefrontJob, art_wavefront,
 * art_wavefront_scratch_doubles).  Per job, with C = det.centre, e1, e2 = rows 0, 1 of det.rot, n = det.normal (the
 * frame of art_focal_field):
 *   reference point  R = C + X e1 + Y e2 - s n       (ref = {X, Y, s}: pixel (X, Y) of art_focal_field in the plane
 *                                                     of shift -s, i.e. Detector.shiftByDistance(s); formed on the
 *                                                     device as ((C + X e1) + Y e2) - s n, unfused: ref = 0 gives C)
 *   wavefront error  W_r = (path_r - L_ref) + ((d_x (R_x - p_x) + d_y (R_y - p_y)) + d_z (R_z - p_z))
 *                    (k_focal_prep's order, no fma: k W_r is art_focal_field's phase of ray r at R, to rounding)
 *   pupil            x_r = (d.e1 - a1) / rho,  y_r = (d.e2 - a2) / rho,   d.e = (d_x e_x + d_y e_y) + d_z e_z
 *                    pupil = {a1, a2, rho}; rho = 0: the largest sqrt((d.e1 - a1)^2 + (d.e2 - a2)^2) over the alive
 *                    rays, found on the device (1 if that is 0).  With an explicit rho a ray with x^2 + y^2 > 1 is not
 *                    used and counted `outside`; with the computed one no ray is outside.
 *   row              v_r = [Z_0 .. Z_{J-1}, d.n, W_r],  K = J + 2 columns, J = (N+1)(N+2)/2, N = order
 *                    Z_j: the unnormalised Zernike polynomials of ART/recursive_zernike_generator.py (Andersen 2018)
 *                    at (x_r, y_r), j = N'(N'+1)/2 + m for the key (N', m) (Z_0 = 1, Z_1 = y, Z_2 = x)
 *   weights          w_r = w[r] (w = NULL: 1) for the USED rays (alive and not outside), 0 for every other slot
 * out (DEVICE, ART_WAVEFRONT_DOUBLES doubles, written):
 *   [0] rays used  [1] rays outside  [2] sum w  [3] rho used  [4] min W  [5] max W  (over the used rays)
 *   [6] K  [7] 0  [8 + i K - i (i - 1) / 2 + (j - i)] = G[i][j] = sum_r w_r v_r[i] v_r[j]  for 0 <= i <= j < K
 * A job with no used ray (n = 0, all slots dead, all outside) gets 0 in [0], [2..5] and G.  Per-ray outputs (optional,
 * DEVICE, n doubles each, NULL to skip): opd[r] = W_r, pupil_x[r] = x_r, pupil_y[r] = y_r for used slots, NaN for the others.
 * Three launches per call (prep over all jobs, the Gram sums per run of jobs of one order, the fold over all jobs); fixed
 * summation order, no float atomics, and a job's slicing depends on its own n and order only: every job gets the same
 * bytes whichever jobs share its call.  jobs_dev: DEVICE copy of the HOST array jobs_host (read for validation and the
 * launch plan; both must hold the same contents).  scratch: DEVICE, art_wavefront_scratch_doubles(jobs_host, n_jobs).
 * Limits: 1 <= n_jobs <= 65535, 0 <= n <= 2^28, 0 <= order <= ART_WAVEFRONT_MAX_ORDER, out non-NULL, finite ref,
 * L_ref and pupil, rho >= 0, views complete when n > 0: ART_ERR_BAD_ARG (ART_ERR_UNSUPPORTED for n) otherwise, with
 * nothing launched.                                                                                                    */
#define ART_WAVEFRONT_MAX_ORDER 10
#define ART_WAVEFRONT_MAX_COLS 68         /* K at ART_WAVEFRONT_MAX_ORDER                                              */
#define ART_WAVEFRONT_DOUBLES 2360        /* 8 + K (K + 1) / 2 at K = 68, padded                                       */
typedef struct ArtWavefrontJob {
  ArtDetectorDesc det;
  ArtBundleView b;
  const double* w;        /* DEVICE weights (Ray.intensity) or NULL (w = 1)                                         */
  int64_t n;              /* slots of b                                                                             */
  double ref[3];          /* X, Y, s of the reference point R (mm)                                                  */
  double L_ref;           /* the optical path of W = 0                                                              */
  double pupil[3];        /* a1, a2 (direction cosines), rho (0 = computed)                                         */
  int32_t order;          /* N, 0 .. ART_WAVEFRONT_MAX_ORDER                                                        */
  int32_t reserved;
  double* opd;            /* DEVICE, n doubles, or NULL                                                             */
  double* pupil_x;        /* DEVICE, n doubles, or NULL                                                             */
  double* pupil_y;        /* DEVICE, n doubles, or NULL                                                             */
  double* out;            /* DEVICE, ART_WAVEFRONT_DOUBLES doubles                                                  */
} ArtWavefrontJob;
int64_t art_wavefront_scratch_doubles(const ArtWavefrontJob* jobs_host, int32_t n_jobs);
int art_wavefront(const ArtWavefrontJob* jobs_dev, const ArtWavefrontJob* jobs_host, int32_t n_jobs, double* scratch,
                  void* stream);

/* Mirror coatings and polarisation of MANY traced chains in one call (added under ABI 14: ArtCoatingMaterial,
 * ArtCoatingLayer, ArtCoating, ArtPolarisationJob, art_polarisation, art_polarisation_scratch_doubles).  One streaming
 * pass over a chain's existing history; the tracing kernels are not involved.  Time dependence exp(-i w t).
 * Per ray and reflecting element, with d_in, d_out the unit directions before and after it (views[e], views[e + 1]):
 *   n = normalize(d_out - d_in), cos t = |d_out - d_in| / 2
 *   s = normalize(d_in x d_out) (|d_in x d_out| < 1e-12: normalize(d_in x a), a the lab axis of d_in's smallest
 *   |component|, the first of equals), p_in = d_in x s, p_out = d_out x s
 *   E' = rs (E.s) s + rp (E.p_in) p_out           (bilinear dot products, no conjugation)
 * A mask (coating index -1) leaves E unchanged.  rs, rp of a coating: N = n + i kappa per material, medium 0 vacuum,
 * layers 1..L top down, L + 1 the substrate, kz_j = k sqrt(N_j^2 - 1 + cos^2 t) with Im kz_j >= 0, k = 2 pi / wavelength;
 *   r^s_{j,j+1} = (kz_j - kz_{j+1}) / (kz_j + kz_{j+1}),
 *   r^p_{j,j+1} = (N_{j+1}^2 kz_j - N_j^2 kz_{j+1}) / (N_{j+1}^2 kz_j + N_j^2 kz_{j+1}),
 *   both times exp(-2 kz_j kz_{j+1} sigma_{j,j+1}^2) (Nevot-Croce) where sigma > 0;
 *   R_{L+1} = 0, R_j = (r_{j,j+1} + R_{j+1} X) / (1 + r_{j,j+1} R_{j+1} X), X = exp(2 i kz_{j+1} t_{j+1});  rs = R^s_0,
 *   rp = R^p_0.  `ideal`: the perfect conductor, rs = -1, rp = +1.
 * kz is formed once per material, ray and element (a periodic stack names few materials), then one Parratt step per layer.
 * Input state: polarised -> E0 = P - (P.d0) d0 over its norm (P = pol, complex, lab frame; d0 the source direction);
 * unpolarised -> the two states u1 = normalize(d0 x a) (a as for s above), u2 = d0 x u1, whose intensities and Stokes
 * sums are averaged.  Per slot, for the rays alive in views[K] (others: w_out = 0, field = 0):
 *   T = |E_K|^2 (unpolarised: the mean of the two states),  w_out = w T  (w = w[r], or 1 when w is NULL)
 *   field (optional, polarised only): E_K as complex128 [3][n] (component c of slot r at 2 (c n + r), re then im)
 * out (DEVICE, ART_POLARISATION_DOUBLES doubles, written):
 *   [0] rays alive in views[K]  [1] sum w0 over the rays alive in views[0] (w0 NULL: their count)  [2] sum w_out
 *   [3] min T  [4] max T  (0 when no ray is alive)
 *   [5..8] S0..S3 = sum w (|Ex|^2 + |Ey|^2), sum w (|Ex|^2 - |Ey|^2), sum w 2 Re(conj(Ex) Ey), sum w 2 Im(conj(Ex) Ey)
 *   [9] sum w |E.nd|^2   with Ex = E.e1, Ey = E.e2, e1, e2 = rows 0, 1 of det.rot, nd = det.normal (0 without has_det)
 *   [10] min over the alive rays of |P - (P.d0) d0| (polarised; 0 otherwise or when no ray is alive)  [11..15] 0
 * Fixed summation order, no float atomics; a job's slicing depends on its own n only: every job gets the same bytes
 * whichever jobs share its call.  jobs_dev / coatings_dev: DEVICE copies of the HOST arrays jobs_host / coatings_host
 * (read for validation and the launch plan).  scratch: DEVICE, art_polarisation_scratch_doubles(jobs_host, n_jobs).
 * Limits: 1 <= n_jobs <= 65535, 0 <= n <= 2^28, 1 <= n_elems <= ART_POLARISATION_MAX_ELEMS, coating indices in
 * [-1, n_coatings), 0 <= n_coatings <= 65535, finite k > 0 and pol, w_out and out non-NULL, views non-NULL; per coating
 * 1 <= n_materials <= ART_COATING_MAX_MATERIALS, 0 <= n_layers <= ART_COATING_MAX_LAYERS, material indices in range,
 * finite n, kappa >= 0, thickness >= 0, roughness >= 0: ART_ERR_BAD_ARG (ART_ERR_UNSUPPORTED for n) otherwise, with
 * nothing launched.  The views' arrays hold n slots each; the rays are read at the slots alive in views[K].         */
#define ART_COATING_MAX_LAYERS 256
#define ART_COATING_MAX_MATERIALS 6
#define ART_POLARISATION_MAX_ELEMS 64
#define ART_POLARISATION_DOUBLES 16
typedef struct ArtCoatingMaterial {
  double n;               /* N = n + i kappa                                                                        */
  double kappa;           /* >= 0                                                                                   */
} ArtCoatingMaterial;
typedef struct ArtCoatingLayer {
  double thickness;       /* mm, >= 0                                                                               */
  double roughness;       /* sigma (mm, >= 0) of the interface at the TOP of this layer                             */
  int32_t material;       /* index into materials                                                                   */
  int32_t reserved;
} ArtCoatingLayer;
typedef struct ArtCoating {
  int32_t ideal;          /* 1: perfect conductor (the rest is ignored)                                             */
  int32_t n_materials;
  int32_t n_layers;       /* L                                                                                      */
  int32_t substrate;      /* material index of the substrate                                                        */
  double roughness;       /* sigma (mm) of the substrate's top interface                                            */
  double reserved;
  ArtCoatingMaterial materials[ART_COATING_MAX_MATERIALS];
  ArtCoatingLayer layers[ART_COATING_MAX_LAYERS];   /* top first                                                     */
} ArtCoating;
typedef struct ArtPolarisationJob {
  const ArtBundleView* views;  /* DEVICE array of n_elems + 1 views: the source, then the bundle after each element  */
  int32_t coating[ART_POLARISATION_MAX_ELEMS];     /* per element: index into the coatings, -1 for a mask          */
  int32_t n_elems;        /* K                                                                                      */
  int32_t polarised;      /* 1: E0 from pol; 0: unpolarised                                                         */
  int64_t n;              /* slots of every view                                                                    */
  double pol[6];          /* P: re x, im x, re y, im y, re z, im z                                                  */
  double k;               /* 2 pi / wavelength (1/mm)                                                               */
  int32_t has_det;        /* 1: Stokes sums in det's frame                                                          */
  int32_t reserved;
  ArtDetectorDesc det;
  const double* w0;       /* DEVICE weights of the source (views[0]) or NULL                                        */
  const double* w;        /* DEVICE weights of the final bundle (views[K]) or NULL                                  */
  double* w_out;          /* DEVICE, n doubles                                                                      */
  double* field;          /* DEVICE, 6 n doubles (complex128 [3][n]), or NULL                                       */
  double* out;            /* DEVICE, ART_POLARISATION_DOUBLES doubles                                               */
} ArtPolarisationJob;
int64_t art_polarisation_scratch_doubles(const ArtPolarisationJob* jobs_host, int32_t n_jobs);
int art_polarisation(const ArtPolarisationJob* jobs_dev, const ArtPolarisationJob* jobs_host, int32_t n_jobs,
                     const ArtCoating* coatings_dev, const ArtCoating* coatings_host, int32_t n_coatings, double* scratch,
                     void* stream);

/* Ray tubes of MANY traced chains in one call: differential ray tracing (added under ABI 14: ArtTubeJob, art_ray_tubes,
 * art_ray_tubes_scratch_doubles).  One streaming pass over a chain's existing history; the tracing kernels are not
 * involved.  Beside each ray travel the first-order changes dP_j, dD_j (j = a, b) of its point and direction with respect
 * to two source parameters that span the plane perpendicular to the source direction:
 *   ART_TUBE_POINT  dP = 0, dD = (u, v): the source measure mu is solid angle;  ART_TUBE_PLANE  dP = (u, v), dD = 0: area.
 * At every element the hit point P (views[e + 1]'s point), the previous point and the incoming direction D (views[e])
 * give, with the gradient g and Hessian H of the surface's implicit form at P in the optic frame and n = -g / |g|,
 *   t = (P - P_prev).D,  a_j = dP_j + t dD_j,  dQ_j = a_j - D (n.a_j) / (n.D),  dn_j = -(H dQ_j - n (n.H dQ_j)) / |g|,
 *   dD'_j = dD_j - 2 [(dD_j.n + D.dn_j) n + (D.n) dn_j]          (a mask: the plane rule, dD unchanged)
 * (forms per kind and the derivation: csrc/art_tubes.h).  Behind the last element, D' the final direction, dX_j the
 * tangents carried onto the detector plane (has_detector) or dQ_j at the last hit point (none):
 *   solid_angle = D'.(dD_a x dD_b)                  dOmega' / dmu, signed, always finite
 *   area        = nd.(dX_a x dX_b) (detector) or D'.(dQ_a x dQ_b): mm^2 per unit mu, signed
 *   kappa1 <= kappa2: the eigenvalues of the symmetric part of the wavefront curvature matrix C = B A^-1 (A = [v_i.dX_j],
 *   B = [v_i.dD_j], v_i perpendicular to D') in 1 / mm, negative = converging, the focal line at -1 / kappa along the
 *   ray; axis: the unit eigenvector of kappa1 in the lab frame, [3][n].  At a caustic A is singular: kappa and axis are
 *   +-inf or NaN there, nothing is clamped.
 * A ray counts when it is alive in EVERY view.  weight[r] = w[r] |solid_angle| (w NULL: 1), 0 for the others, whose
 * entries of the optional arrays are NaN.
 * out (DEVICE, ART_TUBE_DOUBLES doubles per job, written), sums over the counted rays:
 *   [0] their count  [1] sum w  [2] sum w |solid_angle|  [3] min, [4] max |solid_angle| (0 without rays)  [5] sum w |area|
 *   [6], [7] the w-weighted means of kappa1, kappa2 over the rays where both are finite (0 without such rays)
 *   [8] sum w over those rays  [9] their count  [10] max over them of |C_12 - C_21| / (|kappa1| + |kappa2|) (0 where the
 *   denominator is 0; Malus-Dupin: rounding only)  [11..15] 0
 * Fixed summation order, no float atomics; a job's slicing depends on its own n only: every job gets the same bytes
 * whichever jobs share its call.  jobs_dev: a DEVICE copy of jobs_host whose `elems` and `quadrics` point to DEVICE
 * copies; in jobs_host they point to the HOST originals, read for validation.  The elements are the caller's
 * descriptors as art_trace_element takes them (fwd, pos, centre, kind, mp are read).
 * scratch: DEVICE, art_ray_tubes_scratch_doubles(jobs_host, n_jobs).
 * Limits: 1 <= n_jobs <= ART_TUBE_MAX_JOBS, 0 <= n <= 2^28 (ART_ERR_UNSUPPORTED beyond), 1 <= n_elems <=
 * ART_TUBE_MAX_ELEMS, a known seed and kind, views, elems, weight, out and scratch non-NULL, quadrics non-NULL where an
 * element has ART_FLAG_QUADRIC, a unit detector normal: ART_ERR_BAD_ARG otherwise.  ART_ERR_UNSUPPORTED: an element with
 * defects (n_defects, n_grid > 0 or ART_FLAG_PERTURBED_NORMAL), a grating, a freeform (its Hessian needs the figure's
 * second derivatives).  Nothing is launched on failure.                                                              */
#define ART_TUBE_POINT 0
#define ART_TUBE_PLANE 1
#define ART_TUBE_MAX_ELEMS 64
#define ART_TUBE_MAX_JOBS 64
#define ART_TUBE_DOUBLES 16
typedef struct ArtTubeJob {
  const ArtBundleView* views;      /* DEVICE array of n_elems + 1 views: the source, then the bundle after each element */
  const ArtElementDesc* elems;     /* n_elems descriptors (DEVICE in jobs_dev, HOST in jobs_host)                       */
  const ArtQuadricDesc* quadrics;  /* n_elems entries, read where ART_FLAG_QUADRIC is set; may be NULL without any      */
  int32_t n_elems;                 /* K                                                                                 */
  int32_t seed;                    /* ART_TUBE_POINT | ART_TUBE_PLANE                                                   */
  int32_t has_detector;            /* 1: area and curvature on det's plane; 0: at the last hit point                    */
  int32_t reserved;
  ArtDetectorDesc det;
  const double* w;                 /* DEVICE weights [n] or NULL (all 1)                                                */
  int64_t n;                       /* slots of every view                                                               */
  double* weight;                  /* DEVICE [n], always written                                                        */
  double* solid_angle;             /* DEVICE [n] or NULL; likewise the next four                                        */
  double* area;
  double* kappa1;
  double* kappa2;
  double* axis;                    /* DEVICE [3][n] or NULL                                                             */
} ArtTubeJob;
int64_t art_ray_tubes_scratch_doubles(const ArtTubeJob* jobs_host, int32_t n_jobs);
int art_ray_tubes(const ArtTubeJob* jobs_dev, const ArtTubeJob* jobs_host, int32_t n_jobs, double* scratch,
                  double* out /* DEVICE [n_jobs][ART_TUBE_DOUBLES] */, void* stream);

/* Alignment sensitivities of MANY traced chains in one call (added under ABI 14: ArtSensitivityJob, art_sensitivities,
 * art_sensitivities_scratch_doubles): the derivative of every ray's detector coordinates, path and final direction with
 * respect to a rigid motion of each element and of the source, by art_ray_tubes' transport in one streaming pass over
 * the chain's existing history; nothing is re-traced.  Groups g = 0 (the source) and g = 1..K (element g - 1) of
 * ART_SENS_COLS = 6 columns each, column c = 6 g + i, M = 6 (K + 1):
 *   source   i = 0..2 shift along lab x, y, z (dP = e_i, dD = 0); i = 3..5 tilt about lab x, y, z with the points held
 *            (dP = 0, dD = e_i x D0), per radian
 *   element  with r_0, r_1, r_2 the rows of its fwd (major axis, normal x major, normal): i = 0..2 shift along r_i, the
 *            surface point at X moves by s(X) = r_i; i = 3..5 rotation about r_i through pos, s(X) = r_i x (X - pos),
 *            theta = r_i, per radian (roll, pitch, yaw of the optic as a rigid body)
 * At the element that moves (t, a, n, dn_surf as for art_ray_tubes):
 *   dt = -n.(a - s(P)) / (n.D),  dQ = a + D dt,  dn = dn_surf(dQ - s(P)) + theta x n,
 *   dD' = dD - 2 [(dD.n + D.dn) n + (D.n) dn],  dP' = dQ,  dL += dt
 * and at every other element the same with s = theta = 0 (a mask: dD unchanged).  On the detector (centre C, unit normal
 * nd, rot) the transport onto its plane gives dX_lab and dL += dt; (dX, dY) = (rot dX_lab)[0:2].  First order only; the
 * set of counted rays is the nominal trace's (alive in EVERY view): vignetting that changes with the motion is not
 * differentiated.  Per ray X, Y = (rot (Q - C))[0:2] - origin[0:2] with Q the hit point on the detector plane, and
 * L = path of the last view + nd.(C - P) / (nd.D) - origin[2]: the caller passes the weighted means as origin so that
 * the products below do not cancel.
 * out (DEVICE, written): the jobs' tables one after another, job j's [1 + M_j][ART_SENS_DOUBLES] behind those of the jobs
 * before it; sums over the counted rays with the weights w (NULL: 1):
 *   row 0      [0] count [1] sum w [2] sum w X [3] sum w Y [4] sum w L [5] sum w X^2 [6] sum w Y^2 [7] sum w L^2 [8..15] 0
 *   row 1 + c  [0] sum w dX [1] sum w dY [2] sum w dL [3] sum w X dX [4] sum w Y dY [5] sum w L dL [6] sum w dX^2
 *              [7] sum w dY^2 [8] sum w dL^2 [9..11] sum w dD' (lab x, y, z) [12..15] 0
 * The optional arrays dX, dY, dL (DEVICE [M][n] each, or NULL) receive the per-ray values, NaN for the rays that do not
 * count.  Fixed summation order, no float atomics; a job's slicing depends on its own n only: every job gets the same
 * bytes whichever jobs share its call.  jobs_dev / jobs_host and the element tables: as for art_ray_tubes.
 * scratch: DEVICE, art_sensitivities_scratch_doubles(jobs_host, n_jobs): 80 doubles per job, group and tile of 256
 * slots, sized by the call's largest K and n (12.5 B per slot at K = 4).
 * Limits: 1 <= n_jobs <= ART_TUBE_MAX_JOBS, 0 <= n <= 2^28 (ART_ERR_UNSUPPORTED beyond), 1 <= n_elems <=
 * ART_TUBE_MAX_ELEMS, views, elems, out and scratch non-NULL, quadrics non-NULL where an element has ART_FLAG_QUADRIC, a
 * finite origin and detector centre, a unit detector normal: ART_ERR_BAD_ARG otherwise.  ART_ERR_UNSUPPORTED: the
 * elements art_ray_tubes refuses (defects, gratings, freeforms).  Nothing is launched on failure.                     */
#define ART_SENS_DOUBLES 16
#define ART_SENS_COLS 6
typedef struct ArtSensitivityJob {
  const ArtBundleView* views;      /* DEVICE array of n_elems + 1 views: the source, then the bundle after each element */
  const ArtElementDesc* elems;     /* n_elems descriptors (DEVICE in jobs_dev, HOST in jobs_host)                       */
  const ArtQuadricDesc* quadrics;  /* n_elems entries, read where ART_FLAG_QUADRIC is set; may be NULL without any      */
  int32_t n_elems;                 /* K                                                                                 */
  int32_t reserved;
  int64_t n;                       /* slots of every view                                                               */
  ArtDetectorDesc det;             /* required: centre, unit normal, rot                                                */
  const double* w;                 /* DEVICE weights [n] or NULL (all 1)                                                */
  double origin[3];                /* X0, Y0, L0                                                                        */
  double* dX;                      /* DEVICE [6 (K + 1)][n] or NULL; likewise the next two                              */
  double* dY;
  double* dL;
} ArtSensitivityJob;
int64_t art_sensitivities_scratch_doubles(const ArtSensitivityJob* jobs_host, int32_t n_jobs);
int art_sensitivities(const ArtSensitivityJob* jobs_dev, const ArtSensitivityJob* jobs_host, int32_t n_jobs,
                      double* scratch, double* out, void* stream);

/* Compensator sums of MANY traced chains in one call (added under ABI 14: ArtAlignmentJob, art_alignment_sums,
 * art_alignment_sums_scratch_doubles): the products BETWEEN a chosen handful of art_sensitivities' columns, per ray, from
 * which a least-squares solve finds the moves of a few adjusters that make the spot (or the path spread) smallest.
 * dofs[0 .. n_dofs): column ids in art_sensitivities' numbering, c = 6 g + i, in the caller's order, or
 * ART_ALIGN_DOF_DETECTOR: the detector shifted along its normal, per mm, centre' = centre - u normal (the sign of
 * Detector.shiftByDistance): dX_lab = normal - D' / (normal.D'), dL = -1 / (normal.D'), exactly linear in u.
 * All columns of a job travel in ONE lane (a product needs both of its columns there); the lane starts at the earliest
 * element among the chosen groups, and a column of a later group stays clear until its own element.  X, Y, L, the
 * counted rays (alive in EVERY view) and the transport are art_sensitivities'.
 * Centring: a pitch moves the whole spot, |mean dX| >> its spread, so products of uncentred columns would cancel.  A pilot
 * launch on the same stream forms the weighted means of every column over the first min(n, ART_ALIGN_PILOT) slots
 * (zeros when no ray counts there) and leaves them in the table; the main pass sums d'Q_a = dQ_a - centre_a^Q.  Nothing
 * is read back in between.  The covariances do not depend on the centres; the true means are centre + sum w d'Q / sum w.
 * out (DEVICE, written): ART_ALIGN_DOUBLES doubles per job, with Q = X, Y, L for q = 0, 1, 2 and a, b the places in dofs:
 *   [0..8)                             row 0 of art_sensitivities: count, sum w, sum w X, Y, L, sum w X^2, Y^2, L^2
 *   [ART_ALIGN_CENTRES + 8 q + a]      centre_a^Q, the pilot's mean of dQ_a
 *   [ART_ALIGN_MEANS + 8 q + a]        sum w d'Q_a
 *   [ART_ALIGN_CROSS + 8 q + a]        sum w Q d'Q_a
 *   [ART_ALIGN_PAIRS + 36 q + p]       sum w d'Q_a d'Q_b for a <= b, p = a (17 - a) / 2 + (b - a)
 * Entries of places >= n_dofs and [188..192) are 0.  Fixed summation order, no float atomics; a job's slicing and its
 * kernel depend on its own n and n_dofs only: every job gets the same bytes whichever jobs share its call.
 * jobs_dev / jobs_host and the element tables: as for art_ray_tubes.
 * scratch: DEVICE, art_alignment_sums_scratch_doubles(jobs_host, n_jobs): at most 164 doubles per job and tile of 256
 * slots (5.1 B per slot).
 * Limits: those of art_sensitivities, and 1 <= n_dofs <= ART_ALIGN_MAX_DOFS, every id in [-1, 6 (K + 1)) and none twice:
 * ART_ERR_BAD_ARG otherwise.  Nothing is launched on failure.                                                          */
#define ART_ALIGN_MAX_DOFS 8
#define ART_ALIGN_PILOT 1024
#define ART_ALIGN_DOF_DETECTOR (-1)
#define ART_ALIGN_CENTRES 8
#define ART_ALIGN_MEANS 32
#define ART_ALIGN_CROSS 56
#define ART_ALIGN_PAIRS 80
#define ART_ALIGN_DOUBLES 192
/* (declared by its tag, as ArtQuantileDesc is: C callers write `struct ArtAlignmentJob`) */
struct ArtAlignmentJob {
  const ArtBundleView* views;      /* DEVICE array of n_elems + 1 views: the source, then the bundle after each element */
  const ArtElementDesc* elems;     /* n_elems descriptors (DEVICE in jobs_dev, HOST in jobs_host)                       */
  const ArtQuadricDesc* quadrics;  /* n_elems entries, read where ART_FLAG_QUADRIC is set; may be NULL without any      */
  int32_t n_elems;                 /* K                                                                                 */
  int32_t n_dofs;                  /* C                                                                                 */
  int64_t n;                       /* slots of every view                                                               */
  ArtDetectorDesc det;             /* required: centre, unit normal, rot                                                */
  const double* w;                 /* DEVICE weights [n] or NULL (all 1)                                                */
  double origin[3];                /* X0, Y0, L0                                                                        */
  int32_t dofs[ART_ALIGN_MAX_DOFS];
};
int64_t art_alignment_sums_scratch_doubles(const struct ArtAlignmentJob* jobs_host, int32_t n_jobs);
int art_alignment_sums(const struct ArtAlignmentJob* jobs_dev, const struct ArtAlignmentJob* jobs_host, int32_t n_jobs,
                       double* scratch, double* out /* DEVICE [n_jobs][ART_ALIGN_DOUBLES] */, void* stream);

/* Vector focal fields of a pulse behind dispersive coatings (added under ABI 14: ArtFocalVectorSpectrumDesc,
 * art_focal_vector_spectrum, art_focal_vector_spectrum_scratch_doubles): art_focal_spectrum's sum with the complex
 * vector field of art_polarisation, evaluated per ray AND per wavenumber, as each ray's amplitude.  With
 * k_j = s.f.k + j * s.dk (art_focal_spectrum's k_j), u_0, u_1 = rows 0, 1 of s.f.det.rot and u_2 = s.f.det.normal:
 *     a_r(k_j)        = sqrt(w_r) E_r(k_j)          E_r: art_polarisation's E_K of a polarised input `pol` (same initial
 *                                                    field, frames, cos t; a mask, coating index -1, leaves E unchanged),
 *                                                    every coating's rs, rp formed at k_j with the optical constants
 *                                                    materials[j][c][.] in place of coatings[c].materials
 *     field[q][j][c]  = sum_r (a_r(k_j) . u_c) exp(i k_j Phi_r)      (bilinear dot product; c = 0, 1, 2)
 * exp(i k_j Phi_r) is art_focal_spectrum's phase factor of ray r (same separation and operation order), w_r = w[r] (1
 * when w is NULL) for the rays alive in views[n_elems], 0 for every other slot.  b is views[n_elems] as a HOST struct.
 * field (DEVICE, complex128, [planes][nk][3][ny][nx]) is written, not added to; n = 0 writes zeros.  Fixed summation
 * order (no float atomics): the same bytes on every call with the same arguments.
 * The wavenumbers are processed in blocks of nkb; a block needs 6 doubles per slot and wavenumber (the a_r . u_c) besides
 * its partial sums.  scratch_bound (doubles; 0: ART_FOCAL_VECTOR_SCRATCH_DEFAULT) chooses the largest nkb whose scratch
 * stays within it (at least 1, whatever the bound); every (plane, wavenumber, component) is summed on its own, and the
 * slicing of the rays does not depend on nkb: the same bytes for every scratch_bound.
 * scratch: DEVICE, art_focal_vector_spectrum_scratch_doubles(d) doubles.  coatings_dev / materials: DEVICE copies of the
 * HOST arrays coatings_host / materials_host (read for validation), materials as
 * ArtCoatingMaterial[nk][n_coatings][ART_COATING_MAX_MATERIALS]; entries beyond a coating's n_materials are not read.
 * Limits: all of art_focal_spectrum's with planes * nk * 3 <= 65535 in place of planes * nk <= 65535 (the component
 * rides on the grid beside plane and wavenumber); of art_polarisation's: 0 <= n <= 2^28 (ART_ERR_UNSUPPORTED beyond),
 * 1 <= n_elems <= ART_POLARISATION_MAX_ELEMS, coating indices in [-1, n_coatings), 0 <= n_coatings <= 65535, finite
 * pol, every coating valid, and every materials[j][c][m], m < n_materials of a non-ideal coating c, finite with
 * kappa >= 0; scratch_bound >= 0; views, field and scratch non-NULL when n > 0: ART_ERR_BAD_ARG otherwise, with nothing
 * launched and field untouched. */
#define ART_FOCAL_VECTOR_SCRATCH_DEFAULT ((int64_t)1 << 29)   /* doubles: 4 GiB */
typedef struct ArtFocalVectorSpectrumDesc {
  ArtFocalSpectrumDesc s;      /* grid, planes, detector, L_ref, k_0, dk, nk                                         */
  const ArtBundleView* views;  /* DEVICE array of n_elems + 1 views: the source, then the bundle after each element   */
  int32_t coating[ART_POLARISATION_MAX_ELEMS];     /* per element: index into the coatings, -1 for a mask           */
  int32_t n_elems;             /* K                                                                                  */
  int32_t n_coatings;
  int64_t n;                   /* slots of every view                                                                */
  double pol[6];               /* P: re x, im x, re y, im y, re z, im z                                              */
  const double* w;             /* DEVICE weights of the final bundle (views[K]) or NULL                              */
  const ArtCoatingMaterial* materials;   /* DEVICE, [nk][n_coatings][ART_COATING_MAX_MATERIALS]                      */
  int64_t scratch_bound;       /* doubles; 0 = ART_FOCAL_VECTOR_SCRATCH_DEFAULT                                      */
} ArtFocalVectorSpectrumDesc;
int64_t art_focal_vector_spectrum_scratch_doubles(const ArtFocalVectorSpectrumDesc* d);
int art_focal_vector_spectrum(const ArtFocalVectorSpectrumDesc* d, const ArtBundleView* b, const ArtCoating* coatings_dev,
                              const ArtCoating* coatings_host, const ArtCoatingMaterial* materials_host, double* scratch,
                              double* field, void* stream);

/* Vector focal fields of a pulse from a CHROMATIC source behind dispersive coatings (added under ABI 14:
 * ArtFocalVectorChromaticDesc, art_focal_vector_chromatic, art_focal_vector_chromatic_scratch_doubles):
 * art_focal_vector_spectrum's sum with art_focal_chromatic's amplitude and phase per ray and wavenumber, for high
 * harmonics sent through coated mirrors.  b is views[n_elems] and src is views[0] (the source bundle is the first view
 * of the history), both as HOST structs; only src's directions s_r are read.  With the unit vector `axis` = a,
 *     u_r  = 0.5 * (((s_x - a_x)^2 + (s_y - a_y)^2) + (s_z - a_z)^2)      (this order, no fma)
 *     row j of the table = (k_j, c_j, z_j, 0)                             art_focal_chromatic's row, ANY list of k_j
 *     a_r(k_j)        = (sqrt(w_r) * exp(-(u_r * c_j))) * E_r(k_j)        E_r: art_focal_vector_spectrum's field at k_j
 *                                                                         with materials[j][c][.] (row j of the table
 *                                                                         = row j of materials)
 *     field[q][j][c]  = sum_r (a_r(k_j) . u_c) exp(i [k_j * (base_r / k + z_j * u_r) + shift, X and Y terms])
 * base_r / k, the shift, X and Y terms and every rounding are art_focal_chromatic's; the frames, cos t, the Parratt
 * recursion and the projection on u_c = e1, e2, n are art_focal_vector_spectrum's.  v.s.nk is the number of rows;
 * v.s.f.k and v.s.dk are checked as there but NOT used: the table holds the k_j.
 * A row with c_j = 0 and z_j = 0 multiplies by exp(-0) = 1 and adds +0.0: with k_j = v.s.f.k + j * v.s.dk formed as
 * art_focal_spectrum forms them, the call gives art_focal_vector_spectrum's bytes.
 * A dead slot of views[n_elems] contributes nothing, whatever any view holds there (NaN included).
 * field (DEVICE, complex128, [planes][nk][3][ny][nx]) is written, not added to; n = 0 writes zeros.  Fixed summation
 * order (no float atomics): the same bytes on every call with the same arguments.
 * v.scratch_bound blocks the wavenumbers exactly as in art_focal_vector_spectrum, and the slicing of the rays depends
 * neither on nk nor on the block: slice j of the field has the same bytes whichever other rows share the call, whatever
 * their order and whatever the bound -- a comb of harmonics pays for its lines only.
 * table_dev: DEVICE, 4 * nk doubles; table_host: the same values on the HOST, which the validation reads.
 * scratch: DEVICE, art_focal_vector_chromatic_scratch_doubles(d) doubles (the negative error code on a bad descriptor).
 * Limits: all of art_focal_vector_spectrum's, except that the k_j come from the table, and art_focal_chromatic's on the
 * table and the axis: | |axis| - 1 | <= 1e-12, table_host non-NULL, every k_j finite and > 0, every c_j finite and
 * >= 0, every z_j finite, table_dev and src's arrays non-NULL when n > 0: ART_ERR_BAD_ARG otherwise (ART_ERR_UNSUPPORTED
 * for n > 2^28), with nothing launched and field untouched. */
typedef struct ArtFocalVectorChromaticDesc {
  ArtFocalVectorSpectrumDesc v;   /* everything of art_focal_vector_spectrum; v.s.nk = rows of the table              */
  double axis[3];                 /* a: the unit axis of the source                                                    */
} ArtFocalVectorChromaticDesc;
int64_t art_focal_vector_chromatic_scratch_doubles(const ArtFocalVectorChromaticDesc* d);
int art_focal_vector_chromatic(const ArtFocalVectorChromaticDesc* d, const ArtBundleView* b, const ArtBundleView* src,
                               const ArtCoating* coatings_dev, const ArtCoating* coatings_host,
                               const ArtCoatingMaterial* materials_host, const double* table_dev,
                               const double* table_host, double* scratch, double* field, void* stream);

/* Partially coherent focal image of an extended source (added under ABI 14: ArtFocalImageDesc, art_focal_image,
 * art_focal_image_scratch_doubles): the rays of one bundle in mutually incoherent groups of contiguous slots, summed
 * coherently inside a group and as intensities across groups,
 *     image[q][l,j] = sum_g | sum_{r in group g} sqrt(w_r) exp(i k [(path_r - L_ref) + d_r . (x_qjl - p_r)]) |^2
 * with art_focal_field's per-ray terms, formed in the same operation order; group g = slots [seg[g], seg[g+1]).  seg
 * lives on the DEVICE and the host never reads it: every offset is clamped to [0, n], seg[g+1] <= seg[g] is an empty
 * group (it contributes 0), and slots outside every group contribute nothing -- no contents of seg make the call read
 * outside the bundle.  Dead slots contribute nothing.
 * image (DEVICE, fp64, [planes][ny][nx]) is written, not added to; n = 0 writes zeros.  Fixed summation order (no float
 * atomics): the same bytes on every call with the same arguments.
 * scratch: DEVICE, art_focal_image_scratch_doubles(nx, ny, planes, groups, n) doubles (-1 on arguments out of range).
 * Limits: all of art_focal_field's on f, 1 <= groups <= ART_FOCAL_MAX_GROUPS, seg and image non-NULL, scratch non-NULL
 * when n > 0: ART_ERR_BAD_ARG otherwise, with nothing launched and image untouched. */
#define ART_FOCAL_MAX_GROUPS (1 << 20)
typedef struct ArtFocalImageDesc {
  ArtFocalDesc f;         /* grid, planes, detector, k, L_ref: exactly art_focal_field's                           */
  int32_t groups;         /* 1 .. ART_FOCAL_MAX_GROUPS                                                             */
  int32_t reserved;
  const int64_t* seg;     /* DEVICE, groups + 1 slot offsets: group g = slots [seg[g], seg[g+1])                    */
} ArtFocalImageDesc;
int64_t art_focal_image_scratch_doubles(int32_t nx, int32_t ny, int32_t planes, int32_t groups, int64_t n);
int art_focal_image(const ArtFocalImageDesc* d, const ArtBundleView* b, const double* w, int64_t n, double* scratch,
                    double* image, void* stream);

/* Exact weighted quantiles and rank sums of one key per slot and plane (added under ABI 14: ArtQuantileDesc,
 * art_quantiles, art_quantile_scratch_doubles): "which radius holds 50 % of the intensity", the half-energy width, W90,
 * encircled-energy curves, medians and percentiles of any per-ray quantity.  The answer is the key of an actual slot.
 * Keys: one fp64 value per slot and plane, ordered as real numbers with -0 = +0; +-inf are ordinary keys; a NaN key makes
 * the slot INVALID for that plane: it is counted and otherwise ignored.  Dead slots contribute nothing.
 * Weights: q_i = (int64) rint(ldexp(w_i, wshift)), art_histogram's rule; w = NULL: q_i = 1; w must be finite and >= 0 (a
 * negative q counts as 0) and wshift such that no sum overflows int64.  Every sum is a sum of these integers (integer
 * atomics and integer folds only): the same bytes on every run, whatever the grid and the plane blocking.
 * Quantile, per plane, W = sum q_i over the valid slots, per fraction f in [0, 1]:
 *     T = min(W, max(1, (int64) ceil(f * (double) W)))
 *     value = the smallest key v with  sum_{key <= v} q  >=  T
 *     below = sum_{key < v} q,   upto = sum_{key <= v} q           (below < T <= upto)
 * W == 0: value = NaN, below = upto = 0.  totals (per plane): [0] W [1] valid slots [2] invalid slots.
 * Rank sums, per plane and threshold t (sorted ascending per plane, +-inf allowed):
 *     rank_sums = sum q_i [key_i <= t],   rank_counts = the number of valid slots with key_i <= t.
 * The select is a most-significant-digit radix select in six passes (digits of 9 and 5 x 11 bits of the order-preserving
 * uint64 image of the key), all enqueued on the stream with nothing read back in between (csrc/art_quantile.h).
 * Key sources:
 *   ART_QKEY_GIVEN   keys: DEVICE [planes][n]; alive: DEVICE [n] or NULL (every slot alive); b is not read.
 *   detector metrics of the bundle b on the planes det.centre + shift[p] * det.normal (art_focal_field's convention;
 *   plane p is read as a detector of its own, exactly as art_detector reads it), with centres (cx, cy, c) per plane:
 *     ART_QKEY_RADIUS  key = (X - cx)^2 + (Y - cy)^2; values and thresholds are its SQUARE ROOT (mm): a slot is within
 *                      threshold t iff sqrt(key) <= t
 *     ART_QKEY_X       |X - cx|        ART_QKEY_Y   |Y - cy|          (mm)
 *     ART_QKEY_DELAY   |delay - c|, delay = ((opl - L_p) / 299792458000.0) * 1e15 (fs), L_p the mean of opl over the
 *                      alive slots on plane p, formed on the device
 *   centre_given = 1: centre[p] = (cx, cy, c) is used as given; 0: the w-weighted centroid of (X, Y, delay) over the alive
 *   slots of each plane, formed on the device.  centres_out (DEVICE [planes][4] or NULL): cx, cy, c, L_p as used (NaN
 *   without alive slots; L_p is 0 where no delay is formed).
 * Outputs (DEVICE, all written): values [planes][n_fractions] (double), below, upto [planes][n_fractions] (int64),
 * totals [planes][3] (int64), rank_sums, rank_counts [planes][n_thresholds] (int64).
 * thresholds_dev: DEVICE [planes][n_thresholds], a copy of thresholds_host (HOST, read for validation).
 * The planes are processed in blocks whose scratch stays within scratch_bound doubles (0: ART_QUANTILE_SCRATCH_DEFAULT; at
 * least one plane per block whatever the bound); the result does not depend on it.
 * scratch: DEVICE, art_quantile_scratch_doubles(d, n) doubles (negative: the error code of a bad descriptor).
 * Limits: 0 <= n <= 2^28 (ART_ERR_UNSUPPORTED beyond), 1 <= planes <= ART_FOCAL_MAX_PLANES, 1 <= n_fractions <= ART_QUANTILE_MAX_FRACTIONS = 16,
 * 0 <= n_thresholds <= ART_QUANTILE_MAX_THRESHOLDS = 256, fractions in [0, 1], thresholds sorted and not NaN, wshift in
 * [-1074, 1074], finite shifts and given centres, a unit detector normal, scratch_bound >= 0, values, below, upto, totals
 * and scratch non-NULL, the rank outputs and both threshold arrays non-NULL when n_thresholds > 0, keys (GIVEN) or a
 * whole bundle view (metrics) when n > 0: ART_ERR_BAD_ARG otherwise, with nothing launched.  Geometric rays only: the encircled energy of a diffraction image is not this. */
enum ArtQuantileKey { ART_QKEY_GIVEN = 0, ART_QKEY_RADIUS = 1, ART_QKEY_X = 2, ART_QKEY_Y = 3, ART_QKEY_DELAY = 4 };
#define ART_QUANTILE_MAX_FRACTIONS 16
#define ART_QUANTILE_MAX_THRESHOLDS 256
#define ART_QUANTILE_SCRATCH_DEFAULT ((int64_t)1 << 28)   /* doubles: 2 GiB */
/* (declared by its tag: C callers write `struct ArtQuantileDesc`) */
struct ArtQuantileDesc {
  int32_t key;                 /* ArtQuantileKey                                                                     */
  int32_t planes;
  int32_t n_fractions;
  int32_t n_thresholds;
  int32_t wshift;              /* the fixed-point shift of the weights                                               */
  int32_t centre_given;        /* metrics: 1 = centre[] is used, 0 = the weighted centroid is formed on the device   */
  int64_t scratch_bound;       /* doubles; 0: ART_QUANTILE_SCRATCH_DEFAULT                                           */
  const double* keys;          /* GIVEN: DEVICE [planes][n]                                                          */
  const uint8_t* alive;        /* GIVEN: DEVICE [n] or NULL                                                          */
  const double* thresholds_dev;   /* DEVICE [planes][n_thresholds]                                                   */
  const double* thresholds_host;  /* HOST, the same values                                                           */
  double* values;              /* DEVICE outputs, see above                                                          */
  int64_t* below;
  int64_t* upto;
  int64_t* totals;
  int64_t* rank_sums;
  int64_t* rank_counts;
  double* centres_out;
  double fraction[ART_QUANTILE_MAX_FRACTIONS];
  ArtDetectorDesc det;         /* metrics                                                                            */
  double shift[ART_FOCAL_MAX_PLANES];
  double centre[ART_FOCAL_MAX_PLANES][3];
};
int64_t art_quantile_scratch_doubles(const struct ArtQuantileDesc* d, int64_t n);
int art_quantiles(const struct ArtQuantileDesc* d, const ArtBundleView* b, const double* w, int64_t n, double* scratch,
                  void* stream);

/* Masked reductions over alive rays, deterministic (fixed two-level tree, no float atomics).
 * out16 (DEVICE, 16 doubles):
 *   [0] count  [1] sum opl  [2] min X [3] max X [4] min Y [5] max Y  [6] sum X [7] sum Y
 *   [8] sum w  [9] sum w*X [10] sum w*Y [11] sum w*opl  [12] min opl [13] max opl [14..15] 0
 * w = weights (DEVICE) or NULL (then w = 1).  X, Y, opl may be NULL (their entries are then 0).
 * scratch: DEVICE, at least art_reduce_scratch_doubles() doubles.
 * Feeds get_Delays' mean (ModuleDetector.py:277), CentrePointList (ModuleGeometry.py:235-236),
 * getETransmission (ModuleAnalysisAndPlots.py:76).                                                     */
int64_t art_reduce_scratch_doubles(void);
int art_detector_stats(const uint8_t* alive, const double* X, const double* Y, const double* opl,
                       const double* w, int64_t n, double* scratch, double* out16, void* stream);

/* Second moments about given centres (two-pass variance; ModuleProcessing.py:485-532):
 * out8: [0] sum w [1] sum w (X-cx)^2 [2] sum w (Y-cy)^2 [3] sum w (opl-co)^2 [4] count [5..7] 0         */
int art_detector_moments(const uint8_t* alive, const double* X, const double* Y, const double* opl,
                         const double* w, int64_t n, double cx, double cy, double co,
                         double* scratch, double* out8, void* stream);

/* Mean ray of a bundle (FindCentralRay, ModuleProcessing.py:464-482) + sum of intensities:
 * out8: [0] count [1..3] sum point [4..6] sum vector [7] sum w                                          */
int art_bundle_sums(const ArtBundleView* b, const double* w, int64_t n, double* scratch, double* out8,
                    void* stream);

/* Gaussian intensity weights of a source bundle (ApplyGaussianIntensityToRayList, ART/ModuleSource.py:219-261):
 * w = 1 on the axis falling to `fraction` at the edge -- in angle (tan(angle)/max angle) for diverging bundles
 * (max angle to `axis` > 1e-12), in distance from the origin (|point| / max |point|) for collimated ones.
 * Two passes on the stream (max reduction, then weights); nothing returns to the host.  w_out: DEVICE, n doubles. */
int art_gaussian_intensity(const ArtBundleView* b, const double axis[3], double fraction, int64_t n,
                           double* scratch, double* w_out, void* stream);
/* The same about the bundle's OWN central ray (what ApplyGaussianIntensityToRayList passes: FindCentralRay's mean vector,
 * normalised by the Ray.vector setter, ART/ModuleProcessing.py:464-482): art_bundle_sums into `sums8` (DEVICE, 8 doubles,
 * left there for the caller), then the axis is formed ON THE DEVICE from those sums -- four launches, no host round trip
 * between the central ray and the weights (0.2 ms of waiting at the start of every OEPlacement).                          */
int art_gaussian_intensity_central(const ArtBundleView* b, double fraction, int64_t n, double* scratch, double* sums8,
                                   double* w_out, void* stream);

/* Largest angle between `axis` and the direction of any alive ray, and largest |point| (ReturnNumericalAperture,
 * ART/ModuleProcessing.py:536-566; also the first pass of art_gaussian_intensity).  out2: DEVICE, 2 doubles.          */
int art_bundle_max_angle(const ArtBundleView* b, const double axis[3], int64_t n, double* scratch, double* out2,
                         void* stream);

/* Stable compaction: idx_out[j] = slot of the j-th alive ray (source order kept, as the reference's
 * survivor lists ModuleMirror.py:928-939), *count_out = number alive.  block_counts: DEVICE scratch of
 * art_compact_scratch_ints(n) int32.                                                                    */
int64_t art_compact_scratch_ints(int64_t n);
int art_compact(const uint8_t* alive, int64_t n, int32_t* block_counts, int64_t* idx_out,
                int64_t* count_out, void* stream);

/* Deterministic sources on device (ART/ModuleSource.py:23-81, :135-169; Vogel spiral
 * ModuleGeometry.py:61-76) for global ray indices [first, first+n) of a bundle of n_total rays:
 *   kind 0: point source, half-angle `size` (rad);  kind 1: plane-wave disk of radius `size` (mm).
 * rot = RotationPoint(., ez, axis) as a 3x3 map, S = source point / disk centre.
 * Writes origin, direction, path = 0, incidence = NaN, alive = 1.                                        */
int art_make_source(int32_t kind, double size, const double rot[9], const double S[3], int64_t first,
                    int64_t n, int64_t n_total, const ArtBundleView* out, void* stream);
/* The same for the global indices first, first + step, ..., first + (n-1)*step: the STRIDED shard of rank `first` among
 * `step` ranks.  The Vogel spiral orders rays by radius, so contiguous shards of a masked or overfilled scene lose very
 * different numbers of rays; strided shards are balanced (every rank samples the whole aperture).                    */
int art_make_source_strided(int32_t kind, double size, const double rot[9], const double S[3], int64_t first,
                            int64_t step, int64_t n, int64_t n_total, const ArtBundleView* out, void* stream);

/* ExtendedSource (ART/ModuleSource.py:85-131): n_points point sources on a Vogel disk of radius `radius` (mm), each
 * emitting the same Vogel cone of rays_per_point rays with half-angle `divergence` (rad).  Global ray index
 * k = point * rays_per_point + ray-in-cone, the reference's numbering (:124-127); writes indices [first, first+n).
 * The caller derives n_points and rays_per_point from NbRays as the reference does (:111-119).               */
int art_make_extended_source(double radius, double divergence, int64_t n_points, int64_t rays_per_point,
                             const double rot[9], const double S[3], int64_t first, int64_t n,
                             const ArtBundleView* out, void* stream);

/* Multi-GPU exchange at the detector, two tiny kernels around ONE all-gather (sharding.py): every rank packs
 *   send[0..23]            its 24 read-out statistics (art_detector_readout)
 *   send[24 + 4*j + 0..3]  X, Y, opl, alive (0/1) of its sampled slot slots[j], j < k
 * all ranks all-gather their (24 + 4k)-vectors (rank-major `recv`), and art_exchange_fold folds the `world` statistics
 * vectors into the global ones (slots 2,4,12: min; 3,5,13: max; others: sum -- the slot layout of
 * art_detector_readout).  The sample parts stay where the collective put them.  All pointers DEVICE.       */
int art_exchange_pack(const double* stats24, const double* X, const double* Y, const double* opl,
                      const uint8_t* alive, const int64_t* slots, int64_t k, double* send, void* stream);
int art_exchange_fold(const double* recv, int32_t world, int64_t stride_doubles, double* stats_out24, void* stream);

/* Survivor records for the ONE gather of a sharded run (`(number:int32, X, Y, path)` = 28 B per SURVIVING
 * ray; the consumer, ART/ModuleDetector.py:254-279, sees survivors only).  Compacts the read-out of the alive slots, in
 * slot order, into `send` (DEVICE, 8-byte aligned, capacity send_bytes >= art_survivor_bytes(n, 0)):
 *   [0, 8)   int64 count                     number of alive slots
 *   [8, 16)  int64 flags                     bit 0 "dense": every slot is alive and the numbers are implicit -> the number
 *                                            section is absent (24 B per ray); bit 1 "unpacked": written by
 *                                            art_survivor_finish only (below) -- never by art_pack_survivors
 *   [16 ...) double X[count], Y[count], path[count], then int32 number[count] (absent when dense)
 * number[j] = number ? number[slot_j] : first + slot_j * step (the global index of a shard generated by
 * art_make_source / art_make_source_strided; must fit int32, ART_ERR_UNSUPPORTED otherwise).  A rank sends the first
 * art_survivor_bytes(count, dense) bytes; the header tells the receiver how to read them.  scratch_ints: DEVICE,
 * art_compact_scratch_ints(n) int32.  Everything is enqueued on `stream`; nothing returns to the host.                  */
int64_t art_survivor_bytes(int64_t count, int32_t dense);
/* ZERO-COPY form for a shard that is expected to lose nothing: let the read-out write its X, Y, opl of all n slots
 * straight into the dense layout's sections (X = send + 16, Y = X + n, path = Y + n: art_trace_chain_readout / the scene
 * read-outs / art_detector_readout take any pointers), then call art_survivor_finish with the read-out's statistics
 * (stats24[0] = number of alive slots, DEVICE): it writes the header -- (n, dense) if every slot is alive, and the buffer is
 * complete without a pack or a staging copy; otherwise (count, flags bit 1 "unpacked"): the sections hold slot-indexed
 * values with holes and the caller packs them into ANOTHER buffer with art_pack_survivors (X, Y, opl may point into this
 * one).  `send`: DEVICE, 16-byte aligned, >= art_survivor_bytes(n, 1) bytes.
 * `xhdr` (DEVICE, ART_XHDR_DOUBLES doubles, or NULL): the rank's contribution to the per-step HEADER EXCHANGE of a sharded
 * run, filled in the same launch -- [0], [1] = count, flags as int64 bit patterns, [2 .. 25] = stats24.  All ranks all-gather
 * these 208 bytes: every rank learns every shard's count (the size of the next transfer is predicted from it) and the
 * global statistics follow by art_exchange_fold(recv + 2, world, ART_XHDR_DOUBLES, out).  art_survivor_xheader builds the
 * same block behind art_pack_survivors (header read from `send`; stats24 may be NULL: zeros).                          */
#define ART_XHDR_DOUBLES 26
int art_survivor_finish(const double* stats24, int64_t n, void* send, double* xhdr, void* stream);
int art_survivor_xheader(const void* send, const double* stats24, double* xhdr, void* stream);
int art_pack_survivors(const uint8_t* alive, int64_t n, const double* X, const double* Y, const double* opl,
                       const int64_t* number, int64_t first, int64_t step, int32_t* scratch_ints, void* send,
                       int64_t send_bytes, void* stream);

/* Guide rays of the placement (ART/ModuleProcessing.py:98-126: `_singleOEPlacement` traces ONE alignment ray through the
 * chain built so far to find the direction in which the next optic is placed; OEPlacement with a list-valued argument,
 * :203-239, does that for 10-11 chains one after the other).  One launch advances the guide rays of up to `count` chains
 * by one element each: ray j meets elems[j] (any kind, the per-ray code of art_trace_element).  rays: DEVICE, count x 8
 * doubles, row j = ox, oy, oz, dx, dy, dz, path, incidence of guide ray j, updated in place; alive: DEVICE, count bytes
 * (a guide that misses its optic gets 0 and keeps its state).  The descriptors travel as kernel arguments: count <= 8 per
 * call (ART_ERR_BAD_ARG beyond; callers loop).  Elements in the Zernike recurrence layout are refused (ART_ERR_UNSUPPORTED:
 * the guide of such an optic is traced through art_trace_element).                                                       */
#define ART_GUIDES_MAX 8
int art_trace_guides(const ArtElementDesc* elems, int32_t count, double* rays, uint8_t* alive, void* stream);

/* Analysis of MANY bundles in four launches and ZERO host round trips (ART/ARTmain.py:248-300 runs, per chain of a loop
 * list: getETransmission, ART/ModuleAnalysisAndPlots.py:62-77; Detector.autoplace, ART/ModuleDetector.py:109-137;
 * FindOptimalDistance, ART/ModuleProcessing.py:369-460, or GetResultSummary, ModuleAnalysisAndPlots.py:81-129).  Per job
 * (= one bundle of n slots; all jobs of a call share n):
 *   1. sums over the alive rays: count, sum point, sum vector, sum w, sum path;
 *   2. the detector: given (mode ART_JOB_MANUAL) or placed like Detector.autoplace -- normal = -(mean vector, normalised),
 *      centre = mean point - normal * distance, refpoint = mean point; its rotation normal -> ez with the reference's
 *      special cases (ModuleGeometry.py:333-343); the provisional path centre co = mean path + the mean ray's distance
 *      to the detector / |mean vector| (|mean vector| is the rays' mean cosine to the mean ray, so this is their mean
 *      distance to second order in their angles; within a fraction of a millimetre of the mean optical path in any case),
 *      and the provisional centre (cx, cy) of X and Y: the detector coordinates of the point where the mean ray meets
 *      the detector (exactly 0 when auto-placing: the detector's centre IS that point).  Second moments about centres
 *      inside the spot are well conditioned wherever the caller put the detector's centre, so no pass is spent on
 *      finding the exact means;
 *   3. ONE pass of read-out moments on that detector: the 32 sums of art_detector_scan_moments (the read-out of every ray
 *      is linear in a shift s of the detector along its normal, so spot size and duration at ANY s follow from them --
 *      a whole autofocus search without touching the bundle again), the bounding box of (X, Y) and the range of the
 *      optical path at s = 0, the largest angle between a ray and the mean vector (ReturnNumericalAperture,
 *      ModuleProcessing.py:536-566), and the two shifts nearest to 0 at which some ray's hit point passes through its
 *      origin (there |I - A| has a kink and the linear model ends: callers evaluate scans beyond them position by position).
 * Jobs with mode ART_JOB_SUMS stop after step 1 (e.g. the source bundle, for the transmission's denominator).
 * jobs_dev: DEVICE copy of the HOST array jobs_host (the caller's memcpy; jobs_host is read for validation only and must
 * hold the same contents).  out: DEVICE, n_jobs x ART_ANALYSIS_DOUBLES doubles, job-major:
 *   [0] count  [1..3] sum point  [4..6] sum vector  [7] sum w (= count if w is NULL)  [8] sum path  [9] 0
 *   [10..12] detector centre  [13..15] detector normal  [16..18] refpoint (mean point; manual: job.refpoint)  [19] co
 *   [20..51] the 32 moment sums of art_detector_scan_moments, taken of X - cx, Y - cy and opl - co: per weighting (unweighted
 *            at [20], weighted at [36]) sum w, then for each of the three coordinates q with slope q' = dq/ds (opl: dq/ds - 1)
 *            sum w q, sum w q', sum w q q, sum w q q', sum w q' q'.  Variances do not depend on the centres; a MEAN read off
 *            these sums is about them: mean X = cx + [21] / [20], mean opl = co + [31] / [20]                        [52] 0
 *   [53] largest shift s <= 0 and [54] smallest shift s > 0 at which a ray's t changes sign (-inf / +inf if none)
 *   [55] largest angle to the mean vector (rad)
 *   [56] min X [57] max X [58] min Y [59] max Y [60] min opl [61] max opl   (s = 0; +inf / -inf if nothing is alive;
 *            X and Y about the detector's centre, NOT about (cx, cy))
 *   [62] cx  [63] cy   (0 for ART_JOB_SUMS and for a job without alive rays; these two slots were reserved and read 0
 *            before: row size, structs and symbols are unchanged, so ART_ABI_VERSION stays)
 * One call covers bundles of n <= 2^28 slots (ART_ERR_UNSUPPORTED beyond: 32-bit buffer offsets, as in the tracing launches).
 * A job without alive rays gets count 0, NaN detector fields and zero moments.  A manual detector's normal must be a unit
 * vector (| |normal|^2 - 1 | <= 1e-12, ART_ERR_BAD_ARG otherwise); a manual detector parallel to the mean ray (mean vector .
 * normal = 0) makes the provisional path centre infinite and every path moment NaN -- as the reference's read-out of such a
 * detector is.  scratch: DEVICE, art_analysis_scratch_doubles(n_jobs, n) doubles.  Deterministic (fixed grids, fixed fold order, no float atomics); the
 * launches are enqueued on `stream`, nothing returns to the host.                                                        */
#define ART_ANALYSIS_DOUBLES 64
enum ArtJobMode { ART_JOB_AUTOPLACE = 0, ART_JOB_MANUAL = 1, ART_JOB_SUMS = 2 };
typedef struct ArtAnalysisJob {
  ArtBundleView b;        /* the analysed bundle                                                       */
  const double* w;        /* DEVICE weights (Ray.intensity) or NULL (w = 1)                            */
  double distance;        /* ART_JOB_AUTOPLACE: DistanceDetector                                       */
  int32_t mode;           /* ArtJobMode                                                                */
  int32_t reserved;
  double centre[3];       /* ART_JOB_MANUAL: the detector (unit normal, used bit for bit)              */
  double normal[3];
  double refpoint[3];
  const double* sums;     /* DEVICE, 9 doubles, or NULL: the sums of step 1 if something formed them already (the tail of
                             the tracing launch, ArtChainReadout.sums -> its out24).  Jobs that bring them skip step 1; if all
                             do, the bundles are read ONCE (step 3).                                   */
} ArtAnalysisJob;
int64_t art_analysis_scratch_doubles(int32_t n_jobs, int64_t n);
int art_analyse_bundles(const ArtAnalysisJob* jobs_dev, const ArtAnalysisJob* jobs_host, int32_t n_jobs, int64_t n,
                        double* scratch, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ART_HIP_H */

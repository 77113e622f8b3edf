"""ctypes mirror of include/art_hip.h (structs, enums, prototypes).  Keep in sync with ART_ABI_VERSION."""
import ctypes as C

ART_ABI_VERSION = 14

ART_OK = 0
ART_ERR_BAD_ARG = -1
ART_ERR_UNSUPPORTED = -2
ART_ERR_HIP = -3
ART_ERR_NO_DEVICE = -4

# enum ArtOpticKind
ART_PLANE, ART_SPHERE, ART_PARABOLA, ART_TORUS, ART_ELLIPSOID, ART_CYLINDER, ART_MASK = range(7)
# enum ArtSupportKind
ART_SUP_ROUND, ART_SUP_ROUNDHOLE, ART_SUP_RECT, ART_SUP_RECTHOLE, ART_SUP_RECTRECTHOLE = range(5)

ART_FLAG_PERTURBED_NORMAL = 1
ART_FLAG_ZERN_RECURRENCE = 2
ART_FLAG_GRATING = 4
ART_FLAG_QUADRIC = 8
ART_FLAG_FREEFORM = 16
ART_ZERN_RECURRENCE_MAX_ORDER = 64

ART_ZERN_MAX_ORDER = 16
ART_ZERN_DIM = ART_ZERN_MAX_ORDER + 1
ART_ZERN_STRIDE = 2 + 3 * ART_ZERN_DIM * ART_ZERN_DIM
ART_MAX_DEFECTS = 16

c_double_p = C.POINTER(C.c_double)
c_uint8_p = C.POINTER(C.c_uint8)


class ArtGridDefect(C.Structure):
    _fields_ = [("h", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32),
                ("x0", C.c_double), ("y0", C.c_double), ("dx", C.c_double), ("dy", C.c_double)]


class ArtElementDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32),
        ("support_kind", C.c_int32),
        ("n_defects", C.c_int32),
        ("flags", C.c_uint32),
        ("fwd", C.c_double * 9),
        ("bwd", C.c_double * 9),
        ("pos", C.c_double * 3),
        ("centre", C.c_double * 3),
        ("sp", C.c_double * 6),
        ("mp", C.c_double * 4),
        ("zern", C.c_void_p),
        ("grid", C.c_void_p),
        ("n_grid", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ArtBundleView(C.Structure):
    _fields_ = [
        ("ox", C.c_void_p), ("oy", C.c_void_p), ("oz", C.c_void_p),
        ("dx", C.c_void_p), ("dy", C.c_void_p), ("dz", C.c_void_p),
        ("path", C.c_void_p),
        ("incidence", C.c_void_p),
        ("alive", C.c_void_p),
    ]


ART_GRATING_MAX_WAVELENGTHS = 1024


class ArtGratingDesc(C.Structure):
    _fields_ = [
        ("q", C.c_double * 2),
        ("lines_per_mm", C.c_double),
        ("order", C.c_int32),
        ("nw", C.c_int32),
        ("wavelengths", C.c_void_p),
        ("outs", C.c_void_p),
        ("grooves_in", C.c_void_p),
        ("grooves_out", C.c_void_p),
    ]


class ArtQuadricDesc(C.Structure):
    _fields_ = [("q", C.c_double * 6), ("b", C.c_double * 3), ("c", C.c_double)]


class ArtFigureDesc(C.Structure):
    _fields_ = [("table", C.c_void_p), ("radius", C.c_double), ("order", C.c_int32), ("reserved", C.c_int32)]


class ArtDetectorDesc(C.Structure):
    _fields_ = [
        ("centre", C.c_double * 3),
        ("normal", C.c_double * 3),
        ("rot", C.c_double * 9),
    ]


class ArtChainReadout(C.Structure):
    _fields_ = [
        ("det", ArtDetectorDesc),
        ("w", C.c_void_p),
        ("cx", C.c_double), ("cy", C.c_double), ("co", C.c_double),
        ("X", C.c_void_p), ("Y", C.c_void_p), ("opl", C.c_void_p),
        ("scratch", C.c_void_p),
        ("out24", C.c_void_p),
        ("lite", C.c_int32),
        ("sums", C.c_int32),
    ]


ART_GUIDES_MAX = 8
ART_XHDR_DOUBLES = 26
ART_ANALYSIS_DOUBLES = 64
ART_JOB_AUTOPLACE, ART_JOB_MANUAL, ART_JOB_SUMS = range(3)


class ArtAnalysisJob(C.Structure):
    _fields_ = [
        ("b", ArtBundleView),
        ("w", C.c_void_p),
        ("distance", C.c_double),
        ("mode", C.c_int32),
        ("reserved", C.c_int32),
        ("centre", C.c_double * 3),
        ("normal", C.c_double * 3),
        ("refpoint", C.c_double * 3),
        ("sums", C.c_void_p),
    ]


ART_HIST_DETECTOR, ART_HIST_FRAME = range(2)
ART_HAXIS_X, ART_HAXIS_Y, ART_HAXIS_DELAY = 0, 1, 3
ART_HIST_MAX_BINS = 1 << 24


class ArtHistogramDesc(C.Structure):
    _fields_ = [
        ("source", C.c_int32), ("ndim", C.c_int32),
        ("axis", C.c_int32 * 3),
        ("bins", C.c_int32 * 3),
        ("wshift", C.c_int32),
        ("reserved", C.c_int32),
        ("lo", C.c_double * 3), ("hi", C.c_double * 3),
        ("delay_centre", C.c_double),
        ("map", ArtDetectorDesc),
    ]


ART_FOCAL_MAX_PIXELS = 2048
ART_FOCAL_MAX_PLANES = 64


class ArtFocalDesc(C.Structure):
    _fields_ = [
        ("det", ArtDetectorDesc),
        ("k", C.c_double), ("L_ref", C.c_double),
        ("x0", C.c_double), ("dx", C.c_double),
        ("y0", C.c_double), ("dy", C.c_double),
        ("nx", C.c_int32), ("ny", C.c_int32),
        ("planes", C.c_int32),
        ("reserved", C.c_int32),
        ("shift", C.c_double * ART_FOCAL_MAX_PLANES),
    ]


ART_FOCAL_MAX_WAVENUMBERS = 1024


class ArtFocalSpectrumDesc(C.Structure):
    _fields_ = [
        ("f", ArtFocalDesc),
        ("dk", C.c_double),
        ("nk", C.c_int32),
        ("reserved", C.c_int32),
    ]


class ArtFocalChromaticDesc(C.Structure):
    _fields_ = [
        ("f", ArtFocalDesc),
        ("axis", C.c_double * 3),
        ("nk", C.c_int32),
        ("reserved", C.c_int32),
    ]


ART_WAVEFRONT_MAX_ORDER = 10
ART_WAVEFRONT_MAX_COLS = 68
ART_WAVEFRONT_DOUBLES = 2360


class ArtWavefrontJob(C.Structure):
    _fields_ = [
        ("det", ArtDetectorDesc),
        ("b", ArtBundleView),
        ("w", C.c_void_p),
        ("n", C.c_int64),
        ("ref", C.c_double * 3),
        ("L_ref", C.c_double),
        ("pupil", C.c_double * 3),
        ("order", C.c_int32),
        ("reserved", C.c_int32),
        ("opd", C.c_void_p),
        ("pupil_x", C.c_void_p),
        ("pupil_y", C.c_void_p),
        ("out", C.c_void_p),
    ]


ART_COATING_MAX_LAYERS = 256
ART_COATING_MAX_MATERIALS = 6
ART_POLARISATION_MAX_ELEMS = 64
ART_POLARISATION_DOUBLES = 16


class ArtCoatingMaterial(C.Structure):
    _fields_ = [("n", C.c_double), ("kappa", C.c_double)]


class ArtCoatingLayer(C.Structure):
    _fields_ = [("thickness", C.c_double), ("roughness", C.c_double), ("material", C.c_int32), ("reserved", C.c_int32)]


class ArtCoating(C.Structure):
    _fields_ = [
        ("ideal", C.c_int32),
        ("n_materials", C.c_int32),
        ("n_layers", C.c_int32),
        ("substrate", C.c_int32),
        ("roughness", C.c_double),
        ("reserved", C.c_double),
        ("materials", ArtCoatingMaterial * ART_COATING_MAX_MATERIALS),
        ("layers", ArtCoatingLayer * ART_COATING_MAX_LAYERS),
    ]


class ArtPolarisationJob(C.Structure):
    _fields_ = [
        ("views", C.c_void_p),
        ("coating", C.c_int32 * ART_POLARISATION_MAX_ELEMS),
        ("n_elems", C.c_int32),
        ("polarised", C.c_int32),
        ("n", C.c_int64),
        ("pol", C.c_double * 6),
        ("k", C.c_double),
        ("has_det", C.c_int32),
        ("reserved", C.c_int32),
        ("det", ArtDetectorDesc),
        ("w0", C.c_void_p),
        ("w", C.c_void_p),
        ("w_out", C.c_void_p),
        ("field", C.c_void_p),
        ("out", C.c_void_p),
    ]


ART_TUBE_POINT, ART_TUBE_PLANE = range(2)
ART_TUBE_MAX_ELEMS = 64
ART_TUBE_MAX_JOBS = 64
ART_TUBE_DOUBLES = 16


class ArtTubeJob(C.Structure):
    _fields_ = [
        ("views", C.c_void_p),
        ("elems", C.c_void_p),
        ("quadrics", C.c_void_p),
        ("n_elems", C.c_int32),
        ("seed", C.c_int32),
        ("has_detector", C.c_int32),
        ("reserved", C.c_int32),
        ("det", ArtDetectorDesc),
        ("w", C.c_void_p),
        ("n", C.c_int64),
        ("weight", C.c_void_p),
        ("solid_angle", C.c_void_p),
        ("area", C.c_void_p),
        ("kappa1", C.c_void_p),
        ("kappa2", C.c_void_p),
        ("axis", C.c_void_p),
    ]


ART_SENS_DOUBLES = 16
ART_SENS_COLS = 6


class ArtSensitivityJob(C.Structure):
    _fields_ = [
        ("views", C.c_void_p),
        ("elems", C.c_void_p),
        ("quadrics", C.c_void_p),
        ("n_elems", C.c_int32),
        ("reserved", C.c_int32),
        ("n", C.c_int64),
        ("det", ArtDetectorDesc),
        ("w", C.c_void_p),
        ("origin", C.c_double * 3),
        ("dX", C.c_void_p),
        ("dY", C.c_void_p),
        ("dL", C.c_void_p),
    ]


ART_ALIGN_MAX_DOFS = 8
ART_ALIGN_PILOT = 1024
ART_ALIGN_DOF_DETECTOR = -1
ART_ALIGN_CENTRES = 8
ART_ALIGN_MEANS = 32
ART_ALIGN_CROSS = 56
ART_ALIGN_PAIRS = 80
ART_ALIGN_DOUBLES = 192


class ArtAlignmentJob(C.Structure):
    _fields_ = [
        ("views", C.c_void_p),
        ("elems", C.c_void_p),
        ("quadrics", C.c_void_p),
        ("n_elems", C.c_int32),
        ("n_dofs", C.c_int32),
        ("n", C.c_int64),
        ("det", ArtDetectorDesc),
        ("w", C.c_void_p),
        ("origin", C.c_double * 3),
        ("dofs", C.c_int32 * ART_ALIGN_MAX_DOFS),
    ]


ART_FOCAL_VECTOR_SCRATCH_DEFAULT = 1 << 29


class ArtFocalVectorSpectrumDesc(C.Structure):
    _fields_ = [
        ("s", ArtFocalSpectrumDesc),
        ("views", C.c_void_p),
        ("coating", C.c_int32 * ART_POLARISATION_MAX_ELEMS),
        ("n_elems", C.c_int32),
        ("n_coatings", C.c_int32),
        ("n", C.c_int64),
        ("pol", C.c_double * 6),
        ("w", C.c_void_p),
        ("materials", C.c_void_p),
        ("scratch_bound", C.c_int64),
    ]


class ArtFocalVectorChromaticDesc(C.Structure):
    _fields_ = [
        ("v", ArtFocalVectorSpectrumDesc),
        ("axis", C.c_double * 3),
    ]


ART_FOCAL_MAX_GROUPS = 1 << 20


class ArtFocalImageDesc(C.Structure):
    _fields_ = [
        ("f", ArtFocalDesc),
        ("groups", C.c_int32),
        ("reserved", C.c_int32),
        ("seg", C.c_void_p),
    ]


ART_QKEY_GIVEN, ART_QKEY_RADIUS, ART_QKEY_X, ART_QKEY_Y, ART_QKEY_DELAY = range(5)
ART_QUANTILE_MAX_FRACTIONS = 16
ART_QUANTILE_MAX_THRESHOLDS = 256
ART_QUANTILE_SCRATCH_DEFAULT = 1 << 28


class ArtQuantileDesc(C.Structure):
    _fields_ = [
        ("key", C.c_int32), ("planes", C.c_int32),
        ("n_fractions", C.c_int32), ("n_thresholds", C.c_int32),
        ("wshift", C.c_int32), ("centre_given", C.c_int32),
        ("scratch_bound", C.c_int64),
        ("keys", C.c_void_p), ("alive", C.c_void_p),
        ("thresholds_dev", C.c_void_p), ("thresholds_host", C.c_void_p),
        ("values", C.c_void_p), ("below", C.c_void_p), ("upto", C.c_void_p), ("totals", C.c_void_p),
        ("rank_sums", C.c_void_p), ("rank_counts", C.c_void_p), ("centres_out", C.c_void_p),
        ("fraction", C.c_double * ART_QUANTILE_MAX_FRACTIONS),
        ("det", ArtDetectorDesc),
        ("shift", C.c_double * ART_FOCAL_MAX_PLANES),
        ("centre", (C.c_double * 3) * ART_FOCAL_MAX_PLANES),
    ]


# name -> (restype, argtypes); the loader checks every symbol exists (tests/test_abi.py does too)
PROTOTYPES = {
    "art_abi_version": (C.c_int, []),
    "art_last_error": (C.c_char_p, []),
    "art_device_count": (C.c_int, []),
    "art_trace_element": (C.c_int, [C.POINTER(ArtElementDesc), C.POINTER(ArtBundleView), C.POINTER(ArtBundleView),
                                    C.c_int64, C.c_void_p]),
    "art_trace_grating": (C.c_int, [C.POINTER(ArtElementDesc), C.POINTER(ArtGratingDesc), c_double_p,
                                    C.POINTER(ArtBundleView), C.POINTER(ArtBundleView), C.c_int64, C.c_void_p]),
    "art_trace_quadric": (C.c_int, [C.POINTER(ArtElementDesc), C.POINTER(ArtQuadricDesc), C.POINTER(ArtBundleView),
                                    C.POINTER(ArtBundleView), C.c_int64, C.c_void_p]),
    "art_trace_freeform": (C.c_int, [C.POINTER(ArtElementDesc), C.POINTER(ArtQuadricDesc), C.POINTER(ArtFigureDesc),
                                     C.POINTER(ArtBundleView), C.POINTER(ArtBundleView), C.c_int64, C.c_void_p]),
    "art_trace_chain": (C.c_int, [C.POINTER(ArtElementDesc), C.c_int32, C.POINTER(ArtBundleView),
                                  C.POINTER(ArtBundleView), C.c_int64, C.c_void_p]),
    "art_scene_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "art_chain_readout_scratch_doubles": (C.c_int64, [C.c_int64]),
    "art_trace_chain_readout": (C.c_int, [C.POINTER(ArtElementDesc), C.c_int32, C.POINTER(ArtBundleView),
                                          C.POINTER(ArtBundleView), C.POINTER(ArtChainReadout), C.c_int64, C.c_void_p]),
    "art_scene_pack": (C.c_int, [C.POINTER(ArtElementDesc), C.c_int32, C.c_int32, C.POINTER(ArtBundleView),
                                 C.POINTER(ArtBundleView), C.POINTER(ArtChainReadout), C.c_void_p]),
    "art_trace_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "art_row_summary_bytes": (C.c_int64, []),
    "art_bundle_row_summary": (C.c_int, [C.POINTER(ArtBundleView), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "art_scene_set_row_summaries": (C.c_int, [C.c_void_p, C.c_void_p]),
    "art_pack_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ArtBundleView), C.c_void_p]),
    "art_transform_bundle": (C.c_int, [c_double_p, c_double_p, C.c_int32, C.POINTER(ArtBundleView),
                                       C.POINTER(ArtBundleView), C.c_int64, C.c_void_p]),
    "art_detector": (C.c_int, [C.POINTER(ArtDetectorDesc), C.POINTER(ArtBundleView), C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_detector_readout": (C.c_int, [C.POINTER(ArtDetectorDesc), C.POINTER(ArtBundleView), C.c_void_p, C.c_int64,
                                       C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 9),
    "art_detector_scan_moments": (C.c_int, [C.POINTER(ArtDetectorDesc), C.POINTER(ArtBundleView), C.c_void_p,
                                            C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "art_histogram": (C.c_int, [C.POINTER(ArtHistogramDesc), C.POINTER(ArtBundleView), C.c_void_p, C.c_int64, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_focal_scratch_doubles": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "art_focal_field": (C.c_int, [C.POINTER(ArtFocalDesc), C.POINTER(ArtBundleView), C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "art_focal_spectrum_scratch_doubles": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "art_focal_spectrum": (C.c_int, [C.POINTER(ArtFocalSpectrumDesc), C.POINTER(ArtBundleView), C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_focal_chromatic_scratch_doubles": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "art_focal_chromatic": (C.c_int, [C.POINTER(ArtFocalChromaticDesc), C.POINTER(ArtBundleView), C.POINTER(ArtBundleView),
                                      C.c_void_p, C.c_int64, C.c_void_p, c_double_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_wavefront_scratch_doubles": (C.c_int64, [C.POINTER(ArtWavefrontJob), C.c_int32]),
    "art_wavefront": (C.c_int, [C.c_void_p, C.POINTER(ArtWavefrontJob), C.c_int32, C.c_void_p, C.c_void_p]),
    "art_polarisation_scratch_doubles": (C.c_int64, [C.POINTER(ArtPolarisationJob), C.c_int32]),
    "art_polarisation": (C.c_int, [C.c_void_p, C.POINTER(ArtPolarisationJob), C.c_int32, C.c_void_p,
                                   C.POINTER(ArtCoating), C.c_int32, C.c_void_p, C.c_void_p]),
    "art_ray_tubes_scratch_doubles": (C.c_int64, [C.POINTER(ArtTubeJob), C.c_int32]),
    "art_ray_tubes": (C.c_int, [C.c_void_p, C.POINTER(ArtTubeJob), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_sensitivities_scratch_doubles": (C.c_int64, [C.POINTER(ArtSensitivityJob), C.c_int32]),
    "art_sensitivities": (C.c_int, [C.c_void_p, C.POINTER(ArtSensitivityJob), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_alignment_sums_scratch_doubles": (C.c_int64, [C.POINTER(ArtAlignmentJob), C.c_int32]),
    "art_alignment_sums": (C.c_int, [C.c_void_p, C.POINTER(ArtAlignmentJob), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_focal_vector_spectrum_scratch_doubles": (C.c_int64, [C.POINTER(ArtFocalVectorSpectrumDesc)]),
    "art_focal_vector_spectrum": (C.c_int, [C.POINTER(ArtFocalVectorSpectrumDesc), C.POINTER(ArtBundleView), C.c_void_p,
                                            C.POINTER(ArtCoating), C.POINTER(ArtCoatingMaterial), C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "art_focal_vector_chromatic_scratch_doubles": (C.c_int64, [C.POINTER(ArtFocalVectorChromaticDesc)]),
    "art_focal_vector_chromatic": (C.c_int, [C.POINTER(ArtFocalVectorChromaticDesc), C.POINTER(ArtBundleView),
                                             C.POINTER(ArtBundleView), C.c_void_p, C.POINTER(ArtCoating),
                                             C.POINTER(ArtCoatingMaterial), C.c_void_p, c_double_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    "art_focal_image_scratch_doubles": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "art_focal_image": (C.c_int, [C.POINTER(ArtFocalImageDesc), C.POINTER(ArtBundleView), C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_quantile_scratch_doubles": (C.c_int64, [C.POINTER(ArtQuantileDesc), C.c_int64]),
    "art_quantiles": (C.c_int, [C.POINTER(ArtQuantileDesc), C.POINTER(ArtBundleView), C.c_void_p, C.c_int64, C.c_void_p,
                                C.c_void_p]),
    "art_reduce_scratch_doubles": (C.c_int64, []),
    "art_detector_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_detector_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_bundle_sums": (C.c_int, [C.POINTER(ArtBundleView), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "art_gaussian_intensity": (C.c_int, [C.POINTER(ArtBundleView), c_double_p, C.c_double, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "art_gaussian_intensity_central": (C.c_int, [C.POINTER(ArtBundleView), C.c_double, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "art_bundle_max_angle": (C.c_int, [C.POINTER(ArtBundleView), c_double_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "art_compact_scratch_ints": (C.c_int64, [C.c_int64]),
    "art_compact": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_make_source": (C.c_int, [C.c_int32, C.c_double, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_int64,
                                  C.POINTER(ArtBundleView), C.c_void_p]),
    "art_make_source_strided": (C.c_int, [C.c_int32, C.c_double, c_double_p, c_double_p, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_int64, C.POINTER(ArtBundleView), C.c_void_p]),
    "art_exchange_pack": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p]),
    "art_exchange_fold": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "art_survivor_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "art_pack_survivors": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p,
                                                                                    C.c_void_p, C.c_int64, C.c_void_p]),
    "art_survivor_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_survivor_xheader": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_trace_guides": (C.c_int, [C.POINTER(ArtElementDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "art_analysis_scratch_doubles": (C.c_int64, [C.c_int32, C.c_int64]),
    "art_analyse_bundles": (C.c_int, [C.c_void_p, C.POINTER(ArtAnalysisJob), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "art_make_extended_source": (C.c_int, [C.c_double, C.c_double, C.c_int64, C.c_int64, c_double_p, c_double_p,
                                           C.c_int64, C.c_int64, C.POINTER(ArtBundleView), C.c_void_p]),
}


def bind(lib, prefix="art_"):
    """Attach restype/argtypes for every exported entry point; raises AttributeError if one is missing."""
    fns = {}
    for name, (res, args) in PROTOTYPES.items():
        sym = name if prefix == "art_" else prefix + name[len("art_"):]
        f = getattr(lib, sym)
        f.restype = res
        f.argtypes = args
        fns[name] = f
    return fns

"""ctypes declarations for include/stacker.h (the C ABI of libstacker_amd.so).

This is plumbing for tests and bench.py; a Rust `libstacker` shim binds the same symbols
(INTEGRATION.md). There is no fallback: if the shared library is missing or fails to load,
importing it raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STACKER_AMD_LIB") or os.path.join(_HERE, "libstacker_amd.so")   # override: A/B builds

c_status = C.c_int


class KeypointParams(C.Structure):
    _fields_ = [("method", C.c_int32), ("ransac_reproj_threshold", C.c_double),
                ("match_keep_ratio", C.c_float), ("match_ratio", C.c_float),
                ("border_mode", C.c_int32), ("border_value", C.c_double * 4)]


class EccParams(C.Structure):
    _fields_ = [("motion_type", C.c_int32), ("has_max_count", C.c_int32), ("max_count", C.c_int32),
                ("has_epsilon", C.c_int32), ("epsilon", C.c_double), ("gauss_filt_size", C.c_int32)]


class Frames(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_void_p)), ("n", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("channels", C.c_int32), ("depth", C.c_int32),
                ("location", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class FrameGeometry(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class ImageF32(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("channels", C.c_int32), ("location", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class FrameStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("rho", C.c_double),
                ("n_keypoints", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32),
                ("reserved", C.c_int32), ("warp", C.c_double * 9)]


class ClipParams(C.Structure):
    _fields_ = [("kappa_low", C.c_float), ("kappa_high", C.c_float), ("iterations", C.c_int32), ("reserved", C.c_int32)]


class RobustClipParams(C.Structure):
    _fields_ = [("kappa_low", C.c_float), ("kappa_high", C.c_float), ("sigma_floor", C.c_float), ("iterations", C.c_int32)]


class QuantileParams(C.Structure):
    _fields_ = [("quantile", C.c_float), ("reserved", C.c_int32)]


class WeightParams(C.Structure):
    _fields_ = [("normalize", C.c_int32), ("coverage", C.c_int32), ("stat_step", C.c_int32), ("reserved", C.c_int32)]


class FrameWeight(C.Structure):
    _fields_ = [("gain", C.c_float * 4), ("offset", C.c_float * 4), ("weight", C.c_float), ("flags", C.c_int32)]


class LocalParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("threshold", C.c_int32), ("power", C.c_int32), ("floor", C.c_float),
                ("reserved", C.c_int32 * 2)]


class LocalNormParams(C.Structure):
    _fields_ = [("step", C.c_int32), ("stat_step", C.c_int32), ("normalize", C.c_int32), ("coverage", C.c_int32),
                ("min_count", C.c_int32), ("fill", C.c_int32), ("reserved", C.c_int32 * 2)]


class MeshParams(C.Structure):
    _fields_ = [("step", C.c_int32), ("radius", C.c_int32), ("max_iters", C.c_int32), ("epsilon", C.c_float),
                ("max_shift", C.c_float), ("min_eig", C.c_float), ("fill", C.c_int32), ("reserved", C.c_int32)]


class DrizzleParams(C.Structure):
    _fields_ = [("scale", C.c_float), ("pixfrac", C.c_float), ("origin_x", C.c_float), ("origin_y", C.c_float),
                ("fill", C.c_float), ("reserved", C.c_int32)]


class RejectParams(C.Structure):
    _fields_ = [("snr1", C.c_float), ("snr2", C.c_float), ("scale1", C.c_float), ("scale2", C.c_float),
                ("read_noise", C.c_float), ("poisson_gain", C.c_float), ("min_count", C.c_int32), ("reserved", C.c_int32)]


class SelectParams(C.Structure):
    _fields_ = [("metric", C.c_int32), ("ksize", C.c_int32), ("drop_worst", C.c_int32), ("keep_fraction", C.c_float),
                ("weight_mode", C.c_int32), ("reserved", C.c_int32)]


class Star(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("flux", C.c_float), ("px", C.c_int32), ("py", C.c_int32),
                ("peak", C.c_int32), ("npix", C.c_int32), ("reserved", C.c_int32)]


class StarParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("kappa", C.c_float), ("min_contrast", C.c_int32), ("min_pixels", C.c_int32),
                ("max_stars", C.c_int32), ("match_stars", C.c_int32), ("neighbours", C.c_int32), ("tri_tolerance", C.c_double),
                ("min_votes", C.c_int32), ("refine", C.c_int32), ("min_stars", C.c_int32), ("min_inliers", C.c_int32),
                ("method", C.c_int32), ("ransac_reproj_threshold", C.c_double), ("border_mode", C.c_int32),
                ("border_value", C.c_double * 4)]


class StarDeepParams(C.Structure):
    _fields_ = [("f32_scale", C.c_float), ("reserved", C.c_int32)]


class StarMeasureParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("ring_inner", C.c_int32), ("ring_outer", C.c_int32), ("kappa", C.c_float),
                ("min_contrast", C.c_int32), ("min_pixels", C.c_int32), ("saturation", C.c_int32), ("reserved", C.c_int32)]


class StarShape(C.Structure):
    _fields_ = [("S", C.c_int64), ("Sx", C.c_int64), ("Sy", C.c_int64), ("Sxx", C.c_int64), ("Syy", C.c_int64), ("Sxy", C.c_int64),
                ("px", C.c_int32), ("py", C.c_int32), ("bg", C.c_int32), ("mad", C.c_int32), ("thr", C.c_int32), ("npix", C.c_int32),
                ("peak", C.c_int32), ("n_ring", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("x", C.c_double), ("y", C.c_double), ("cxx", C.c_double), ("cyy", C.c_double), ("cxy", C.c_double),
                ("fwhm", C.c_double), ("ecc", C.c_double), ("snr", C.c_double)]


class StarQuality(C.Structure):
    _fields_ = [("fwhm", C.c_double), ("ecc", C.c_double), ("snr", C.c_double), ("bg", C.c_double), ("noise", C.c_double),
                ("n_stars", C.c_int32), ("n_measured", C.c_int32)]


class StarQualityParams(C.Structure):
    _fields_ = [("fwhm_max", C.c_double), ("ecc_max", C.c_double), ("min_measured", C.c_int32), ("fwhm_power", C.c_int32),
                ("ecc_power", C.c_int32), ("snr_power", C.c_int32), ("reserved", C.c_int32)]


class NoiseStat(C.Structure):
    _fields_ = [("median", C.c_int32), ("mad", C.c_int32), ("res_median", C.c_int32), ("flags", C.c_int32),
                ("sigma", C.c_double), ("kept", C.c_int64)]


class BgCell(C.Structure):
    _fields_ = [("n", C.c_int32), ("kept", C.c_int32), ("med", C.c_int32), ("mad", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32),
                ("reserved", C.c_int32 * 2), ("sum", C.c_int64), ("sum2", C.c_uint64)]


class BackgroundParams(C.Structure):
    _fields_ = [("step", C.c_int32), ("clip_iters", C.c_int32), ("kappa", C.c_float), ("f32_scale", C.c_float),
                ("estimator", C.c_int32), ("min_count", C.c_int32), ("max_reject", C.c_float), ("recentre", C.c_int32),
                ("filter", C.c_int32), ("fill", C.c_int32), ("target", C.c_float * 4), ("out_depth", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class DeconvParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("radius", C.c_int32), ("floor", C.c_float), ("pedestal", C.c_float),
                ("lambda", C.c_float), ("tv_eps", C.c_float), ("amount", C.c_float), ("reserved", C.c_int32)]


class WaveletParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("mode", C.c_int32), ("sigma_given", C.c_int32), ("reserved", C.c_int32),
                ("gain", C.c_float * 8), ("threshold", C.c_float * 8), ("layer_amount", C.c_float * 8),
                ("residual_gain", C.c_float), ("amount", C.c_float), ("sigma", C.c_float * 4)]


class ImageStat(C.Structure):
    _fields_ = [("count", C.c_int64), ("min", C.c_float), ("max", C.c_float), ("median", C.c_float), ("mad", C.c_float),
                ("q", C.c_float * 4)]


class StretchParams(C.Structure):
    _fields_ = [("curve", C.c_int32), ("colour", C.c_int32), ("out_depth", C.c_int32), ("reserved", C.c_int32),
                ("black", C.c_float * 4), ("white", C.c_float * 4), ("midtone", C.c_float * 4), ("out_scale", C.c_float)]


class StretchAutoParams(C.Structure):
    _fields_ = [("shadows_clip", C.c_double), ("target_background", C.c_double), ("white", C.c_double),
                ("white_quantile", C.c_double), ("linked", C.c_int32), ("white_mode", C.c_int32)]


class ImageOut(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("depth", C.c_int32), ("location", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class HgProblem(C.Structure):
    _fields_ = [("src_pts", C.c_void_p), ("dst_pts", C.c_void_p), ("n", C.c_int32), ("inlier_mask_or_null", C.c_void_p)]


class HgOutcome(C.Structure):
    _fields_ = [("rc", C.c_int32), ("found", C.c_int32), ("H", C.c_double * 9), ("n_inliers", C.c_int32),
                ("models_evaluated", C.c_int32)]


class Calibration(C.Structure):
    _fields_ = [("bias_or_null", C.POINTER(ImageF32)), ("dark_or_null", C.POINTER(ImageF32)), ("flat_or_null", C.POINTER(ImageF32)),
                ("dark_scale_or_null", C.c_void_p), ("flat_mean", C.c_float * 4), ("flat_min", C.c_float), ("pedestal", C.c_float),
                ("reserved", C.c_int32), ("defects_or_null", C.c_void_p), ("defects_location", C.c_int32),
                ("defect_step", C.c_int32), ("out_depth", C.c_int32), ("reserved2", C.c_int32)]


class DefectParams(C.Structure):
    _fields_ = [("tests", C.c_int32), ("high_abs", C.c_float), ("low_ratio", C.c_float), ("step", C.c_int32),
                ("accumulate", C.c_int32), ("reserved", C.c_int32)]


class Mosaic(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_void_p)), ("n", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("depth", C.c_int32), ("location", C.c_int32), ("pattern", C.c_int32), ("row_stride_bytes", C.c_size_t)]


class Timing(C.Structure):
    _fields_ = [("prep_ms", C.c_double), ("align_ms", C.c_double), ("warp_ms", C.c_double),
                ("finalize_ms", C.c_double), ("ecc_iter_launches", C.c_int64),
                ("ecc_slot_iterations", C.c_int64), ("warp_launches", C.c_int64),
                ("warp_frames", C.c_int64), ("ecc_iter_ms", C.c_double), ("ecc_iter_timed", C.c_int64),
                ("h2d_ms", C.c_double), ("h2d_bytes", C.c_int64), ("fast_ms", C.c_double), ("fast_launches", C.c_int64),
                ("fast_pixels", C.c_int64), ("ecc_ring_fallbacks", C.c_int64)]


# every symbol include/stacker.h declares, with its signature
SIGNATURES = {
    "stk_version": (C.c_char_p, []),
    "stk_create": (c_status, [C.c_int32, C.POINTER(C.c_void_p)]),
    "stk_create_multi": (c_status, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "stk_shard_moving_frames": (c_status, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stk_rccl_selftest": (c_status, [C.c_void_p, C.c_int64]),
    "stk_host_alloc": (c_status, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "stk_host_free": (None, [C.c_void_p]),
    "stk_destroy": (None, [C.c_void_p]),
    "stk_last_error": (C.c_char_p, [C.c_void_p]),
    "stk_set_stream": (c_status, [C.c_void_p, C.c_void_p]),
    "stk_get_timing": (c_status, [C.c_void_p, C.POINTER(Timing)]),
    "stk_get_counter": (c_status, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "stk_set_option": (c_status, [C.c_void_p, C.c_char_p, C.c_int64]),
    "stk_keypoint_match": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                      C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_keypoint_match_mixed": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(FrameGeometry), C.POINTER(KeypointParams),
                                            C.c_float, C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_ecc_match": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                 C.POINTER(ImageF32), C.POINTER(FrameStats)]),
    "stk_ecc_match_shard": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.c_int32,
                                       C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_keypoint_match_shard": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                            C.c_int32, C.POINTER(ImageF32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_finalize_mean": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_int64, C.POINTER(ImageF32)]),
    "stk_ecc_match_clipped": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(ClipParams),
                                         C.POINTER(ImageF32), C.c_void_p, C.POINTER(FrameStats)]),
    "stk_keypoint_match_clipped": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                              C.POINTER(ClipParams), C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p,
                                              C.POINTER(FrameStats)]),
    "stk_clip_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_double, C.POINTER(ClipParams), C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_quantile": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(QuantileParams),
                                          C.POINTER(ImageF32), C.POINTER(FrameStats)]),
    "stk_keypoint_match_quantile": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                               C.POINTER(QuantileParams), C.POINTER(ImageF32), C.POINTER(C.c_int32),
                                               C.POINTER(FrameStats)]),
    "stk_quantile_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_double, C.POINTER(QuantileParams), C.POINTER(ImageF32)]),
    "stk_ecc_match_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(WeightParams),
                                          C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_keypoint_match_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                               C.POINTER(WeightParams), C.c_void_p, C.POINTER(ImageF32), C.POINTER(C.c_int32),
                                               C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_weighted_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_double, C.POINTER(FrameWeight), C.c_int32, C.POINTER(ImageF32), C.c_void_p]),
    "stk_overlap_moments": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_double, C.c_int32, C.c_void_p]),
    "stk_local_sharpness": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(LocalParams), C.c_void_p]),
    "stk_local_weighted_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_double, C.POINTER(FrameWeight), C.c_void_p, C.c_float, C.c_int32,
                                            C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_local_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                C.POINTER(WeightParams), C.c_void_p, C.POINTER(LocalParams), C.POINTER(ImageF32),
                                                C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_keypoint_match_local_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                     C.POINTER(WeightParams), C.c_void_p, C.POINTER(LocalParams),
                                                     C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(FrameWeight),
                                                     C.POINTER(FrameStats)]),
    "stk_mesh_grid": (c_status, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stk_local_align": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MeshParams), C.c_void_p,
                                   C.c_void_p]),
    "stk_mesh_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_double, C.c_void_p, C.c_int32, C.POINTER(ImageF32)]),
    "stk_mesh_local_weighted_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_double, C.POINTER(FrameWeight), C.c_void_p, C.c_float, C.c_int32,
                                                 C.c_void_p, C.c_int32, C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_local_aligned": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(MeshParams),
                                               C.POINTER(LocalParams), C.POINTER(ImageF32), C.POINTER(FrameStats)]),
    "stk_keypoint_match_local_aligned": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                    C.POINTER(MeshParams), C.POINTER(LocalParams), C.POINTER(ImageF32),
                                                    C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_grey_pyramid": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_int32, C.c_void_p]),
    "stk_local_align_pyramid": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MeshParams),
                                           C.c_int32, C.c_void_p, C.c_void_p]),
    "stk_ecc_match_local_aligned_pyramid": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                       C.POINTER(MeshParams), C.c_int32, C.POINTER(LocalParams), C.POINTER(ImageF32),
                                                       C.POINTER(FrameStats)]),
    "stk_keypoint_match_local_aligned_pyramid": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                            C.POINTER(MeshParams), C.c_int32, C.POINTER(LocalParams),
                                                            C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_drizzle_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                     C.POINTER(DrizzleParams), C.POINTER(FrameWeight), C.c_void_p, C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_drizzle": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(DrizzleParams),
                                         C.POINTER(ImageF32), C.c_void_p, C.POINTER(FrameStats)]),
    "stk_keypoint_match_drizzle": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                              C.POINTER(DrizzleParams), C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p,
                                              C.POINTER(FrameStats)]),
    "stk_mesh_drizzle_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                          C.POINTER(DrizzleParams), C.POINTER(FrameWeight), C.c_void_p, C.c_void_p, C.c_int32,
                                          C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_local_aligned_drizzle": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                       C.POINTER(MeshParams), C.POINTER(DrizzleParams), C.POINTER(ImageF32), C.c_void_p,
                                                       C.POINTER(FrameStats)]),
    "stk_keypoint_match_local_aligned_drizzle": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                            C.POINTER(MeshParams), C.POINTER(DrizzleParams), C.POINTER(ImageF32),
                                                            C.POINTER(C.c_int32), C.c_void_p, C.POINTER(FrameStats)]),
    "stk_reject_maps": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.POINTER(FrameWeight),
                                   C.c_void_p, C.c_void_p, C.POINTER(RejectParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "stk_ecc_match_drizzle_rejected": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                  C.POINTER(DrizzleParams), C.POINTER(WeightParams), C.c_void_p,
                                                  C.POINTER(RejectParams), C.POINTER(ImageF32), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_keypoint_match_drizzle_rejected": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                       C.POINTER(DrizzleParams), C.POINTER(WeightParams), C.c_void_p,
                                                       C.POINTER(RejectParams), C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_clip_stack_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_double, C.POINTER(ClipParams), C.POINTER(FrameWeight), C.c_int32, C.POINTER(ImageF32),
                                           C.c_void_p, C.c_void_p]),
    "stk_quantile_stack_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                               C.c_double, C.POINTER(QuantileParams), C.POINTER(FrameWeight), C.c_int32,
                                               C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_clipped_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(ClipParams),
                                                  C.POINTER(WeightParams), C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.c_void_p,
                                                  C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_keypoint_match_clipped_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                       C.POINTER(ClipParams), C.POINTER(WeightParams), C.c_void_p, C.POINTER(ImageF32),
                                                       C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.POINTER(FrameWeight),
                                                       C.POINTER(FrameStats)]),
    "stk_ecc_match_quantile_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                   C.POINTER(QuantileParams), C.POINTER(WeightParams), C.c_void_p, C.POINTER(ImageF32),
                                                   C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_keypoint_match_quantile_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                        C.POINTER(QuantileParams), C.POINTER(WeightParams), C.c_void_p,
                                                        C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(FrameWeight),
                                                        C.POINTER(FrameStats)]),
    "stk_ecc_match_robust_clipped": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                C.POINTER(RobustClipParams), C.POINTER(ImageF32), C.c_void_p, C.POINTER(FrameStats)]),
    "stk_keypoint_match_robust_clipped": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                     C.POINTER(RobustClipParams), C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p,
                                                     C.POINTER(FrameStats)]),
    "stk_robust_clip_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_double, C.POINTER(RobustClipParams), C.POINTER(ImageF32), C.c_void_p]),
    "stk_robust_clip_stack_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_double, C.POINTER(RobustClipParams), C.POINTER(FrameWeight),
                                                  C.c_int32, C.POINTER(ImageF32), C.c_void_p, C.c_void_p]),
    "stk_ecc_match_robust_clipped_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                         C.POINTER(RobustClipParams), C.POINTER(WeightParams), C.c_void_p,
                                                         C.POINTER(ImageF32), C.c_void_p, C.c_void_p, C.POINTER(FrameWeight),
                                                         C.POINTER(FrameStats)]),
    "stk_keypoint_match_robust_clipped_weighted": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                              C.POINTER(RobustClipParams), C.POINTER(WeightParams), C.c_void_p,
                                                              C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                                              C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_local_moments": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_double, C.c_int32, C.c_int32, C.c_void_p]),
    "stk_local_norm_estimate": (c_status, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(LocalNormParams), C.c_void_p, C.c_void_p,
                                           C.POINTER(FrameWeight), C.c_void_p]),
    "stk_local_norm_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_double, C.POINTER(FrameWeight), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ImageF32),
                                        C.c_void_p]),
    "stk_quantile_stack_local_norm": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p, C.c_double, C.POINTER(QuantileParams), C.POINTER(FrameWeight),
                                                 C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ImageF32), C.c_void_p]),
    "stk_ecc_match_local_normalized": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                  C.POINTER(LocalNormParams), C.POINTER(QuantileParams), C.c_void_p,
                                                  C.POINTER(ImageF32), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FrameWeight),
                                                  C.POINTER(FrameStats)]),
    "stk_keypoint_match_local_normalized": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                       C.POINTER(LocalNormParams), C.POINTER(QuantileParams), C.c_void_p,
                                                       C.POINTER(ImageF32), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_clip_stack_local_norm": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_double, C.POINTER(ClipParams), C.POINTER(FrameWeight), C.c_void_p, C.c_int32,
                                             C.c_int32, C.POINTER(ImageF32), C.c_void_p, C.c_void_p]),
    "stk_robust_clip_stack_local_norm": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                    C.c_void_p, C.c_double, C.POINTER(RobustClipParams), C.POINTER(FrameWeight),
                                                    C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ImageF32), C.c_void_p, C.c_void_p]),
    "stk_ecc_match_local_normalized_clipped": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float,
                                                          C.POINTER(LocalNormParams), C.POINTER(ClipParams),
                                                          C.POINTER(RobustClipParams), C.c_void_p, C.POINTER(ImageF32), C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_keypoint_match_local_normalized_clipped": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                                               C.POINTER(LocalNormParams), C.POINTER(ClipParams),
                                                               C.POINTER(RobustClipParams), C.c_void_p, C.POINTER(ImageF32),
                                                               C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                                               C.POINTER(FrameWeight), C.POINTER(FrameStats)]),
    "stk_star_detect": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(StarParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "stk_star_match_lists": (c_status, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(StarParams), C.c_void_p,
                                        C.POINTER(C.c_int32)]),
    "stk_star_align": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(StarParams), C.POINTER(C.c_int32),
                                  C.POINTER(FrameStats)]),
    "stk_star_match": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(StarParams), C.POINTER(ImageF32), C.POINTER(C.c_int32),
                                  C.POINTER(FrameStats)]),
    # (the deep star calls take their stk_frames by address, as a void pointer, like the noise calls below: api.py passes
    # byref(m.c_frames) all the same, and tests/test_cpu_star_deep.py reads the structure back through that address)
    "stk_star_detect_deep": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(StarParams), C.POINTER(StarDeepParams), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "stk_star_align_deep": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(StarParams), C.POINTER(StarDeepParams), C.POINTER(C.c_int32),
                                       C.POINTER(FrameStats)]),
    "stk_star_match_deep": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(StarParams), C.POINTER(StarDeepParams), C.c_double,
                                       C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    # (star measurement: the stk_frames by address as a void pointer, like the deep star calls above)
    "stk_star_measure": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(StarDeepParams), C.POINTER(StarMeasureParams), C.c_void_p,
                                    C.c_void_p, C.c_int32, C.POINTER(StarShape)]),
    "stk_star_shape_derive": (c_status, [C.POINTER(StarShape), C.c_int32]),
    "stk_star_frame_quality": (c_status, [C.POINTER(StarShape), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(StarQuality)]),
    "stk_star_quality_scores": (c_status, [C.POINTER(StarQuality), C.c_int32, C.c_void_p]),
    "stk_star_quality_weights": (c_status, [C.POINTER(StarQuality), C.c_int32, C.POINTER(StarQualityParams), C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "stk_star_match_quality_weighted": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(StarParams), C.POINTER(StarDeepParams),
                                                   C.POINTER(StarMeasureParams), C.POINTER(StarQualityParams), C.c_double, C.c_int32,
                                                   C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_int32), C.POINTER(FrameWeight), C.POINTER(FrameStats),
                                                   C.POINTER(StarQuality)]),
    "stk_calibrate": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(Calibration), C.c_void_p, C.c_size_t]),
    "stk_defect_map": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.POINTER(DefectParams), C.c_void_p, C.c_int32, C.c_void_p]),
    "stk_image_mean": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_void_p]),
    "stk_master_stack": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_int32, C.c_int32, C.POINTER(RobustClipParams),
                                    C.POINTER(ImageF32), C.c_void_p]),
    "stk_demosaic": (c_status, [C.c_void_p, C.POINTER(Mosaic), C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "stk_cfa_mask": (c_status, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "stk_grey":(c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p]),
    "stk_convert_f32": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_double, C.c_void_p]),
    "stk_hybrid_match": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.POINTER(EccParams),
                                    C.POINTER(ImageF32), C.POINTER(FrameStats)]),
    "stk_hybrid_match_shard": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.POINTER(EccParams), C.c_int32,
                                          C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_imread": (c_status, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stk_keypoint_match_files": (c_status, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(KeypointParams), C.c_float,
                                            C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "stk_ecc_match_files": (c_status, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(EccParams), C.c_float,
                                       C.POINTER(ImageF32), C.POINTER(FrameStats)]),
    "stk_hybrid_match_files": (c_status, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(KeypointParams),
                                          C.POINTER(EccParams), C.POINTER(ImageF32), C.POINTER(FrameStats)]),
    "stk_sharpness": (c_status, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.POINTER(C.c_double)]),
    "stk_stack_sharpness": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_int32, C.c_void_p]),
    "stk_rank_frames": (c_status, [C.c_void_p, C.c_int32, C.POINTER(SelectParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.c_void_p]),
    "stk_ecc_match_ranked": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(EccParams), C.c_float, C.POINTER(ImageF32),
                                        C.POINTER(FrameStats), C.POINTER(SelectParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.c_void_p]),
    "stk_keypoint_match_ranked": (c_status, [C.c_void_p, C.POINTER(Frames), C.POINTER(KeypointParams), C.c_float,
                                             C.POINTER(ImageF32), C.POINTER(C.c_int32), C.POINTER(FrameStats),
                                             C.POINTER(SelectParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "stk_noise_from_hist": (c_status, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(NoiseStat)]),
    # (the noise calls take their stk_frames by address, as a void pointer: api.py passes byref(m.c_frames) all the same, and
    # tests/test_cpu_noise.py reads the structure back through that address)
    "stk_stack_noise": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(NoiseStat), C.c_void_p]),
    "stk_noise_weights": (c_status, [C.POINTER(NoiseStat), C.c_int32, C.c_int32, C.POINTER(FrameWeight), C.c_void_p, C.c_void_p,
                                     C.c_double, C.c_void_p]),
    "stk_ecc_match_noise_weighted": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(EccParams), C.c_float, C.POINTER(WeightParams),
                                                C.c_void_p, C.c_double, C.POINTER(ImageF32), C.c_void_p, C.POINTER(FrameWeight),
                                                C.POINTER(FrameStats), C.POINTER(NoiseStat)]),
    "stk_keypoint_match_noise_weighted": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(KeypointParams), C.c_float,
                                                     C.POINTER(WeightParams), C.c_void_p, C.c_double, C.POINTER(ImageF32),
                                                     C.POINTER(C.c_int32), C.c_void_p, C.POINTER(FrameWeight), C.POINTER(FrameStats),
                                                     C.POINTER(NoiseStat)]),
    # (the background calls take their stk_frames by address, as a void pointer, like the noise and deep star calls above)
    "stk_background_cells": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(BackgroundParams), C.c_void_p, C.c_int32, C.POINTER(BgCell)]),
    "stk_background_estimate": (c_status, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(BackgroundParams), C.POINTER(BgCell),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "stk_background_apply": (c_status, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "stk_background_flatten": (c_status, [C.c_void_p, C.c_void_p, C.POINTER(BackgroundParams), C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(BgCell)]),
    "stk_deconvolve": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.POINTER(DeconvParams), C.c_void_p, C.c_size_t, C.c_int32,
                                  C.POINTER(ImageF32)]),
    "stk_psf_model": (c_status, [C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "stk_psf_from_shapes": (c_status, [C.POINTER(StarShape), C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "stk_wavelet_process": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.POINTER(WaveletParams), C.c_void_p, C.c_size_t, C.c_int32,
                                       C.POINTER(ImageF32), C.c_void_p]),
    "stk_wavelet_layers": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_int32, C.POINTER(ImageF32)]),
    "stk_wavelet_sigma": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.c_void_p]),
    "stk_wavelet_noise_table": (c_status, [C.c_int32, C.POINTER(C.c_double)]),
    "stk_image_stats": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_double), C.c_int32,
                                   C.POINTER(ImageStat)]),
    "stk_stretch": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.POINTER(StretchParams), C.c_void_p, C.c_int32, C.POINTER(ImageOut)]),
    "stk_stretch_auto": (c_status, [C.POINTER(ImageStat), C.c_int32, C.POINTER(StretchAutoParams), C.POINTER(StretchParams)]),
    "stk_stretch_table": (c_status, [C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_float)]),
    "stk_auto_stretch": (c_status, [C.c_void_p, C.POINTER(ImageF32), C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(StretchAutoParams),
                                    C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.POINTER(ImageOut), C.POINTER(ImageStat),
                                    C.POINTER(StretchParams)]),
    "stk_grey_blur_f32": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_int32, C.c_void_p]),
    "stk_gaussian_blur_f32": (c_status, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p]),
    "stk_find_transform_ecc": (c_status, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.POINTER(EccParams), C.c_void_p, C.POINTER(C.c_double),
                                          C.POINTER(C.c_int32)]),
    "stk_ecc_prepared_geometry": (c_status, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
    "stk_ecc_prepared": (c_status, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "stk_warp_accumulate": (c_status, [C.c_void_p, C.POINTER(Frames), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_double, C.c_int32, C.POINTER(ImageF32)]),
    "stk_scale_image_grey": (c_status, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stk_scale_image_grey_f32": (c_status, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "stk_orb_detect_and_compute": (c_status, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "stk_bf_knn2_hamming": (c_status, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "stk_find_homography": (c_status, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                       C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "stk_find_homography_batch": (c_status, [C.c_void_p, C.POINTER(HgProblem), C.c_int32, C.c_int32, C.c_double,
                                             C.POINTER(HgOutcome)]),
}

_lib = None


def load() -> C.CDLL:
    """Load libstacker_amd.so (built by __graft_entry__.build() / csrc/Makefile). Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C libstacker_rs_amd/csrc)")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64
        # and a second copy (from /opt/rocm) in the same process leaves whichever initialises last
        # without a GPU. Importing torch first makes the loader resolve our NEEDED libamdhip64.so.7 to
        # the copy torch already mapped, so tensors, streams and our kernels share one runtime.
        # (Without torch installed the library binds to /opt/rocm through its RUNPATH.)
        try:
            import torch  # noqa: F401
        except ImportError:  # pragma: no cover - torch is part of the target image
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib

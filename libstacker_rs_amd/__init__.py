"""libstacker_rs_amd — MI355X-native drop-in for the hot path of eadf/libstacker.rs.

`keypoint_match()` / `ecc_match()` (reference: src/lib.rs:129-144, 702-717) implemented as
hand-written HIP kernels for gfx950 behind a C ABI (include/stacker.h, libstacker_amd.so).
The directory is also reachable under the dotted name `libstacker.rs_amd/` (a symlink): a dot
cannot appear in an importable Python package name.

Importing the package is cheap and never touches the GPU; the shared library is loaded on first
use (api.Stacker / _ffi.load) and there is no CPU fallback.
"""
from .api import (BORDER_CONSTANT, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_WRAP,  # noqa: F401
                  CFA_BGGR, CFA_GBRG, CFA_GRBG, CFA_RGGB, DEMOSAIC_BILINEAR, DEMOSAIC_HA, DEMOSAIC_MHC, DEMOSAIC_SUPERPIXEL,
                  INTER_CUBIC, INTER_LINEAR,
                  LEAST_SQUARES, LMEDS, RANSAC, RHO, CalibrationParameters, DefectParameters, DrizzleParameters, EccMatchParameters, HipError, InvalidParams, IoError,
                  KeyPointMatchParameters, LocalNormParameters, LocalParameters, MeshParameters, MotionType, NOISE_DTYPE, NoiseParameters, NotEnoughFiles, NotImplementedYet, OpenCvError,
                  ProcessingError, QuantileParameters, RejectParameters, RobustClipParameters, SelectParameters, SigmaClipParameters, Stacker,
                  StackerError, StarDeepParameters, StarParameters, STAR_DTYPE, WeightParameters,
                  default_stacker, ecc_match, keypoint_match, local_norm_estimate, local_norm_grid, mesh_grid, mesh_pyramid_shapes, noise_from_hist, noise_weights,
                  rank_frames,
                  star_match_lists,
                  QUALITY_DTYPE, SHAPE_DTYPE, STAR_SCORE_COUNT, STAR_SCORE_FWHM, STAR_SCORE_ROUND, STAR_SCORE_SNR, StarMeasureParameters,
                  StarQualityParameters, star_frame_quality, star_quality_scores, star_quality_weights, star_shape_derive,
                  BG_CELL_DTYPE, BG_MEAN, BG_MEDIAN, BG_MODE, BackgroundParameters, background_estimate,
                  PSF_GAUSSIAN, PSF_MOFFAT, DeconvolveParameters, psf_from_shapes, psf_model,
                  WAVELET_HARD, WAVELET_SOFT, WaveletParameters, wavelet_noise_table,
                  STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE, CURVE_ASINH, CURVE_GAMMA, CURVE_SRGB, DEPTH_U8, DEPTH_U16, DEPTH_F32,
                  STAT_DTYPE, StretchParameters, AutoStretchParameters, stretch_auto, stretch_table)

__all__ = ["keypoint_match", "ecc_match", "KeyPointMatchParameters", "EccMatchParameters", "MotionType",
           "StackerError", "Stacker", "SigmaClipParameters", "RobustClipParameters", "QuantileParameters", "WeightParameters",
           "SelectParameters", "rank_frames", "LocalParameters", "MeshParameters", "mesh_grid", "mesh_pyramid_shapes", "DrizzleParameters",
           "RejectParameters", "LocalNormParameters", "local_norm_estimate", "local_norm_grid",
           "StarParameters", "StarDeepParameters", "STAR_DTYPE", "star_match_lists", "CalibrationParameters", "DefectParameters",
           "NoiseParameters", "NOISE_DTYPE", "noise_from_hist", "noise_weights",
           "StarMeasureParameters", "StarQualityParameters", "SHAPE_DTYPE", "QUALITY_DTYPE", "star_shape_derive", "star_frame_quality",
           "star_quality_scores", "star_quality_weights", "STAR_SCORE_FWHM", "STAR_SCORE_ROUND", "STAR_SCORE_SNR", "STAR_SCORE_COUNT",
           "BackgroundParameters", "background_estimate", "BG_CELL_DTYPE", "BG_MEDIAN", "BG_MEAN", "BG_MODE",
           "DeconvolveParameters", "psf_model", "psf_from_shapes", "PSF_GAUSSIAN", "PSF_MOFFAT",
           "WaveletParameters", "wavelet_noise_table", "WAVELET_HARD", "WAVELET_SOFT",
           "StretchParameters", "AutoStretchParameters", "stretch_auto", "stretch_table", "STAT_DTYPE", "STRETCH_LINEAR", "STRETCH_MTF",
           "STRETCH_TABLE", "CURVE_ASINH", "CURVE_GAMMA", "CURVE_SRGB", "DEPTH_U8", "DEPTH_U16", "DEPTH_F32",
           "CFA_RGGB", "CFA_GRBG", "CFA_GBRG", "CFA_BGGR", "DEMOSAIC_BILINEAR", "DEMOSAIC_MHC", "DEMOSAIC_HA", "DEMOSAIC_SUPERPIXEL"]

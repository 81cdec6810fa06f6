"""Host-side mirror of libstacker's public API over the C ABI (include/stacker.h).

Same names, argument meaning and error behaviour as the reference (src/lib.rs):
``keypoint_match(files, KeyPointMatchParameters, scale_down_width) -> (dropped, image)``
(lib.rs:129-144) and ``ecc_match(files, EccMatchParameters, scale_down_width) -> image``
(lib.rs:702-717); `StackerError` variants follow lib.rs:27-45. "files" are decoded frames here
(numpy arrays on the host or torch tensors already resident in HBM, BGR interleaved like
imread(IMREAD_UNCHANGED) returns, utils.rs:132); the first one is the reference frame.

All arithmetic happens in libstacker_amd.so (hand-written HIP for gfx950). This module only
marshals pointers; it has no CPU fallback and raises if the library is missing.
"""
from __future__ import annotations

import ctypes as C
import os
import enum
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _ffi

# OpenCV constants the reference passes through
RANSAC, LMEDS, RHO, LEAST_SQUARES = 8, 4, 16, 0
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101, BORDER_TRANSPARENT = range(6)
INTER_LINEAR, INTER_CUBIC = 1, 2          # option "warp_interpolation" (OpenCV's numbers)
HOST, DEVICE = 0, 1
CFA_RGGB, CFA_GRBG, CFA_GBRG, CFA_BGGR = range(4)          # STK_CFA_*: the 2 x 2 cell in reading order
DEMOSAIC_BILINEAR, DEMOSAIC_MHC, DEMOSAIC_HA, DEMOSAIC_SUPERPIXEL = range(4)


class StackerError(Exception):
    """Base of the reference's StackerError enum (lib.rs:27-45)."""


class NotEnoughFiles(StackerError):
    pass


class InvalidParams(StackerError):
    pass


class ProcessingError(StackerError):
    pass


class OpenCvError(StackerError):
    """The reference's OpenCvError: failures the OpenCV backend would have raised (ECC no-convergence ...)."""


class IoError(StackerError):
    pass


class HipError(StackerError):
    pass


class NotImplementedYet(StackerError):
    pass


_STATUS_EXC = {1: NotEnoughFiles, 2: InvalidParams, 3: ProcessingError, 4: OpenCvError, 5: IoError, 6: HipError,
               7: NotImplementedYet}


class MotionType(enum.IntEnum):   # lib.rs:603-609 (= OpenCV MOTION_*)
    Translation = 0
    Euclidean = 1
    Affine = 2
    Homography = 3


@dataclass
class KeyPointMatchParameters:    # lib.rs:48-73, defaults utils.rs:250-261
    method: int = RANSAC
    ransac_reproj_threshold: float = 3.0
    match_keep_ratio: float = 0.75
    match_ratio: float = 0.8
    border_mode: int = BORDER_CONSTANT
    border_value: Sequence[float] = field(default_factory=lambda: (0.0, 0.0, 0.0, 0.0))

    def _c(self) -> _ffi.KeypointParams:
        bv = (list(self.border_value) + [0.0] * 4)[:4]
        return _ffi.KeypointParams(int(self.method), float(self.ransac_reproj_threshold), float(self.match_keep_ratio),
                                   float(self.match_ratio), int(self.border_mode), (C.c_double * 4)(*bv))


@dataclass
class EccMatchParameters:         # lib.rs:611-623 (no Default in the reference)
    motion_type: MotionType
    max_count: Optional[int]
    epsilon: Optional[float]
    gauss_filt_size: int

    def _c(self) -> _ffi.EccParams:
        return _ffi.EccParams(int(self.motion_type), int(self.max_count is not None), int(self.max_count or 0),
                              int(self.epsilon is not None), float(self.epsilon or 0.0), int(self.gauss_filt_size))

    def term_criteria(self):
        """TermCriteria{typ, max_count, epsilon} as utils.rs:159-170 builds it (COUNT=1, EPS=2)."""
        typ = (1 if self.max_count is not None else 0) | (2 if self.epsilon is not None else 0)
        return typ, (self.max_count or 0), (self.epsilon or 0.0)


@dataclass
class SigmaClipParameters:        # extension beyond the reference: include/stacker.h, stk_clip_params
    """Kappa-sigma rejection for the *_clipped combines: samples below c - kappa_low sigma or above c + kappa_high sigma
    are left out, `iterations` times, before the final mean of the kept samples."""
    kappa_low: float = 3.0
    kappa_high: float = 3.0
    iterations: int = 2

    def _c(self) -> _ffi.ClipParams:
        return _ffi.ClipParams(float(self.kappa_low), float(self.kappa_high), int(self.iterations), 0)


@dataclass
class RobustClipParameters:       # extension beyond the reference: include/stacker.h, stk_robust_clip_params
    """Median / MAD rejection for the *_robust_clipped combines: samples below c - kappa_low sigma or above
    c + kappa_high sigma are left out, `iterations` times, with c the median and sigma = max(1.4826 MAD, sigma_floor) of
    the samples still kept, before the final mean of the kept samples. sigma_floor is in the units of the samples (after
    alpha): half a quantisation step of 8-bit input by default; 0 is allowed."""
    kappa_low: float = 3.0
    kappa_high: float = 3.0
    sigma_floor: float = 0.5 / 255.0
    iterations: int = 2

    def _c(self) -> _ffi.RobustClipParams:
        return _ffi.RobustClipParams(float(self.kappa_low), float(self.kappa_high), float(self.sigma_floor), int(self.iterations))


@dataclass
class CalibrationParameters:      # extension beyond the reference: include/stacker.h, stk_calibration
    """What Stacker.calibrate applies to every frame: v = ((raw - bias) - dark_scale[i] * dark) * flat_mean / max(flat,
    flat_min) + pedestal per colour channel, then the repair of the pixels flagged in `defects` by the median of their good
    neighbours at +-defect_step. bias, dark, flat: H x W x C float32 in the frames' raw sample units (numpy arrays or
    tensors, host or device, whatever the frames' location), any subset. flat_mean None: Stacker.image_mean(flat);
    flat_min None: a thousandth of the smallest flat_mean. out_depth None: the frames' own depth (rounded half to even,
    saturated); 32: float32."""
    bias: object = None
    dark: object = None
    flat: object = None
    dark_scale: Optional[Sequence[float]] = None
    flat_mean: Optional[Sequence[float]] = None
    flat_min: Optional[float] = None
    pedestal: float = 0.0
    defects: object = None
    defect_step: int = 1
    out_depth: Optional[int] = None


@dataclass
class DefectParameters:           # extension beyond the reference: include/stacker.h, stk_defect_params
    """Stacker.defect_map's tests of a master against the median of its neighbours at +-step: high (hot pixels of a dark):
    X - med > high_abs; low (dead pixels and dust of a flat): X < low_ratio * med. accumulate: OR into the map handed in."""
    high: bool = True
    low: bool = False
    high_abs: float = 0.0
    low_ratio: float = 0.5
    step: int = 1
    accumulate: bool = False

    def _c(self) -> _ffi.DefectParams:
        return _ffi.DefectParams((1 if self.high else 0) | (2 if self.low else 0), float(self.high_abs), float(self.low_ratio),
                                 int(self.step), int(bool(self.accumulate)), 0)


@dataclass
class QuantileParameters:         # extension beyond the reference: include/stacker.h, stk_quantile_params
    """The order statistic for the *_quantile combines: 0 = min, 0.5 = median, 1 = max, linear interpolation between
    the two nearest samples otherwise (numpy.quantile's default method)."""
    quantile: float = 0.5

    def _c(self) -> _ffi.QuantileParams:
        return _ffi.QuantileParams(float(self.quantile), 0)


NORMALIZE_NONE, NORMALIZE_OFFSET, NORMALIZE_GAIN, NORMALIZE_LINEAR = 0, 1, 2, 3


@dataclass
class WeightParameters:           # extension beyond the reference: include/stacker.h, stk_weight_params
    """The *_weighted combines: `normalize` maps every frame onto frame 0's level before the mean (0 none, 1 offset = sky
    level, 2 gain = exposure / transparency, 3 linear), estimated from the overlap on every `stat_step`-th row and column
    (0 = 4); `coverage` divides each pixel by the weight that actually covered it instead of counting border samples."""
    normalize: int = NORMALIZE_NONE
    coverage: bool = True
    stat_step: int = 0

    def _c(self) -> _ffi.WeightParams:
        return _ffi.WeightParams(int(self.normalize), int(self.coverage), int(self.stat_step), 0)


@dataclass
class LocalParameters:            # extension beyond the reference: include/stacker.h, stk_local_params
    """The local-sharpness (lucky-region) combines: the quality map of a frame is the sum of its modified-Laplacian values
    of at least `threshold` (0 .. 1020) over a (2 radius + 1)^2 window (radius 1 .. 15); a frame's weight at a pixel is
    (quality there + `floor`) to the `power` (1 .. 4)."""
    radius: int = 4
    threshold: int = 16
    power: int = 2
    floor: float = 1.0

    def _c(self) -> _ffi.LocalParams:
        return _ffi.LocalParams(int(self.radius), int(self.threshold), int(self.power), float(self.floor), (C.c_int32 * 2)(0, 0))


STAR_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("flux", "<f4"), ("px", "<i4"), ("py", "<i4"), ("peak", "<i4"),
                       ("npix", "<i4"), ("reserved", "<i4")])          # stk_star


@dataclass
class StarParameters:             # extension beyond the reference: include/stacker.h, stk_star_params
    """Star registration. Detection: a peak is the maximum of its (2 radius + 1)^2 window, at least
    max(ceil(kappa 1.4826 MAD), min_contrast) above its 64 x 64 tile's median, with at least min_pixels window pixels that
    high; the max_stars brightest are kept. Matching: triangles over each of the match_stars brightest stars and its
    `neighbours` nearest, matched within tri_tolerance, at least min_votes per pair; `refine` re-matches all stars under
    the first homography. A frame with fewer than min_stars stars or min_inliers inliers is dropped. method, threshold
    and border as KeyPointMatchParameters."""
    radius: int = 4
    kappa: float = 4.0
    min_contrast: int = 8
    min_pixels: int = 3
    max_stars: int = 200
    match_stars: int = 50
    neighbours: int = 5
    tri_tolerance: float = 0.01
    min_votes: int = 2
    refine: bool = True
    min_stars: int = 6
    min_inliers: int = 7              # not 4: four pairs always fit a homography exactly, so 4 rejects nothing
    method: int = 8                   # RANSAC
    ransac_reproj_threshold: float = 2.0
    border_mode: int = 0              # BORDER_CONSTANT
    border_value: Sequence[float] = (0.0, 0.0, 0.0, 0.0)

    def _c(self) -> _ffi.StarParams:
        bv = (C.c_double * 4)(*([float(v) for v in self.border_value] + [0.0] * 4)[:4])
        return _ffi.StarParams(int(self.radius), float(self.kappa), int(self.min_contrast), int(self.min_pixels), int(self.max_stars),
                               int(self.match_stars), int(self.neighbours), float(self.tri_tolerance), int(self.min_votes),
                               int(self.refine), int(self.min_stars), int(self.min_inliers), int(self.method),
                               float(self.ransac_reproj_threshold), int(self.border_mode), bv)


@dataclass
class StarDeepParameters:         # extension beyond the reference: include/stacker.h, stk_star_deep_params
    """The key of star detection on deep frames. f32_scale: an f32 frame's key is rint(grey * f32_scale) clamped to
    0 .. 65535 (1.0 for frames in 16-bit counts, 65535.0 for frames in 0 .. 1); not read for u8 and u16 frames."""
    f32_scale: float = 1.0

    def _c(self) -> _ffi.StarDeepParams:
        return _ffi.StarDeepParams(float(self.f32_scale), 0)


def star_match_lists(moving, ref, params: Optional["StarParameters"] = None):
    """Triangle matching of two star lists (stk_star_match_lists; host code, no GPU): a k x 2 int32 array of (moving index,
    reference index) pairs in ascending moving index. The lists are STAR_DTYPE arrays, or n x 2 arrays of (x, y)."""
    def as_stars(a):
        a = np.asarray(a)
        if a.dtype == STAR_DTYPE:
            return np.ascontiguousarray(a)
        s = np.zeros(len(a), STAR_DTYPE)
        if len(a):
            xy = np.asarray(a, np.float32).reshape(len(a), -1)
            s["x"], s["y"] = xy[:, 0], xy[:, 1]
        return s
    mv, rf = as_stars(moving), as_stars(ref)
    p = (params or StarParameters())._c()
    pairs = np.zeros((max(int(p.match_stars), 1), 2), np.int32)
    n = C.c_int32(0)
    st = _ffi.load().stk_star_match_lists(C.c_void_p(mv.ctypes.data if len(mv) else 0), len(mv), C.c_void_p(rf.ctypes.data if len(rf) else 0),
                                          len(rf), C.byref(p), C.c_void_p(pairs.ctypes.data), C.byref(n))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("star_match_lists: bad parameters or star lists")
    return pairs[:n.value].copy()


# one stk_star_shape and one stk_star_quality (include/stacker.h)
SHAPE_DTYPE = np.dtype([("S", "<i8"), ("Sx", "<i8"), ("Sy", "<i8"), ("Sxx", "<i8"), ("Syy", "<i8"), ("Sxy", "<i8"),
                        ("px", "<i4"), ("py", "<i4"), ("bg", "<i4"), ("mad", "<i4"), ("thr", "<i4"), ("npix", "<i4"), ("peak", "<i4"),
                        ("n_ring", "<i4"), ("flags", "<i4"), ("reserved", "<i4"),
                        ("x", "<f8"), ("y", "<f8"), ("cxx", "<f8"), ("cyy", "<f8"), ("cxy", "<f8"), ("fwhm", "<f8"), ("ecc", "<f8"),
                        ("snr", "<f8")])
QUALITY_DTYPE = np.dtype([("fwhm", "<f8"), ("ecc", "<f8"), ("snr", "<f8"), ("bg", "<f8"), ("noise", "<f8"), ("n_stars", "<i4"),
                          ("n_measured", "<i4")])
STAR_SCORE_FWHM, STAR_SCORE_ROUND, STAR_SCORE_SNR, STAR_SCORE_COUNT = 0, 1, 2, 3


@dataclass
class StarMeasureParameters:      # extension beyond the reference: include/stacker.h, stk_star_measure_params
    """Star measurement on the 16-bit key. The background and its MAD are the exact medians of the ring ring_inner ..
    ring_outer around the star; the moments are summed over the aperture of `radius` on the pixels at least
    max(ceil(kappa 1.4826 MAD), min_contrast) above the background. A star with fewer than min_pixels such pixels, or with a
    peak at or above `saturation` (0 = off), is flagged and takes no part in a frame's quality."""
    radius: int = 7
    ring_inner: int = 10
    ring_outer: int = 14
    kappa: float = 3.0
    min_contrast: int = 1
    min_pixels: int = 5
    saturation: int = 0

    def _c(self) -> _ffi.StarMeasureParams:
        return _ffi.StarMeasureParams(int(self.radius), int(self.ring_inner), int(self.ring_outer), float(self.kappa),
                                      int(self.min_contrast), int(self.min_pixels), int(self.saturation), 0)


@dataclass
class StarQualityParameters:      # extension beyond the reference: include/stacker.h, stk_star_quality_params
    """How a frame's star quality becomes its weight: a frame with fewer than min_measured measured stars, a median FWHM
    above fwhm_max or a median eccentricity above ecc_max (0 = no limit) is rejected; a kept frame's weight is
    (best FWHM / FWHM)^fwhm_power x (roundness / best roundness)^ecc_power x (SNR / best SNR)^snr_power, powers 0 .. 4."""
    fwhm_max: float = 0.0
    ecc_max: float = 0.0
    min_measured: int = 5
    fwhm_power: int = 2
    ecc_power: int = 0
    snr_power: int = 0

    def _c(self) -> _ffi.StarQualityParams:
        return _ffi.StarQualityParams(float(self.fwhm_max), float(self.ecc_max), int(self.min_measured), int(self.fwhm_power),
                                      int(self.ecc_power), int(self.snr_power), 0)


def _shape_table(shapes):
    """A list of per-frame SHAPE_DTYPE arrays (or one n x max_stars array) as (n x max_stars array, n counts)."""
    if isinstance(shapes, np.ndarray) and shapes.ndim == 2:
        tab = np.ascontiguousarray(shapes.astype(SHAPE_DTYPE, copy=False))
        return tab, np.full(tab.shape[0], tab.shape[1], np.int32)
    lists = [np.asarray(s, SHAPE_DTYPE).reshape(-1) for s in shapes]
    tab = np.zeros((len(lists), max([len(s) for s in lists] + [1])), SHAPE_DTYPE)
    for i, s in enumerate(lists):
        tab[i, :len(s)] = s
    return tab, np.array([len(s) for s in lists], np.int32)


def star_shape_derive(shapes):
    """stk_star_shape_derive on a SHAPE_DTYPE array of any shape: a copy with x, y, the central moments, fwhm, ecc and snr
    filled from the integer sums (and flags bit 3 where there is no positive minor axis). Host code: needs the library, not a
    GPU."""
    s = np.array(shapes, SHAPE_DTYPE, copy=True, order="C")
    st = _ffi.load().stk_star_shape_derive(s.ctypes.data_as(C.POINTER(_ffi.StarShape)), s.size)
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("star_shape_derive: a list of shapes expected")
    return s


def star_frame_quality(shapes):
    """stk_star_frame_quality: one QUALITY_DTYPE record per frame from the frames' shapes (Stacker.star_measure): the lower
    medians of fwhm, ecc, snr, bg and 1.4826 mad over the shapes with flags == 0. Host code."""
    tab, counts = _shape_table(shapes)
    n = tab.shape[0]
    out = np.zeros(max(n, 1), QUALITY_DTYPE)
    st = _ffi.load().stk_star_frame_quality(tab.ctypes.data_as(C.POINTER(_ffi.StarShape)), C.c_void_p(counts.ctypes.data), n, tab.shape[1],
                                            out.ctypes.data_as(C.POINTER(_ffi.StarQuality)))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("star_frame_quality: at least one frame's shapes expected")
    return out[:n]


def star_quality_scores(quality):
    """stk_star_quality_scores: an n x 4 float64 array (1 / fwhm, 1 - ecc, snr, measured stars; higher is better) that
    rank_frames takes with SelectParameters(metric=STAR_SCORE_*). Host code."""
    q = np.ascontiguousarray(np.asarray(quality, QUALITY_DTYPE).reshape(-1))
    scores = np.zeros((max(q.size, 1), 4), np.float64)
    st = _ffi.load().stk_star_quality_scores(q.ctypes.data_as(C.POINTER(_ffi.StarQuality)), q.size, C.c_void_p(scores.ctypes.data))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("star_quality_scores: at least one frame's quality expected")
    return scores[:q.size]


def star_quality_weights(quality, params: Optional["StarQualityParameters"] = None, reference: int = -1, include=None, weights=None):
    """stk_star_quality_weights: (weights, include, rejected): n float32 frame weights and n int32 flags for any *_stack
    combine, and the number of included frames the limits rejected. reference: a frame that passes whatever the limits say
    (-1 = none); include: per-frame flags (None = all); weights: the caller's own per-frame factors (None = 1). Host code."""
    q = np.ascontiguousarray(np.asarray(quality, QUALITY_DTYPE).reshape(-1))
    n = q.size
    inc = None if include is None else np.ascontiguousarray(np.asarray(include, np.int32).reshape(-1))
    u = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if (inc is not None and inc.size != n) or (u is not None and u.size != n):
        raise InvalidParams("one include flag and one weight per frame expected")
    p = (params or StarQualityParameters())._c()
    out, inc_out, rejected = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32), C.c_int32(0)
    st = _ffi.load().stk_star_quality_weights(q.ctypes.data_as(C.POINTER(_ffi.StarQuality)), n, C.byref(p), int(reference),
                                              None if inc is None else C.c_void_p(inc.ctypes.data),
                                              None if u is None else C.c_void_p(u.ctypes.data), C.c_void_p(out.ctypes.data),
                                              C.c_void_p(inc_out.ctypes.data), C.byref(rejected))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("star_quality_weights: limits finite and >= 0, min_measured >= 1, powers 0 .. 4, "
                                                "weights finite and >= 0, a measured and included reference, one frame passing")
    return out[:n], inc_out[:n], rejected.value


@dataclass
class LocalNormParameters:        # extension beyond the reference: include/stacker.h, stk_local_norm_params
    """Local normalisation: per frame a gain and an offset field on a grid of nodes `step` destination pixels apart (a power
    of two, 8 .. 256), each node estimated (`normalize` as in WeightParameters) from the moments of the 2 step window around
    it on every `stat_step`-th row and column (0 = 4). A node with fewer than `min_count` pixels (0 = 16), a degenerate
    formula or a gain outside [0.25, 4] is invalid; `fill` passes fill such holes from their neighbours, the rest takes the
    frame's global gain and offset."""
    step: int = 64
    stat_step: int = 0
    normalize: int = NORMALIZE_LINEAR
    coverage: bool = True
    min_count: int = 0
    fill: int = 4

    def _c(self) -> _ffi.LocalNormParams:
        return _ffi.LocalNormParams(int(self.step), int(self.stat_step), int(self.normalize), int(self.coverage), int(self.min_count),
                                    int(self.fill), (C.c_int32 * 2)(0, 0))


def local_norm_grid(width: int, height: int, step: int):
    """(gh, gw, ch, cw): the node grid (mesh_grid's) and the cell grid of local normalisation for a width x height image."""
    gw, gh = mesh_grid(width, height, step)
    return gh, gw, (height + step - 1) // step, (width + step - 1) // step


def local_norm_estimate(width: int, height: int, channels: int, cell_moments, norm: Optional["LocalNormParameters"] = None,
                        return_global: bool = False, return_valid: bool = False):
    """Estimator and fill of local normalisation for one frame (stk_local_norm_estimate; host code, no GPU): the
    gh x gw x 2 channels f32 plane from the frame's (ch cw) x channels x 6 cell moments, then the global record
    (return_global) and the per-node validity masks before the fill (return_valid, gh x gw int32)."""
    p = (norm or LocalNormParameters())._c()
    gh, gw, ch, cw = local_norm_grid(width, height, int(p.step))
    mom = np.ascontiguousarray(np.asarray(cell_moments, np.float64).reshape(-1))
    if mom.size != ch * cw * channels * 6:
        raise InvalidParams("cell moments: (ch cw) x channels x 6 expected")
    plane = np.zeros((gh, gw, 2 * channels), np.float32)
    glob = _ffi.FrameWeight()
    valid = np.zeros((gh, gw), np.int32)
    st = _ffi.load().stk_local_norm_estimate(int(width), int(height), int(channels), C.byref(p), C.c_void_p(mom.ctypes.data),
                                             C.c_void_p(plane.ctypes.data), C.byref(glob), C.c_void_p(valid.ctypes.data))
    if st:
        raise InvalidParams("stk_local_norm_estimate refused its arguments")
    res = (plane,) + ((Stacker._applied_list([glob], 1, channels)[0],) if return_global else ()) + ((valid,) if return_valid else ())
    return res if len(res) > 1 else plane


@dataclass
class MeshParameters:             # extension beyond the reference: include/stacker.h, stk_mesh_params
    """Local alignment: per frame a residual displacement on a grid of nodes `step` destination pixels apart (a power of
    two, 8 .. 256), each from a (2 radius + 1)^2 patch (radius 2 .. 32) by at most `max_iters` Lucas-Kanade iterations that
    stop below `epsilon` px. A node that moves beyond `max_shift` px, sees less than half its patch or has less texture
    than `min_eig` (grey levels^2 per pixel) is invalid; `fill` passes fill such holes from their neighbours."""
    step: int = 16
    radius: int = 8
    max_iters: int = 10
    epsilon: float = 0.01
    max_shift: float = 8.0
    min_eig: float = 1.0
    fill: int = 2

    def _c(self) -> _ffi.MeshParams:
        return _ffi.MeshParams(int(self.step), int(self.radius), int(self.max_iters), float(self.epsilon), float(self.max_shift),
                               float(self.min_eig), int(self.fill), 0)


@dataclass
class DrizzleParameters:          # extension beyond the reference: include/stacker.h, stk_drizzle_params
    """Drizzle integration: the output grid has `scale` (1 .. 4) pixels per frame-0 pixel and starts at frame-0 coordinate
    (`origin_x`, `origin_y`); every source pixel is shrunk to a drop of side `pixfrac` (0 < pixfrac <= 1) before it is
    spread over the output pixels it overlaps. An output pixel nothing landed on gets `fill`."""
    scale: float = 2.0
    pixfrac: float = 0.5
    origin_x: float = 0.0
    origin_y: float = 0.0
    fill: float = 0.0

    def _c(self) -> _ffi.DrizzleParams:
        return _ffi.DrizzleParams(float(self.scale), float(self.pixfrac), float(self.origin_x), float(self.origin_y),
                                  float(self.fill), 0)

    def out_shape(self, height: int, width: int):
        """(oh, ow) of the output that covers a height x width frame 0 from the origin on: ceil(scale * size)."""
        return int(np.ceil(float(self.scale) * height)), int(np.ceil(float(self.scale) * width))


@dataclass
class RejectParameters:           # extension beyond the reference: include/stacker.h, stk_reject_params
    """Blot-and-compare rejection maps: a frame pixel is rejected where it differs from the blotted clean image by more than
    `scale1` x the model's local gradient + `snr1` x sigma, or, next to such a pixel, by more than `scale2` x gradient +
    `snr2` x sigma; sigma = sqrt(read_noise^2 + poisson_gain x model), in the units of the samples after alpha. With a
    counts plane a clean pixel made from fewer than `min_count` samples judges nothing."""
    snr1: float = 4.0
    snr2: float = 3.0
    scale1: float = 1.2
    scale2: float = 0.7
    read_noise: float = 2.0 / 255.0
    poisson_gain: float = 0.0
    min_count: int = 3

    def _c(self) -> _ffi.RejectParams:
        return _ffi.RejectParams(float(self.snr1), float(self.snr2), float(self.scale1), float(self.scale2), float(self.read_noise),
                                 float(self.poisson_gain), int(self.min_count), 0)


def mesh_grid(width: int, height: int, step: int):
    """(gw, gh): the node grid of a width x height destination at spacing `step` (stk_mesh_grid)."""
    gw, gh = C.c_int32(0), C.c_int32(0)
    if _ffi.load().stk_mesh_grid(int(width), int(height), int(step), C.byref(gw), C.byref(gh)) != 0:
        raise InvalidParams("mesh_grid: width and height must be positive, step a power of two in 8 .. 256")
    return gw.value, gh.value


def mesh_pyramid_shapes(width: int, height: int, levels: int):
    """[(h >> l, w >> l) for l = 0 .. levels - 1]: the level images of the coarse-to-fine local alignment
    (local_align_pyramid, grey_pyramid); an odd last column or row is dropped at every halving."""
    if not 1 <= int(levels) <= 4 or width <= 0 or height <= 0:
        raise InvalidParams("mesh_pyramid_shapes: width and height must be positive, levels 1 .. 4")
    return [(int(height) >> l, int(width) >> l) for l in range(int(levels))]


SHARPNESS_LAPM, SHARPNESS_LAPV, SHARPNESS_TENG, SHARPNESS_GLVN = 0, 1, 2, 3
QUALITY_WEIGHT_NONE, QUALITY_WEIGHT_SCORE = 0, 1


@dataclass
class SelectParameters:           # extension beyond the reference's library: include/stacker.h, stk_select_params
    """How a scored stack is ranked and cut (the sort / skip(1) / rev() of examples/main.rs:53, 64): by `metric` (TENG with
    `ksize` in the example), dropping the `drop_worst` lowest frames or keeping the best `keep_fraction` of them (0 = off);
    `weight_mode` SCORE also gives every kept frame the weight score / best score for the weighted combines."""
    metric: int = SHARPNESS_TENG
    ksize: int = 3
    drop_worst: int = 0
    keep_fraction: float = 0.0
    weight_mode: int = QUALITY_WEIGHT_NONE

    def _c(self) -> _ffi.SelectParams:
        return _ffi.SelectParams(int(self.metric), int(self.ksize), int(self.drop_worst), float(self.keep_fraction),
                                 int(self.weight_mode), 0)


def rank_frames(scores, select: Optional["SelectParameters"] = None):
    """stk_rank_frames on an n x 4 array of scores (Stacker.stack_sharpness): (order, n_kept, weights). order[:n_kept] are the
    kept frames, best first; weights[i] belongs to frame order[i]. Host code: needs the library, not a GPU."""
    sc = np.ascontiguousarray(np.asarray(scores, np.float64))
    if sc.ndim != 2 or sc.shape[1] != 4:
        raise InvalidParams("scores: an n x 4 array expected")
    n = sc.shape[0]
    order = np.zeros(max(n, 1), np.int32)
    weights = np.ones(max(n, 1), np.float32)
    kept = C.c_int32(0)
    sp = (select or SelectParameters())._c()
    st = _ffi.load().stk_rank_frames(C.c_void_p(sc.ctypes.data), n, C.byref(sp), order.ctypes.data_as(C.POINTER(C.c_int32)),
                                     C.byref(kept), C.c_void_p(weights.ctypes.data))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("Not enough files" if st == 1 else "rank_frames: invalid select parameters")
    return order[:n], kept.value, weights[:n]


# one stk_noise_stat (include/stacker.h)
NOISE_DTYPE = np.dtype([("median", "<i4"), ("mad", "<i4"), ("res_median", "<i4"), ("flags", "<i4"), ("sigma", "<f8"), ("kept", "<i8")])


@dataclass
class NoiseParameters:            # extension beyond the reference: include/stacker.h, stk_noise_weights
    """How noise statistics become frame weights: `sigma_floor`, in grey levels of the frames' depth, is the least noise a
    frame is credited with (a frame cannot earn unbounded weight from a clipped or quantised background). None: 0.25 for
    8-bit and 64 for 16-bit frames."""
    sigma_floor: Optional[float] = None

    def floor(self, depth: int = 8) -> float:
        return float(self.sigma_floor) if self.sigma_floor is not None else (0.25 if depth == 8 else 64.0)


def noise_from_hist(hv, hr, overflow_bin: bool = False):
    """stk_noise_from_hist on one (frame, channel)'s value and residual histograms (Stacker.stack_noise(return_hist=True)):
    one NOISE_DTYPE record. overflow_bin: the last residual bin collects everything above it (16-bit frames). Host code:
    needs the library, not a GPU."""
    hv = np.ascontiguousarray(np.asarray(hv, np.uint32).reshape(-1))
    hr = np.ascontiguousarray(np.asarray(hr, np.uint32).reshape(-1))
    out = np.zeros(1, NOISE_DTYPE)
    st = _ffi.load().stk_noise_from_hist(C.c_void_p(hv.ctypes.data), hv.size, C.c_void_p(hr.ctypes.data), hr.size, int(overflow_bin),
                                         out.ctypes.data_as(C.POINTER(_ffi.NoiseStat)))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("noise_from_hist: 1 .. 65536 value bins and 2 .. 65536 residual bins expected")
    return out[0]


def noise_weights(stats, channels: int, gain=None, include=None, weights=None, sigma_floor: float = 0.25, *, applied=None):
    """stk_noise_weights: n float32 inverse-variance weights from an n x 4 NOISE_DTYPE array (Stacker.stack_noise). gain:
    n x channels, the gains the combine will apply (None = 1), or `applied`: the records a weighted call returned; include:
    per-frame flags (None = all; an excluded frame gets 0); weights: the caller's own per-frame factors (None = 1). Host code:
    needs the library, not a GPU."""
    ns = np.ascontiguousarray(np.asarray(stats, NOISE_DTYPE))
    if ns.ndim != 2 or ns.shape[1] != 4:
        raise InvalidParams("stats: an n x 4 array of NOISE_DTYPE expected")
    n = ns.shape[0]
    rec = None
    if applied is not None:
        gain = [list(a["gain"]) + [1.0] * (4 - len(a["gain"])) for a in applied]
    if gain is not None:
        g = np.asarray(gain, np.float32).reshape(n, -1)
        rec = (_ffi.FrameWeight * max(n, 1))()
        for i in range(n):
            for c in range(4):
                rec[i].gain[c] = float(g[i, c]) if c < g.shape[1] else 1.0
            rec[i].weight = 1.0
    inc = None if include is None else np.ascontiguousarray(np.asarray(include, np.int32).reshape(-1))
    u = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if (inc is not None and inc.size != n) or (u is not None and u.size != n):
        raise InvalidParams("one include flag and one weight per frame expected")
    out = np.zeros(max(n, 1), np.float32)
    st = _ffi.load().stk_noise_weights(ns.ctypes.data_as(C.POINTER(_ffi.NoiseStat)), n, int(channels), rec,
                                       None if inc is None else C.c_void_p(inc.ctypes.data),
                                       None if u is None else C.c_void_p(u.ctypes.data), float(sigma_floor), C.c_void_p(out.ctypes.data))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("noise_weights: sigma_floor must be finite and > 0, weights finite and >= 0, "
                                                "sigmas and gains finite, one frame included")
    return out[:n]


BG_MEDIAN, BG_MEAN, BG_MODE = range(3)                     # STK_BG_*: the level estimator of the background model
BG_CELL_DTYPE = np.dtype([("n", "<i4"), ("kept", "<i4"), ("med", "<i4"), ("mad", "<i4"), ("lo", "<i4"), ("hi", "<i4"),
                          ("reserved", "<i4", (2,)), ("sum", "<i8"), ("sum2", "<u8")])


@dataclass
class BackgroundParameters:       # extension beyond the reference: include/stacker.h, stk_background_params
    """The background model: per frame and colour channel the sky level on a grid of nodes `step` pixels apart (16, 32, 64
    or 128), each from the window of step + 1 pixels around it: the median and MAD of the window's 16-bit keys (f32 frames:
    rint(sample * f32_scale)), clipped `clip_iters` times (0 .. 5) at `kappa` robust sigmas. `estimator`: BG_MEDIAN, BG_MEAN
    (of the kept keys) or BG_MODE (2.5 median - 1.5 mean where the two agree). A node that keeps fewer than `min_count` keys
    (0 = 64), or rejects more than `max_reject` of its window, is invalid; `recentre` moves the level of a window cut by the
    frame back to its node, `filter` is a 3 x 3 median of the nodes, `fill` passes fill holes from their neighbours. The
    flattened sky is put at `target` (per channel) in `out_depth` (None: the frames' depth)."""
    step: int = 64
    clip_iters: int = 3
    kappa: float = 3.0
    f32_scale: float = 1.0
    estimator: int = BG_MODE
    min_count: int = 0
    max_reject: float = 0.5
    recentre: bool = True
    filter: bool = True
    fill: int = 4
    target: Sequence[float] = (0.0, 0.0, 0.0, 0.0)
    out_depth: Optional[int] = None

    def _target(self):
        t = np.asarray(self.target, np.float32).reshape(-1)
        return (C.c_float * 4)(*((list(t) + [float(t[-1])] * 4)[:4]))

    def _c(self, depth: int = 0) -> _ffi.BackgroundParams:
        return _ffi.BackgroundParams(int(self.step), int(self.clip_iters), float(self.kappa), float(self.f32_scale), int(self.estimator),
                                     int(self.min_count), float(self.max_reject), int(self.recentre), int(self.filter), int(self.fill),
                                     self._target(), int(depth if self.out_depth is None else self.out_depth), (C.c_int32 * 3)(0, 0, 0))


def background_estimate(width: int, height: int, channels: int, depth: int, cells, params: Optional["BackgroundParameters"] = None,
                        return_rms: bool = False, return_valid: bool = False, return_flags: bool = False):
    """The estimator of the background model for one frame (stk_background_estimate; host code, no GPU): the
    gh x gw x min(channels, 3) f32 level plane from the frame's window records (BG_CELL_DTYPE, gh x gw x min(channels, 3)),
    then the rms plane (return_rms), the per-node validity masks before the edge extrapolation (return_valid, gh x gw int32)
    and the flags (return_flags: bit c = channel c had no valid node)."""
    p = (params or BackgroundParameters())._c(depth)
    gw, gh = mesh_grid(width, height, int(p.step))
    cc = min(int(channels), 3)
    rec = np.ascontiguousarray(np.asarray(cells, BG_CELL_DTYPE).reshape(-1))
    if rec.size != gh * gw * cc:
        raise InvalidParams("window records: gh x gw x min(channels, 3) expected")
    level = np.zeros((gh, gw, cc), np.float32)
    rms = np.zeros((gh, gw, cc), np.float32) if return_rms else None
    valid = np.zeros((gh, gw), np.int32)
    flags = C.c_int32(0)
    st = _ffi.load().stk_background_estimate(int(width), int(height), int(channels), int(depth), C.byref(p),
                                             rec.ctypes.data_as(C.POINTER(_ffi.BgCell)), C.c_void_p(level.ctypes.data),
                                             None if rms is None else C.c_void_p(rms.ctypes.data), C.c_void_p(valid.ctypes.data),
                                             C.byref(flags))
    if st:
        raise InvalidParams("stk_background_estimate refused its arguments")
    res = (level,) + ((rms,) if return_rms else ()) + ((valid,) if return_valid else ()) + ((flags.value,) if return_flags else ())
    return res if len(res) > 1 else level


PSF_GAUSSIAN, PSF_MOFFAT = range(2)                        # STK_PSF_*: the PSF model of deconvolution


@dataclass
class DeconvolveParameters:       # extension beyond the reference: include/stacker.h, stk_deconv_params
    """Richardson-Lucy deconvolution of a linear f32 image: `iterations` (1 .. 1000) rounds with a PSF of `radius` (1 .. 16;
    the PSF has (2 radius + 1)^2 taps). `floor` bounds the blurred estimate from below before the division; `pedestal` is
    added to the image first (and taken off at the end) so that a sky around 0 stays positive; `lambda_` > 0 turns on the
    total-variation regulariser with `tv_eps`; `amount` (0 .. 1) blends the result with the input, per pixel times the mask."""
    iterations: int = 30
    radius: int = 8
    floor: float = 1e-6
    pedestal: float = 0.0
    lambda_: float = 0.0
    tv_eps: float = 1e-3
    amount: float = 1.0

    def _c(self) -> _ffi.DeconvParams:
        return _ffi.DeconvParams(int(self.iterations), int(self.radius), float(self.floor), float(self.pedestal), float(self.lambda_),
                                 float(self.tv_eps), float(self.amount), 0)


def psf_model(radius: int, cxx: float, cyy: float, cxy: float = 0.0, kind: int = PSF_GAUSSIAN, beta: float = 2.5):
    """A PSF from a covariance (stk_psf_model; host code, no GPU): a (2 radius + 1)^2 float32 array that sums to 1, a
    Gaussian exp(-q / 2), q = d^T S^-1 d, or a Moffat profile of exponent `beta` with the same half-maximum contour."""
    r = int(radius)
    out = np.zeros((max(2 * r + 1, 1), max(2 * r + 1, 1)), np.float32)
    st = _ffi.load().stk_psf_model(int(kind), float(beta), r, float(cxx), float(cyy), float(cxy), C.c_void_p(out.ctypes.data))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("psf_model: radius 1 .. 16, a positive definite covariance, beta > 1 for Moffat")
    return out


def psf_from_shapes(shapes, min_snr: float = 0.0, scale: float = 1.0, return_used: bool = False):
    """The covariance of a frame's stars (stk_psf_from_shapes; host code): (cxx, cyy, cxy), the lower medians over the
    shapes (SHAPE_DTYPE, Stacker.star_measure) with flags == 0 and snr >= min_snr, times scale^2; return_used adds how many
    shapes that were."""
    s = np.ascontiguousarray(np.asarray(shapes, SHAPE_DTYPE).reshape(-1))
    cxx, cyy, cxy, used = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int32(0)
    st = _ffi.load().stk_psf_from_shapes(s.ctypes.data_as(C.POINTER(_ffi.StarShape)), s.size, float(min_snr), float(scale), C.byref(cxx),
                                         C.byref(cyy), C.byref(cxy), C.byref(used))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("psf_from_shapes: no measured star left, or their moments are not positive definite")
    res = (cxx.value, cyy.value, cxy.value)
    return res + (used.value,) if return_used else res


WAVELET_HARD, WAVELET_SOFT = range(2)                      # STK_WAVELET_*: the layer operation of the wavelet layers


@dataclass
class WaveletParameters:          # extension beyond the reference: include/stacker.h, stk_wavelet_params
    """The a trous wavelet layers of a linear f32 image: `levels` (1 .. 8) layers w_0 .. w_{levels-1} of scale 2^j and the
    residual. Per layer: `gains` (1 = as it is, > 1 sharpens), `thresholds` in units of the layer's noise (0 = none) below
    which a coefficient is shrunk (`mode` WAVELET_HARD: multiplied by 1 - layer_amount; WAVELET_SOFT: moved towards 0 by the
    threshold, blended by layer_amount), `layer_amounts` (0 .. 1). A scalar stands for every level. `residual_gain` scales
    the residual, `amount` (0 .. 1) blends the result with the input, per pixel times the mask. `sigma`: the noise per
    channel (a scalar or up to 4 values); None: estimated from the first layer's median where a threshold needs it. The
    defaults reconstruct the input."""
    levels: int = 4
    mode: int = WAVELET_HARD
    gains: object = 1.0
    thresholds: object = 0.0
    layer_amounts: object = 1.0
    residual_gain: float = 1.0
    amount: float = 1.0
    sigma: object = None

    @staticmethod
    def _table(v, n, what):
        a = np.asarray(v, np.float64).reshape(-1)
        if a.size == 1:
            a = np.repeat(a, n)
        if a.size > n:
            raise InvalidParams(f"{what}: at most {n} values")
        return a

    def _c(self) -> _ffi.WaveletParams:
        c = _ffi.WaveletParams(int(self.levels), int(self.mode), 0 if self.sigma is None else 1, 0)
        for name, v, fill in (("gain", self.gains, 1.0), ("threshold", self.thresholds, 0.0), ("layer_amount", self.layer_amounts, 1.0)):
            a = self._table(v, 8, name)
            getattr(c, name)[:] = [float(x) for x in a] + [fill] * (8 - a.size)
        c.residual_gain, c.amount = float(self.residual_gain), float(self.amount)
        if self.sigma is not None:
            a = self._table(self.sigma, 4, "sigma")
            c.sigma[:] = [float(x) for x in a] + [0.0] * (4 - a.size)
        return c


def wavelet_noise_table(levels: int = 8):
    """e_0 .. e_{levels-1}: the standard deviation of each wavelet layer of unit white noise (stk_wavelet_noise_table; host
    code, no GPU), float64."""
    if not 1 <= int(levels) <= 8:
        raise InvalidParams("wavelet_noise_table: levels 1 .. 8")
    e = np.zeros(int(levels), np.float64)
    st = _ffi.load().stk_wavelet_noise_table(int(levels), e.ctypes.data_as(C.POINTER(C.c_double)))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("wavelet_noise_table: levels 1 .. 8")
    return e


STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE = range(3)      # STK_STRETCH_*: the curve of the display stretch
CURVE_ASINH, CURVE_GAMMA, CURVE_SRGB = range(3)            # STK_CURVE_*: the tables stretch_table builds
DEPTH_U8, DEPTH_U16, DEPTH_F32 = 8, 16, 32                 # STK_DEPTH_*
STAT_DTYPE = np.dtype([("count", np.int64), ("min", np.float32), ("max", np.float32), ("median", np.float32), ("mad", np.float32),
                       ("q", np.float32, 4)])                # stk_image_stat
_DEPTH_DTYPE = {DEPTH_U8: np.uint8, DEPTH_U16: np.uint16, DEPTH_F32: np.float32}


def _four(v, what, fill):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 4)
    if a.size > 4:
        raise InvalidParams(f"{what}: at most 4 values")
    return [float(x) for x in a] + [fill] * (4 - a.size)


@dataclass
class StretchParameters:          # extension beyond the reference: include/stacker.h, stk_stretch_params
    """The display stretch of a linear f32 image: per colour channel x = clamp((v - black) / (white - black), 0, 1), then the
    `curve` (STRETCH_LINEAR; STRETCH_MTF: the midtones transfer function with `midtone` in (0, 1), 0.5 = the identity;
    STRETCH_TABLE: a table of knots + 1 values in 0 .. 1, see stretch_table, linearly interpolated), then the conversion to
    `out_depth` (DEPTH_U8 / DEPTH_U16: rounded half to even; DEPTH_F32: times out_scale). `colour` 1 applies the curve to
    the mean of the three x and scales every channel by the same factor, which keeps hue and saturation. black, white and
    midtone: a scalar or up to 4 values. `table`: read under STRETCH_TABLE."""
    curve: int = STRETCH_MTF
    colour: int = 0
    out_depth: int = DEPTH_F32
    black: object = 0.0
    white: object = 1.0
    midtone: object = 0.5
    out_scale: float = 1.0
    table: object = None

    def _c(self) -> _ffi.StretchParams:
        c = _ffi.StretchParams(int(self.curve), int(self.colour), int(self.out_depth), 0)
        c.black[:], c.white[:], c.midtone[:] = _four(self.black, "black", 0.0), _four(self.white, "white", 1.0), _four(self.midtone, "midtone", 0.5)
        c.out_scale = float(self.out_scale)
        return c

    @staticmethod
    def _from_c(c, table=None) -> "StretchParameters":
        return StretchParameters(c.curve, c.colour, c.out_depth, np.array(c.black[:], np.float32), np.array(c.white[:], np.float32),
                                 np.array(c.midtone[:], np.float32), float(c.out_scale), table)


@dataclass
class AutoStretchParameters:      # extension beyond the reference: include/stacker.h, stk_stretch_auto_params
    """The screen-transfer-function rule: the black point `shadows_clip` (<= 0) robust sigmas below the median (never below the
    minimum), the midtone that sends the median to `target_background`; `linked` 0: per channel (a neutral background), 1: one
    rule from the channels' means. `white_mode` 0: the value `white`; 1: the channel's maximum; 2: its quantile
    `white_quantile` (q[0] of the statistics)."""
    shadows_clip: float = -2.8
    target_background: float = 0.25
    linked: int = 0
    white_mode: int = 0
    white: float = 1.0
    white_quantile: float = 0.999

    def _c(self) -> _ffi.StretchAutoParams:
        return _ffi.StretchAutoParams(float(self.shadows_clip), float(self.target_background), float(self.white), float(self.white_quantile),
                                      int(self.linked), int(self.white_mode))


def _stats_c(stats):
    a = np.zeros(4, STAT_DTYPE)
    s = np.asarray(stats)
    if s.dtype != STAT_DTYPE or s.ndim != 1 or not 1 <= s.size <= 4:
        raise InvalidParams("stats: 1 .. 4 records of STAT_DTYPE expected (Stacker.image_stats)")
    a[:s.size] = s
    return a


def stretch_auto(stats, params: Optional["AutoStretchParameters"] = None) -> "StretchParameters":
    """The auto-stretch rule (stk_stretch_auto; host code, no GPU): from the records of Stacker.image_stats (one per colour
    channel) the StretchParameters with black, white and midtone set, curve STRETCH_MTF, float32 output."""
    s = np.asarray(stats)
    a = _stats_c(s)
    channels = 4 if s.size == 4 else s.size
    if channels == 2:
        raise InvalidParams("stats: 1, 3 or 4 records expected")
    out = _ffi.StretchParams()
    p = (params or AutoStretchParameters())._c()
    st = _ffi.load().stk_stretch_auto(a.ctypes.data_as(C.POINTER(_ffi.ImageStat)), channels, C.byref(p), C.byref(out))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("stretch_auto: parameters out of range or records that are not finite")
    return StretchParameters._from_c(out)


def stretch_table(kind: int = CURVE_ASINH, param: float = 100.0, knots: int = 4096):
    """A table for STRETCH_TABLE (stk_stretch_table; host code, no GPU): knots + 1 float32 values from 0 to 1: CURVE_ASINH:
    asinh(param x) / asinh(param); CURVE_GAMMA: x^(1 / param); CURVE_SRGB: the sRGB encoding."""
    if not 2 <= int(knots) <= 65536:
        raise InvalidParams("stretch_table: knots 2 .. 65536")
    t = np.zeros(int(knots) + 1, np.float32)
    st = _ffi.load().stk_stretch_table(int(kind), float(param), int(knots), t.ctypes.data_as(C.POINTER(C.c_float)))
    if st != 0:
        raise _STATUS_EXC.get(st, StackerError)("stretch_table: an unknown kind or a parameter that is not positive and finite")
    return t


def _quantile_c(q) -> _ffi.QuantileParams:
    """QuantileParameters, a bare float, or None (the median)."""
    if q is None:
        q = QuantileParameters()
    elif not isinstance(q, QuantileParameters):
        q = QuantileParameters(float(q))
    return q._c()


# ---------------------------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


_DEPTH = {"uint8": 8, "uint16": 16, "float32": 32}


def _row_stride_bytes(shape, strides, el):
    """The row step in bytes of a frame (h x w or h x w x c, strides in bytes) whose ONLY non-contiguity is that step: pixels
    and channels packed, rows at least a tight row apart, going forward, on an element boundary. None for anything else."""
    if len(shape) not in (2, 3):
        return None
    c = shape[2] if len(shape) == 3 else 1
    if (len(shape) == 3 and strides[2] != el) or strides[1] != c * el:
        return None
    rs = int(strides[0])
    return rs if rs >= shape[1] * c * el and rs % el == 0 else None


class _Marshalled:
    """Pointers + geometry of a frame stack, keeping the owners alive. A frame that is a row-strided view (a window of a
    wider image, rows padded: _row_stride_bytes) is handed over where it lies, with stk_frames.row_stride_bytes set, if all
    frames of the stack share that stride; every other non-contiguous layout is copied into a contiguous frame first."""

    def __init__(self, frames):
        if _is_torch(frames) and frames.dim() == 4 and frames.is_contiguous() and frames.shape[0] > 0 \
                and str(frames.dtype).replace("torch.", "") in _DEPTH:
            # one tensor holding the whole stack: the pointers are an arithmetic progression — no per-frame Python work
            # (unbinding 256 frames cost ~2 ms per call, 3 % of a 57 ms stack)
            self.keep = [frames]
            self.n = int(frames.shape[0])
            self.location = DEVICE if frames.is_cuda else HOST
            self.torch_device = frames.device if frames.is_cuda else None
            self.devices = {frames.device} if frames.is_cuda else set()
            self.h, self.w, self.c = (int(v) for v in frames.shape[1:])
            self.depth = _DEPTH[str(frames.dtype).replace("torch.", "")]
            step = self.h * self.w * self.c * (self.depth // 8)
            addr = (frames.data_ptr() + np.arange(self.n, dtype=np.uint64) * np.uint64(step)).astype(np.uint64)
            self.ptr_arr = (C.c_void_p * self.n).from_buffer_copy(addr.tobytes())
            self.c_frames = _ffi.Frames(C.cast(self.ptr_arr, C.POINTER(C.c_void_p)), self.n, self.w, self.h, self.c,
                                        self.depth, self.location, 0)
            return
        if _is_torch(frames) and frames.dim() == 4:
            frames = list(frames.unbind(0))
        elif isinstance(frames, np.ndarray) and frames.ndim == 4:
            frames = list(frames)
        frames = list(frames)
        self.keep = []
        self.n = len(frames)
        self.location = HOST
        self.torch_device = None
        self.devices = set()
        ptrs = []
        geo = None
        views = []                        # (index, owner as handed in, row stride in bytes) of the frames that are row-strided views
        for f in frames:
            if _is_torch(f) and f.is_cuda:
                self.location = DEVICE
                if self.torch_device is None:
                    self.torch_device = f.device         # outputs go where the reference frame lives
                self.devices.add(f.device)
                rs = None if f.is_contiguous() else _row_stride_bytes(tuple(f.shape), [s * f.element_size() for s in f.stride()], f.element_size())
                t = f if rs else f.contiguous()
                self.keep.append(t)
                ptrs.append(t.data_ptr())
                g = (tuple(t.shape), str(t.dtype).replace("torch.", ""))
            else:
                v = f.numpy() if _is_torch(f) else f
                rs = None
                if isinstance(v, np.ndarray) and not v.flags.c_contiguous:
                    rs = _row_stride_bytes(v.shape, v.strides, v.itemsize)
                a = v if rs else np.ascontiguousarray(v)
                self.keep.append(a)
                ptrs.append(a.ctypes.data)
                g = (a.shape, str(a.dtype))
            if rs:
                views.append((len(ptrs) - 1, f, rs))
            if len(g[0]) == 2:
                g = ((g[0][0], g[0][1], 1), g[1])
            if geo is None:
                geo = g
            elif g != geo:
                raise InvalidParams("all frames must share size, channels and dtype")
        if self.n:
            (self.h, self.w, self.c), dt = geo
            if dt not in _DEPTH:
                raise InvalidParams(f"unsupported pixel type {dt}")
            self.depth = _DEPTH[dt]
        else:
            self.h = self.w = self.c = 0
            self.depth = 8
        # stk_frames has ONE row stride: the views keep their own memory only if every frame of the stack steps its rows
        # alike (a contiguous frame steps them by the tight row); otherwise they are made contiguous like any other layout
        stride = 0
        if views:
            tight = self.w * self.c * (self.depth // 8)
            if {rs for _, _, rs in views} | ({tight} if len(views) < self.n else set()) == {views[0][2]}:
                stride = views[0][2]
            else:
                for i, f, _ in views:
                    if _is_torch(f) and f.is_cuda:
                        self.keep[i] = f.contiguous()
                        ptrs[i] = self.keep[i].data_ptr()
                    else:
                        self.keep[i] = np.ascontiguousarray(f.numpy() if _is_torch(f) else f)
                        ptrs[i] = self.keep[i].ctypes.data
        self.ptr_arr = (C.c_void_p * max(self.n, 1))(*ptrs)
        self.c_frames = _ffi.Frames(C.cast(self.ptr_arr, C.POINTER(C.c_void_p)), self.n, self.w, self.h, self.c,
                                    self.depth, self.location, stride)


def _image_stride_bytes(img) -> int:
    """row_stride_bytes of an f32 h x w x c image the caller holds: 0 for a contiguous one, the row step of a row-strided
    view (a window of a wider image)."""
    if (img.is_contiguous() if _is_torch(img) else img.flags.c_contiguous):
        return 0
    strides = [s * img.element_size() for s in img.stride()] if _is_torch(img) else img.strides
    rs = _row_stride_bytes(tuple(img.shape), strides, 4)
    if not rs:
        raise InvalidParams("the image must be contiguous or a view whose only non-contiguity is its row step")
    return rs


class Stacker:
    """One engine context (stk_ctx): one GPU, or — `devices=[...]` — several GPUs of the node behind ONE context, the
    moving frames sharded over them and the accumulators reduced with RCCL inside the library (stk_create_multi).
    Not thread-safe: one call at a time per instance."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None):
        self._lib = _ffi.load()
        h = C.c_void_p()
        if devices is not None:
            ids = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            st = self._lib.stk_create_multi(len(devices), ids, C.byref(h))
            device = int(devices[0]) if len(devices) else 0
        else:
            st = self._lib.stk_create(int(device), C.byref(h))
        if st != 0:
            raise HipError(f"stk_create(device={device}, devices={devices}) failed with status {st} (no usable GPU?)")
        self._h = h
        self.device = int(device)
        self.devices = [int(d) for d in devices] if devices is not None else [int(device)]
        self._bound_stream = None          # cuda_stream handle of the torch stream this context runs on, if any

    def _marshal(self, frames) -> "_Marshalled":
        """Pointers of a frame stack; device tensors must be complete before the engine's stream reads them. If this
        context runs ON torch's current stream of that device (use_torch_stream) stream order already guarantees it;
        otherwise — an unbound context, a `with torch.cuda.stream(...)` block, another device — the producer streams
        are drained first (behind the .contiguous() copies _Marshalled itself makes of frames in other layouts)."""
        m = _Marshalled(frames)
        if m.location == DEVICE:
            import torch
            for d in m.devices:
                cur = torch.cuda.current_stream(d)
                if not (self._bound_stream is not None and d.index == self.device and cur.cuda_stream == self._bound_stream):
                    cur.synchronize()
        return m

    def _tensor_ready(self, t):
        """A device tensor the engine is about to touch is complete: the LAST thing the wrapper does with it, behind
        every torch op (a fill, a cast, a .contiguous() copy) the wrapper itself enqueued on it after _marshal's drain.
        Nothing on a context bound to torch's current stream (stream order holds there); a drain of that stream otherwise."""
        import torch
        cur = torch.cuda.current_stream(t.device)
        if not (self._bound_stream is not None and t.device.index == self.device and cur.cuda_stream == self._bound_stream):
            cur.synchronize()

    def rccl_selftest(self, count: int = 1 << 20):
        """Load RCCL, build a communicator over this context's devices and check a sum-reduce (stk_rccl_selftest)."""
        self._check(self._lib.stk_rccl_selftest(self._h, int(count)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.stk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -------------------------------------------------------------------------------
    def _check(self, st: int):
        if st != 0:
            msg = self._lib.stk_last_error(self._h)
            raise _STATUS_EXC.get(st, StackerError)((msg or b"").decode("utf-8", "replace"))

    def set_option(self, name: str, value: int):
        self._check(self._lib.stk_set_option(self._h, name.encode(), int(value)))

    def set_stream(self, stream_ptr: int | None):
        self._check(self._lib.stk_set_stream(self._h, C.c_void_p(stream_ptr or 0)))
        self._bound_stream = None

    def use_torch_stream(self):
        """Run this context on torch's CURRENT stream of its device (captured now; call again after switching streams)."""
        import torch
        h = torch.cuda.current_stream(self.device).cuda_stream
        self.set_stream(h)
        self._bound_stream = h

    def timing(self) -> dict:
        t = _ffi.Timing()
        self._check(self._lib.stk_get_timing(self._h, C.byref(t)))
        d = {k: getattr(t, k) for k, _ in _ffi.Timing._fields_}
        for name in ("ecc_first_iter_slots", "robust_select_us", "prep_stream_frames",
                     "workspaces_empty", "debug_poison_bytes"):   # counters outside stk_timing (stk_get_counter)
            v = C.c_int64(0)
            self._check(self._lib.stk_get_counter(self._h, name.encode(), C.byref(v)))
            d[name] = v.value
        return d

    # -- what every call is built from ------------------------------------------------------
    # Stream ordering: _marshal and _tensor_ready are always called through self; _tensor_ready is the last torch-visible
    # thing done to a device argument and to a freshly filled result. Ownership: every array whose address goes into a
    # call stays referenced until that call has returned — a helper that returns an address returns or holds its owner.
    # Refusals come in one order within a call: sizes (ECC), the empty stack, warps and include flags, records, maps,
    # fields, norm planes, then the output's shape; records are NULL only where _records_arg(optional=True) says so.
    def _stack(self, files) -> "_Marshalled":
        """self._marshal and the empty-stack refusal."""
        m = self._marshal(files)
        if m.n == 0:
            raise NotEnoughFiles("Not enough files")
        return m

    def _alloc(self, where, shape, dtype, fill=None):
        """An array of `shape` and `dtype` (numpy's) where the frames live (`where`: the marshalled stack; or a torch device,
        or None = the host), and its address: (array, address). fill None: uninitialised, the engine writes all of it; else
        filled, and a filled tensor is made ready for the engine here (_tensor_ready behind the fill)."""
        device = getattr(where, "torch_device", where)
        if device is not None:
            import torch
            a = torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=device)
            if fill is not None:
                a.fill_(fill)
                self._tensor_ready(a)
            return a, a.data_ptr()
        a = np.empty(tuple(shape), dtype)
        if fill is not None:
            a.fill(fill)
        return a, a.ctypes.data

    def _image(self, m: _Marshalled, shape=None):
        """The f32 h x w x C output (default: the frames' size) where the frames live: (array, stk_image_f32)."""
        h, w = shape or (m.h, m.w)
        out, addr = self._alloc(m, (h, w, m.c), np.float32)
        return out, _ffi.ImageF32(addr, w, h, m.c, m.location, 0)

    def _optional(self, m: _Marshalled, wanted, dtype, per_channel=False, shape=None):
        """An optional output plane (H x W, or H x W x C, or `shape`) where the frames live: (array, c_void_p), or
        (None, None) = NULL when it is not wanted."""
        if not wanted:
            return None, None
        a, addr = self._alloc(m, shape or ((m.h, m.w, m.c) if per_channel else (m.h, m.w)), dtype)
        return a, C.c_void_p(addr)

    def _plane_table(self, m: _Marshalled, shape, dtype, fill=None):
        """n planes in one n x shape array where the frames live, and the table of their addresses: (array, c_void_p of the
        table). The table is its own owner (ctypes keeps the array a cast pointer came from)."""
        a, base = self._alloc(m, (m.n,) + tuple(shape), dtype, fill)
        step = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return a, C.cast((C.c_void_p * m.n)(*[base + i * step for i in range(m.n)]), C.c_void_p)

    def _as_array(self, m: _Marshalled, x, dtype, shape, error: str):
        """`x` as a contiguous array of `dtype` (and `shape`, unless None; InvalidParams(error) otherwise) where the frames
        live: (owner, address). An array that is already that is used as it is, so that a caller's buffer can be written
        in place. A device conversion is enqueued on torch's stream: the caller ends with _tensor_ready on the owner."""
        if m.location == DEVICE:
            import torch
            t = x if _is_torch(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype)))
            t = t.to(device=m.torch_device, dtype=getattr(torch, np.dtype(dtype).name)).contiguous()
            if shape is not None and tuple(t.shape) != tuple(shape):
                raise InvalidParams(error)
            return t, t.data_ptr()
        a = np.ascontiguousarray(np.asarray(x.cpu().numpy() if _is_torch(x) else x, dtype))
        if shape is not None and a.shape != tuple(shape):
            raise InvalidParams(error)
        return a, a.ctypes.data

    def _array_arg(self, m: _Marshalled, x, dtype, shape, what: str):
        """One argument through _as_array, ready for the engine: (owner, address)."""
        k, addr = self._as_array(m, x, dtype, shape, f"{what}: shape {tuple(shape)} expected")
        if m.location == DEVICE:
            self._tensor_ready(k)
        return k, addr

    def _planes_arg(self, m: _Marshalled, planes, shape, count_error: str, shape_error: str, allow_none: bool = False):
        """n float32 planes through _as_array: (owners, pointer array). allow_none: an entry may be None (a NULL plane).
        One _tensor_ready behind the last conversion: the casts and copies all went onto one stream."""
        planes = list(planes)
        if len(planes) != m.n:
            raise InvalidParams(count_error)
        keep, ptrs = [], []
        for p in planes:
            if p is None and allow_none:
                ptrs.append(None)
                continue
            k, addr = self._as_array(m, p, np.float32, shape, shape_error)
            keep.append(k)
            ptrs.append(addr)
        if m.location == DEVICE and keep:
            self._tensor_ready(keep[-1])
        return keep, (C.c_void_p * m.n)(*ptrs)

    def _maps_arg(self, m: _Marshalled, maps, optional: bool = False):
        """n tightly packed H x W float32 planes where the frames live: (owners, pointer array). optional: `maps` may be
        None (no table: (None, None)) and single entries may be None (NULL planes: all ones)."""
        if optional and maps is None:
            return None, None
        return self._planes_arg(m, maps, (m.h, m.w), "one weight map (or None) per frame expected" if optional
                                else "one weight map per frame expected", "weight maps: H x W planes expected", optional)

    def _fields_arg(self, m: _Marshalled, fields, step, allow_none: bool = False):
        """n tightly packed gh x gw x 2 float32 planes where the frames live: (owners, pointer array). allow_none: an entry
        may be None (a NULL plane: no displacement). A bad step is left to the engine."""
        shape = mesh_grid(m.w, m.h, step)[::-1] + (2,) if step in (8, 16, 32, 64, 128, 256) else None
        return self._planes_arg(m, fields, shape, "one field per frame expected", "fields: gh x gw x 2 planes expected (mesh_grid)",
                                allow_none)

    def _warps_arg(self, warps, include, n):
        Ms = []
        for w in warps:
            Md = np.asarray(w, np.float64).reshape(-1)
            Ms.append(np.concatenate([Md, [0.0, 0.0, 1.0]]) if Md.size == 6 else Md)
        if len(Ms) != n or any(x.size != 9 for x in Ms):
            raise InvalidParams("one 3x3 (or 2x3) warp per frame expected")
        inc = None if include is None else np.ascontiguousarray(np.asarray(include, np.int32).reshape(-1))
        if inc is not None and inc.size != n:
            raise InvalidParams("one include flag per frame expected")
        return np.ascontiguousarray(np.stack(Ms)), inc

    @staticmethod
    def _border_arg(border_value):
        """border_value padded to the four doubles the ABI reads."""
        return np.asarray((list(border_value) + [0.0] * 4)[:4], np.float64)

    def _warped(self, files, warps, include, is_affine, border=None, alpha=None):
        """The head of every caller-held-warps call: self._stack, the warps and include flags (_warps_arg: the first
        refusals of such a call), and the run every such ABI function starts with — [ctx, frames, warps, include,
        is_affine, (border_mode, border_value), (alpha)], border = (border_mode, border_value) and alpha present or absent
        as the function has them (drizzle and reject: no border; local_align: neither). Returns (m, head); the arrays behind
        the head's addresses go into m.keep, so hold m until the C call has returned."""
        m = self._stack(files)
        Md, inc = self._warps_arg(warps, include, m.n)
        m.keep += [Md, inc]
        head = [self._h, C.byref(m.c_frames), C.c_void_p(Md.ctypes.data), None if inc is None else C.c_void_p(inc.ctypes.data),
                int(is_affine)]
        if border is not None:
            bv = self._border_arg(border[1])
            m.keep.append(bv)
            head += [int(border[0]), C.c_void_p(bv.ctypes.data)]
        if alpha is not None:
            head.append(float(alpha))
        return m, head

    def _whole_stack(self, kind, suffix, files, params, scale_down_width, return_stats, combine=(), outputs=(), after_stats=(),
                     image_shape=None, n_stats=None):
        """Every ecc_match* / keypoint_match* form (kind "ecc" or "keypoint", stk_<kind>_match<suffix>): the ECC-only size
        refusal, self._stack, the output image, stats and dropped, the call, the result. The ABI's fixed order —
        [ctx, frames, params, scale_down_width, *combine, image, (dropped if keypoint), *outputs, stats, *after_stats].
        combine: the combine-specific arguments: a ctypes structure goes by reference, a numpy array by address, None as
        NULL, a scalar as it is; a function is called with m first (what needs n: per-frame weights). They stay referenced
        here until the call has returned. outputs, after_stats: [(wanted, make)], make(m, wanted) -> (argument or list of
        arguments, value(stats list)) — built after the image, in the ABI's order, which is the order of the result.
        image_shape(m): another output size than the frames'; n_stats(): how many stats the result carries (default n).
        The result: a keypoint form always returns a tuple that starts with dropped; an ECC form the bare image when
        nothing else is wanted, else the tuple; then the wanted values in order; the stats last."""
        if kind == "ecc" and isinstance(files, (list, tuple)) and len({tuple(f.shape[:2]) for f in files}) > 1:
            raise OpenCvError("the frames differ in size: the reference fails on such a stack in cv::add (lib.rs:809)")
        m = self._stack(files)
        out, img = self._image(m, image_shape(m) if image_shape else None)
        stats = (_ffi.FrameStats * m.n)()
        dropped = C.c_int32(0)
        p = params._c()
        keep = [x(m) if callable(x) else x for x in combine]
        args = [self._h, C.byref(m.c_frames), C.byref(p), float(scale_down_width or 0.0)]
        args += [C.byref(x) if isinstance(x, C.Structure) else C.c_void_p(x.ctypes.data) if isinstance(x, np.ndarray) else x for x in keep]
        args += [C.byref(img)] + ([C.byref(dropped)] if kind == "keypoint" else [])
        values = []
        for group, end in ((outputs, [stats]), (after_stats, [])):
            for wanted, make in group:
                arg, value = make(m, wanted)
                args += arg if isinstance(arg, list) else [arg]
                if wanted:
                    values.append(value)
            args += end
        self._check(getattr(self._lib, f"stk_{kind}_match{suffix}")(*args))
        stl = self._stats_list(stats, m.n if n_stats is None else n_stats())
        res = ((dropped.value,) if kind == "keypoint" else ()) + (out,) + tuple(v(stl) for v in values) + ((stl,) if return_stats else ())
        return res if kind == "keypoint" or len(res) > 1 else out

    # the makers of _whole_stack's optional outputs
    def _out_plane(self, dtype, per_channel=False, shape=None):
        """An optional output plane (_optional), NULL when not wanted; shape(m): another size than H x W."""
        def make(m, wanted):
            a, ptr = self._optional(m, wanted, dtype, per_channel, shape(m) if shape else None)
            return ptr, lambda stl: a
        return make

    @staticmethod
    def _out_applied(m, wanted):
        """The per-frame records the fold used: always passed."""
        applied = (_ffi.FrameWeight * m.n)()
        return applied, lambda stl: Stacker._applied_list(applied, m.n, m.c)

    def _out_norm_planes(self, kind, step):
        """The local-normalisation planes by frame index, zeroed; frame 0 and dropped frames have none (None in the result)."""
        def make(m, wanted):
            if not wanted:
                return None, None
            gw, gh = mesh_grid(m.w, m.h, int(step))
            planes = [np.zeros((gh, gw, 2 * m.c), np.float32) for _ in range(m.n)]
            return (C.c_void_p * m.n)(*[p.ctypes.data for p in planes]), \
                lambda stl: [None if i == 0 or (kind == "keypoint" and stl[i]["status"] != 0) else planes[i] for i in range(m.n)]
        return make

    def _weights_combine(self, weights):
        """The per-frame weights of a whole-stack call as a combine argument: n f32, or NULL = all 1."""
        return lambda m: self._weights_arg(weights, m.n)

    @staticmethod
    def _stats_list(stats, n):
        return [dict(status=s.status, iterations=s.iterations, rho=s.rho, n_keypoints=s.n_keypoints,
                     n_matches=s.n_matches, n_inliers=s.n_inliers, warp=np.array(list(s.warp)).reshape(3, 3))
                for s in stats[:n]]

    # -- whole-stack API (the reference's two entry points) ---------------------------------------
    def ecc_match(self, files, params: EccMatchParameters, scale_down_width: Optional[float] = None,
                  return_stats: bool = False):
        return self._whole_stack("ecc", "", files, params, scale_down_width, return_stats)

    def _keypoint_match_mixed(self, frames, params: KeyPointMatchParameters, return_stats: bool, scale_down_width=None):
        """Frames of differing size (host arrays, HxWx3 u8): ORB at each frame's own size, every frame warped into the FIRST
        frame's size, as the reference does (lib.rs:166, 200-204, 290-299) — stk_keypoint_match_mixed."""
        arrs = [np.ascontiguousarray(f.cpu().numpy() if _is_torch(f) else f) for f in frames]
        cn = arrs[0].shape[2] if arrs[0].ndim == 3 else 0
        for a in arrs:
            if a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[2] != cn or a.dtype != np.uint8:
                raise OpenCvError("ORB: 8-bit BGR / BGRA frames of one type expected")
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        geo = (_ffi.FrameGeometry * n)(*[_ffi.FrameGeometry(a.shape[1], a.shape[0], 0) for a in arrs])
        h0, w0 = arrs[0].shape[:2]
        fr = _ffi.Frames(C.cast(ptrs, C.POINTER(C.c_void_p)), n, w0, h0, cn, 8, HOST, 0)
        out = np.empty((h0, w0, cn), np.float32)
        img = _ffi.ImageF32(out.ctypes.data, w0, h0, cn, HOST, 0)
        stats = (_ffi.FrameStats * n)()
        dropped = C.c_int32(0)
        p = params._c()
        self._check(self._lib.stk_keypoint_match_mixed(self._h, C.byref(fr), geo, C.byref(p), float(scale_down_width or 0.0), C.byref(img), C.byref(dropped), stats))
        return (dropped.value, out, self._stats_list(stats, n)) if return_stats else (dropped.value, out)

    def keypoint_match(self, files, params: KeyPointMatchParameters, scale_down_width: Optional[float] = None,
                       return_stats: bool = False):
        if isinstance(files, (list, tuple)) and len({tuple(f.shape) for f in files}) > 1:
            return self._keypoint_match_mixed(files, params, return_stats, scale_down_width)
        return self._whole_stack("keypoint", "", files, params, scale_down_width, return_stats)

    # -- score and rank a whole stack (the first half of examples/main.rs) ---------------------------------
    def stack_sharpness(self, files, ksize: int = 3):
        """LAPM, LAPV, TENG(ksize) and GLVN of every frame of an 8-bit stack in one device pass (stk_stack_sharpness): an
        n x 4 float64 array, the doubles sharpness_*(grey(frame)) return."""
        m = self._stack(files)
        scores = np.zeros((m.n, 4), np.float64)
        self._check(self._lib.stk_stack_sharpness(self._h, C.byref(m.c_frames), int(ksize), C.c_void_p(scores.ctypes.data)))
        return scores

    def rank(self, files, select: Optional["SelectParameters"] = None):
        """Score the stack and select: (order, n_kept, scores, weights) — stack_sharpness followed by rank_frames."""
        select = select or SelectParameters()
        scores = self.stack_sharpness(files, select.ksize)
        order, n_kept, weights = rank_frames(scores, select)
        return order, n_kept, scores, weights

    def _ranked_match(self, kind, files, params, select, scale_down_width, return_stats, return_scores):
        """The ranked forms pass their ranking behind the stats — [.., stats, select, order, kept, scores] — and return
        order[:kept] and the stats of the kept list."""
        sp, kept = (select or SelectParameters())._c(), C.c_int32(0)

        def ranking(m, wanted):
            order = (C.c_int32 * m.n)()
            return [C.byref(sp), order, C.byref(kept)], lambda stl: np.array(order[:kept.value], np.int32)

        def scores(m, wanted):
            sc = np.zeros((m.n, 4), np.float64)
            return C.c_void_p(sc.ctypes.data), lambda stl: sc
        return self._whole_stack(kind, "_ranked", files, params, scale_down_width, return_stats,
                                 after_stats=[(True, ranking), (return_scores, scores)], n_stats=lambda: kept.value)

    def ecc_match_ranked(self, files, params: EccMatchParameters, select: Optional["SelectParameters"] = None,
                         scale_down_width: Optional[float] = None, return_scores: bool = False, return_stats: bool = False):
        """Rank the stack on the device, drop what `select` drops, make the sharpest frame the reference and run ecc_match on
        that list (stk_ecc_match_ranked): (image, order[:n_kept][, scores][, stats]); the stats follow the kept list."""
        return self._ranked_match("ecc", files, params, select, scale_down_width, return_stats, return_scores)

    def keypoint_match_ranked(self, files, params: KeyPointMatchParameters, select: Optional["SelectParameters"] = None,
                              scale_down_width: Optional[float] = None, return_scores: bool = False, return_stats: bool = False):
        """keypoint_match behind the ranking (stk_keypoint_match_ranked): (dropped, image, order[:n_kept][, scores][, stats])."""
        return self._ranked_match("keypoint", files, params, select, scale_down_width, return_stats, return_scores)

    # -- sigma-clipped combines (extension beyond the reference) -----------------------------------------
    def _match_clipped(self, kind, suffix, cp, files, params, scale_down_width, return_stats, return_counts):
        return self._whole_stack(kind, suffix, files, params, scale_down_width, return_stats, [cp],
                                 [(return_counts, self._out_plane(np.int32, True))])

    def ecc_match_clipped(self, files, params: EccMatchParameters, clip: Optional["SigmaClipParameters"] = None,
                          scale_down_width: Optional[float] = None, return_stats: bool = False, return_counts: bool = False):
        """ecc_match with kappa-sigma rejection over the aligned frames instead of the plain mean (stk_ecc_match_clipped).
        Returns the image, then the per-pixel counts of kept samples (return_counts) and the stats (return_stats)."""
        return self._match_clipped("ecc", "_clipped", (clip or SigmaClipParameters())._c(), files, params, scale_down_width,
                                   return_stats, return_counts)

    def keypoint_match_clipped(self, files, params: KeyPointMatchParameters, clip: Optional["SigmaClipParameters"] = None,
                               scale_down_width: Optional[float] = None, return_stats: bool = False, return_counts: bool = False):
        """keypoint_match with kappa-sigma rejection (stk_keypoint_match_clipped): (dropped, image[, counts][, stats])."""
        return self._match_clipped("keypoint", "_clipped", (clip or SigmaClipParameters())._c(), files, params, scale_down_width,
                                   return_stats, return_counts)

    def clip_stack(self, files, warps, clip: Optional["SigmaClipParameters"] = None, include=None, *, is_affine=False,
                   border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0, return_counts: bool = False):
        """The clipped combine alone over caller-held warps (stk_clip_stack): warps[i] is frame i's forward matrix as
        warp_accumulate takes it (3x3, or 2x3 for affine), frame 0's included; include: per-frame flags or None = all."""
        return self._clip_stack(self._lib.stk_clip_stack, (clip or SigmaClipParameters())._c(), files, warps, include, is_affine,
                                border_mode, border_value, alpha, return_counts)

    def _clip_stack(self, fn, cp, files, warps, include, is_affine, border_mode, border_value, alpha, return_counts):
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        out, img = self._image(m)
        cnt, cptr = self._optional(m, return_counts, np.int32, True)
        self._check(fn(*head, C.byref(cp), C.byref(img), cptr))
        return (out, cnt) if return_counts else out

    # -- median / MAD clipped combines (extension beyond the reference) --------------------------------
    def ecc_match_robust_clipped(self, files, params: EccMatchParameters, clip: Optional["RobustClipParameters"] = None,
                                 scale_down_width: Optional[float] = None, return_stats: bool = False, return_counts: bool = False):
        """ecc_match with median / MAD rejection over the aligned frames (stk_ecc_match_robust_clipped): the clip that
        still rejects on a handful of frames. Returns as ecc_match_clipped."""
        return self._match_clipped("ecc", "_robust_clipped", (clip or RobustClipParameters())._c(), files, params, scale_down_width,
                                   return_stats, return_counts)

    def keypoint_match_robust_clipped(self, files, params: KeyPointMatchParameters, clip: Optional["RobustClipParameters"] = None,
                                      scale_down_width: Optional[float] = None, return_stats: bool = False,
                                      return_counts: bool = False):
        """keypoint_match with median / MAD rejection (stk_keypoint_match_robust_clipped): (dropped, image[, counts][, stats])."""
        return self._match_clipped("keypoint", "_robust_clipped", (clip or RobustClipParameters())._c(), files, params,
                                   scale_down_width, return_stats, return_counts)

    def robust_clip_stack(self, files, warps, clip: Optional["RobustClipParameters"] = None, include=None, *, is_affine=False,
                          border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0, return_counts: bool = False):
        """The median / MAD clip alone over caller-held warps (stk_robust_clip_stack), with the arguments of clip_stack."""
        return self._clip_stack(self._lib.stk_robust_clip_stack, (clip or RobustClipParameters())._c(), files, warps, include,
                                is_affine, border_mode, border_value, alpha, return_counts)

    # -- median / quantile combines (extension beyond the reference) -----------------------------------
    def ecc_match_quantile(self, files, params: EccMatchParameters, quantile=None, scale_down_width: Optional[float] = None,
                           return_stats: bool = False):
        """ecc_match with a per-pixel quantile of the aligned frames instead of the plain mean (stk_ecc_match_quantile).
        quantile: QuantileParameters or a float in [0, 1]; None = the median."""
        return self._whole_stack("ecc", "_quantile", files, params, scale_down_width, return_stats, [_quantile_c(quantile)])

    def keypoint_match_quantile(self, files, params: KeyPointMatchParameters, quantile=None,
                                scale_down_width: Optional[float] = None, return_stats: bool = False):
        """keypoint_match with the quantile combine (stk_keypoint_match_quantile): (dropped, image[, stats])."""
        return self._whole_stack("keypoint", "_quantile", files, params, scale_down_width, return_stats, [_quantile_c(quantile)])

    def quantile_stack(self, files, warps, quantile=None, include=None, *, is_affine=False, border_mode=BORDER_CONSTANT,
                       border_value=(0, 0, 0, 0), alpha=1.0 / 255.0):
        """The quantile combine alone over caller-held warps (stk_quantile_stack), with the arguments of clip_stack."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        out, img = self._image(m)
        qp = _quantile_c(quantile)
        self._check(self._lib.stk_quantile_stack(*head, C.byref(qp), C.byref(img)))
        return out

    # -- weighted, coverage-aware combines (extension beyond the reference) ----------------------------
    @staticmethod
    def _applied_list(applied, n, cn):
        return [dict(gain=np.array(list(a.gain)[:cn], np.float32), offset=np.array(list(a.offset)[:cn], np.float32),
                     weight=float(a.weight), flags=int(a.flags)) for a in applied[:n]]

    @staticmethod
    def _weights_arg(weights, n):
        """n per-frame weights as an f32 array, or None = all 1."""
        if weights is None:
            return None
        w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
        if w.size != n:
            raise InvalidParams("one weight per frame expected")
        return w

    def _match_weighted(self, kind, suffix, files, params, weight, weights, local, scale_down_width, return_stats, return_coverage,
                        return_applied):
        combine = [(weight or WeightParameters())._c(), self._weights_combine(weights)] + ([local._c()] if local else [])
        return self._whole_stack(kind, suffix, files, params, scale_down_width, return_stats, combine,
                                 [(return_coverage, self._out_plane(np.float32)), (return_applied, self._out_applied)])

    def ecc_match_weighted(self, files, params: EccMatchParameters, weight: Optional["WeightParameters"] = None, weights=None,
                           scale_down_width: Optional[float] = None, return_stats: bool = False, return_coverage: bool = False,
                           return_applied: bool = False):
        """ecc_match with the weighted, coverage-aware mean and per-frame normalisation instead of the plain mean
        (stk_ecc_match_weighted). weights: one per frame or None = all 1. Returns the image, then the summed-weight plane
        (return_coverage), the per-frame records the fold used (return_applied) and the stats (return_stats)."""
        return self._match_weighted("ecc", "_weighted", files, params, weight, weights, None, scale_down_width, return_stats,
                                    return_coverage, return_applied)

    def keypoint_match_weighted(self, files, params: KeyPointMatchParameters, weight: Optional["WeightParameters"] = None,
                                weights=None, scale_down_width: Optional[float] = None, return_stats: bool = False,
                                return_coverage: bool = False, return_applied: bool = False):
        """keypoint_match with the weighted combine (stk_keypoint_match_weighted): (dropped, image[, coverage][, applied]
        [, stats]). A dropped frame is no sample: weight 0 in `applied`."""
        return self._match_weighted("keypoint", "_weighted", files, params, weight, weights, None, scale_down_width, return_stats,
                                    return_coverage, return_applied)

    # -- noise estimation and inverse-variance weights (extension beyond the reference) ---------------
    def stack_noise(self, files, return_hist: bool = False):
        """The noise statistics of every frame and channel of a u8 or u16 stack in one device pass (stk_stack_noise): an
        n x 4 NOISE_DTYPE array (the unused channel slots zeroed); with return_hist also the exact histograms, an
        n x channels x (BV + BR) uint32 array: the values' (256 / 65 536 bins), then the capped residuals' (2041 / 65 536)."""
        m = self._stack(files)
        stats = np.zeros((m.n, 4), NOISE_DTYPE)
        hist = np.zeros((m.n, m.c, (256 + 2041) if m.depth == 8 else 131072), np.uint32) if return_hist else None
        self._check(self._lib.stk_stack_noise(self._h, C.byref(m.c_frames), stats.ctypes.data_as(C.POINTER(_ffi.NoiseStat)),
                                              None if hist is None else C.c_void_p(hist.ctypes.data)))
        return (stats, hist) if return_hist else stats

    def _match_noise_weighted(self, kind, files, params, weight, weights, noise, scale_down_width, return_stats, return_coverage,
                              return_applied, return_noise):
        """The noise-weighted forms pass sigma_floor behind the weights and the statistics behind the stats."""
        def noise_out(m, wanted):
            if not wanted:
                return None, None
            ns = np.zeros((m.n, 4), NOISE_DTYPE)
            return ns.ctypes.data_as(C.POINTER(_ffi.NoiseStat)), lambda stl: ns
        combine = [(weight or WeightParameters())._c(), self._weights_combine(weights),
                   lambda m: C.c_double((noise or NoiseParameters()).floor(m.depth))]
        return self._whole_stack(kind, "_noise_weighted", files, params, scale_down_width, return_stats, combine,
                                 [(return_coverage, self._out_plane(np.float32)), (return_applied, self._out_applied)],
                                 after_stats=[(return_noise, noise_out)])

    def ecc_match_noise_weighted(self, files, params: EccMatchParameters, weight: Optional["WeightParameters"] = None, weights=None,
                                 noise: Optional["NoiseParameters"] = None, scale_down_width: Optional[float] = None,
                                 return_stats: bool = False, return_coverage: bool = False, return_applied: bool = False,
                                 return_noise: bool = False):
        """ecc_match_weighted with every frame weighted by the inverse of its measured noise variance
        (stk_ecc_match_noise_weighted): stack_noise, noise_weights under the gains of `weight`'s normalisation, one weighted
        fold. weights: the caller's own per-frame factors. Returns the image, then as asked the coverage, the applied
        records, the noise statistics (return_noise) and, last, the stats."""
        return self._match_noise_weighted("ecc", files, params, weight, weights, noise, scale_down_width, return_stats, return_coverage,
                                          return_applied, return_noise)

    def keypoint_match_noise_weighted(self, files, params: KeyPointMatchParameters, weight: Optional["WeightParameters"] = None,
                                      weights=None, noise: Optional["NoiseParameters"] = None, scale_down_width: Optional[float] = None,
                                      return_stats: bool = False, return_coverage: bool = False, return_applied: bool = False,
                                      return_noise: bool = False):
        """keypoint_match_weighted with noise weights (stk_keypoint_match_noise_weighted): (dropped, image[, coverage]
        [, applied][, noise][, stats]). A dropped frame is no sample: weight 0 in `applied`."""
        return self._match_noise_weighted("keypoint", files, params, weight, weights, noise, scale_down_width, return_stats,
                                          return_coverage, return_applied, return_noise)

    def weighted_stack(self, files, warps, gain=None, offset=None, weights=None, include=None, *, applied=None, coverage: bool = True,
                       is_affine=False, border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0,
                       return_coverage: bool = False):
        """The weighted combine alone over caller-held warps (stk_weighted_stack), with the arguments of clip_stack.
        gain, offset: n x channels (None = 1 / 0); weights: n (None = 1); or `applied`: the per-frame records another
        weighted call returned, used as given."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        rec = self._records_arg(m, gain, offset, weights, applied)
        out, img = self._image(m)
        cov, cptr = self._optional(m, return_coverage, np.float32)
        self._check(self._lib.stk_weighted_stack(*head, rec, int(coverage), C.byref(img), cptr))
        return (out, cov) if return_coverage else out

    def overlap_moments(self, files, warps, include=None, *, stat_step: int = 4, is_affine=False, border_mode=BORDER_CONSTANT,
                        border_value=(0, 0, 0, 0), alpha=1.0 / 255.0):
        """The overlap moments of every included frame against frame 0 (stk_overlap_moments): an n x channels x 6 float64
        array (n, sum X, sum Y, sum X^2, sum Y^2, sum XY), zeros for frame 0 and excluded frames."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        mom = np.zeros((m.n, m.c, 6), np.float64)
        self._check(self._lib.stk_overlap_moments(*head, int(stat_step), C.c_void_p(mom.ctypes.data)))
        return mom

    # -- local normalisation: gain and offset fields on a node grid (extension beyond the reference) ------
    def local_moments(self, files, warps, step: int, include=None, *, stat_step: int = 4, is_affine=False,
                      border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0):
        """The cell moments of every included frame against frame 0 (stk_local_moments): an n x ch x cw x channels x 6
        float64 array, zeros for frame 0 and excluded frames."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        step = int(step)
        ch, cw = ((m.h + step - 1) // step, (m.w + step - 1) // step) if step > 0 else (1, 1)
        mom = np.zeros((m.n, ch, cw, m.c, 6), np.float64)
        self._check(self._lib.stk_local_moments(*head, step, int(stat_step), C.c_void_p(mom.ctypes.data)))
        return mom

    def _norm_arg(self, m: _Marshalled, norm, step):
        """n host planes by frame index (None entries allowed) for the grid of `step` -> (keep-alive list, pointer array or
        None)."""
        if norm is None:
            return None, None
        if len(norm) != m.n:
            raise InvalidParams("one normalisation plane (or None) per frame expected")
        keep = [None if p is None else np.ascontiguousarray(np.asarray(p, np.float32)) for p in norm]
        if any(p is not None and (p.ndim != 3 or p.shape[2] != 2 * m.c) for p in keep):
            raise InvalidParams("normalisation planes: gh x gw x 2 channels f32 expected")
        self._norm_shapes(m, keep, step)
        return keep, (C.c_void_p * m.n)(*[None if p is None else p.ctypes.data for p in keep])

    @staticmethod
    def _norm_shapes(m: _Marshalled, keep, step):
        try:
            gw, gh = mesh_grid(m.w, m.h, int(step))
        except InvalidParams:
            return                                # the engine reports the bad step
        if any(p is not None and p.shape[:2] != (gh, gw) for p in keep):
            raise InvalidParams("normalisation planes: gh x gw x 2 channels f32 expected")

    def _local_norm_stack(self, fn, cp, files, warps, norm, step, gain, offset, weights, include, applied, coverage, is_affine,
                          border_mode, border_value, alpha, outputs):
        """The *_local_norm stacks: [head, (combine parameters), records, planes, step, coverage, image, *outputs];
        outputs: [(wanted, dtype, per_channel)]. The records are always built."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        rec = self._records_arg(m, gain, offset, weights, applied)
        keep, nptr = self._norm_arg(m, norm, step)
        out, img = self._image(m)
        outs = [self._optional(m, *o) for o in outputs]
        self._check(fn(*head, *([] if cp is None else [C.byref(cp)]), rec, nptr, int(step), int(coverage), C.byref(img),
                       *[ptr for _, ptr in outs]))
        res = (out,) + tuple(a for a, _ in outs if a is not None)
        return res if len(res) > 1 else out

    def local_norm_stack(self, files, warps, norm, step: int, gain=None, offset=None, weights=None, include=None, *, applied=None,
                         coverage: bool = True, is_affine=False, border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0),
                         alpha=1.0 / 255.0, return_den: bool = False):
        """The locally normalised mean alone over caller-held warps (stk_local_norm_stack): weighted_stack whose gain and
        offset come from `norm`, n planes (gh x gw x 2 channels, numpy) by frame index for the grid of `step`; a frame whose
        plane is None uses its record (gain / offset / `applied`)."""
        return self._local_norm_stack(self._lib.stk_local_norm_stack, None, files, warps, norm, step, gain, offset, weights, include,
                                      applied, coverage, is_affine, border_mode, border_value, alpha, [(return_den, np.float32)])

    def quantile_stack_local_norm(self, files, warps, norm, step: int, quantile=None, gain=None, offset=None, weights=None,
                                  include=None, *, applied=None, coverage: bool = True, is_affine=False,
                                  border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0,
                                  return_counts: bool = False):
        """The locally normalised quantile alone over caller-held warps (stk_quantile_stack_local_norm):
        quantile_stack_weighted through the planes of local_norm_stack."""
        return self._local_norm_stack(self._lib.stk_quantile_stack_local_norm, _quantile_c(quantile), files, warps, norm, step, gain,
                                      offset, weights, include, applied, coverage, is_affine, border_mode, border_value, alpha,
                                      [(return_counts, np.int32)])

    def _match_local_normalized(self, kind, suffix, files, params, norm, combine, weights, scale_down_width, return_stats, outputs,
                                return_norm, return_applied):
        """Both local-normalised families: [.., norm parameters, *combine, weights, image, .., *outputs, planes, applied,
        stats]; frame 0 and dropped frames have no plane (_out_norm_planes)."""
        np_ = (norm or LocalNormParameters())._c()
        return self._whole_stack(kind, suffix, files, params, scale_down_width, return_stats,
                                 [np_] + combine + [self._weights_combine(weights)],
                                 outputs + [(return_norm, self._out_norm_planes(kind, np_.step)), (return_applied, self._out_applied)])

    def ecc_match_local_normalized(self, files, params: EccMatchParameters, norm: Optional["LocalNormParameters"] = None,
                                   quantile=None, weights=None, scale_down_width: Optional[float] = None, return_stats: bool = False,
                                   return_den: bool = False, return_counts: bool = False, return_norm: bool = False,
                                   return_applied: bool = False):
        """ecc_match with local normalisation (stk_ecc_match_local_normalized): the locally normalised mean, or with
        `quantile` the locally normalised quantile. Returns the image, then den (return_den, mean only), the counts
        (return_counts, quantile only), the planes by frame index (return_norm; None for frame 0), the global records
        (return_applied) and the stats."""
        return self._match_local_normalized("ecc", "_local_normalized", files, params, norm,
                                            [None if quantile is None else _quantile_c(quantile)], weights, scale_down_width, return_stats,
                                            [(return_den, self._out_plane(np.float32)), (return_counts, self._out_plane(np.int32))],
                                            return_norm, return_applied)

    def keypoint_match_local_normalized(self, files, params: KeyPointMatchParameters, norm: Optional["LocalNormParameters"] = None,
                                        quantile=None, weights=None, scale_down_width: Optional[float] = None,
                                        return_stats: bool = False, return_den: bool = False, return_counts: bool = False,
                                        return_norm: bool = False, return_applied: bool = False):
        """keypoint_match with local normalisation (stk_keypoint_match_local_normalized): (dropped, image, ...) as
        ecc_match_local_normalized; a dropped frame has no plane and weight 0 in `applied`."""
        return self._match_local_normalized("keypoint", "_local_normalized", files, params, norm,
                                            [None if quantile is None else _quantile_c(quantile)], weights, scale_down_width, return_stats,
                                            [(return_den, self._out_plane(np.float32)), (return_counts, self._out_plane(np.int32))],
                                            return_norm, return_applied)

    # -- the two clip combines through the planes --
    def clip_stack_local_norm(self, files, warps, norm, step: int, clip: Optional["SigmaClipParameters"] = None, gain=None,
                              offset=None, weights=None, include=None, *, applied=None, coverage: bool = True, is_affine=False,
                              border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0,
                              return_counts: bool = False, return_kept_weight: bool = False):
        """The locally normalised sigma clip alone over caller-held warps (stk_clip_stack_local_norm): clip_stack_weighted
        through the planes of local_norm_stack. Returns the image, then the counts and the kept weight per pixel and channel."""
        return self._local_norm_stack(self._lib.stk_clip_stack_local_norm, (clip or SigmaClipParameters())._c(), files, warps, norm,
                                      step, gain, offset, weights, include, applied, coverage, is_affine, border_mode, border_value,
                                      alpha, [(return_counts, np.int32, True), (return_kept_weight, np.float32, True)])

    def robust_clip_stack_local_norm(self, files, warps, norm, step: int, clip: Optional["RobustClipParameters"] = None, gain=None,
                                     offset=None, weights=None, include=None, *, applied=None, coverage: bool = True,
                                     is_affine=False, border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0,
                                     return_counts: bool = False, return_kept_weight: bool = False):
        """The locally normalised median / MAD clip alone over caller-held warps (stk_robust_clip_stack_local_norm), with the
        arguments and results of clip_stack_local_norm."""
        return self._local_norm_stack(self._lib.stk_robust_clip_stack_local_norm, (clip or RobustClipParameters())._c(), files, warps,
                                      norm, step, gain, offset, weights, include, applied, coverage, is_affine, border_mode,
                                      border_value, alpha, [(return_counts, np.int32, True), (return_kept_weight, np.float32, True)])

    @staticmethod
    def _clip_choice(clip):
        """clip= of the *_local_normalized_clipped calls -> (stk_clip_params or None, stk_robust_clip_params or None)."""
        if isinstance(clip, SigmaClipParameters):
            return clip._c(), None
        if isinstance(clip, RobustClipParameters):
            return None, clip._c()
        if isinstance(clip, (tuple, list)) and len(clip) == 2 and all(c is not None for c in clip):
            raise InvalidParams("clip: one of SigmaClipParameters and RobustClipParameters expected, not both")
        raise InvalidParams("clip: a SigmaClipParameters or a RobustClipParameters expected")

    def ecc_match_local_normalized_clipped(self, files, params: EccMatchParameters, norm: Optional["LocalNormParameters"] = None,
                                           clip=None, weights=None, scale_down_width: Optional[float] = None,
                                           return_stats: bool = False, return_counts: bool = False, return_kept_weight: bool = False,
                                           return_norm: bool = False, return_applied: bool = False):
        """ecc_match with local normalisation and rejection (stk_ecc_match_local_normalized_clipped). clip: a
        SigmaClipParameters (the locally normalised sigma clip) or a RobustClipParameters (the median / MAD clip); exactly
        one. Returns the image, then the counts, the kept weight, the planes by frame index, the global records and the stats."""
        return self._match_local_normalized("ecc", "_local_normalized_clipped", files, params, norm, list(self._clip_choice(clip)),
                                            weights, scale_down_width, return_stats,
                                            [(return_counts, self._out_plane(np.int32, True)),
                                             (return_kept_weight, self._out_plane(np.float32, True))], return_norm, return_applied)

    def keypoint_match_local_normalized_clipped(self, files, params: KeyPointMatchParameters,
                                                norm: Optional["LocalNormParameters"] = None, clip=None, weights=None,
                                                scale_down_width: Optional[float] = None, return_stats: bool = False,
                                                return_counts: bool = False, return_kept_weight: bool = False,
                                                return_norm: bool = False, return_applied: bool = False):
        """keypoint_match with local normalisation and rejection (stk_keypoint_match_local_normalized_clipped): (dropped,
        image, ...) as ecc_match_local_normalized_clipped."""
        return self._match_local_normalized("keypoint", "_local_normalized_clipped", files, params, norm, list(self._clip_choice(clip)),
                                            weights, scale_down_width, return_stats,
                                            [(return_counts, self._out_plane(np.int32, True)),
                                             (return_kept_weight, self._out_plane(np.float32, True))], return_norm, return_applied)

    # -- per-pixel weight maps and local-sharpness stacking (extension beyond the reference) --------------
    def local_sharpness(self, files, local: Optional["LocalParameters"] = None):
        """The local quality map of every frame of an 8-bit stack (stk_local_sharpness): n x H x W float32, exact integers,
        placed where the frames live (a numpy array for host frames, a tensor for device frames)."""
        m = self._stack(files)
        maps, ptrs = self._plane_table(m, (m.h, m.w), np.float32)
        lp = (local or LocalParameters())._c()
        self._check(self._lib.stk_local_sharpness(self._h, C.byref(m.c_frames), C.byref(lp), ptrs))
        return maps

    # -- star registration (extension beyond the reference) ------------------------------------------------
    def _star_detect(self, fn, m, params, extra, return_peaks):
        """stk_star_detect / stk_star_detect_deep: `extra` = the arguments between the params and the outputs"""
        p = (params or StarParameters())._c()
        cap = max(int(p.max_stars), 1)
        stars = np.zeros((m.n, cap), STAR_DTYPE)
        n_stars = np.zeros(m.n, np.int32)
        n_peaks = np.zeros(m.n, np.int32)
        self._check(fn(self._h, C.byref(m.c_frames), C.byref(p), *extra, C.c_void_p(stars.ctypes.data),
                       C.c_void_p(n_stars.ctypes.data), C.c_void_p(n_peaks.ctypes.data)))
        lists = [stars[i, :n_stars[i]].copy() for i in range(m.n)]
        return (lists, n_peaks) if return_peaks else lists

    def _star_align(self, fn, m, params, extra):
        p = (params or StarParameters())._c()
        stats = (_ffi.FrameStats * m.n)()
        dropped = C.c_int32(0)
        self._check(fn(self._h, C.byref(m.c_frames), C.byref(p), *extra, C.byref(dropped), stats))
        return dropped.value, self._stats_list(stats, m.n)

    def _star_match(self, fn, m, params, extra, return_stats):
        p = (params or StarParameters())._c()
        out, img = self._image(m)
        stats = (_ffi.FrameStats * m.n)()
        dropped = C.c_int32(0)
        self._check(fn(self._h, C.byref(m.c_frames), C.byref(p), *extra, C.byref(img), C.byref(dropped), stats))
        return (dropped.value, out, self._stats_list(stats, m.n)) if return_stats else (dropped.value, out)

    def star_detect(self, files, params: Optional["StarParameters"] = None, return_peaks: bool = False):
        """The stars of every frame of an 8-bit stack (stk_star_detect), brightest first: a list of n STAR_DTYPE arrays;
        return_peaks adds the n peak counts before truncation."""
        return self._star_detect(self._lib.stk_star_detect, self._stack(files), params, (), return_peaks)

    star_match_lists = staticmethod(star_match_lists)

    def star_align(self, files, params: Optional["StarParameters"] = None):
        """Star registration without the fold (stk_star_align): (dropped, stats). The stats' warps feed any *_stack combine
        with include = [s["status"] == 0 for s in stats] and is_affine = False."""
        return self._star_align(self._lib.stk_star_align, self._stack(files), params, ())

    def star_match(self, files, params: Optional["StarParameters"] = None, return_stats: bool = False):
        """Star registration and the plain mean over frame 0 and the kept frames (stk_star_match): (dropped, image[, stats])."""
        return self._star_match(self._lib.stk_star_match, self._stack(files), params, (), return_stats)

    # -- star registration on 8-bit, 16-bit and f32 frames (stk_star_deep_params) ---------------------------
    def star_detect_deep(self, files, params: Optional["StarParameters"] = None, deep: Optional["StarDeepParameters"] = None,
                         return_peaks: bool = False):
        """star_detect on the 16-bit key of a u8, u16 or f32 stack (stk_star_detect_deep); params.min_contrast is in key
        units, 1 .. 65535."""
        dp = (deep or StarDeepParameters())._c()
        return self._star_detect(self._lib.stk_star_detect_deep, self._stack(files), params, (C.byref(dp),), return_peaks)

    def star_align_deep(self, files, params: Optional["StarParameters"] = None, deep: Optional["StarDeepParameters"] = None):
        """star_align on the key (stk_star_align_deep): (dropped, stats); the stats feed any *_stack combine of the frames."""
        dp = (deep or StarDeepParameters())._c()
        return self._star_align(self._lib.stk_star_align_deep, self._stack(files), params, (C.byref(dp),))

    def star_match_deep(self, files, params: Optional["StarParameters"] = None, deep: Optional["StarDeepParameters"] = None,
                        alpha: Optional[float] = None, return_stats: bool = False):
        """star_align_deep and the plain mean of frame 0 and the kept frames at their own depth (stk_star_match_deep):
        (dropped, image[, stats]). alpha: the fold's scale, by default 1 / 255, 1 / 65535 or 1 / f32_scale by depth."""
        m = self._stack(files)
        deep = deep or StarDeepParameters()
        if alpha is None:
            alpha = {8: 1.0 / 255.0, 16: 1.0 / 65535.0}.get(m.depth, 1.0 / float(deep.f32_scale) if deep.f32_scale else float("nan"))
        dp = deep._c()
        return self._star_match(self._lib.stk_star_match_deep, m, params, (C.byref(dp), C.c_double(float(alpha))), return_stats)

    # -- star shapes, frame quality and quality weights (stk_star_measure_params) -----------------------------
    def star_measure(self, files, stars, measure: Optional["StarMeasureParameters"] = None, deep: Optional["StarDeepParameters"] = None):
        """The shape of every star of every frame (stk_star_measure): a list of n SHAPE_DTYPE arrays, one entry per entry of
        `stars`, the lists star_detect / star_detect_deep returned for the same frames (only px and py are read).
        star_frame_quality, star_quality_scores and star_quality_weights turn them into frame quality, scores for rank_frames
        and weights for any *_stack combine."""
        m = self._stack(files)
        lists = [np.asarray(s, STAR_DTYPE).reshape(-1) for s in stars]
        if len(lists) != m.n:
            raise InvalidParams("one star list per frame expected")
        cap = max([len(s) for s in lists] + [1])
        tab = np.zeros((m.n, cap), STAR_DTYPE)
        for i, s in enumerate(lists):
            tab[i, :len(s)] = s
        counts = np.array([len(s) for s in lists], np.int32)
        shapes = np.zeros((m.n, cap), SHAPE_DTYPE)
        dp, mp = (deep or StarDeepParameters())._c(), (measure or StarMeasureParameters())._c()
        self._check(self._lib.stk_star_measure(self._h, C.byref(m.c_frames), C.byref(dp), C.byref(mp), C.c_void_p(tab.ctypes.data),
                                               C.c_void_p(counts.ctypes.data), cap, shapes.ctypes.data_as(C.POINTER(_ffi.StarShape))))
        return [shapes[i, :counts[i]].copy() for i in range(m.n)]

    def star_match_quality_weighted(self, files, params: Optional["StarParameters"] = None, deep: Optional["StarDeepParameters"] = None,
                                    measure: Optional["StarMeasureParameters"] = None, quality: Optional["StarQualityParameters"] = None,
                                    alpha: Optional[float] = None, coverage: bool = True, weights=None, return_coverage: bool = False,
                                    return_applied: bool = False, return_quality: bool = False, return_stats: bool = False):
        """star_align_deep, the shapes of every frame's stars, their quality weights and one weighted fold
        (stk_star_match_quality_weighted): (dropped, rejected, image[, coverage][, applied][, quality][, stats]). dropped:
        the frames the alignment dropped; rejected: the aligned frames the quality limits rejected; both have weight 0 in
        `applied`. alpha as in star_match_deep."""
        m = self._stack(files)
        deep = deep or StarDeepParameters()
        if alpha is None:
            alpha = {8: 1.0 / 255.0, 16: 1.0 / 65535.0}.get(m.depth, 1.0 / float(deep.f32_scale) if deep.f32_scale else float("nan"))
        p, dp = (params or StarParameters())._c(), deep._c()
        mp, qp = (measure or StarMeasureParameters())._c(), (quality or StarQualityParameters())._c()
        u = self._weights_arg(weights, m.n)
        out, img = self._image(m)
        cov, cptr = self._optional(m, return_coverage, np.float32)
        dropped, rejected = C.c_int32(0), C.c_int32(0)
        applied, stats = (_ffi.FrameWeight * m.n)(), (_ffi.FrameStats * m.n)()
        q = np.zeros(m.n, QUALITY_DTYPE)
        self._check(self._lib.stk_star_match_quality_weighted(
            self._h, C.byref(m.c_frames), C.byref(p), C.byref(dp), C.byref(mp), C.byref(qp), C.c_double(float(alpha)), int(coverage),
            None if u is None else C.c_void_p(u.ctypes.data), C.byref(img), cptr, C.byref(dropped), C.byref(rejected), applied, stats,
            q.ctypes.data_as(C.POINTER(_ffi.StarQuality))))
        res = (dropped.value, rejected.value, out)
        res += ((cov,) if return_coverage else ()) + ((self._applied_list(applied, m.n, m.c),) if return_applied else ())
        return res + ((q,) if return_quality else ()) + ((self._stats_list(stats, m.n),) if return_stats else ())

    # -- frame calibration (extension beyond the reference) -------------------------------------------------
    def _image_arg(self, x, keep, what: str = "image"):
        """An H x W x C (or H x W) float32 image the caller holds, host or device, contiguous or a row-strided view, as an
        stk_image_f32; the owner is appended to `keep`."""
        if _is_torch(x):
            if str(x.dtype) != "torch.float32" or x.dim() not in (2, 3):
                raise InvalidParams(f"{what}: an H x W x C float32 image expected")
            if not x.is_cuda:
                x = x.numpy()
        if not _is_torch(x):
            x = np.asarray(x)
            if x.dtype != np.float32 or x.ndim not in (2, 3):
                raise InvalidParams(f"{what}: an H x W x C float32 image expected")
        try:
            rs = _image_stride_bytes(x)
        except InvalidParams:
            x = x.contiguous() if _is_torch(x) else np.ascontiguousarray(x)
            rs = 0
        if _is_torch(x):
            self._tensor_ready(x)                 # behind the copy above, if there was one
        keep.append(x)
        h, w = int(x.shape[0]), int(x.shape[1])
        c = int(x.shape[2]) if len(x.shape) == 3 else 1
        if _is_torch(x):
            return _ffi.ImageF32(x.data_ptr(), w, h, c, DEVICE, rs)
        return _ffi.ImageF32(x.ctypes.data, w, h, c, HOST, rs)

    def _bytes_arg(self, x, keep, h, w, what: str):
        """An H x W uint8 plane, host or device, tightly packed: (pointer, location)."""
        if _is_torch(x) and x.is_cuda:
            if str(x.dtype) != "torch.uint8" or tuple(x.shape) != (h, w):
                raise InvalidParams(f"{what}: an H x W uint8 plane expected")
            x = x.contiguous()
            self._tensor_ready(x)
            keep.append(x)
            return x.data_ptr(), DEVICE
        a = np.ascontiguousarray(x.numpy() if _is_torch(x) else x)
        if a.dtype != np.uint8 or a.shape != (h, w):
            raise InvalidParams(f"{what}: an H x W uint8 plane expected")
        keep.append(a)
        return a.ctypes.data, HOST

    # -- the background model (include/stacker.h, stk_background_params) -------------------------
    def _mask_arg(self, mask, keep, m):
        if mask is None:
            return None, HOST
        ptr, loc = self._bytes_arg(mask, keep, m.h, m.w, "mask")
        return C.c_void_p(ptr), loc

    def background_cells(self, files, params: Optional["BackgroundParameters"] = None, mask=None):
        """The window records of every frame of a stack in one device pass (stk_background_cells): an
        n x gh x gw x min(C, 3) BG_CELL_DTYPE array. `mask`: an H x W uint8 plane, host or device; non-zero excludes the pixel."""
        m = self._stack(files)
        p = (params or BackgroundParameters())._c(m.depth)
        keep = []
        mptr, mloc = self._mask_arg(mask, keep, m)
        gw, gh = mesh_grid(m.w, m.h, int(p.step))
        cells = np.zeros((m.n, gh, gw, min(m.c, 3)), BG_CELL_DTYPE)
        self._check(self._lib.stk_background_cells(self._h, C.byref(m.c_frames), C.byref(p), mptr, mloc,
                                                   cells.ctypes.data_as(C.POINTER(_ffi.BgCell))))
        return cells

    def _level_planes_arg(self, planes, m, step, keep):
        """n host level planes (None entries allowed) as the pointer table the C ABI takes."""
        gw, gh = mesh_grid(m.w, m.h, int(step))
        if planes is None:
            return None
        planes = list(planes)
        if len(planes) != m.n:
            raise InvalidParams("one level plane (or None) per frame expected")
        ptrs = []
        for pl in planes:
            if pl is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(np.asarray(pl, np.float32))
            if a.size != gh * gw * min(m.c, 3):
                raise InvalidParams("a level plane must be gh x gw x min(C, 3) float32")
            keep.append(a)
            ptrs.append(a.ctypes.data)
        arr = (C.c_void_p * m.n)(*ptrs)
        keep.append(arr)
        return C.cast(arr, C.c_void_p)

    def background_apply(self, files, planes, step: int, target=(0.0, 0.0, 0.0, 0.0), out_depth: Optional[int] = None, out=None):
        """Subtract the interpolated level planes from a stack (stk_background_apply): ((float)raw - B) + target per colour
        channel, alpha untouched. planes: n host planes gh x gw x min(C, 3) for the grid of `step`, None entries = 0. Returns
        the flattened stack where the frames live (see calibrate for `out`)."""
        m = self._stack(files)
        keep = []
        tbl = self._level_planes_arg(planes, m, step, keep)
        tgt = BackgroundParameters(target=target)._target()
        depth = int(m.depth if out_depth is None else out_depth)
        res, arr, stride = self._frame_outputs(m, depth, out, keep)
        self._check(self._lib.stk_background_apply(self._h, C.byref(m.c_frames), tbl, int(step), C.cast(tgt, C.c_void_p), depth,
                                                   C.cast(arr, C.c_void_p), stride))
        return res

    def background_flatten(self, files, params: Optional["BackgroundParameters"] = None, mask=None, out=None, return_planes: bool = False,
                           return_rms: bool = False, return_cells: bool = False):
        """Model and remove the background of every frame (stk_background_flatten = background_cells, background_estimate
        per frame and background_apply with params.target, bit for bit). Returns the flattened stack where the frames live,
        then the level planes (return_planes: n x gh x gw x min(C, 3) float32), the rms planes (return_rms) and the window
        records (return_cells)."""
        m = self._stack(files)
        p = (params or BackgroundParameters())._c(m.depth)
        keep = []
        mptr, mloc = self._mask_arg(mask, keep, m)
        gw, gh = mesh_grid(m.w, m.h, int(p.step))
        cc = min(m.c, 3)
        res, arr, stride = self._frame_outputs(m, int(p.out_depth), out, keep)

        def table(wanted):
            if not wanted:
                return None, None
            a = np.zeros((m.n, gh, gw, cc), np.float32)
            t = (C.c_void_p * m.n)(*[a.ctypes.data + i * gh * gw * cc * 4 for i in range(m.n)])
            keep.append(t)
            return a, C.cast(t, C.c_void_p)
        planes, pt = table(return_planes)
        rms, rt = table(return_rms)
        cells = np.zeros((m.n, gh, gw, cc), BG_CELL_DTYPE) if return_cells else None
        self._check(self._lib.stk_background_flatten(self._h, C.byref(m.c_frames), C.byref(p), mptr, mloc, C.cast(arr, C.c_void_p), stride, pt, rt,
                                                     None if cells is None else cells.ctypes.data_as(C.POINTER(_ffi.BgCell))))
        extra = tuple(x for x in (planes, rms, cells) if x is not None)
        return (res,) + extra if extra else res

    def flatten_image(self, image, params: Optional["BackgroundParameters"] = None, mask=None, return_plane: bool = False):
        """Flatten a finished stack: an H x W x C float32 image (array or device tensor) as a one-frame stack through
        background_flatten. Set params.f32_scale so that sample * f32_scale spans the 16-bit key range (65535 for a stack
        in [0, 1])."""
        if str(image.dtype).replace("torch.", "") != "float32" or len(image.shape) not in (2, 3):
            raise InvalidParams("flatten_image: an H x W x C float32 image expected")
        res = self.background_flatten([image], params, mask, return_planes=return_plane)
        return (res[0][0], res[1][0]) if return_plane else res[0]

    # -- deconvolution (include/stacker.h, stk_deconv_params) ------------------------------------
    def deconvolve_image(self, image, psf, params: Optional["DeconvolveParameters"] = None, mask=None, out=None):
        """Richardson-Lucy deconvolution of a finished stack (stk_deconvolve): an H x W (x C) float32 image, array or device
        tensor, C = 1, 3 or 4 (alpha is copied through), with `psf`, (2 R + 1)^2 float32 taps that sum to 1 (psf_model).
        params None: the defaults with the PSF's radius. `mask`: an H x W float32 plane, host or device; the result is blended
        with the input by amount * mask per pixel. Returns an H x W x C image where the input lives; `out`: the image to
        write instead, which may be the input itself."""
        taps = np.ascontiguousarray(np.asarray(psf.cpu().numpy() if _is_torch(psf) else psf, np.float32))
        side = int(round(taps.size ** 0.5))
        p = (params or DeconvolveParameters(radius=(side - 1) // 2))._c()
        if taps.size != (2 * int(p.radius) + 1) ** 2:
            raise InvalidParams("deconvolve_image: the PSF must have (2 radius + 1)^2 taps")
        keep = []
        img = self._image_arg(image, keep)
        mptr, mstride, mloc = None, 0, HOST
        if mask is not None:
            mk = self._image_arg(mask, keep, "mask")
            if (mk.width, mk.height, mk.channels) != (img.width, img.height, 1):
                raise InvalidParams("mask: an H x W float32 plane expected")
            mptr, mstride, mloc = C.c_void_p(mk.data), mk.row_stride_bytes, mk.location
        if out is None:
            res, addr = self._alloc(keep[0].device if img.location == DEVICE else None, (img.height, img.width, img.channels), np.float32)
            o = _ffi.ImageF32(addr, img.width, img.height, img.channels, img.location, 0)
        else:
            res = out
            if _is_torch(out) and not out.is_cuda:
                out = out.numpy()
            if str(out.dtype).replace("torch.", "") != "float32" or len(out.shape) not in (2, 3):
                raise InvalidParams("out: an H x W x C float32 image expected")
            rs = _image_stride_bytes(out)
            if _is_torch(out):
                self._tensor_ready(out)
            keep.append(out)
            o = _ffi.ImageF32(out.data_ptr() if _is_torch(out) else out.ctypes.data, int(out.shape[1]), int(out.shape[0]),
                              int(out.shape[2]) if len(out.shape) == 3 else 1, DEVICE if _is_torch(out) else HOST, rs)
        self._check(self._lib.stk_deconvolve(self._h, C.byref(img), C.c_void_p(taps.ctypes.data), C.byref(p), mptr, mstride, mloc, C.byref(o)))
        return res

    def psf_from_image(self, image, radius: int, deep: Optional["StarDeepParameters"] = None, measure: Optional["StarMeasureParameters"] = None,
                       star: Optional["StarParameters"] = None, kind: int = PSF_GAUSSIAN, beta: float = 2.5, min_snr: float = 0.0,
                       scale: float = 1.0, return_covariance: bool = False):
        """The PSF of a finished stack from its own stars: star_detect_deep and star_measure on the image as a one-frame f32
        stack, then psf_from_shapes and psf_model. Set deep.f32_scale so that sample * f32_scale spans the 16-bit key range.
        Returns the (2 radius + 1)^2 float32 PSF; return_covariance adds (cxx, cyy, cxy, stars used)."""
        if str(image.dtype).replace("torch.", "") != "float32" or len(image.shape) not in (2, 3):
            raise InvalidParams("psf_from_image: an H x W x C float32 image expected")
        stars = self.star_detect_deep([image], star, deep)
        shapes = self.star_measure([image], stars, measure, deep)
        cxx, cyy, cxy, used = psf_from_shapes(shapes[0], min_snr, scale, return_used=True)
        psf = psf_model(radius, cxx, cyy, cxy, kind, beta)
        return (psf, (cxx, cyy, cxy, used)) if return_covariance else psf

    # -- wavelet layers (include/stacker.h, stk_wavelet_params) ---------------------------------
    def _image_out(self, out, keep):
        """An H x W x C float32 image the caller holds, to be written: its stk_image_f32."""
        if _is_torch(out) and not out.is_cuda:
            out = out.numpy()
        if str(out.dtype).replace("torch.", "") != "float32" or len(out.shape) not in (2, 3):
            raise InvalidParams("out: an H x W x C float32 image expected")
        rs = _image_stride_bytes(out)
        if _is_torch(out):
            self._tensor_ready(out)
        keep.append(out)
        return _ffi.ImageF32(out.data_ptr() if _is_torch(out) else out.ctypes.data, int(out.shape[1]), int(out.shape[0]),
                             int(out.shape[2]) if len(out.shape) == 3 else 1, DEVICE if _is_torch(out) else HOST, rs)

    def wavelet_image(self, image, params: Optional["WaveletParameters"] = None, mask=None, out=None, return_sigma: bool = False):
        """Multiscale denoising and sharpening of a finished stack (stk_wavelet_process): an H x W (x C) float32 image, array or
        device tensor, C = 1, 3 or 4 (alpha is copied through). `mask`: an H x W float32 plane, host or device; the result is
        blended with the input by amount * mask per pixel. Returns an H x W x C image where the input lives; `out`: the image
        to write instead, which may be the input itself. return_sigma adds the noise of each colour channel as used (given,
        estimated, or 0 where no threshold asked for it; asking estimates it), a float32 array of min(C, 3) values."""
        p = (params or WaveletParameters())._c()
        keep = []
        img = self._image_arg(image, keep)
        mptr, mstride, mloc = None, 0, HOST
        if mask is not None:
            mk = self._image_arg(mask, keep, "mask")
            if (mk.width, mk.height, mk.channels) != (img.width, img.height, 1):
                raise InvalidParams("mask: an H x W float32 plane expected")
            mptr, mstride, mloc = C.c_void_p(mk.data), mk.row_stride_bytes, mk.location
        if out is None:
            res, addr = self._alloc(keep[0].device if img.location == DEVICE else None, (img.height, img.width, img.channels), np.float32)
            o = _ffi.ImageF32(addr, img.width, img.height, img.channels, img.location, 0)
        else:
            res, o = out, self._image_out(out, keep)
        sigma = np.zeros(4, np.float32)
        self._check(self._lib.stk_wavelet_process(self._h, C.byref(img), C.byref(p), mptr, mstride, mloc, C.byref(o),
                                                  C.c_void_p(sigma.ctypes.data) if return_sigma else None))
        return (res, sigma[:min(img.channels, 3)].copy()) if return_sigma else res

    def wavelet_layers(self, image, levels: int = 4):
        """The wavelet layers of an image (stk_wavelet_layers): a list of levels + 1 H x W x C float32 images where the input
        lives, w_0 .. w_{levels-1} and the residual c_levels; bit for bit what wavelet_image works on. Their sum is the
        sanitised input to within rounding. With 4 channels every image's alpha is the input's."""
        n = int(levels)
        if not 1 <= n <= 8:
            raise InvalidParams("wavelet_layers: levels must be 1 .. 8")
        keep = []
        img = self._image_arg(image, keep)
        outs, arr = [], (_ffi.ImageF32 * (n + 1))()
        for k in range(n + 1):
            res, addr = self._alloc(keep[0].device if img.location == DEVICE else None, (img.height, img.width, img.channels), np.float32)
            outs.append(res)
            arr[k] = _ffi.ImageF32(addr, img.width, img.height, img.channels, img.location, 0)
        self._check(self._lib.stk_wavelet_layers(self._h, C.byref(img), n, C.cast(arr, C.POINTER(_ffi.ImageF32))))
        return outs

    def wavelet_sigma(self, image, return_median: bool = False):
        """The noise of a finished f32 stack (stk_wavelet_sigma): per colour channel 1.4826 / e_0 times the exact lower median
        of the first wavelet layer's magnitudes; a float32 array of min(C, 3) values. return_median adds those medians."""
        keep = []
        img = self._image_arg(image, keep)
        sigma, med = np.zeros(4, np.float32), np.zeros(4, np.float32)
        self._check(self._lib.stk_wavelet_sigma(self._h, C.byref(img), C.c_void_p(sigma.ctypes.data), C.c_void_p(med.ctypes.data) if return_median else None))
        cc = min(img.channels, 3)
        return (sigma[:cc].copy(), med[:cc].copy()) if return_median else sigma[:cc].copy()

    # -- display stretch (include/stacker.h, "display stretch") ------------------------------------
    def _image_mask_arg(self, mask, img, keep):
        """An optional H x W float32 mask plane of an image: (pointer, row stride in bytes, location)."""
        if mask is None:
            return None, 0, HOST
        mk = self._image_arg(mask, keep, "mask")
        if (mk.width, mk.height, mk.channels) != (img.width, img.height, 1):
            raise InvalidParams("mask: an H x W float32 plane expected")
        return C.c_void_p(mk.data), mk.row_stride_bytes, mk.location

    def _stretch_out(self, img, depth, out, keep):
        """The image a stretch writes: a fresh H x W x C array or tensor of `depth` where the input lives, or the caller's `out`
        (contiguous, or a view whose only non-contiguity is its row step): (result, stk_image_out)."""
        if depth not in _DEPTH_DTYPE:
            raise InvalidParams("out_depth: DEPTH_U8, DEPTH_U16 or DEPTH_F32")
        if out is None:
            res, addr = self._alloc(keep[0].device if img.location == DEVICE else None, (img.height, img.width, img.channels), _DEPTH_DTYPE[depth])
            return res, _ffi.ImageOut(addr, img.width, img.height, img.channels, depth, img.location, 0)
        o = out.numpy() if _is_torch(out) and not out.is_cuda else out
        if str(o.dtype).replace("torch.", "") != np.dtype(_DEPTH_DTYPE[depth]).name or len(o.shape) not in (2, 3):
            raise InvalidParams("out: an H x W x C image of the output depth expected")
        el = depth // 8
        if (o.is_contiguous() if _is_torch(o) else o.flags.c_contiguous):
            rs = 0
        else:
            rs = _row_stride_bytes(tuple(o.shape), [s * el for s in o.stride()] if _is_torch(o) else o.strides, el)
            if not rs:
                raise InvalidParams("out: contiguous, or a view whose only non-contiguity is its row step")
        if _is_torch(o):
            self._tensor_ready(o)
        keep.append(o)
        return out, _ffi.ImageOut(o.data_ptr() if _is_torch(o) else o.ctypes.data, int(o.shape[1]), int(o.shape[0]),
                                  int(o.shape[2]) if len(o.shape) == 3 else 1, depth, DEVICE if _is_torch(o) else HOST, rs)

    @staticmethod
    def _table_arg(curve, table, keep):
        if int(curve) != STRETCH_TABLE:
            return None, 0
        if table is None:
            raise InvalidParams("table: STRETCH_TABLE needs a table (stretch_table)")
        t = np.ascontiguousarray(np.asarray(table, np.float32).reshape(-1))
        if not 3 <= t.size <= 65537:
            raise InvalidParams("table: 3 .. 65537 values (knots + 1)")
        keep.append(t)
        return C.c_void_p(t.ctypes.data), t.size - 1

    def image_stats(self, image, mask=None, quantiles=()):
        """Exact statistics of a float32 image per colour channel (stk_image_stats): an H x W (x C) array or device tensor, C =
        1, 3 or 4 (alpha is not measured). Counted are the finite samples, under a `mask` (H x W float32, host or device)
        those where it is > 0. Returns min(C, 3) records of STAT_DTYPE: count, min, max, the lower median, the MAD about it
        and `q`: the k-th smallest for each of up to four `quantiles` in 0 .. 1."""
        qs = np.ascontiguousarray(np.asarray(quantiles, np.float64).reshape(-1))
        if qs.size > 4:
            raise InvalidParams("quantiles: at most 4")
        keep = []
        img = self._image_arg(image, keep)
        mptr, mstride, mloc = self._image_mask_arg(mask, img, keep)
        stats = np.zeros(4, STAT_DTYPE)
        self._check(self._lib.stk_image_stats(self._h, C.byref(img), mptr, mstride, mloc, qs.ctypes.data_as(C.POINTER(C.c_double)) if qs.size else None,
                                              int(qs.size), stats.ctypes.data_as(C.POINTER(_ffi.ImageStat))))
        return stats[:min(img.channels, 3)].copy()

    def stretch_image(self, image, params: Optional["StretchParameters"] = None, out=None):
        """The display stretch of a float32 image (stk_stretch): black and white point, curve and conversion to
        params.out_depth in one launch. Returns an H x W x C image of that depth where the input lives; `out`: the image to
        write instead, which for float32 output may be the input itself."""
        sp = params or StretchParameters()
        p = sp._c()
        keep = []
        img = self._image_arg(image, keep)
        tptr, knots = self._table_arg(sp.curve, sp.table, keep)
        res, o = self._stretch_out(img, int(sp.out_depth), out, keep)
        self._check(self._lib.stk_stretch(self._h, C.byref(img), C.byref(p), tptr, knots, C.byref(o)))
        return res

    def auto_stretch_image(self, image, auto: Optional["AutoStretchParameters"] = None, curve: int = STRETCH_MTF, colour: int = 0,
                           out_depth: int = DEPTH_F32, out_scale: float = 1.0, table=None, mask=None, out=None, return_stats: bool = False,
                           return_params: bool = False):
        """Statistics, the auto rule and the stretch in one call (stk_auto_stretch): bit for bit image_stats (under `mask`),
        stretch_auto and stretch_image with the rule's black, white and midtone and this call's curve, colour, out_depth and
        out_scale. return_stats adds the records, return_params the StretchParameters as used."""
        ap = (auto or AutoStretchParameters())._c()
        keep = []
        img = self._image_arg(image, keep)
        mptr, mstride, mloc = self._image_mask_arg(mask, img, keep)
        tptr, knots = self._table_arg(curve, table, keep)
        res, o = self._stretch_out(img, int(out_depth), out, keep)
        stats, used = np.zeros(4, STAT_DTYPE), _ffi.StretchParams()
        self._check(self._lib.stk_auto_stretch(self._h, C.byref(img), mptr, mstride, mloc, C.byref(ap), int(curve), int(colour), float(out_scale), tptr, knots,
                                               C.byref(o), stats.ctypes.data_as(C.POINTER(_ffi.ImageStat)) if return_stats else None,
                                               C.byref(used) if return_params else None))
        ret = (res,)
        if return_stats:
            ret += (stats[:min(img.channels, 3)].copy(),)
        if return_params:
            ret += (StretchParameters._from_c(used, table),)
        return ret[0] if len(ret) == 1 else ret

    def _frame_outputs(self, m, out_depth: int, out, keep):
        """The per-frame outputs of a call that writes one image per frame (stk_calibrate, the background calls): a fresh
        n x H x W x C array or tensor of `out_depth` where the frames live, or the caller's `out` (n images in the frames'
        location; row-strided views allowed, all with one row step). Returns (result, the pointer array, the row stride)."""
        dt = {8: "uint8", 16: "uint16", 32: "float32"}.get(out_depth)
        stride = 0
        if out is None:
            if dt is None:
                raise InvalidParams("out_depth must be 8, 16 or 32")
            res, base = self._alloc(m, (m.n, m.h, m.w, m.c), dt)
            ptrs = [base + i * m.h * m.w * m.c * (out_depth // 8) for i in range(m.n)]
        else:
            res = out
            outs = list(out)
            if len(outs) != m.n:
                raise InvalidParams("one output per frame expected")
            ptrs, strides = [], set()
            el = out_depth // 8
            for o in outs:
                dev = _is_torch(o) and o.is_cuda
                if dev != (m.location == DEVICE):
                    raise InvalidParams("the outputs must live where the frames live")
                name = str(o.dtype).replace("torch.", "")
                shape = tuple(int(v) for v in o.shape)
                if name != dt or shape not in ((m.h, m.w, m.c),) + (((m.h, m.w),) if m.c == 1 else ()):
                    raise InvalidParams("every output must be H x W x C of the output depth")
                if not dev and _is_torch(o):
                    o = o.numpy()
                if dev:
                    self._tensor_ready(o)
                    rs = m.w * m.c * el if o.is_contiguous() else _row_stride_bytes(shape, [s * el for s in o.stride()], el)
                    ptrs.append(o.data_ptr())
                else:
                    rs = m.w * m.c * el if o.flags.c_contiguous else _row_stride_bytes(shape, o.strides, el)
                    ptrs.append(o.ctypes.data)
                if not rs:
                    raise InvalidParams("an output must be contiguous or a view whose only non-contiguity is its row step")
                strides.add(rs)
                keep.append(o)
            if len(strides) != 1:
                raise InvalidParams("all outputs must share one row step")
            stride = strides.pop()
        return res, (C.c_void_p * m.n)(*ptrs), stride

    def calibrate(self, files, cal: "CalibrationParameters", out=None):
        """Apply masters and defect repair to every frame of a stack (stk_calibrate). Returns the calibrated stack where
        the frames live: an n x H x W x C array or tensor of the frames' dtype (or float32, cal.out_depth = 32). `out`: n
        images the caller holds instead (same location as the frames; row-strided views allowed, all with one row step);
        only their pixel bytes are written, and they must not overlap the frames or the masters."""
        m = self._stack(files)
        keep = []
        c = _ffi.Calibration()
        for name in ("bias", "dark", "flat"):
            x = getattr(cal, name)
            if x is not None:
                setattr(c, name + "_or_null", C.pointer(self._image_arg(x, keep, name + " master")))
        if cal.dark_scale is not None:
            ds = np.ascontiguousarray(np.asarray(cal.dark_scale, np.float32).reshape(-1))
            if ds.size != m.n:
                raise InvalidParams("one dark_scale per frame expected")
            keep.append(ds)
            c.dark_scale_or_null = ds.ctypes.data
        fm = cal.flat_mean
        if cal.flat is not None and fm is None:
            fm = self.image_mean(cal.flat)
        fm = [1.0] * 4 if fm is None else (list(np.asarray(fm, np.float64).reshape(-1)) + [1.0] * 4)[:4]
        for k in range(4):
            c.flat_mean[k] = float(fm[k])
        c.flat_min = float(cal.flat_min) if cal.flat_min is not None else 1e-3 * float(min(fm[:min(m.c, 3)]))
        c.pedestal = float(cal.pedestal)
        if cal.defects is not None:
            c.defects_or_null, c.defects_location = self._bytes_arg(cal.defects, keep, m.h, m.w, "defects")
        c.defect_step = int(cal.defect_step)
        c.out_depth = int(m.depth if cal.out_depth is None else cal.out_depth)
        res, arr, stride = self._frame_outputs(m, c.out_depth, out, keep)
        self._check(self._lib.stk_calibrate(self._h, C.byref(m.c_frames), C.byref(c), C.cast(arr, C.c_void_p), stride))
        return res

    def defect_map(self, master, params: Optional["DefectParameters"] = None, map=None, return_counts: bool = False):
        """The defect map of a master (stk_defect_map): H x W uint8, bit c = channel c is hot / dead / not finite, placed
        where the master lives. `map`: the map to write (params.accumulate: to OR into). return_counts adds the set bits
        per channel after the call."""
        keep = []
        img = self._image_arg(master, keep, "master")
        p = (params or DefectParameters())._c()
        if map is None:
            if p.accumulate:
                raise InvalidParams("accumulate needs the map to accumulate into")
            map = self._alloc(keep[0].device if img.location == DEVICE else None, (img.height, img.width), np.uint8)[0]
        if _is_torch(map) and not map.is_cuda:
            map = map.numpy()
        if (_is_torch(map) and not map.is_contiguous()) or (not _is_torch(map) and not (isinstance(map, np.ndarray) and map.flags.c_contiguous)):
            raise InvalidParams("the map must be a contiguous H x W uint8 plane")
        ptr, loc = self._bytes_arg(map, keep, img.height, img.width, "map")
        counts = np.zeros(4, np.int64)
        self._check(self._lib.stk_defect_map(self._h, C.byref(img), C.byref(p), C.c_void_p(ptr), loc, C.c_void_p(counts.ctypes.data)))
        return (map, counts) if return_counts else map

    @staticmethod
    def defect_weights(map):
        """A defect map as the weight plane stk_drizzle_stack takes through `maps`: float32, 1 where the byte is 0."""
        if _is_torch(map):
            import torch
            return (map == 0).to(torch.float32)
        return (np.asarray(map) == 0).astype(np.float32)

    def image_mean(self, image):
        """Per-channel means of a float32 image (stk_image_mean): `channels` float64 values, the same bits on every call."""
        keep = []
        img = self._image_arg(image, keep)
        mean = np.zeros(4, np.float64)
        self._check(self._lib.stk_image_mean(self._h, C.byref(img), C.c_void_p(mean.ctypes.data)))
        return mean[:img.channels].copy()

    def master_stack(self, files, normalize: int = 0, clip: Optional["RobustClipParameters"] = None, *, stat_step: int = 4,
                     return_counts: bool = False):
        """A master from a stack of calibration frames (stk_master_stack): the median / MAD clip over all frames under
        identity warps in raw sample units; normalize = 2 (flats) brings every frame to frame 0's level first. clip None:
        kappa 3 / 3, sigma_floor 0.5 (half a step of integer frames), 2 iterations."""
        m = self._stack(files)
        cp = (clip or RobustClipParameters(3.0, 3.0, 0.5, 2))._c()
        out, img = self._image(m)
        cnt, cptr = self._optional(m, return_counts, np.int32, True)
        self._check(self._lib.stk_master_stack(self._h, C.byref(m.c_frames), int(normalize), int(stat_step), C.byref(cp), C.byref(img), cptr))
        return (out, cnt) if return_counts else out

    def master_dark(self, darks, bias=None, clip: Optional["RobustClipParameters"] = None):
        """The master dark (or, without `bias`, the master bias of a stack of bias frames): the frames minus the master
        bias as float32, then master_stack(normalize = 0)."""
        return self.master_stack(self.calibrate(darks, CalibrationParameters(bias=bias, out_depth=32)), 0, clip)

    def master_flat(self, flats, bias=None, dark=None, dark_scale=None, clip: Optional["RobustClipParameters"] = None, *,
                    stat_step: int = 4):
        """The master flat: the frames minus bias and scaled dark as float32, then master_stack(normalize = 2)."""
        cal = self.calibrate(flats, CalibrationParameters(bias=bias, dark=dark, dark_scale=dark_scale, out_depth=32))
        return self.master_stack(cal, 2, clip, stat_step=stat_step)

    # -- colour-filter mosaics (extension beyond the reference) ------------------------------------------------
    def demosaic(self, files, pattern: int, method: int = DEMOSAIC_MHC, out_depth: Optional[int] = None, out=None):
        """A stack of single-channel Bayer mosaics (H x W or H x W x 1; host arrays or device tensors; padded row views as
        calibrate takes them) as B G R frames (stk_demosaic). pattern: CFA_*; method: DEMOSAIC_*. Returns n x H x W x 3
        (DEMOSAIC_SUPERPIXEL: n x H/2 x W/2 x 3) of the mosaics' dtype (or float32, out_depth = 32) where the mosaics live.
        `out`: n images the caller holds instead, by calibrate's rules (same location, row-strided views allowed, all with one
        row step); only their pixel bytes are written, and they must not overlap the mosaics."""
        m = self._stack(files)
        if m.c != 1:
            raise InvalidParams("demosaic takes single-channel mosaics (H x W or H x W x 1)")
        od = int(m.depth if out_depth is None else out_depth)
        dt = {8: "uint8", 16: "uint16", 32: "float32"}.get(od)
        if dt is None:
            raise InvalidParams("out_depth must be 8, 16 or 32")
        half = int(method) == DEMOSAIC_SUPERPIXEL
        oh, ow = (m.h // 2, m.w // 2) if half else (m.h, m.w)
        el = od // 8
        keep = []
        stride = 0
        if out is None:
            res, base = self._alloc(m, (m.n, oh, ow, 3), dt)
            ptrs = [base + i * oh * ow * 3 * el for i in range(m.n)]
        else:
            res = out
            outs = list(out)
            if len(outs) != m.n:
                raise InvalidParams("one output per mosaic expected")
            ptrs, strides = [], set()
            for o in outs:
                dev = _is_torch(o) and o.is_cuda
                if dev != (m.location == DEVICE):
                    raise InvalidParams("the outputs must live where the mosaics live")
                shape = tuple(int(v) for v in o.shape)
                if str(o.dtype).replace("torch.", "") != dt or shape != (oh, ow, 3):
                    raise InvalidParams("every output must be H x W x 3 of the output depth")
                if not dev and _is_torch(o):
                    o = o.numpy()
                if dev:
                    self._tensor_ready(o)
                    rs = ow * 3 * el if o.is_contiguous() else _row_stride_bytes(shape, [s * el for s in o.stride()], el)
                    ptrs.append(o.data_ptr())
                else:
                    rs = ow * 3 * el if o.flags.c_contiguous else _row_stride_bytes(shape, o.strides, el)
                    ptrs.append(o.ctypes.data)
                if not rs:
                    raise InvalidParams("an output must be contiguous or a view whose only non-contiguity is its row step")
                strides.add(rs)
                keep.append(o)
            if len(strides) != 1:
                raise InvalidParams("all outputs must share one row step")
            stride = strides.pop()
        f = m.c_frames
        mosaic = _ffi.Mosaic(f.data, m.n, m.w, m.h, m.depth, m.location, int(pattern), f.row_stride_bytes)
        arr = (C.c_void_p * m.n)(*ptrs)
        self._check(self._lib.stk_demosaic(self._h, C.byref(mosaic), int(method), od, C.cast(arr, C.c_void_p), stride))
        return res

    def cfa_mask(self, width: int, height: int, pattern: int, channel: int, device=False):
        """The H x W float32 plane that is 1 where the colour of a pattern's site is `channel` (0 = B, 1 = G, 2 = R) and 0
        elsewhere (stk_cfa_mask): what drizzle_stack, local_weighted_stack and reject_maps take through `maps`. device:
        False = a numpy array, True = a tensor on this context's device, or a torch device."""
        where = None
        if device is not False and device is not None:
            import torch
            where = torch.device("cuda", self.device) if device is True else torch.device(device)
        plane, addr = self._alloc(where, (int(height), int(width)), np.float32)
        self._check(self._lib.stk_cfa_mask(self._h, int(width), int(height), int(pattern), int(channel), C.c_void_p(addr),
                                           HOST if where is None else DEVICE))
        return plane

    def cfa_drizzle_stack(self, files, warps, pattern: int, drizzle: Optional["DrizzleParameters"] = None, **drizzle_kw):
        """Bayer drizzle: the single-channel mosaics drizzled once per colour with that colour's cfa_mask as every frame's
        map, so that no interpolated sample enters the result. By definition three drizzle_stack calls (drizzle_kw goes to
        each; `maps` and `return_den` are this call's own), stacked: returns (image, den), both oh x ow x 3 in B G R order;
        den shows the 1 : 2 : 1 coverage of the colours."""
        if "maps" in drizzle_kw or "return_den" in drizzle_kw:
            raise InvalidParams("cfa_drizzle_stack sets maps and return_den itself")
        files = files if hasattr(files, "shape") else list(files)
        m = self._stack(files)
        if m.c != 1:
            raise InvalidParams("cfa_drizzle_stack takes single-channel mosaics (H x W or H x W x 1)")
        images, dens = [], []
        for channel in range(3):
            mask = self.cfa_mask(m.w, m.h, pattern, channel, device=m.torch_device if m.location == DEVICE else False)
            img, den = self.drizzle_stack(files, warps, drizzle, maps=[mask] * m.n, return_den=True, **drizzle_kw)
            images.append(img.reshape(den.shape))
            dens.append(den)
        if _is_torch(dens[0]):
            import torch
            return torch.stack(images, -1), torch.stack(dens, -1)
        return np.stack(images, -1), np.stack(dens, -1)

    def local_weighted_stack(self, files, warps, maps, gain=None, offset=None, weights=None, include=None, *, applied=None,
                             floor: float = 1.0, power: int = 2, is_affine=False, border_mode=BORDER_CONSTANT,
                             border_value=(0, 0, 0, 0), alpha=1.0 / 255.0, return_coverage: bool = False):
        """The local-weighted fold alone over caller-held warps and caller-held per-pixel weight maps
        (stk_local_weighted_stack): weighted_stack with the weight of frame i at a pixel multiplied by (the bilinear sample
        of maps[i] there + floor) ** power. maps: n H x W float32 planes of non-negative weights (a quality map from
        local_sharpness, a mask, an inverse variance). return_coverage adds the summed weight den."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        rec = self._records_arg(m, gain, offset, weights, applied, optional=True)
        mkeep, mptrs = self._maps_arg(m, maps)
        out, img = self._image(m)
        cov, cptr = self._optional(m, return_coverage, np.float32)
        self._check(self._lib.stk_local_weighted_stack(*head, rec, C.cast(mptrs, C.c_void_p), float(floor), int(power), C.byref(img),
                                                       cptr))
        return (out, cov) if return_coverage else out

    def ecc_match_local_weighted(self, files, params: EccMatchParameters, local: Optional["LocalParameters"] = None,
                                 weight: Optional["WeightParameters"] = None, weights=None, scale_down_width: Optional[float] = None,
                                 return_stats: bool = False, return_coverage: bool = False, return_applied: bool = False):
        """ecc_match with the local-weighted fold (stk_ecc_match_local_weighted): every frame weighs in at a pixel by its
        local sharpness there. Arguments and results as ecc_match_weighted; weight.coverage must be True."""
        return self._match_weighted("ecc", "_local_weighted", files, params, weight, weights, local or LocalParameters(),
                                    scale_down_width, return_stats, return_coverage, return_applied)

    def keypoint_match_local_weighted(self, files, params: KeyPointMatchParameters, local: Optional["LocalParameters"] = None,
                                      weight: Optional["WeightParameters"] = None, weights=None,
                                      scale_down_width: Optional[float] = None, return_stats: bool = False,
                                      return_coverage: bool = False, return_applied: bool = False):
        """keypoint_match with the local-weighted fold (stk_keypoint_match_local_weighted): (dropped, image[, coverage]
        [, applied][, stats]). A dropped frame is no sample: weight 0 in `applied`."""
        return self._match_weighted("keypoint", "_local_weighted", files, params, weight, weights, local or LocalParameters(),
                                    scale_down_width, return_stats, return_coverage, return_applied)

    # -- local alignment: displacement fields on a node grid (extension beyond the reference) -----------
    def local_align(self, files, warps, mesh: Optional["MeshParameters"] = None, include=None, *, is_affine=False,
                    return_status: bool = False):
        """The displacement fields of an 8-bit stack over caller-held warps (stk_local_align): n x gh x gw x 2 float32
        (dx, dy), placed where the frames live; frame 0's and excluded frames' are zero. return_status adds the
        n x gh x gw int32 status planes (iterations run, or -1 .. -4; 0 for frames without a field)."""
        return self._local_align(files, warps, mesh, include, is_affine, return_status, None)

    def local_align_pyramid(self, files, warps, mesh: Optional["MeshParameters"] = None, levels: int = 3, include=None, *,
                            is_affine=False, return_status: bool = False):
        """local_align, coarse to fine over `levels` = 1 .. 4 pyramid levels (stk_local_align_pyramid): for shifts beyond a
        patch's capture range. The status planes are level 0's; levels = 1 gives local_align's bits. The fields go into
        mesh_stack, mesh_local_weighted_stack and mesh_drizzle_stack as they are."""
        return self._local_align(files, warps, mesh, include, is_affine, return_status, int(levels))

    def grey_pyramid(self, frame, levels: int):
        """Levels 1 .. levels - 1 of the box pyramid of one 8-bit frame's integer grey (stk_grey_pyramid): a list of
        (h >> l) x (w >> l) uint8 planes, placed where the frame lives."""
        m = self._marshal([frame] if getattr(frame, "ndim", 0) == 3 else frame)
        if m.n != 1:
            raise InvalidParams("grey_pyramid: one frame expected")
        levels = int(levels)
        made = [self._alloc(m, (max(m.h >> l, 1), max(m.w >> l, 1)), np.uint8, 0) for l in range(1, max(levels, 1))]
        pp = (C.c_void_p * (len(made) + 1))(None, *[addr for _, addr in made])
        self._check(self._lib.stk_grey_pyramid(self._h, C.byref(m.c_frames), levels, C.cast(pp, C.c_void_p)))
        return [a for a, _ in made]

    def _local_align(self, files, warps, mesh, include, is_affine, return_status, levels):
        m, head = self._warped(files, warps, include, is_affine)
        mp = (mesh or MeshParameters())._c()
        gw, gh = mesh_grid(m.w, m.h, mp.step) if mp.step in (8, 16, 32, 64, 128, 256) else (1, 1)
        fields, fptr = self._plane_table(m, (gh, gw, 2), np.float32, 0)      # zeroed: the engine writes over them
        status, sptr = self._plane_table(m, (gh, gw), np.int32, 0)
        if levels is None:
            self._check(self._lib.stk_local_align(*head, C.byref(mp), fptr, sptr if return_status else None))
        else:
            self._check(self._lib.stk_local_align_pyramid(*head, C.byref(mp), levels, fptr, sptr if return_status else None))
        return (fields, status) if return_status else fields

    def mesh_stack(self, files, warps, fields, step: int, include=None, *, is_affine=False, border_mode=BORDER_CONSTANT,
                   border_value=(0, 0, 0, 0), alpha=1.0 / 255.0):
        """The plain mean of the included frames, each folded through its warp and its displacement field
        (stk_mesh_stack). fields: n gh x gw x 2 float32 planes for the grid of `step` (local_align's result)."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        fkeep, fptrs = self._fields_arg(m, fields, step)
        out, img = self._image(m)
        self._check(self._lib.stk_mesh_stack(*head, C.cast(fptrs, C.c_void_p), int(step), C.byref(img)))
        return out

    def mesh_local_weighted_stack(self, files, warps, maps, fields, step: int, gain=None, offset=None, weights=None, include=None, *,
                                  applied=None, floor: float = 1.0, power: int = 2, is_affine=False, border_mode=BORDER_CONSTANT,
                                  border_value=(0, 0, 0, 0), alpha=1.0 / 255.0, return_coverage: bool = False):
        """local_weighted_stack through displacement fields (stk_mesh_local_weighted_stack): samples, coverage and the
        weight maps are all taken at the displaced coordinates."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        rec = self._records_arg(m, gain, offset, weights, applied, optional=True)
        mkeep, mptrs = self._maps_arg(m, maps)
        fkeep, fptrs = self._fields_arg(m, fields, step)
        out, img = self._image(m)
        cov, cptr = self._optional(m, return_coverage, np.float32)
        self._check(self._lib.stk_mesh_local_weighted_stack(*head, rec, C.cast(mptrs, C.c_void_p), float(floor), int(power),
                                                            C.cast(fptrs, C.c_void_p), int(step), C.byref(img), cptr))
        return (out, cov) if return_coverage else out

    def _match_local_aligned(self, kind, files, params, mesh, local, scale_down_width, return_stats, levels):
        """The plain function, or with `levels` the pyramid one: [.., mesh, (levels), local or NULL, image, ..]."""
        mp, lp = (mesh or MeshParameters())._c(), None if local is None else local._c()
        if levels is None:
            return self._whole_stack(kind, "_local_aligned", files, params, scale_down_width, return_stats, [mp, lp])
        return self._whole_stack(kind, "_local_aligned_pyramid", files, params, scale_down_width, return_stats, [mp, int(levels), lp])

    def ecc_match_local_aligned(self, files, params: EccMatchParameters, mesh: Optional["MeshParameters"] = None,
                                local: Optional["LocalParameters"] = None, scale_down_width: Optional[float] = None,
                                return_stats: bool = False, *, _levels: Optional[int] = None):
        """ecc_match with local alignment (stk_ecc_match_local_aligned): every frame is folded through its ECC warp and the
        displacement field measured on top of it. local = None: the plain mean; else the local-sharpness weighted fold."""
        return self._match_local_aligned("ecc", files, params, mesh, local, scale_down_width, return_stats, _levels)

    def ecc_match_local_aligned_pyramid(self, files, params: EccMatchParameters, mesh: Optional["MeshParameters"] = None,
                                        levels: int = 3, local: Optional["LocalParameters"] = None,
                                        scale_down_width: Optional[float] = None, return_stats: bool = False):
        """ecc_match_local_aligned with the coarse-to-fine field pass (stk_ecc_match_local_aligned_pyramid)."""
        return self.ecc_match_local_aligned(files, params, mesh, local, scale_down_width, return_stats, _levels=int(levels))

    def keypoint_match_local_aligned_pyramid(self, files, params: KeyPointMatchParameters, mesh: Optional["MeshParameters"] = None,
                                             levels: int = 3, local: Optional["LocalParameters"] = None,
                                             scale_down_width: Optional[float] = None, return_stats: bool = False):
        """keypoint_match_local_aligned with the coarse-to-fine field pass (stk_keypoint_match_local_aligned_pyramid)."""
        return self.keypoint_match_local_aligned(files, params, mesh, local, scale_down_width, return_stats, _levels=int(levels))

    def keypoint_match_local_aligned(self, files, params: KeyPointMatchParameters, mesh: Optional["MeshParameters"] = None,
                                     local: Optional["LocalParameters"] = None, scale_down_width: Optional[float] = None,
                                     return_stats: bool = False, *, _levels: Optional[int] = None):
        """keypoint_match with local alignment (stk_keypoint_match_local_aligned): (dropped, image[, stats])."""
        return self._match_local_aligned("keypoint", files, params, mesh, local, scale_down_width, return_stats, _levels)

    # -- drizzle integration onto a finer or larger output grid (extension beyond the reference) ----------
    @staticmethod
    def _drizzle_shape(drizzle: "DrizzleParameters", out_shape):
        """m -> the (oh, ow) of a drizzle output: out_shape, or what covers frame 0 at the scale."""
        def shape(m):
            oh, ow = (int(v) for v in out_shape) if out_shape is not None else drizzle.out_shape(m.h, m.w)
            if oh < 1 or ow < 1:
                raise InvalidParams("drizzle: the output must be at least one pixel wide and high")
            return oh, ow
        return shape

    def _drizzle_stack(self, fn, files, warps, mesh, drizzle, gain, offset, weights, include, applied, maps, out_shape,
                       is_affine, alpha, return_den):
        """Both drizzle stacks: [head, drizzle, records or NULL, maps or NULL, (fields, step), image, den]."""
        m, head = self._warped(files, warps, include, is_affine, None, alpha)
        dz = drizzle or DrizzleParameters()
        rec = self._records_arg(m, gain, offset, weights, applied, optional=True)
        mkeep, mptrs = self._maps_arg(m, maps, optional=True)
        if mesh is not None:                          # (fields, step)
            fkeep, fptrs = self._fields_arg(m, mesh[0], mesh[1], allow_none=True)
            mesh = [C.cast(fptrs, C.c_void_p), int(mesh[1])]
        shape = self._drizzle_shape(dz, out_shape)(m)
        out, img = self._image(m, shape)
        den, dptr = self._optional(m, return_den, np.float32, shape=shape)
        p = dz._c()
        self._check(fn(*head, C.byref(p), rec, None if mptrs is None else C.cast(mptrs, C.c_void_p), *(mesh or []), C.byref(img), dptr))
        return (out, den) if return_den else out

    def drizzle_stack(self, files, warps, drizzle: Optional["DrizzleParameters"] = None, gain=None, offset=None, weights=None,
                      include=None, *, applied=None, maps=None, out_shape=None, is_affine=False, alpha=1.0 / 255.0,
                      return_den: bool = False):
        """Drizzle over caller-held warps (stk_drizzle_stack) onto an out_shape = (oh, ow) grid (default: what covers frame 0
        at the scale). gain, offset, weights, applied: as in weighted_stack (None = 1 / 0 / 1). maps: None, or one H x W
        float32 plane of non-negative weights per frame (a bad-pixel mask, an inverse variance), single entries may be None
        = all ones. Returns the image, with return_den also the weight image."""
        return self._drizzle_stack(self._lib.stk_drizzle_stack, files, warps, None, drizzle, gain, offset, weights, include,
                                   applied, maps, out_shape, is_affine, alpha, return_den)

    def _match_drizzle(self, kind, suffix, files, params, combine, drizzle, scale_down_width, out_shape, return_den, return_stats):
        dz = drizzle or DrizzleParameters()
        shape = self._drizzle_shape(dz, out_shape)
        return self._whole_stack(kind, suffix, files, params, scale_down_width, return_stats, combine + [dz._c()],
                                 [(return_den, self._out_plane(np.float32, shape=shape))], image_shape=shape)

    def ecc_match_drizzle(self, files, params: EccMatchParameters, drizzle: Optional["DrizzleParameters"] = None,
                          scale_down_width: Optional[float] = None, *, out_shape=None, return_den: bool = False,
                          return_stats: bool = False):
        """ecc_match with the drizzle combine (stk_ecc_match_drizzle): aligned as ecc_match aligns, then frame 0 and every
        frame under its warp drizzled onto the output grid. Returns the image[, the weight image][, the stats]."""
        return self._match_drizzle("ecc", "_drizzle", files, params, [], drizzle, scale_down_width, out_shape, return_den, return_stats)

    def keypoint_match_drizzle(self, files, params: KeyPointMatchParameters, drizzle: Optional["DrizzleParameters"] = None,
                               scale_down_width: Optional[float] = None, *, out_shape=None, return_den: bool = False,
                               return_stats: bool = False):
        """keypoint_match with the drizzle combine (stk_keypoint_match_drizzle): (dropped, image[, weight image][, stats]).
        A dropped frame is no sample: it is absent from the weight image."""
        return self._match_drizzle("keypoint", "_drizzle", files, params, [], drizzle, scale_down_width, out_shape, return_den,
                                   return_stats)

    # -- mesh-displaced drizzle: drizzle through local-alignment fields (extension beyond the reference) --
    def mesh_drizzle_stack(self, files, warps, fields, step: int, drizzle: Optional["DrizzleParameters"] = None, gain=None, offset=None,
                           weights=None, include=None, *, applied=None, maps=None, out_shape=None, is_affine=False, alpha=1.0 / 255.0,
                           return_den: bool = False):
        """drizzle_stack through displacement fields (stk_mesh_drizzle_stack). fields: n gh x gw x 2 float32 planes for the
        grid of `step` (local_align's result), single entries may be None = not displaced; frame 0's is not read."""
        return self._drizzle_stack(self._lib.stk_mesh_drizzle_stack, files, warps, (fields, step), drizzle, gain, offset, weights,
                                   include, applied, maps, out_shape, is_affine, alpha, return_den)

    def ecc_match_local_aligned_drizzle(self, files, params: EccMatchParameters, mesh: Optional["MeshParameters"] = None,
                                        drizzle: Optional["DrizzleParameters"] = None, scale_down_width: Optional[float] = None, *,
                                        out_shape=None, return_den: bool = False, return_stats: bool = False):
        """ecc_match_drizzle with local alignment (stk_ecc_match_local_aligned_drizzle): every frame is drizzled through its
        ECC warp and the displacement field measured on top of it. Returns the image[, the weight image][, the stats]."""
        return self._match_drizzle("ecc", "_local_aligned_drizzle", files, params, [(mesh or MeshParameters())._c()], drizzle,
                                   scale_down_width, out_shape, return_den, return_stats)

    def keypoint_match_local_aligned_drizzle(self, files, params: KeyPointMatchParameters, mesh: Optional["MeshParameters"] = None,
                                             drizzle: Optional["DrizzleParameters"] = None, scale_down_width: Optional[float] = None, *,
                                             out_shape=None, return_den: bool = False, return_stats: bool = False):
        """keypoint_match_drizzle with local alignment (stk_keypoint_match_local_aligned_drizzle):
        (dropped, image[, weight image][, stats])."""
        return self._match_drizzle("keypoint", "_local_aligned_drizzle", files, params, [(mesh or MeshParameters())._c()], drizzle,
                                   scale_down_width, out_shape, return_den, return_stats)

    # -- blot-and-compare rejection maps for drizzle (extension beyond the reference) ---------------------
    def reject_maps(self, files, warps, clean, reject: Optional["RejectParameters"] = None, counts=None, gain=None, offset=None,
                    include=None, *, applied=None, maps=None, out=None, is_affine=False, alpha=1.0 / 255.0,
                    return_counts: bool = False):
        """Blot-and-compare rejection maps over caller-held warps (stk_reject_maps). clean: the H x W x C float32 clean image
        on frame 0's grid (quantile_stack_weighted at 0.5); counts: its H x W int32 participation counts, or None; gain,
        offset, applied: as in weighted_stack (None = 1 / 0); maps: None, or one H x W float32 input plane per frame (an
        n x H x W array, or a list whose entries may be None = all ones). out: None, or an n x H x W float32 array where the
        frames live to write into; it may be `maps` itself (in place). Returns the n x H x W maps (0 = rejected, else the
        input value or 1; an excluded frame's plane is left as it is, all ones in a fresh array), with return_counts also
        the per-frame numbers of rejected and of judged pixels (int64)."""
        m, head = self._warped(files, warps, include, is_affine, None, alpha)
        rp = (reject or RejectParameters())._c()
        rec = self._records_arg(m, gain, offset, None, applied, optional=True)
        ckeep, cptr = self._array_arg(m, clean, np.float32, (m.h, m.w, m.c), "clean image")
        nkeep, nptr = (None, None) if counts is None else self._array_arg(m, counts, np.int32, (m.h, m.w), "counts")
        plane = m.h * m.w * 4
        res = self._alloc(m, (m.n, m.h, m.w), np.float32, 1)[0] if out is None else out     # fresh planes: all ones
        okeep, optr = self._array_arg(m, res, np.float32, (m.n, m.h, m.w), "out")
        if out is not None and okeep is not out:
            raise InvalidParams("out: a contiguous n x H x W float32 array where the frames live expected")
        optrs = (C.c_void_p * m.n)(*[optr + i * plane for i in range(m.n)])
        ikeep, iptrs = None, None
        if maps is not None and (maps is out or not isinstance(maps, (list, tuple))):
            ikeep, base = self._array_arg(m, maps, np.float32, (m.n, m.h, m.w), "maps")
            iptrs = (C.c_void_p * m.n)(*[base + i * plane for i in range(m.n)])
        elif maps is not None:
            ikeep, iptrs = self._planes_arg(m, maps, (m.h, m.w), "one input map (or None) per frame expected",
                                            f"maps: shape {(m.h, m.w)} expected", allow_none=True)
        rej = np.zeros(m.n, np.int64)
        jud = np.zeros(m.n, np.int64)
        self._check(self._lib.stk_reject_maps(*head, rec, C.c_void_p(cptr), None if nptr is None else C.c_void_p(nptr), C.byref(rp),
                                              None if iptrs is None else C.cast(iptrs, C.c_void_p), C.cast(optrs, C.c_void_p),
                                              C.c_void_p(rej.ctypes.data), C.c_void_p(jud.ctypes.data)))
        return (res, rej, jud) if return_counts else res

    def _drizzle_rejected(self, kind, files, params, drizzle, reject, weight, weights, scale_down_width, out_shape, return_den,
                          return_maps, return_rejected, return_applied, return_stats):
        dz = drizzle or DrizzleParameters()
        shape = self._drizzle_shape(dz, out_shape)

        def maps(m, wanted):                          # the planes the drizzle used: all ones where nothing was rejected
            a, ptrs = self._plane_table(m, (m.h, m.w), np.float32, 1) if wanted else (None, None)
            return ptrs, lambda stl: a

        def rejected(m, wanted):                      # always passed
            rej = np.zeros(m.n, np.int64)
            return C.c_void_p(rej.ctypes.data), lambda stl: rej
        combine = [dz._c(), (weight or WeightParameters())._c(), self._weights_combine(weights), (reject or RejectParameters())._c()]
        return self._whole_stack(kind, "_drizzle_rejected", files, params, scale_down_width, return_stats, combine,
                                 [(return_den, self._out_plane(np.float32, shape=shape)), (return_maps, maps),
                                  (return_rejected, rejected), (return_applied, self._out_applied)], image_shape=shape)

    def ecc_match_drizzle_rejected(self, files, params: EccMatchParameters, drizzle: Optional["DrizzleParameters"] = None,
                                   reject: Optional["RejectParameters"] = None, weight: Optional["WeightParameters"] = None,
                                   weights=None, scale_down_width: Optional[float] = None, *, out_shape=None, return_den: bool = False,
                                   return_maps: bool = False, return_rejected: bool = False, return_applied: bool = False,
                                   return_stats: bool = False):
        """ecc_match_drizzle with blot-and-compare rejection (stk_ecc_match_drizzle_rejected): aligned as ecc_match aligns,
        the records of ecc_match_weighted, the coverage-aware median as the clean image, the rejection maps against it, then
        the drizzle with the records and the maps. weight.coverage must be True. Returns the image[, the weight image]
        [, the n x H x W maps the drizzle used][, the per-frame numbers of rejected pixels][, the records][, the stats]."""
        return self._drizzle_rejected("ecc", files, params, drizzle, reject, weight, weights, scale_down_width, out_shape, return_den,
                                      return_maps, return_rejected, return_applied, return_stats)

    def keypoint_match_drizzle_rejected(self, files, params: KeyPointMatchParameters, drizzle: Optional["DrizzleParameters"] = None,
                                        reject: Optional["RejectParameters"] = None, weight: Optional["WeightParameters"] = None,
                                        weights=None, scale_down_width: Optional[float] = None, *, out_shape=None,
                                        return_den: bool = False, return_maps: bool = False, return_rejected: bool = False,
                                        return_applied: bool = False, return_stats: bool = False):
        """keypoint_match_drizzle with blot-and-compare rejection (stk_keypoint_match_drizzle_rejected): (dropped, image
        [, weight image][, maps][, rejected][, applied][, stats]). A dropped frame is no sample: its map stays all ones and
        its count 0."""
        return self._drizzle_rejected("keypoint", files, params, drizzle, reject, weight, weights, scale_down_width, out_shape,
                                      return_den, return_maps, return_rejected, return_applied, return_stats)

    # -- normalised, coverage-aware rejection combines (extension beyond the reference) -----------------
    @staticmethod
    def _records_arg(m: _Marshalled, gain, offset, weights, applied, optional: bool = False):
        """n stk_frame_weight records from gain / offset (n x channels), weights (n) or another call's `applied`.
        optional: None = NULL when nothing was given (the engine's defaults); else the records are always built."""
        if optional and gain is None and offset is None and weights is None and applied is None:
            return None
        rec = (_ffi.FrameWeight * m.n)()
        if applied is not None:
            if len(applied) != m.n:
                raise InvalidParams("one record per frame expected")
            gain = [a["gain"] for a in applied]
            offset = [a["offset"] for a in applied]
            weights = [a["weight"] for a in applied]
        g = np.ones((m.n, m.c), np.float32) if gain is None else np.asarray(gain, np.float32).reshape(m.n, -1)
        o = np.zeros((m.n, m.c), np.float32) if offset is None else np.asarray(offset, np.float32).reshape(m.n, -1)
        w = np.ones(m.n, np.float32) if weights is None else np.asarray(weights, np.float32).reshape(-1)
        if g.shape != (m.n, m.c) or o.shape != (m.n, m.c) or w.size != m.n:
            raise InvalidParams("gain and offset: n x channels, weights: n expected")
        for i in range(m.n):
            for c in range(4):
                rec[i].gain[c] = float(g[i, c]) if c < m.c else 1.0
                rec[i].offset[c] = float(o[i, c]) if c < m.c else 0.0
            rec[i].weight = float(w[i])
        return rec

    def clip_stack_weighted(self, files, warps, clip: Optional["SigmaClipParameters"] = None, gain=None, offset=None, weights=None,
                            include=None, *, applied=None, coverage: bool = True, is_affine=False, border_mode=BORDER_CONSTANT,
                            border_value=(0, 0, 0, 0), alpha=1.0 / 255.0, return_counts: bool = False,
                            return_kept_weight: bool = False):
        """The normalised, coverage-aware clip alone over caller-held warps (stk_clip_stack_weighted): clip_stack with
        weighted_stack's gain / offset / weights (or `applied`) and coverage. Returns the image, then the counts of kept
        samples (return_counts) and the kept weight (return_kept_weight), both per pixel and channel."""
        return self._stack_weighted(self._lib.stk_clip_stack_weighted, (clip or SigmaClipParameters())._c(), files, warps, gain,
                                    offset, weights, include, applied, coverage, is_affine, border_mode, border_value, alpha,
                                    [(return_counts, np.int32, True), (return_kept_weight, np.float32, True)])

    def robust_clip_stack_weighted(self, files, warps, clip: Optional["RobustClipParameters"] = None, gain=None, offset=None,
                                   weights=None, include=None, *, applied=None, coverage: bool = True, is_affine=False,
                                   border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0 / 255.0,
                                   return_counts: bool = False, return_kept_weight: bool = False):
        """The median / MAD clip with participation over caller-held warps (stk_robust_clip_stack_weighted), with the
        arguments and results of clip_stack_weighted."""
        return self._stack_weighted(self._lib.stk_robust_clip_stack_weighted, (clip or RobustClipParameters())._c(), files, warps,
                                    gain, offset, weights, include, applied, coverage, is_affine, border_mode, border_value, alpha,
                                    [(return_counts, np.int32, True), (return_kept_weight, np.float32, True)])

    def _stack_weighted(self, fn, cp, files, warps, gain, offset, weights, include, applied, coverage, is_affine, border_mode,
                        border_value, alpha, outputs):
        """The clip and quantile stacks with records: [head, combine parameters, records, coverage, image, *outputs];
        outputs: [(wanted, dtype, per_channel)]. The records are always built."""
        m, head = self._warped(files, warps, include, is_affine, (border_mode, border_value), alpha)
        rec = self._records_arg(m, gain, offset, weights, applied)
        out, img = self._image(m)
        outs = [self._optional(m, *o) for o in outputs]
        self._check(fn(*head, C.byref(cp), rec, int(coverage), C.byref(img), *[ptr for _, ptr in outs]))
        res = (out,) + tuple(a for a, _ in outs if a is not None)
        return res if len(res) > 1 else out

    def quantile_stack_weighted(self, files, warps, quantile=None, gain=None, offset=None, weights=None, include=None, *,
                                applied=None, coverage: bool = True, is_affine=False, border_mode=BORDER_CONSTANT,
                                border_value=(0, 0, 0, 0), alpha=1.0 / 255.0, return_counts: bool = False):
        """The normalised, coverage-aware quantile alone over caller-held warps (stk_quantile_stack_weighted). Returns the
        image, then the per-pixel number of participating frames (return_counts, HxW)."""
        return self._stack_weighted(self._lib.stk_quantile_stack_weighted, _quantile_c(quantile), files, warps, gain, offset, weights,
                                    include, applied, coverage, is_affine, border_mode, border_value, alpha, [(return_counts, np.int32)])

    def _robust_match(self, kind, suffix, cp, per_channel, files, params, weight, weights, scale_down_width, return_stats,
                      return_counts, return_kept_weight, return_applied):
        """The clip and quantile forms with records: [.., combine parameters, weight, weights, image, .., counts,
        (kept weight: the clips only), applied, stats]; the clips count per pixel and channel, the quantile per pixel."""
        kept = [(return_kept_weight, self._out_plane(np.float32, True))] if per_channel else []
        return self._whole_stack(kind, suffix, files, params, scale_down_width, return_stats,
                                 [cp, (weight or WeightParameters())._c(), self._weights_combine(weights)],
                                 [(return_counts, self._out_plane(np.int32, per_channel))] + kept + [(return_applied, self._out_applied)])

    def ecc_match_clipped_weighted(self, files, params: EccMatchParameters, clip: Optional["SigmaClipParameters"] = None,
                                   weight: Optional["WeightParameters"] = None, weights=None, scale_down_width: Optional[float] = None,
                                   return_stats: bool = False, return_counts: bool = False, return_kept_weight: bool = False,
                                   return_applied: bool = False):
        """ecc_match with the normalised, coverage-aware sigma clip (stk_ecc_match_clipped_weighted): the image, then the
        counts (return_counts), the kept weight (return_kept_weight), the per-frame records used (return_applied) and the
        stats (return_stats)."""
        return self._robust_match("ecc", "_clipped_weighted", (clip or SigmaClipParameters())._c(), True, files, params, weight, weights,
                                  scale_down_width, return_stats, return_counts, return_kept_weight, return_applied)

    def keypoint_match_clipped_weighted(self, files, params: KeyPointMatchParameters, clip: Optional["SigmaClipParameters"] = None,
                                        weight: Optional["WeightParameters"] = None, weights=None,
                                        scale_down_width: Optional[float] = None, return_stats: bool = False,
                                        return_counts: bool = False, return_kept_weight: bool = False, return_applied: bool = False):
        """keypoint_match with the normalised, coverage-aware sigma clip (stk_keypoint_match_clipped_weighted):
        (dropped, image[, counts][, kept weight][, applied][, stats])."""
        return self._robust_match("keypoint", "_clipped_weighted", (clip or SigmaClipParameters())._c(), True, files, params, weight,
                                  weights, scale_down_width, return_stats, return_counts, return_kept_weight, return_applied)

    def ecc_match_robust_clipped_weighted(self, files, params: EccMatchParameters, clip: Optional["RobustClipParameters"] = None,
                                          weight: Optional["WeightParameters"] = None, weights=None,
                                          scale_down_width: Optional[float] = None, return_stats: bool = False,
                                          return_counts: bool = False, return_kept_weight: bool = False, return_applied: bool = False):
        """ecc_match with the median / MAD clip with participation (stk_ecc_match_robust_clipped_weighted); results as
        ecc_match_clipped_weighted."""
        return self._robust_match("ecc", "_robust_clipped_weighted", (clip or RobustClipParameters())._c(), True, files, params, weight,
                                  weights, scale_down_width, return_stats, return_counts, return_kept_weight, return_applied)

    def keypoint_match_robust_clipped_weighted(self, files, params: KeyPointMatchParameters,
                                               clip: Optional["RobustClipParameters"] = None,
                                               weight: Optional["WeightParameters"] = None, weights=None,
                                               scale_down_width: Optional[float] = None, return_stats: bool = False,
                                               return_counts: bool = False, return_kept_weight: bool = False,
                                               return_applied: bool = False):
        """keypoint_match with the median / MAD clip with participation (stk_keypoint_match_robust_clipped_weighted); results
        as keypoint_match_clipped_weighted."""
        return self._robust_match("keypoint", "_robust_clipped_weighted", (clip or RobustClipParameters())._c(), True, files, params,
                                  weight, weights, scale_down_width, return_stats, return_counts, return_kept_weight, return_applied)

    def ecc_match_quantile_weighted(self, files, params: EccMatchParameters, quantile=None,
                                    weight: Optional["WeightParameters"] = None, weights=None, scale_down_width: Optional[float] = None,
                                    return_stats: bool = False, return_counts: bool = False, return_applied: bool = False):
        """ecc_match with the normalised, coverage-aware quantile (stk_ecc_match_quantile_weighted): the image, then the
        per-pixel number of participating frames (return_counts), the records (return_applied) and the stats."""
        return self._robust_match("ecc", "_quantile_weighted", _quantile_c(quantile), False, files, params, weight, weights,
                                  scale_down_width, return_stats, return_counts, False, return_applied)

    def keypoint_match_quantile_weighted(self, files, params: KeyPointMatchParameters, quantile=None,
                                         weight: Optional["WeightParameters"] = None, weights=None,
                                         scale_down_width: Optional[float] = None, return_stats: bool = False,
                                         return_counts: bool = False, return_applied: bool = False):
        """keypoint_match with the normalised, coverage-aware quantile (stk_keypoint_match_quantile_weighted):
        (dropped, image[, counts][, applied][, stats])."""
        return self._robust_match("keypoint", "_quantile_weighted", _quantile_c(quantile), False, files, params, weight, weights,
                                  scale_down_width, return_stats, return_counts, False, return_applied)

    # -- shard-level (one process per GPU; frames[0] = reference frame) ------------------------------
    def ecc_match_shard(self, files, params: EccMatchParameters, add_reference: bool, sum_out,
                        scale_down_width: Optional[float] = None, return_stats: bool = True):
        """Un-normalised f32 sum of this rank's aligned frames into `sum_out` (cuda tensor HxWx3)."""
        m = self._stack(files)
        self._tensor_ready(sum_out)
        img = _ffi.ImageF32(sum_out.data_ptr(), m.w, m.h, 3, DEVICE, _image_stride_bytes(sum_out))
        added = C.c_int32(0)
        stats = (_ffi.FrameStats * m.n)()
        p = params._c()
        st = self._lib.stk_ecc_match_shard(self._h, C.byref(m.c_frames), C.byref(p), float(scale_down_width or 0.0),
                                           int(bool(add_reference)), C.byref(img), C.byref(added), stats)
        self._check(st)
        return added.value, (self._stats_list(stats, m.n) if return_stats else None)

    def keypoint_match_shard(self, files, params: KeyPointMatchParameters, add_reference: bool, sum_out,
                             scale_down_width: Optional[float] = None, return_stats: bool = True):
        m = self._stack(files)
        self._tensor_ready(sum_out)
        img = _ffi.ImageF32(sum_out.data_ptr(), m.w, m.h, 3, DEVICE, _image_stride_bytes(sum_out))
        added, dropped = C.c_int32(0), C.c_int32(0)
        stats = (_ffi.FrameStats * m.n)()
        p = params._c()
        st = self._lib.stk_keypoint_match_shard(self._h, C.byref(m.c_frames), C.byref(p),
                                                float(scale_down_width or 0.0), int(bool(add_reference)),
                                                C.byref(img), C.byref(added), C.byref(dropped), stats)
        self._check(st)
        return added.value, dropped.value, (self._stats_list(stats, m.n) if return_stats else None)

    def finalize_mean(self, sum_img, n_frames: int, out=None):
        """img / n  (lib.rs:339-345, 836-839) on a cuda tensor; in place when out is None."""
        self._tensor_ready(sum_img)
        h, w, c = sum_img.shape
        out = sum_img if out is None else out
        if out is not sum_img:
            self._tensor_ready(out)
        a = _ffi.ImageF32(sum_img.data_ptr(), w, h, c, DEVICE, 0)
        b = _ffi.ImageF32(out.data_ptr(), w, h, c, DEVICE, 0)
        self._check(self._lib.stk_finalize_mean(self._h, C.byref(a), int(n_frames), C.byref(b)))
        return out

    # -- stage-level (parity tests) ------------------------------------------------------------------
    def grey(self, frame):
        m = self._marshal([frame])
        out, ptr = self._alloc(m, (m.h, m.w), {8: np.uint8, 16: np.uint16, 32: np.float32}[m.depth])
        self._check(self._lib.stk_grey(self._h, C.byref(m.c_frames), C.c_void_p(ptr)))
        return out

    def convert_f32(self, frame, alpha: float = 1.0 / 255.0):
        m = self._marshal([frame])
        out, ptr = self._alloc(m, tuple(m.keep[0].shape), np.float32)
        self._check(self._lib.stk_convert_f32(self._h, C.byref(m.c_frames), float(alpha), C.c_void_p(ptr)))
        return out

    # -- BASELINE configs[4] (extension): ORB-seeded ECC on 8- or 16-bit stacks --------------------------------
    def hybrid_match(self, files, kp_params: KeyPointMatchParameters, ecc_params: EccMatchParameters, return_stats=False):
        """ORB + RANSAC homography as the initial warp of findTransformECC; 16-bit frames folded with alpha 1/65535."""
        m = self._stack(files)
        out, img = self._image(m)
        stats = (_ffi.FrameStats * m.n)()
        kp, ep = kp_params._c(), ecc_params._c()
        self._check(self._lib.stk_hybrid_match(self._h, C.byref(m.c_frames), C.byref(kp), C.byref(ep), C.byref(img), stats))
        return (out, self._stats_list(stats, m.n)) if return_stats else out

    def hybrid_match_shard(self, files, kp_params: KeyPointMatchParameters, ecc_params: EccMatchParameters,
                           add_reference: bool, sum_out, return_stats: bool = True):
        m = self._stack(files)
        self._tensor_ready(sum_out)
        img = _ffi.ImageF32(sum_out.data_ptr(), m.w, m.h, 3, DEVICE, _image_stride_bytes(sum_out))
        added = C.c_int32(0)
        stats = (_ffi.FrameStats * m.n)()
        kp, ep = kp_params._c(), ecc_params._c()
        self._check(self._lib.stk_hybrid_match_shard(self._h, C.byref(m.c_frames), C.byref(kp), C.byref(ep),
                                                     int(bool(add_reference)), C.byref(img), C.byref(added), stats))
        return added.value, (self._stats_list(stats, m.n) if return_stats else None)

    # -- file front-end: the reference's entry points take paths ------------------------------
    def imread(self, path):
        """imgcodecs::imread(path, IMREAD_UNCHANGED) for binary PNM, 8-bit PNG and 8/16-bit TIFF: HxW or HxWx3 (BGR) array."""
        w, h, c, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        bp = os.fsencode(path)
        self._check(self._lib.stk_imread(self._h, bp, None, 0, C.byref(w), C.byref(h), C.byref(c), C.byref(d)))
        out = np.empty((h.value, w.value, c.value), np.uint8 if d.value == 8 else np.uint16)
        self._check(self._lib.stk_imread(self._h, bp, C.c_void_p(out.ctypes.data), out.nbytes, None, None, None, None))
        return out[..., 0] if c.value == 1 else out

    def _paths(self, files):
        enc = [os.fsencode(f) for f in files]
        arr = (C.c_char_p * max(len(enc), 1))(*enc)
        return enc, arr

    def _file_geometry(self, files):
        w, h, c, d = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.stk_imread(self._h, os.fsencode(files[0]), None, 0, C.byref(w), C.byref(h), C.byref(c), C.byref(d)))
        return w.value, h.value, (4 if c.value == 4 else 3)       # (an RGBA file gives a CV_32FC4 stack, like the reference)

    def keypoint_match_files(self, files, params: KeyPointMatchParameters, scale_down_width: Optional[float] = None):
        """keypoint_match(files, params, scale_down_width) -> (dropped, HxWx3 f32)   lib.rs:129-137"""
        files = list(files)
        if not files:
            raise NotEnoughFiles("Not enough files")
        w, h, cn = self._file_geometry(files)
        out = np.empty((h, w, cn), np.float32)
        img = _ffi.ImageF32(out.ctypes.data, w, h, cn, HOST, 0)
        keep, arr = self._paths(files)
        dropped = C.c_int32(0)
        p = params._c()
        self._check(self._lib.stk_keypoint_match_files(self._h, arr, len(files), C.byref(p), float(scale_down_width or 0.0),
                                                       C.byref(img), C.byref(dropped), None))
        return dropped.value, out

    def ecc_match_files(self, files, params: EccMatchParameters, scale_down_width: Optional[float] = None):
        """ecc_match(files, params, scale_down_width) -> HxWx3 f32   lib.rs:702-710"""
        files = list(files)
        if not files:
            raise NotEnoughFiles("Not enough files")
        w, h, cn = self._file_geometry(files)
        out = np.empty((h, w, cn), np.float32)
        img = _ffi.ImageF32(out.ctypes.data, w, h, cn, HOST, 0)
        keep, arr = self._paths(files)
        p = params._c()
        self._check(self._lib.stk_ecc_match_files(self._h, arr, len(files), C.byref(p), float(scale_down_width or 0.0),
                                                  C.byref(img), None))
        return out

    def hybrid_match_files(self, files, kp_params: KeyPointMatchParameters, ecc_params: EccMatchParameters):
        """stk_hybrid_match on a list of paths (e.g. a 16-bit TIFF stack)."""
        files = list(files)
        if not files:
            raise NotEnoughFiles("Not enough files")
        w, h, cn = self._file_geometry(files)
        out = np.empty((h, w, cn), np.float32)
        img = _ffi.ImageF32(out.ctypes.data, w, h, cn, HOST, 0)
        keep, arr = self._paths(files)
        kp, ep = kp_params._c(), ecc_params._c()
        self._check(self._lib.stk_hybrid_match_files(self._h, arr, len(files), C.byref(kp), C.byref(ep), C.byref(img), None))
        return out

    def _sharpness(self, grey, metric: int, ksize: int = 0) -> float:
        g = np.ascontiguousarray(grey)
        if g.ndim != 2 or str(g.dtype) not in ("uint8", "float32"):
            raise InvalidParams("sharpness metrics take a single-channel uint8 or float32 image")
        h, w = g.shape
        out = C.c_double(0.0)
        self._check(self._lib.stk_sharpness(self._h, C.c_void_p(g.ctypes.data), _DEPTH[str(g.dtype)], w, h, HOST,
                                            int(metric), int(ksize), C.byref(out)))
        return out.value

    def sharpness_modified_laplacian(self, grey) -> float:
        """lib.rs:1032-1071 (LAPM, Nayar89)."""
        return self._sharpness(grey, 0)

    def sharpness_variance_of_laplacian(self, grey) -> float:
        """lib.rs:1075-1091 (LAPV, Pech2000)."""
        return self._sharpness(grey, 1)

    def sharpness_tenengrad(self, grey, k_size: int) -> float:
        """lib.rs:1103-1147 (TENG, Krotkov86); k_size must be 1, 3, 5 or 7."""
        return self._sharpness(grey, 2, k_size)

    def sharpness_normalized_gray_level_variance(self, grey) -> float:
        """lib.rs:1151-1166 (GLVN, Santos97)."""
        return self._sharpness(grey, 3)

    def grey_blur_f32(self, frame, ksize: int):
        """cvt_color(BGR2GRAY) + findTransformECC's GaussianBlur of one frame, fused (the per-frame ECC preparation)."""
        m = self._marshal([frame])
        out, ptr = self._alloc(m, (m.h, m.w), np.float32)
        self._check(self._lib.stk_grey_blur_f32(self._h, C.byref(m.c_frames), int(ksize), C.c_void_p(ptr)))
        return out

    def gaussian_blur_f32(self, grey, ksize: int):
        g = np.ascontiguousarray(grey)
        h, w = g.shape
        out = np.empty((h, w), np.float32)
        self._check(self._lib.stk_gaussian_blur_f32(self._h, C.c_void_p(g.ctypes.data), _DEPTH[str(g.dtype)], w, h,
                                                    HOST, int(ksize), C.c_void_p(out.ctypes.data)))
        return out

    def find_transform_ecc(self, templ, inp, warp, params: EccMatchParameters):
        """video::find_transform_ecc(template, input, warp, ...) lib.rs:769-777 -> (warp3x3 f32, rho, iterations)."""
        t = np.ascontiguousarray(templ)
        i = np.ascontiguousarray(inp)
        if t.shape != i.shape or t.dtype != i.dtype:
            raise InvalidParams("template and input must share size and type")
        wm = np.eye(3, dtype=np.float32)
        wv = np.asarray(warp, np.float32)
        wm[: wv.shape[0], :] = wv
        rho, its = C.c_double(0), C.c_int32(0)
        p = params._c()
        st = self._lib.stk_find_transform_ecc(self._h, C.c_void_p(t.ctypes.data), C.c_void_p(i.ctypes.data),
                                              _DEPTH[str(t.dtype)], t.shape[1], t.shape[0], HOST, C.byref(p),
                                              C.c_void_p(wm.ctypes.data), C.byref(rho), C.byref(its))
        self._check(st)
        return wm, rho.value, its.value

    def ecc_prepared(self) -> dict:
        """Test hook (stk_ecc_prepared): the planes the last ECC preparation on this context left for the iteration kernels,
        as host arrays: "templates" [n, h, w]; "I", "gx", "gy" [h + 2 pad, w + 2 pad] and the interleaved "gxy" [.., 2] and
        "igg" [.., 3], all with their zero border; "pad" its width."""
        w, h, n, pad = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        st = self._lib.stk_ecc_prepared_geometry(self._h, C.byref(w), C.byref(h), C.byref(n), C.byref(pad))
        if st != 0:
            raise InvalidParams("no ECC preparation has run on this context")
        w, h, n, pad = w.value, h.value, n.value, pad.value

        def fetch(what, index, shape):
            a = np.empty(shape, np.float32)
            self._check(self._lib.stk_ecc_prepared(self._h, what, index, C.c_void_p(a.ctypes.data), a.size))
            return a
        out = {"templates": np.stack([fetch(0, i, (h, w)) for i in range(n)]) if n else np.empty((0, h, w), np.float32), "pad": pad}
        hp, wp = h + 2 * pad, w + 2 * pad
        for what, (name, k) in enumerate((("I", 1), ("gx", 1), ("gy", 1), ("gxy", 2), ("igg", 3)), start=1):
            out[name] = fetch(what, 0, (hp, wp) if k == 1 else (hp, wp, k))
        return out

    def warp_accumulate(self, frame, M, *, is_affine=False, border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0),
                        alpha=1.0 / 255.0, acc=None):
        """warp_perspective/warp_affine(convert(frame, alpha), M) (+ acc). Returns the f32 image."""
        m = self._marshal([frame])
        Md = np.ascontiguousarray(np.asarray(M, np.float64).reshape(-1))
        if Md.size == 6:
            Md = np.concatenate([Md, [0.0, 0.0, 1.0]])
        bv = self._border_arg(border_value)
        accumulate = acc is not None
        if accumulate:
            out = acc
            if _is_torch(out):
                if out.is_cuda:
                    self._tensor_ready(out)
                img = _ffi.ImageF32(out.data_ptr(), m.w, m.h, m.c, DEVICE if out.is_cuda else HOST, _image_stride_bytes(out))
            else:
                img = _ffi.ImageF32(out.ctypes.data, m.w, m.h, m.c, HOST, _image_stride_bytes(out))
        else:
            out, img = self._image(m)
        st = self._lib.stk_warp_accumulate(self._h, C.byref(m.c_frames), C.c_void_p(Md.ctypes.data), int(is_affine),
                                           int(border_mode), C.c_void_p(bv.ctypes.data), float(alpha),
                                           int(accumulate), C.byref(img))
        self._check(st)
        return out

    def scale_image_grey(self, grey, scale_down: float):
        """utils::scale_image (utils.rs:186-214) on a grey image, 8-bit or f32 (the depths cvtColor leaves where the reference
        shrinks a grey): INTER_AREA, smaller dimension -> scale_down."""
        f32 = np.asarray(grey).dtype == np.float32
        g = np.ascontiguousarray(grey, np.float32 if f32 else np.uint8)
        h, w = g.shape
        f = float(np.float32(scale_down)) / min(w, h)              # utils.rs:191-199: the smaller dimension becomes scale_down
        out = np.empty(max(h * w, (int(w * f) + 1) * (int(h * f) + 1)), g.dtype)
        nw, nh = C.c_int32(0), C.c_int32(0)
        fn = self._lib.stk_scale_image_grey_f32 if f32 else self._lib.stk_scale_image_grey
        self._check(fn(self._h, C.c_void_p(g.ctypes.data), w, h, HOST, float(scale_down), C.c_void_p(out.ctypes.data), C.byref(nw), C.byref(nh)))
        return out[: nw.value * nh.value].reshape(nh.value, nw.value).copy()

    def orb_detect_and_compute(self, grey, max_keypoints: int = 2000):
        g = np.ascontiguousarray(grey, np.uint8)
        h, w = g.shape
        kps = np.zeros((max_keypoints, 7), np.float32)
        des = np.zeros((max_keypoints, 32), np.uint8)
        n = C.c_int32(0)
        st = self._lib.stk_orb_detect_and_compute(self._h, C.c_void_p(g.ctypes.data), w, h, HOST, int(max_keypoints),
                                                  C.c_void_p(kps.ctypes.data), C.c_void_p(des.ctypes.data), C.byref(n))
        self._check(st)
        return kps[: n.value].copy(), des[: n.value].copy()

    def bf_knn2_hamming(self, query, train):
        q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
        out = np.full((q.shape[0], 4), -1, np.int32)
        st = self._lib.stk_bf_knn2_hamming(self._h, C.c_void_p(q.ctypes.data), q.shape[0], C.c_void_p(t.ctypes.data),
                                           t.shape[0], C.c_void_p(out.ctypes.data))
        self._check(st)
        return out

    def find_homography(self, src_pts, dst_pts, method: int = RANSAC, ransac_reproj_threshold: float = 3.0):
        s = np.ascontiguousarray(src_pts, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(dst_pts, np.float32).reshape(-1, 2)
        H = np.zeros(9, np.float64)
        mask = np.zeros(s.shape[0], np.uint8)
        found = C.c_int32(0)
        st = self._lib.stk_find_homography(self._h, C.c_void_p(s.ctypes.data), C.c_void_p(d.ctypes.data), s.shape[0],
                                           int(method), float(ransac_reproj_threshold), C.c_void_p(H.ctypes.data),
                                           C.c_void_p(mask.ctypes.data), C.byref(found))
        self._check(st)
        return (H.reshape(3, 3) if found.value else None), mask

    def find_homography_batch(self, problems, method: int = RANSAC, ransac_reproj_threshold: float = 3.0):
        """find_homography for a list of (src, dst) point pairs in one call. One dict per problem: H (3x3 f64, or None when
        nothing is found or rc != 0), mask (n x uint8), rc (0, or 3 / 7 as findHomography would throw: the call itself does
        not raise for them), n_inliers, models_evaluated. Problem i returns the bits it returns alone."""
        pairs = [(np.ascontiguousarray(s, np.float32).reshape(-1, 2), np.ascontiguousarray(d, np.float32).reshape(-1, 2))
                 for s, d in problems]
        if not pairs:
            return []
        for s, d in pairs:
            if s.shape != d.shape:
                raise InvalidParams("find_homography_batch: src and dst of a problem differ in length")
        masks = [np.zeros(s.shape[0], np.uint8) for s, _ in pairs]
        probs = (_ffi.HgProblem * len(pairs))()
        for p, (s, d), m in zip(probs, pairs, masks):
            p.src_pts, p.dst_pts, p.n, p.inlier_mask_or_null = s.ctypes.data, d.ctypes.data, s.shape[0], m.ctypes.data
        outc = (_ffi.HgOutcome * len(pairs))()
        st = self._lib.stk_find_homography_batch(self._h, probs, len(pairs), int(method), float(ransac_reproj_threshold), outc)
        self._check(st)
        return [dict(H=np.array(o.H, np.float64).reshape(3, 3) if o.rc == 0 and o.found else None, mask=m, rc=int(o.rc),
                     n_inliers=int(o.n_inliers), models_evaluated=int(o.models_evaluated)) for o, m in zip(outc, masks)]


_default: dict[int, Stacker] = {}


def default_stacker(device: int = 0) -> Stacker:
    if device not in _default:
        _default[device] = Stacker(device)
    return _default[device]


def keypoint_match(files, params: KeyPointMatchParameters, scale_down_width: Optional[float] = None):
    """Drop-in for libstacker::keypoint_match (lib.rs:129-144): returns (dropped, image)."""
    return default_stacker().keypoint_match(files, params, scale_down_width)


def ecc_match(files, params: EccMatchParameters, scale_down_width: Optional[float] = None):
    """Drop-in for libstacker::ecc_match (lib.rs:702-717): returns the stacked f32 image."""
    return default_stacker().ecc_match(files, params, scale_down_width)

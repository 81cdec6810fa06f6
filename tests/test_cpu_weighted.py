"""Weighted, coverage-aware stacking, CPU side: the numpy restatements of the definition (include/stacker.h,
stk_weight_params) that the GPU tests (test_gpu_weighted.py) compare the engine against bit for bit — `weighted_restate`
(the combine) and `estimate` (gain and offset from the overlap moments) — checked here against hand-computed answers, and
the ctypes mirrors of stk_weight_params / stk_frame_weight."""
import ctypes

import numpy as np

from libstacker_rs_amd import WeightParameters, _ffi

NONE, OFFSET, GAIN, LINEAR = 0, 1, 2, 3


def weighted_restate(samples, kappa, g, o, w):
    """The weighted combine of `samples` (N x H x W x C, the fold's samples in fold order) with the coverage weights
    `kappa` (N x H x W), per-entry gains and offsets (N x C) and weights (N): every operation in f32 and rounded on its
    own, as the engine defines it. Returns (out H x W x C f32, den H x W f32)."""
    s = np.asarray(samples, np.float32)
    k = np.asarray(kappa, np.float32)
    g = np.asarray(g, np.float32).reshape(s.shape[0], -1)
    o = np.asarray(o, np.float32).reshape(s.shape[0], -1)
    w = np.asarray(w, np.float32).reshape(-1)
    num = np.zeros(s.shape[1:], np.float32)
    den = np.zeros(s.shape[1:3], np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(s.shape[0]):
            v = s[i] * g[i][None, None, :] + o[i][None, None, :] * k[i][..., None]
            num = num + w[i] * v
            den = den + w[i] * k[i]
        out = np.where(den[..., None] > 0, num / den[..., None], np.float32(0)).astype(np.float32)
    assert num.dtype == np.float32 and den.dtype == np.float32
    return out, den


def estimate(moments, mode):
    """Gain and offset from the overlap moments (... x C x 6: n, sum X, sum Y, sum X^2, sum Y^2, sum XY) in f64, each
    operation rounded on its own, results rounded to f32. Returns (gain f32, offset f32, fell_back bool), each ... x C."""
    m = np.asarray(moments, np.float64)
    n, sx, sy, sxx, syy = (m[..., k] for k in range(5))
    one, zero = np.ones(n.shape), np.zeros(n.shape)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx, my = sx / n, sy / n
        ok = n > 0
        if mode == NONE:
            g, o, ok = one, zero, np.ones(n.shape, bool)
        elif mode == OFFSET:
            g, o = one, my - mx
        elif mode == GAIN:
            ok = ok & (mx > 0)
            g, o = my / mx, zero
        else:
            vx, vy = sxx / n - mx * mx, syy / n - my * my
            ok = ok & (vx > 0)
            g = np.sqrt(vy / vx)
            o = my - g * mx
        gf, of = g.astype(np.float32), o.astype(np.float32)
    ok = ok & np.isfinite(gf) & np.isfinite(of)
    return np.where(ok, gf, np.float32(1)).astype(np.float32), np.where(ok, of, np.float32(0)).astype(np.float32), ~ok


# ---- the combine, by hand --------------------------------------------------------------------------------------
def _hand_case():
    # 2 pixels (one row), 3 frames, 1 channel; frame 1 does not cover pixel 1, frame 2 covers half of it
    s = np.array([[0.5, 0.25], [1.0, 0.0], [0.25, 0.5]], np.float32).reshape(3, 1, 2, 1)
    k = np.array([[1.0, 1.0], [1.0, 0.0], [1.0, 0.5]], np.float32).reshape(3, 1, 2)
    g = np.array([[1.0], [0.5], [2.0]], np.float32)
    o = np.array([[0.0], [0.25], [-0.125]], np.float32)
    return s, k, g, o


def test_restatement_matches_a_hand_computed_case():
    s, k, g, o = _hand_case()
    out, den = weighted_restate(s, k, g, o, [1.0, 2.0, 0.5])
    # pixel 0: v = 0.5, 0.75, 0.375; num = 0.5 + 2 * 0.75 + 0.5 * 0.375 = 2.1875; den = 1 + 2 + 0.5 = 3.5
    # pixel 1: v = 0.25, 0 (uncovered: s = 0, o * 0 = 0), 1 - 0.0625 = 0.9375; num = 0.25 + 0 + 0.46875 = 0.71875; den = 1 + 0 + 0.25
    assert den.reshape(-1).tolist() == [3.5, 1.25]
    assert out.reshape(-1)[0] == np.float32(0.625)
    assert out.reshape(-1)[1] == np.float32(0.71875) / np.float32(1.25)
    assert out.dtype == np.float32 and den.dtype == np.float32


def test_zero_weight_and_uncovered_pixels():
    s, k, g, o = _hand_case()
    # a zero weight: the frame adds nothing to num or den
    out, den = weighted_restate(s, k, g, o, [1.0, 0.0, 0.0])
    assert den.reshape(-1).tolist() == [1.0, 1.0] and out.reshape(-1).tolist() == [0.5, 0.25]
    # den == 0 -> 0: only frame 1 has weight, and it does not cover pixel 1
    out, den = weighted_restate(s, k, g, o, [0.0, 2.0, 0.0])
    assert den.reshape(-1).tolist() == [2.0, 0.0] and out.reshape(-1).tolist() == [0.75, 0.0]
    # kappa = 1 everywhere (coverage = 0): the border sample counts, offset and weight in full
    out, den = weighted_restate(s, np.ones_like(k), g, o, [1.0, 2.0, 0.5])
    assert den.reshape(-1).tolist() == [3.5, 3.5]
    assert out.reshape(-1)[1] == (np.float32(0.25) + np.float32(2.0) * np.float32(0.25) + np.float32(0.5) * np.float32(0.875)) / np.float32(3.5)


def test_restatement_is_channelwise_with_one_coverage_per_pixel():
    rng = np.random.default_rng(1)
    s = rng.random((4, 3, 5, 3)).astype(np.float32)
    k = rng.random((4, 3, 5)).astype(np.float32)
    g = rng.uniform(0.5, 2, (4, 3)).astype(np.float32)
    o = rng.uniform(-0.1, 0.1, (4, 3)).astype(np.float32)
    w = rng.uniform(0, 2, 4).astype(np.float32)
    out, den = weighted_restate(s, k, g, o, w)
    for c in range(3):
        oc, dc = weighted_restate(s[..., c:c + 1], k, g[:, c:c + 1], o[:, c:c + 1], w)
        assert np.array_equal(oc[..., 0], out[..., c]) and np.array_equal(dc, den)


# ---- the estimator, by hand --------------------------------------------------------------------------------------
# n = 4, X = (1, 1, 3, 3), Y = (1, 1, 5, 5): mx = 2, my = 3, vx = 5 - 4 = 1, vy = 13 - 9 = 4
HAND = [4.0, 8.0, 12.0, 20.0, 52.0, 32.0]


def test_estimator_modes_on_hand_moments():
    m = np.array([[HAND]])
    assert [float(v[0, 0]) for v in estimate(m, NONE)[:2]] == [1.0, 0.0]
    assert [float(v[0, 0]) for v in estimate(m, OFFSET)[:2]] == [1.0, 1.0]
    assert [float(v[0, 0]) for v in estimate(m, GAIN)[:2]] == [1.5, 0.0]
    assert [float(v[0, 0]) for v in estimate(m, LINEAR)[:2]] == [2.0, -1.0]
    for mode in (NONE, OFFSET, GAIN, LINEAR):
        g, o, fb = estimate(m, mode)
        assert g.dtype == np.float32 and o.dtype == np.float32 and not fb.any()


def test_estimator_falls_back_to_identity():
    empty = [0.0] * 6                                   # n = 0
    flat = [4.0, 8.0, 12.0, 16.0, 52.0, 24.0]           # vx = 16 / 4 - 4 = 0
    dark = [4.0, 0.0, 12.0, 20.0, 52.0, 0.0]            # mx = 0
    for mode in (OFFSET, GAIN, LINEAR):
        g, o, fb = estimate(np.array([empty]), mode)
        assert g[0] == 1 and o[0] == 0 and fb[0]
    g, o, fb = estimate(np.array([flat]), LINEAR)
    assert g[0] == 1 and o[0] == 0 and fb[0]
    g, o, fb = estimate(np.array([flat]), GAIN)         # GAIN does not need a variance
    assert g[0] == 1.5 and o[0] == 0 and not fb[0]
    g, o, fb = estimate(np.array([dark]), GAIN)
    assert g[0] == 1 and o[0] == 0 and fb[0]
    g, o, fb = estimate(np.array([dark]), OFFSET)       # OFFSET has no denominator but n
    assert g[0] == 1 and o[0] == 3 and not fb[0]
    # channels fall back one by one
    g, o, fb = estimate(np.array([HAND, empty, flat]), LINEAR)
    assert g.tolist() == [2.0, 1.0, 1.0] and o.tolist() == [-1.0, 0.0, 0.0] and fb.tolist() == [False, True, True]


def test_estimator_rounds_to_f32_once():
    m = np.array([[3.0, 1.0, 2.0, 1.0, 2.0, 1.0]])      # mx = 1/3, my = 2/3
    g, _, _ = estimate(m, GAIN)
    assert g[0] == np.float32((2.0 / 3.0) / (1.0 / 3.0))
    _, o, _ = estimate(m, OFFSET)
    assert o[0] == np.float32(2.0 / 3.0 - 1.0 / 3.0)


def test_ctypes_mirrors():
    p = WeightParameters(normalize=LINEAR, coverage=True, stat_step=2)._c()
    assert (p.normalize, p.coverage, p.stat_step, p.reserved) == (3, 1, 2, 0)
    assert ctypes.sizeof(_ffi.WeightParams) == 16 and ctypes.sizeof(_ffi.FrameWeight) == 40
    d = WeightParameters()._c()
    assert (d.normalize, d.coverage, d.stat_step) == (0, 1, 0)
    for name in ("stk_ecc_match_weighted", "stk_keypoint_match_weighted", "stk_weighted_stack", "stk_overlap_moments"):
        assert name in _ffi.SIGNATURES

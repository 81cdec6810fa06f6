"""Sigma-clipped stacking, CPU side: the numpy restatement of the definition (include/stacker.h, stk_clip_params) that
the GPU tests (test_gpu_clip.py) compare the engine against bit for bit, checked here against hand-computed answers, and
the ctypes mirror of stk_clip_params."""
import ctypes

import numpy as np

from libstacker_rs_amd import SigmaClipParameters, _ffi


def clip_restate(samples, kappa_low: float, kappa_high: float, iterations: int):
    """Kappa-sigma clipping of `samples` (N x ...; the fold's samples in fold order), every operation in f32 and rounded
    on its own, as the engine defines it. Returns (out f32, counts int32)."""
    s = np.asarray(samples, np.float32)
    n = s.shape[0]
    acc = np.zeros(s.shape[1:], np.float32)
    for i in range(n):
        acc = acc + s[i]
    c = acc * np.float32(1.0 / n)                     # the plain mean: sum * (float)(1.0 / N)
    L = np.full(s.shape[1:], -np.inf, np.float32)
    U = np.full(s.shape[1:], np.inf, np.float32)
    kl, kh = np.float32(kappa_low), np.float32(kappa_high)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, iterations + 2):
            k = np.zeros(s.shape[1:], np.int32)
            a = np.zeros(s.shape[1:], np.float32)
            b = np.zeros(s.shape[1:], np.float32)
            for i in range(n):
                d = s[i] - c
                m = (L <= s[i]) & (s[i] <= U)
                k += m.astype(np.int32)
                a = np.where(m, a + d, a)
                b = np.where(m, b + d * d, b)
            kf = k.astype(np.float32)
            if t == iterations + 1:
                return np.where(k > 0, c + a / kf, c).astype(np.float32), k
            upd = k >= 3
            ma = a / kf
            mm = c + ma
            v = b / kf - ma * ma
            sigma = np.sqrt(np.maximum(v, np.float32(0)))
            L = np.where(upd, np.maximum(L, mm - kl * sigma), L)
            U = np.where(upd, np.minimum(U, mm + kh * sigma), U)
            c = np.where(upd, mm, c)


def test_clip_params_struct_matches_header():
    assert ctypes.sizeof(_ffi.ClipParams) == 16
    assert [f for f, _ in _ffi.ClipParams._fields_] == ["kappa_low", "kappa_high", "iterations", "reserved"]
    p = SigmaClipParameters()
    assert (p.kappa_low, p.kappa_high, p.iterations) == (3.0, 3.0, 2)
    c = SigmaClipParameters(1.5, 2.5, 4)._c()
    assert (c.kappa_low, c.kappa_high, c.iterations, c.reserved) == (1.5, 2.5, 4, 0)


def test_restatement_rejects_one_bright_sample():
    s = np.array([0.1] * 7 + [0.9], np.float32).reshape(8, 1)
    out, k = clip_restate(s, 2.0, 2.0, 2)
    assert k[0] == 7
    assert abs(float(out[0]) - 0.1) <= 1e-7
    # the plain mean is off by 1/8 of the outlier's excess
    assert abs(float(s.mean()) - 0.2) <= 1e-7


def test_restatement_rejects_low_and_high_asymmetrically():
    s = np.array([0.5] * 10 + [0.0, 1.0], np.float32).reshape(12, 1)
    out, k = clip_restate(s, 1.0, 1e6, 1)      # only the low side clips
    assert k[0] == 11 and abs(float(out[0]) - (5.0 + 1.0) / 11) <= 1e-6
    out, k = clip_restate(s, 1e6, 1.0, 1)      # only the high side clips
    assert k[0] == 11 and abs(float(out[0]) - 5.0 / 11) <= 1e-6


def test_restatement_leaves_pixels_with_fewer_than_three_samples():
    s = np.array([[0.0, 0.2], [1.0, 0.3]], np.float32)      # two samples per pixel: no statistics, nothing rejected
    out, k = clip_restate(s, 0.1, 0.1, 3)
    assert list(k) == [2, 2]
    assert np.array_equal(out, (s[0] + s[1]) * np.float32(0.5))


def test_restatement_falls_back_to_centre_when_everything_is_rejected():
    s = np.array([0.0, 0.0, 1.0, 1.0], np.float32).reshape(4, 1)
    out, k = clip_restate(s, 1e-3, 1e-3, 1)   # [L, U] shrinks to 0.5 +- 5e-4: no sample left
    assert k[0] == 0
    assert float(out[0]) == 0.5


def test_restatement_with_huge_kappas_is_the_mean():
    rng = np.random.default_rng(3)
    s = rng.random((9, 5, 3), dtype=np.float32)
    out, k = clip_restate(s, 1e30, 1e30, 3)
    assert (k == 9).all()
    acc = np.zeros((5, 3), np.float32)
    for i in range(9):
        acc = acc + s[i]
    assert np.max(np.abs(out - acc * np.float32(1 / 9))) <= 1e-6

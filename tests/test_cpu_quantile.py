"""Median and quantile stacking, CPU side: the numpy restatement of the definition (include/stacker.h,
stk_quantile_params) that the GPU tests (test_gpu_quantile.py) compare the engine against bit for bit, checked here against
hand-computed answers and against numpy.quantile, and the ctypes mirror of stk_quantile_params."""
import ctypes

import numpy as np
import pytest

from libstacker_rs_amd import QuantileParameters, _ffi


def quantile_restate(samples, q: float):
    """The quantile of `samples` (N x ...; the fold's samples in fold order) along axis 0, every operation in f32 and
    rounded on its own, as the engine defines it: numpy.quantile(samples, q, axis=0) (method 'linear') except that g == 0
    returns s_(j) itself, where numpy's lerp gives NaN for a finite s_(j) next to an infinite s_(j+1)."""
    s = np.asarray(samples, np.float32)
    n = s.shape[0]
    vi = np.float32(n - 1) * np.float32(q)
    jf = np.floor(vi)
    g = np.float32(vi - jf)
    j = int(jf)
    srt = np.sort(s, axis=0)                          # NaN last
    lo, hi = srt[j], srt[min(j + 1, n - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        if g == 0:
            out = lo
        elif g >= np.float32(0.5):
            out = hi - d * (np.float32(1) - g)
        else:
            out = lo + d * g
    return np.where(np.isnan(s).any(axis=0), np.float32(np.nan), out).astype(np.float32)


def test_quantile_params_struct_matches_header():
    assert ctypes.sizeof(_ffi.QuantileParams) == 8
    assert [f for f, _ in _ffi.QuantileParams._fields_] == ["quantile", "reserved"]
    assert QuantileParameters().quantile == 0.5
    c = QuantileParameters(0.25)._c()
    assert (c.quantile, c.reserved) == (0.25, 0)
    sig = _ffi.SIGNATURES
    assert {"stk_quantile_stack", "stk_ecc_match_quantile", "stk_keypoint_match_quantile"} <= set(sig)


def _col(v):
    return np.asarray(v, np.float32).reshape(-1, 1)


def test_one_sample_is_itself_at_every_quantile():
    for q in (0.0, 0.1, 0.5, 0.73, 1.0):
        assert quantile_restate(_col([0.3]), q)[0] == np.float32(0.3)


def test_two_samples_median_is_the_midpoint():
    assert quantile_restate(_col([0.25, 0.75]), 0.5)[0] == np.float32(0.5)
    assert quantile_restate(_col([3.0, 1.0]), 0.5)[0] == np.float32(2.0)


def test_odd_count_median_is_the_middle_sample():
    assert quantile_restate(_col([5.0, 1.0, 4.0, 2.0, 3.0]), 0.5)[0] == np.float32(3.0)
    assert quantile_restate(_col([0.9, 0.1, 0.1]), 0.5)[0] == np.float32(0.1)


def test_zero_and_one_are_min_and_max():
    s = _col([0.5, -2.0, 7.0, 1.0])
    assert quantile_restate(s, 0.0)[0] == np.float32(-2.0)
    assert quantile_restate(s, 1.0)[0] == np.float32(7.0)


def test_interpolation_between_neighbours():
    s = _col([0.0, 10.0, 20.0, 30.0, 40.0])
    assert quantile_restate(s, 0.1)[0] == np.float32(4.0)       # vi = 0.4: 0 + 10 * 0.4
    assert quantile_restate(s, 0.875)[0] == np.float32(35.0)    # vi = 3.5: g >= 0.5, 40 - 10 * 0.5


def test_an_infinite_hot_pixel_does_not_poison_the_median():
    assert quantile_restate(_col([1.0, 2.0, np.inf]), 0.5)[0] == np.float32(2.0)
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.quantile(np.array([1.0, 2.0, np.inf], np.float32), 0.5))    # numpy itself: NaN
    assert quantile_restate(_col([-np.inf, 1.0, 2.0]), 0.5)[0] == np.float32(1.0)
    assert quantile_restate(_col([1.0, np.inf, np.inf]), 1.0)[0] == np.inf


def test_nan_propagates():
    s = np.array([[0.1, 0.2], [np.nan, 0.3], [0.5, 0.4]], np.float32)
    for q in (0.0, 0.5, 1.0):
        out = quantile_restate(s, q)
        assert np.isnan(out[0]) and not np.isnan(out[1])


@pytest.mark.parametrize("q", [0.0, 0.1, 0.25, 0.5, 0.73, 0.9, 1.0, 1.0 / 3.0])
def test_restatement_is_numpy_quantile_on_finite_stacks(q):
    rng = np.random.default_rng(int(q * 1000) + 11)
    for n in list(range(1, 14)) + [64, 255, 256, 1024]:
        s = rng.normal(0, 1, (n, 37)).astype(np.float32)
        s[:, :5] = np.round(s[:, :5])                      # ties
        ref = np.quantile(s, q, axis=0)
        assert ref.dtype == np.float32
        np.testing.assert_array_equal(quantile_restate(s, q), ref)

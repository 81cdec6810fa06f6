"""Median / MAD sigma clipping, CPU side: the numpy restatements of the definition (include/stacker.h, "median / MAD
sigma clipping") that the GPU tests (test_gpu_robust_clip.py) compare the engine against bit for bit, checked here against
hand-computed answers, and the ctypes mirrors of the struct and the six entry points."""
import ctypes
import re
from pathlib import Path

import numpy as np

from libstacker_rs_amd import RobustClipParameters, _ffi
from test_cpu_quantile import quantile_restate
from test_cpu_robust import _normalised

F = np.float32
HEADER = Path(__file__).resolve().parent.parent / "include" / "stacker.h"


def _med(values, member):
    """med(K) of the definition per pixel-channel: `values` N x ..., `member` the same shape (K = the members), k = |K|
    per pixel-channel. quantile_restate's formula at q = 0.5 with the pixel-channel's own k; a NaN value ranks above every
    number (numpy's sort puts NaN last, and the non-members, made NaN, behind or among them: indistinguishable). k == 0:
    unspecified (the callers do not use it). Returns (med, k)."""
    v = np.asarray(values, F)
    n = v.shape[0]
    k = member.sum(axis=0)
    srt = np.sort(np.where(member, v, F(np.nan)), axis=0)
    vi = (k - 1).astype(F) * F(0.5)
    jf = np.floor(vi)
    g = (vi - jf).astype(F)
    j = np.clip(jf.astype(np.int64), 0, n - 1)
    j1 = np.clip(np.minimum(j + 1, k - 1), 0, n - 1)
    lo = np.take_along_axis(srt, j[None], axis=0)[0]
    hi = np.take_along_axis(srt, j1[None], axis=0)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        out = np.where(g == 0, lo, hi - d * (F(1) - g))
    return out.astype(F), k


def robust_clip_restate_weighted(samples, participates, g, o, w, kappa_low, kappa_high, sigma_floor, iterations):
    """The median / MAD clip with participation of `samples` (N x ... x C, fold order) with the per-pixel participation
    flags (N x ...), gains and offsets (N x C) and weights (N): (out, counts, kept_weight), each ... x C. Every operation
    in f32 and rounded on its own, in the order the definition states; max and min are C's fmaxf / fminf."""
    u, part, w = _normalised(samples, participates, g, o, w)
    n = u.shape[0]
    kl, kh, fl = F(kappa_low), F(kappa_high), F(sigma_floor)
    shape = u.shape[1:]
    present = np.broadcast_to(part[..., None], u.shape)
    nan = (np.isnan(u) & present).any(axis=0)
    member = present.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c, k = _med(u, member)
        c = np.where(k == 0, F(0), c)
        c = np.where(nan, F(np.nan), c).astype(F)
        L = np.full(shape, -np.inf, F)
        U = np.full(shape, np.inf, F)
        for _ in range(iterations):
            live = ~nan & (k >= 3)                      # k < 3: stop (c, L, U stay); a NaN sample: nothing is clipped
            e = np.abs(u - c).astype(F)
            mad, _k = _med(e, member)
            sigma = np.fmax(F(1.4826) * mad, fl).astype(F)
            L = np.where(live, np.fmax(L, c - kl * sigma), L).astype(F)
            U = np.where(live, np.fmin(U, c + kh * sigma), U).astype(F)
            member = np.where(live, present & (L <= u) & (u <= U), member)
            cn, k = _med(u, member)
            c = np.where(live & (k > 0), cn, c).astype(F)
        # the weighted clip's last pass, the samples in fold order
        k = np.zeros(shape, np.int32)
        sw = np.zeros(shape, F)
        a = np.zeros(shape, F)
        for i in range(n):
            d = u[i] - c
            inn = part[i][..., None] & (L <= u[i]) & (u[i] <= U)
            k = k + inn
            sw = np.where(inn, sw + w[i], sw)
            a = np.where(inn, a + w[i] * d, a)
        out = np.where(k > 0, c + a / np.where(k > 0, sw, F(1)), c).astype(F)
    return out, k.astype(np.int32), sw.astype(F)


def robust_clip_restate(samples, kappa_low, kappa_high, sigma_floor, iterations):
    """The median / MAD clip of `samples` (N x ..., fold order): (out, counts). The participation form with every entry
    participating, weight 1, gain 1 and offset 0: a = a + 1 * d and sw = k exactly, which are the plain form's formulas."""
    s = np.asarray(samples, F)
    n = s.shape[0]
    s2 = s.reshape(n, -1, 1)
    out, k, _ = robust_clip_restate_weighted(s2, np.ones(s2.shape[:-1], bool), np.ones((n, 1), F), np.zeros((n, 1), F), np.ones(n, F),
                                             kappa_low, kappa_high, sigma_floor, iterations)
    return out.reshape(s.shape[1:]), k.reshape(s.shape[1:])


def _col(v):
    return np.asarray(v, F).reshape(len(v), 1)


FLOOR = 0.5 / 255.0


# ---- 1. hand-computed answers -------------------------------------------------------------------------------------
def test_med_is_the_quantile_restatement_at_full_membership():
    rng = np.random.default_rng(1)
    for n in list(range(1, 14)) + [64, 65]:
        s = rng.normal(0, 1, (n, 40)).astype(F)
        s[:, :6] = np.round(s[:, :6])
        m, k = _med(s, np.ones(s.shape, bool))
        np.testing.assert_array_equal(m, quantile_restate(s, 0.5))
        assert (k == n).all()


def test_one_outlier_among_seven_equal_samples_is_rejected():
    v = F(102) * F(1.0 / 255.0)
    out, k = robust_clip_restate(_col([v] * 7 + [0.9]), 3, 3, FLOOR, 2)
    assert out[0] == v and k[0] == 7                          # MAD = 0: sigma = the floor; U = v + 1.5 / 255
    # the plain clip's test cannot reject it: |0.9 - mean| = 7/8 (0.9 - v) < 3 std = 3 sqrt(7)/8 (0.9 - v)
    s = np.array([v] * 7 + [0.9], np.float64)
    assert abs(0.9 - s.mean()) < 3 * s.std()


def test_asymmetric_kappas():
    s = _col([1, 2, 3, 4, 5, 6, 7, -20, 30])                   # c = 4; e sorted 0 1 1 2 2 3 3 24 26: mad = 2, sigma = 2.9652
    out, k = robust_clip_restate(s, 3, 1e6, 0, 1)              # L = 4 - 8.9: -20 out; 30 stays
    assert k[0] == 8 and abs(float(out[0]) - 58.0 / 8) <= 1e-6
    out, k = robust_clip_restate(s, 1e6, 3, 0, 1)              # U = 4 + 8.9: 30 out; -20 stays
    assert k[0] == 8 and abs(float(out[0]) - 8.0 / 8) <= 1e-6
    out, k = robust_clip_restate(s, 3, 3, 0, 3)                # both out; then 1 .. 7: mad = 2 again, nothing more
    assert k[0] == 7 and out[0] == F(4)


def test_fewer_than_three_samples_are_left_alone():
    out, k = robust_clip_restate(_col([0, 1]), 0.01, 0.01, 0, 5)
    assert out[0] == F(0.5) and k[0] == 2
    out, k = robust_clip_restate(_col([0.25]), 0.01, 0.01, 0, 5)
    assert out[0] == F(0.25) and k[0] == 1
    # three samples are clipped; the two that stay are then left alone, whatever their spread
    out, k = robust_clip_restate(_col([0, 1, 100]), 2, 2, 0, 5)         # c = 1, mad = 1: U = 3.97 -> {0, 1}: c = 0.5
    assert out[0] == F(0.5) and k[0] == 2


def test_zero_mad_keeps_the_majority_value_and_the_floor_keeps_its_neighbours():
    v, q = F(128) * F(1.0 / 255.0), F(1.0 / 255.0)
    s = _col([v] * 5 + [v + q, v - q, 0.9])
    out, k = robust_clip_restate(s, 3, 3, 0, 2)                # sigma = 0: L = U = v
    assert out[0] == v and k[0] == 5
    out, k = robust_clip_restate(s, 3, 3, FLOOR, 2)            # sigma = 0.5 / 255: +-1.5 / 255 keeps v +- 1 / 255
    assert k[0] == 7 and abs(float(out[0]) - float(v)) <= 1e-7


def test_even_k_takes_the_midpoint_and_may_keep_nothing():
    out, k = robust_clip_restate(_col([1, 2, 3, 4]), 1e6, 1e6, 0, 1)
    assert out[0] == F(2.5) and k[0] == 4
    # c = 1.5, every deviation 0.5: sigma = 0.7413; kappa 0.5 -> [1.13, 1.87] holds no sample: c stays, counts 0
    out, k = robust_clip_restate(_col([1, 1, 2, 2]), 0.5, 0.5, 0, 3)
    assert out[0] == F(1.5) and k[0] == 0


def test_one_infinite_sample_is_rejected():
    for bad in (np.inf, -np.inf):
        out, k = robust_clip_restate(_col(list(range(1, 11)) + [bad]), 3, 3, 0, 2)
        assert k[0] == 10 and out[0] == F(5.5)


def test_nan_propagates_and_an_infinite_median_gives_nan():
    out, k = robust_clip_restate(_col([1, 2, np.nan, 3, 4]), 3, 3, FLOOR, 2)
    assert np.isnan(out[0]) and k[0] == 4                      # nothing is clipped: the four numbers pass [-inf, +inf]
    out, k = robust_clip_restate(_col([np.nan] * 3), 3, 3, FLOOR, 2)
    assert np.isnan(out[0]) and k[0] == 0
    # six +inf among eleven: c = inf, deviations inf (finite samples) and NaN (inf - inf): mad = NaN -> sigma = the floor,
    # L = U = inf keeps the six, and their sum of inf - inf is NaN
    out, k = robust_clip_restate(_col([np.inf] * 6 + [1, 2, 3, 4, 5]), 3, 3, FLOOR, 2)
    assert np.isnan(out[0]) and k[0] == 6
    # three of six: the midpoint of 3 and inf is inf - inf * 0.5 = NaN with no NaN sample: nothing is ever clipped
    out, k = robust_clip_restate(_col([np.inf] * 3 + [1, 2, 3]), 3, 3, FLOOR, 2)
    assert np.isnan(out[0]) and k[0] == 6


def test_huge_kappas_give_the_mean_about_the_median():
    rng = np.random.default_rng(3)
    s = rng.normal(0.5, 0.1, (9, 200)).astype(F)
    out, k = robust_clip_restate(s, 1e30, 1e30, 0, 3)
    c = quantile_restate(s, 0.5)
    a = np.zeros(200, F)
    for i in range(9):
        a = a + (s[i] - c)
    np.testing.assert_array_equal(out, c + a / F(9))
    assert (k == 9).all()
    assert np.abs(out - s.mean(axis=0)).max() <= 2e-7


# ---- 2. the participation form ------------------------------------------------------------------------------------------
def _ones(n):
    return np.ones((n, 1), F), np.zeros((n, 1), F)


def test_absent_and_zero_weight_entries_are_no_samples():
    s = np.asarray([1, 100, 2, 3, 50], F).reshape(5, 1, 1)
    g, o = _ones(5)
    part = np.ones((5, 1), bool)
    part[4] = False
    out, k, sw = robust_clip_restate_weighted(s, part, g, o, [1, 0, 2, 1, 1], 1e6, 1e6, 0, 1)
    # samples 1, 2, 3 with weights 1, 2, 1: c = 2, a = -1 + 0 + 1
    assert k[0, 0] == 3 and sw[0, 0] == F(4) and out[0, 0] == F(2)
    # the weights enter the final mean only: 1, 2, 9 -> c = 2, huge kappas: 2 + (1 * -1 + 1 * 0 + 2 * 7) / 4
    s = np.asarray([1, 2, 9], F).reshape(3, 1, 1)
    g, o = _ones(3)
    out, k, sw = robust_clip_restate_weighted(s, np.ones((3, 1), bool), g, o, [1, 1, 2], 1e6, 1e6, 0, 1)
    assert k[0, 0] == 3 and sw[0, 0] == F(4) and out[0, 0] == F(2) + F(13) / F(4)


def test_a_pixel_nobody_covers_gives_zeros():
    s = np.full((4, 2, 1), 0.5, F)
    part = np.ones((4, 2), bool)
    part[:, 1] = False
    g, o = _ones(4)
    out, k, sw = robust_clip_restate_weighted(s, part, g, o, np.ones(4, F), 3, 3, FLOOR, 2)
    assert (out[1, 0], k[1, 0], sw[1, 0]) == (0, 0, 0) and (out[0, 0], k[0, 0], sw[0, 0]) == (F(0.5), 4, 4)


def test_gains_and_offsets_are_applied_before_anything_is_ranked():
    s = np.asarray([0.5, 0.25, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5], F).reshape(8, 1, 1)
    g = np.ones((8, 1), F)
    g[1] = 2                                                   # frame 1 is half as bright: after its gain it is no outlier
    out, k, sw = robust_clip_restate_weighted(s, np.ones((8, 1), bool), g, np.zeros((8, 1), F), np.ones(8, F), 3, 3, FLOOR, 2)
    assert k[0, 0] == 8 and out[0, 0] == F(0.5)
    out, k, sw = robust_clip_restate_weighted(s, np.ones((8, 1), bool), np.ones((8, 1), F), np.zeros((8, 1), F), np.ones(8, F), 3, 3,
                                              FLOOR, 2)
    assert k[0, 0] == 7 and out[0, 0] == F(0.5)


# ---- 3. the C ABI mirrors ---------------------------------------------------------------------------------------------
NEW = ["stk_robust_clip_stack", "stk_ecc_match_robust_clipped", "stk_keypoint_match_robust_clipped",
       "stk_robust_clip_stack_weighted", "stk_ecc_match_robust_clipped_weighted", "stk_keypoint_match_robust_clipped_weighted"]


def test_robust_clip_params_struct_matches_header():
    assert ctypes.sizeof(_ffi.RobustClipParams) == 16
    assert [f for f, _ in _ffi.RobustClipParams._fields_] == ["kappa_low", "kappa_high", "sigma_floor", "iterations"]
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*stk_robust_clip_params\s*;", text).group(1)
    fields = []
    for decl in body.split(";"):
        toks = decl.replace(",", " ").split()
        if toks:
            fields += [(toks[0], name) for name in toks[1:]]
    assert fields == [("float", "kappa_low"), ("float", "kappa_high"), ("float", "sigma_floor"), ("int32_t", "iterations")]
    p = RobustClipParameters()
    assert (p.kappa_low, p.kappa_high, p.sigma_floor, p.iterations) == (3.0, 3.0, 0.5 / 255.0, 2)
    c = RobustClipParameters(1.5, 2.5, 0.25, 4)._c()
    assert (c.kappa_low, c.kappa_high, c.sigma_floor, c.iterations) == (1.5, 2.5, 0.25, 4)


def test_ctypes_table_holds_the_new_symbols():
    sig = _ffi.SIGNATURES
    assert set(NEW) <= set(sig)
    # the arguments mirror the clip forms', with the new struct in place of stk_clip_params
    for name in NEW:
        old = sig[name.replace("robust_clipped", "clipped").replace("robust_clip", "clip")]
        assert sig[name][0] is _ffi.c_status
        assert [ctypes.POINTER(_ffi.RobustClipParams) if a is ctypes.POINTER(_ffi.ClipParams) else a for a in old[1]] == sig[name][1]
    lib = _ffi.load()
    for name in NEW:
        assert getattr(lib, name) is not None
    import libstacker_rs_amd as ls
    for m in ("robust_clip_stack", "ecc_match_robust_clipped", "keypoint_match_robust_clipped", "robust_clip_stack_weighted",
              "ecc_match_robust_clipped_weighted", "keypoint_match_robust_clipped_weighted"):
        assert callable(getattr(ls.Stacker, m))

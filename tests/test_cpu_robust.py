"""Normalised, coverage-aware sigma-clip and quantile stacking, CPU side: the numpy restatements of the definitions
(include/stacker.h, "normalised, coverage-aware sigma-clip and quantile stacking") that the GPU tests
(test_gpu_robust.py) compare the engine against bit for bit, checked here against hand-computed answers, constant and
dyadic ground truths and numpy.nanquantile, and the ctypes mirrors of the six entry points."""
import ctypes as C

import numpy as np
import pytest

from libstacker_rs_amd import _ffi
from test_cpu_quantile import quantile_restate

F = np.float32


def _normalised(samples, participates, g, o, w):
    s = np.asarray(samples, F)
    n, cn = s.shape[0], s.shape[-1]
    g = np.asarray(g, F).reshape(n, cn)
    o = np.asarray(o, F).reshape(n, cn)
    w = np.asarray(w, F).reshape(n)
    part = np.asarray(participates, bool).reshape(s.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.stack([s[i] * g[i] + o[i] for i in range(n)]).astype(F)
    part = part & (w > 0).reshape((n,) + (1,) * (part.ndim - 1))
    return u, part, w


def robust_clip_restate(samples, participates, g, o, w, kappa_low, kappa_high, T):
    """The normalised, coverage-aware clip of `samples` (N x ... x C, fold order) with the per-pixel participation flags
    (N x ...), gains and offsets (N x C) and weights (N): (out, counts, kept_weight), each ... x C. Every operation in
    f32 and rounded on its own, in the order the definition states; max and min are C's fmaxf / fminf (a NaN operand
    gives the other one), as the engine computes them."""
    u, part, w = _normalised(samples, participates, g, o, w)
    n = u.shape[0]
    kl, kh = F(kappa_low), F(kappa_high)
    shape = u.shape[1:]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sw = np.zeros(shape, F)
        a = np.zeros(shape, F)
        for i in range(n):
            p = part[i][..., None]
            sw = np.where(p, sw + w[i], sw)
            a = np.where(p, a + w[i] * u[i], a)
        c = np.where(sw > 0, a / np.where(sw > 0, sw, F(1)), F(0)).astype(F)
        L = np.full(shape, -np.inf, F)
        U = np.full(shape, np.inf, F)
        for t in range(1, T + 2):
            k = np.zeros(shape, np.int32)
            sw = np.zeros(shape, F)
            a = np.zeros(shape, F)
            b = np.zeros(shape, F)
            for i in range(n):
                d = u[i] - c
                inn = part[i][..., None] & (L <= u[i]) & (u[i] <= U)
                k = k + inn
                sw = np.where(inn, sw + w[i], sw)
                a = np.where(inn, a + w[i] * d, a)
                b = np.where(inn, b + w[i] * (d * d), b)
            safe = np.where(k > 0, sw, F(1))
            if t == T + 1:
                out = np.where(k > 0, c + a / safe, c).astype(F)
                return out, k.astype(np.int32), sw.astype(F)
            ma = a / safe
            m = c + ma
            v = b / safe - ma * ma
            sigma = np.sqrt(np.fmax(v, F(0)))
            upd = k >= 3
            L = np.where(upd, np.fmax(L, m - kl * sigma), L).astype(F)
            U = np.where(upd, np.fmin(U, m + kh * sigma), U).astype(F)
            c = np.where(upd, m, c).astype(F)


def robust_quantile_restate(samples, participates, g, o, w, q):
    """The normalised, coverage-aware quantile: (out ... x C, counts ... = N_p per pixel)."""
    u, part, w = _normalised(samples, participates, g, o, w)
    n = u.shape[0]
    n_p = part.sum(axis=0).astype(np.int32)
    present = np.broadcast_to(part[..., None], u.shape)
    nan = (np.isnan(u) & present).any(axis=0)
    srt = np.sort(np.where(present, u, F(np.nan)), axis=0)               # absent entries (and NaN) last
    npc = np.broadcast_to(n_p[..., None], u.shape[1:])
    vi = (npc - 1).astype(F) * F(q)
    jf = np.floor(vi)
    gq = (vi - jf).astype(F)
    j = np.clip(jf.astype(np.int64), 0, n - 1)
    j1 = np.clip(np.minimum(j + 1, npc - 1), 0, n - 1)
    lo = np.take_along_axis(srt, j[None], axis=0)[0]
    hi = np.take_along_axis(srt, j1[None], axis=0)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        out = np.where(gq == 0, lo, np.where(gq >= F(0.5), hi - d * (F(1) - gq), lo + d * gq))
    out = np.where(nan, F(np.nan), out)
    out = np.where(npc == 0, F(0), out)
    return out.astype(F), n_p


def dyadic_stack(n=12, h=24, w=40, trail_frame=5):
    """Frames scene + b_i with scene and b_i multiples of 2^-10 and a trail of 2^-5 in one frame: (scene h x w x 1,
    b, trail value, trail mask h x w). The b_i are evenly spaced (no frame is an outlier at kappa = 2) with a standard
    deviation above the trail; the trail frame's own offset is the one nearest 0."""
    rng = np.random.default_rng(12)
    scene = (rng.integers(256, 769, (h, w, 1)) * 2.0 ** -10).astype(F)              # 0.25 .. 0.75
    p = np.concatenate([[5], rng.permutation([v for v in range(n) if v != 5])])
    p[[0, trail_frame]] = p[[trail_frame, 0]]
    b = ((2 * p - (n - 1)) * 5 * 2.0 ** -10).astype(F)
    trail = F(2.0 ** -5)
    assert np.std(b.astype(np.float64)) > trail
    mask = np.zeros((h, w), bool)
    mask[h // 2, 8:w - 8] = True
    return scene, b, trail, mask


def _col(v):
    return np.asarray(v, F).reshape(len(v), 1, 1)


def _ones(n):
    return np.ones((n, 1), F), np.zeros((n, 1), F)


# ---- 1. hand-computed cases -------------------------------------------------------------------------------------
def test_a_bright_sample_is_rejected_with_unequal_weights():
    # u = 1, 1, 1, 1, 9 with weights 1, 2, 1, 2, 2: centre = (1 + 2 + 1 + 2 + 18) / 8 = 3; pass 1: d = -2 x 4, 6;
    # a = -2 - 4 - 2 - 4 + 12 = 0, b = 4 + 8 + 4 + 8 + 72 = 96; m = 3, v = 12, sigma = sqrt(12) = 3.46; kappa 1.5: U = 8.2
    # -> 9 is out; pass 2 (last): k = 4, sw = 6, a = -12, out = 3 - 2 = 1
    g, o = _ones(5)
    out, k, sw = robust_clip_restate(_col([1, 1, 1, 1, 9]), np.ones((5, 1), bool), g, o, [1, 2, 1, 2, 2], 1.5, 1.5, 1)
    assert out[0, 0] == F(1) and k[0, 0] == 4 and sw[0, 0] == F(6)
    # gains and offsets are applied before anything is compared: s = 0.5 g + o
    out, k, sw = robust_clip_restate(_col([0.5] * 4 + [4.5]), np.ones((5, 1), bool), np.full((5, 1), 2, F), np.zeros((5, 1), F),
                                     [1, 2, 1, 2, 2], 1.5, 1.5, 1)
    assert out[0, 0] == F(1) and k[0, 0] == 4 and sw[0, 0] == F(6)


def test_zero_one_and_two_participating_entries():
    s = np.zeros((3, 3, 1), F)
    s[:, :, 0] = [[0.5, 0.25, 0.75], [0.125, 0.5, 0.25], [0.875, 0.75, 0.5]]
    part = np.array([[False, True, True], [False, False, True], [False, False, False]])     # pixel 0: none, 1: one, 2: two
    g, o = _ones(3)
    out, k, sw = robust_clip_restate(s, part, g, o, [1, 3, 1], 2, 2, 2)
    assert list(k[:, 0]) == [0, 1, 2] and list(sw[:, 0]) == [0, 1, 4]
    assert out[0, 0] == 0 and out[1, 0] == F(0.25) and out[2, 0] == F((0.75 + 3 * 0.25) / 4)
    for q in (0.5, 0.3):
        qo, n_p = robust_quantile_restate(s, part, g, o, [1, 3, 1], q)
        assert list(n_p) == [0, 1, 2]
        assert qo[0, 0] == 0 and qo[1, 0] == F(0.25)
    assert robust_quantile_restate(s, part, g, o, [1, 3, 1], 0.5)[0][2, 0] == F(0.5)        # midpoint of 0.25, 0.75
    assert robust_quantile_restate(s, part, g, o, [1, 3, 1], 0.3)[0][2, 0] == F(0.25) + F(0.5) * F(0.3)


def test_a_zero_weight_entry_is_no_sample():
    g, o = _ones(4)
    s = _col([1, 100, 2, 3])
    out, k, sw = robust_clip_restate(s, np.ones((4, 1), bool), g, o, [1, 0, 1, 1], 3, 3, 1)
    assert k[0, 0] == 3 and sw[0, 0] == F(3) and out[0, 0] == F(2)
    qo, n_p = robust_quantile_restate(s, np.ones((4, 1), bool), g, o, [1, 0, 1, 1], 0.5)
    assert n_p[0] == 3 and qo[0, 0] == F(2)
    qo, n_p = robust_quantile_restate(s, np.ones((4, 1), bool), g, o, [1, 0, 1, 1], 1.0)
    assert qo[0, 0] == F(3)


def test_the_rank_follows_the_pixels_own_count():
    s = np.zeros((5, 2, 1), F)
    s[:, 0, 0] = [10, 50, 20, 40, 30]            # pixel 0: all five
    s[:, 1, 0] = [10, 50, 20, 40, 30]            # pixel 1: entries 0, 1, 2 only -> 10, 20, 50
    part = np.ones((5, 2), bool)
    part[3:, 1] = False
    g, o = _ones(5)
    w = np.ones(5, F)
    q5, n_p = robust_quantile_restate(s, part, g, o, w, 0.5)
    assert list(n_p) == [5, 3] and q5[0, 0] == F(30) and q5[1, 0] == F(20)
    q3, _ = robust_quantile_restate(s, part, g, o, w, 0.3)
    # pixel 0: vi = 4 * 0.3f = 1.2 -> 20 + 10 * 0.2; pixel 1: vi = 2 * 0.3f = 0.6 -> g >= 0.5: 20 - 10 * (1 - 0.6)
    vi0, vi1 = F(4) * F(0.3), F(2) * F(0.3)
    assert q3[0, 0] == F(20) + F(10) * F(vi0 - F(1))
    assert q3[1, 0] == F(20) - F(10) * (F(1) - F(vi1 - F(0)))


def test_a_participating_nan_makes_the_quantile_nan_and_an_absent_one_does_not():
    s = _col([1, np.nan, 3])
    g, o = _ones(3)
    part = np.ones((3, 1), bool)
    assert np.isnan(robust_quantile_restate(s, part, g, o, [1, 1, 1], 0.5)[0][0, 0])
    part[1] = False
    assert robust_quantile_restate(s, part, g, o, [1, 1, 1], 0.5)[0][0, 0] == F(2)
    assert robust_quantile_restate(s, np.ones((3, 1), bool), g, o, [1, 0, 1], 0.5)[0][0, 0] == F(2)


# ---- 2. constant scene: exact, whatever the participation and the weights ---------------------------------------------
def test_a_constant_scene_comes_back_exactly():
    rng = np.random.default_rng(2)
    for trial in range(60):
        n = int(rng.integers(1, 40))
        T = int(rng.integers(1, 4))
        v = F(rng.integers(1, 256)) * F(1.0 / 255.0)
        s = np.full((n, 50, 1), v, F)
        part = rng.random((n, 50)) < rng.uniform(0.1, 0.9)
        w = rng.uniform(0.05, 3.0, n).astype(F)
        g, o = _ones(n)
        out, k, sw = robust_clip_restate(s, part, g, o, w, 2.0, 2.5, T)
        assert (k[..., 0] == part.sum(axis=0)).all()
        assert (out[k > 0] == v).all() and (out[k == 0] == 0).all() and (sw[k == 0] == 0).all()
        for q in (0.5, 0.3):
            qo, n_p = robust_quantile_restate(s, part, g, o, w, q)
            assert (n_p == part.sum(axis=0)).all()
            assert (qo[n_p > 0] == v).all() and (qo[n_p == 0] == 0).all()


# ---- 3. the masked quantile is numpy.nanquantile, and the plain restatement when everything participates ---------------
@pytest.mark.parametrize("q", [0.0, 0.1, 0.25, 0.5, 0.73, 0.9, 1.0, 1.0 / 3.0])
def test_masked_quantile_is_numpy_nanquantile(q):
    rng = np.random.default_rng(int(q * 1000) + 23)
    for n in list(range(1, 14)) + [64, 255, 256]:
        s = rng.normal(0, 1, (n, 37, 1)).astype(F)
        s[:, :5] = np.round(s[:, :5])                      # ties
        part = rng.random((n, 37)) < 0.6
        part[:, 0] = True
        part[0, :] = True                                  # numpy.nanquantile of an all-NaN column warns; N_p = 0 is case 1's
        g, o = _ones(n)
        out, n_p = robust_quantile_restate(s, part, g, o, np.ones(n, F), q)
        ref = np.nanquantile(np.where(part[..., None], s, F(np.nan)), q, axis=0, method="linear")
        assert ref.dtype == F
        np.testing.assert_array_equal(out, ref)
        assert (n_p == part.sum(axis=0)).all()
        everything, n_all = robust_quantile_restate(s, np.ones((n, 37), bool), g, o, np.ones(n, F), q)
        np.testing.assert_array_equal(everything, quantile_restate(s, q))
        assert (n_all == n).all()


# ---- 4. dyadic ground truth: frames at different levels, a trail fainter than their spread ---------------------------
def test_normalisation_lets_the_clip_see_a_faint_trail():
    n, t = 12, 5
    scene, b, trail, mask = dyadic_stack(n, trail_frame=t)
    s = np.stack([scene + b[i] for i in range(n)]).astype(F)
    s[t][mask] += trail
    part = np.ones((n,) + scene.shape[:2], bool)
    g = np.ones((n, 1), F)
    w = np.ones(n, F)
    out, k, sw = robust_clip_restate(s, part, g, -b.reshape(n, 1), w, 2.0, 2.0, 2)
    assert np.array_equal(out, scene)
    assert (k[mask] == n - 1).all() and (k[~mask] == n).all() and np.array_equal(sw, k.astype(F))
    med, n_p = robust_quantile_restate(s, part, g, -b.reshape(n, 1), w, 0.5)
    assert np.array_equal(med, scene) and (n_p == n).all()
    # without the normalisation the frame levels are the scatter: the trail is kept and the result is off
    raw, rk, _ = robust_clip_restate(s, part, g, np.zeros((n, 1), F), w, 2.0, 2.0, 2)
    assert (rk[mask] == n).all()
    err = np.abs(raw - scene)[mask].max()
    print("un-normalised clip on the trail: kept", int(rk[mask].min()), "of", n, "max error", err)
    assert err > 1e-3


# ---- 5. the C ABI mirrors ------------------------------------------------------------------------------------------
NEW = ["stk_clip_stack_weighted", "stk_quantile_stack_weighted", "stk_ecc_match_clipped_weighted",
       "stk_keypoint_match_clipped_weighted", "stk_ecc_match_quantile_weighted", "stk_keypoint_match_quantile_weighted"]


def test_ctypes_table_holds_the_new_symbols():
    sig = _ffi.SIGNATURES
    assert set(NEW) <= set(sig)
    assert len(sig["stk_clip_stack_weighted"][1]) == 14 and len(sig["stk_quantile_stack_weighted"][1]) == 13
    assert len(sig["stk_ecc_match_clipped_weighted"][1]) == 12 and len(sig["stk_keypoint_match_clipped_weighted"][1]) == 13
    assert len(sig["stk_ecc_match_quantile_weighted"][1]) == 11 and len(sig["stk_keypoint_match_quantile_weighted"][1]) == 12
    for name in NEW:
        assert sig[name][0] is _ffi.c_status
        assert C.POINTER(_ffi.FrameWeight) in sig[name][1]
    lib = _ffi.load()
    for name in NEW:
        assert getattr(lib, name) is not None
    import libstacker_rs_amd as ls
    for m in ("clip_stack_weighted", "quantile_stack_weighted", "ecc_match_clipped_weighted", "keypoint_match_clipped_weighted",
              "ecc_match_quantile_weighted", "keypoint_match_quantile_weighted"):
        assert callable(getattr(ls.Stacker, m))

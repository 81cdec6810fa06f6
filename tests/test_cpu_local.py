"""Per-pixel weight maps and local-sharpness stacking, CPU side: the numpy restatements of the definition
(include/stacker.h, stk_local_params) that the GPU tests (test_gpu_local.py) compare the engine against bit for bit —
`local_sharpness_restate` (the quality map, integers) and `local_weighted_restate` (the fold, f32) — checked here against
closed forms and a brute-force loop, the quality stack that shows what the combine buys, and the ctypes mirrors."""
import ctypes

import numpy as np
import pytest

from libstacker_rs_amd import LocalParameters, _ffi


def r101(p, n):
    """OpenCV's borderInterpolate(p, n, BORDER_REFLECT_101) on an index array, iterated until every index is inside."""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))
    return p


def grey_restate(frame):
    """stk_grey's integer grey of an 8-bit frame (H x W, or H x W x 1 / 3 / 4 in BGR(A) order), as int64."""
    f = np.asarray(frame)
    assert f.dtype == np.uint8
    if f.ndim == 2 or f.shape[2] == 1:
        return f.reshape(f.shape[0], f.shape[1]).astype(np.int64)
    b, g, r = (f[..., c].astype(np.int64) for c in range(3))
    return (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15


def ml_restate(frame, threshold):
    """The thresholded modified Laplacian of every pixel, int64."""
    g = grey_restate(frame)
    h, w = g.shape
    xs, ys = np.arange(w), np.arange(h)
    lx = 2 * g - g[:, r101(xs - 1, w)] - g[:, r101(xs + 1, w)]
    ly = 2 * g - g[r101(ys - 1, h), :] - g[r101(ys + 1, h), :]
    ml = np.abs(lx) + np.abs(ly)
    return np.where(ml >= threshold, ml, 0)


def local_sharpness_restate(frame, radius, threshold):
    """Q of the definition: the sum of mlT over the (2 radius + 1)^2 window with both indices reflected (explicit index
    arrays, not np.pad, which differs on one-pixel axes); int64 throughout, cast to f32 at the end (exact: < 2^24)."""
    m = ml_restate(frame, threshold)
    h, w = m.shape
    xs, ys = np.arange(w), np.arange(h)
    rows = np.zeros_like(m)
    for d in range(-radius, radius + 1):
        rows = rows + m[:, r101(xs + d, w)]
    q = np.zeros_like(m)
    for d in range(-radius, radius + 1):
        q = q + rows[r101(ys + d, h), :]
    assert q.dtype == np.int64 and q.max(initial=0) < 1 << 24
    return q.astype(np.float32)


def local_weighted_restate(samples, kappa, omega, g, o, w, floor, power):
    """The local-weighted fold of `samples` (N x H x W x C, the fold's samples in fold order) with the coverage weights
    `kappa` and the sampled weight maps `omega` (N x H x W each), per-entry gains and offsets (N x C) and weights (N):
    every operation in f32 and rounded on its own, as the engine defines it. Returns (out H x W x C f32, den H x W f32)."""
    s = np.asarray(samples, np.float32)
    k = np.asarray(kappa, np.float32)
    om = np.asarray(omega, np.float32)
    g = np.asarray(g, np.float32).reshape(s.shape[0], -1)
    o = np.asarray(o, np.float32).reshape(s.shape[0], -1)
    w = np.asarray(w, np.float32).reshape(-1)
    floor = np.float32(floor)
    num = np.zeros(s.shape[1:], np.float32)
    den = np.zeros(s.shape[1:3], np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(s.shape[0]):
            b = om[i] + floor * k[i]
            u = b
            for _ in range(int(power) - 1):
                u = u * b
            W = w[i] * u
            v = s[i] * g[i][None, None, :] + o[i][None, None, :] * k[i][..., None]
            num = num + W[..., None] * v
            den = den + W * k[i]
            assert b.dtype == np.float32 and u.dtype == np.float32 and W.dtype == np.float32 and v.dtype == np.float32
        out = np.where(den[..., None] > 0, num / den[..., None], np.float32(0)).astype(np.float32)
    assert num.dtype == np.float32 and den.dtype == np.float32
    return out, den


# ---- the quality stack: 8 frames, each sharp in its own vertical band ------------------------------------------------
def _gauss(a, sigma, axes=(0, 1)):
    """Gaussian blur (reflected border, taps to 4 sigma) along the given axes, f64."""
    r = int(np.ceil(4 * sigma))
    t = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    t /= t.sum()
    out = np.asarray(a, np.float64)
    for ax in axes:
        idx = r101(np.arange(-r, out.shape[ax] + r), out.shape[ax])
        padded = np.take(out, idx, axis=ax)
        out = sum(t[k] * np.take(padded, np.arange(k, k + out.shape[ax]), axis=ax) for k in range(2 * r + 1))
    return out


QS = dict(h=96, w=128, n=8, blur=2.5, mask_blur=3.0, seed=5, noise=2.0, radius=4, threshold=16, power=2, floor=1.0, margin=8)


def quality_stack(noise=QS["noise"]):
    """(scene H x W f64 in grey levels, frames: n x H x W u8). Frame i is the scene inside vertical band i and the scene
    blurred with sigma 2.5 px elsewhere (the band's mask blurred with sigma 3 along x), plus Gaussian noise, rounded."""
    rng = np.random.default_rng(QS["seed"])
    h, w, n = QS["h"], QS["w"], QS["n"]
    scene = _gauss(rng.random((h, w)), 1.0)
    scene = 128.0 + (scene - scene.mean()) / scene.std() * 40.0
    soft = _gauss(scene, QS["blur"])
    frames = []
    for i in range(n):
        mask = np.zeros((h, w))
        mask[:, i * w // n:(i + 1) * w // n] = 1.0
        mask = _gauss(mask, QS["mask_blur"], axes=(1,))
        f = mask * scene + (1.0 - mask) * soft + rng.normal(0.0, noise, (h, w))
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return scene, np.stack(frames)


def interior_rms(img, scene):
    m = QS["margin"]
    d = np.asarray(img, np.float64)[m:-m, m:-m] - scene[m:-m, m:-m]
    return float(np.sqrt((d * d).mean()))


def quality_stack_restated(frames):
    """The definition on the quality stack under identity warps (kappa = 1, omega = Q): (local, plain mean), grey levels."""
    n = len(frames)
    s = (frames.astype(np.float32) * np.float32(1.0 / 255.0))[..., None]
    q = np.stack([local_sharpness_restate(f, QS["radius"], QS["threshold"]) for f in frames])
    one = np.ones((n, 1), np.float32)
    out, _ = local_weighted_restate(s, np.ones_like(q), q, one, 0 * one, np.ones(n, np.float32), QS["floor"], QS["power"])
    mean, _ = local_weighted_restate(s, np.ones_like(q), 0 * q, one, 0 * one, np.ones(n, np.float32), 1.0, 1)
    return out[..., 0] * 255.0, mean[..., 0] * 255.0


def test_quality_stack_local_beats_the_mean():
    scene, frames = quality_stack()
    local, mean = quality_stack_restated(frames)
    r_local, r_mean = interior_rms(local, scene), interior_rms(mean, scene)
    print("quality stack: RMS local", r_local, "RMS mean", r_mean, "ratio", r_local / r_mean)
    # the issue's bound: its f64 prototype measured 0.31; the margin covers f32 and a generator that is not the prototype's
    assert r_local <= 0.45 * r_mean


# ---- the map ------------------------------------------------------------------------------------------------------------
def test_constant_frame_has_no_quality():
    for shape in ((7, 9), (1, 5), (3, 1), (6, 5, 3)):
        assert (local_sharpness_restate(np.full(shape, 77, np.uint8), 4, 0) == 0).all()


def test_single_bright_pixel_closed_form():
    a = 50
    f = np.zeros((21, 23), np.uint8)
    f[10, 11] = a
    m = ml_restate(f, 0)
    expect = np.zeros((21, 23), np.int64)
    expect[10, 11] = 4 * a
    expect[9, 11] = expect[11, 11] = expect[10, 10] = expect[10, 12] = a
    assert np.array_equal(m, expect)
    q1 = local_sharpness_restate(f, 1, 0)
    assert q1[10, 11] == 8 * a and q1[9, 10] == 6 * a and q1[10, 13] == a and q1[8, 11] == a and q1[10, 14] == 0
    q4 = local_sharpness_restate(f, 4, 0)
    assert (q4[7:14, 8:15] == 8 * a).all() and q4[6, 11] == 7 * a and q4[5, 11] == a and q4[4, 11] == 0 and q4[6, 6] == a
    # a threshold above a and at most 4a keeps the centre only
    assert local_sharpness_restate(f, 1, a + 1)[10, 11] == 4 * a and local_sharpness_restate(f, 1, 4 * a + 1).max() == 0


def _brute(frame, radius, threshold):
    g = grey_restate(frame)
    h, w = g.shape

    def rf(p, n):
        if n == 1:
            return 0
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * n - 2 - p
        return p

    def mlt(x, y):
        v = abs(2 * g[y, x] - g[y, rf(x - 1, w)] - g[y, rf(x + 1, w)]) + abs(2 * g[y, x] - g[rf(y - 1, h), x] - g[rf(y + 1, h), x])
        return v if v >= threshold else 0

    q = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            q[y, x] = sum(mlt(rf(x + dx, w), rf(y + dy, h)) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1))
    return q.astype(np.float32)


@pytest.mark.parametrize("shape", [(7, 9), (1, 5), (3, 1)])
@pytest.mark.parametrize("radius", [1, 4, 15])
def test_box_sum_matches_brute_force(shape, radius):
    rng = np.random.default_rng(shape[0] * 100 + shape[1] + radius)
    f = rng.integers(0, 256, shape, dtype=np.uint8)
    for thr in (0, 16):
        assert np.array_equal(local_sharpness_restate(f, radius, thr), _brute(f, radius, thr))


def test_threshold_is_inclusive():
    f = np.zeros((9, 9), np.uint8)
    f[4, 4] = 4                                  # ml = 16 at the pixel, 4 at its four neighbours
    assert ml_restate(f, 16)[4, 4] == 16 and ml_restate(f, 17)[4, 4] == 0
    assert ml_restate(f, 4)[4, 3] == 4 and ml_restate(f, 5)[4, 3] == 0
    assert local_sharpness_restate(f, 1, 16)[4, 4] == 16 and local_sharpness_restate(f, 1, 17).max() == 0


def test_grey_of_bgr_and_bgra():
    rng = np.random.default_rng(2)
    f = rng.integers(0, 256, (5, 6, 4), dtype=np.uint8)
    assert np.array_equal(grey_restate(f), grey_restate(f[..., :3]))
    flat = np.repeat(f[..., :1], 3, axis=2)
    assert np.array_equal(grey_restate(flat), f[..., 0])           # the coefficients sum to 2^15


# ---- the fold ---------------------------------------------------------------------------------------------------------
def test_fold_restatement_by_hand():
    # one pixel, two entries, one channel: b = (3 + 1, 0 + 0.5 * 1) -> u = b^2 = (16, 0.25); W = w u = (16, 0.5)
    s = np.array([0.5, 0.25], np.float32).reshape(2, 1, 1, 1)
    k = np.array([1.0, 0.5], np.float32).reshape(2, 1, 1)
    om = np.array([3.0, 0.0], np.float32).reshape(2, 1, 1)
    out, den = local_weighted_restate(s, k, om, [[1.0], [2.0]], [[0.0], [0.5]], [1.0, 2.0], 1.0, 2)
    # v = (0.5, 0.25 * 2 + 0.5 * 0.5 = 0.75); num = 16 * 0.5 + 0.5 * 0.75 = 8.375; den = 16 + 0.5 * 0.5 = 16.25
    assert den[0, 0] == np.float32(16.25) and out[0, 0, 0] == np.float32(8.375) / np.float32(16.25)
    # zero maps and floor 0: every weight is 0, the pixel is 0
    out, den = local_weighted_restate(s, k, 0 * om, [[1.0], [2.0]], [[0.0], [0.5]], [1.0, 2.0], 0.0, 3)
    assert den[0, 0] == 0 and out[0, 0, 0] == 0
    # zero maps, floor 1, power 1: the weighted combine with coverage
    from test_cpu_weighted import weighted_restate
    rng = np.random.default_rng(1)
    s = rng.random((4, 3, 5, 3)).astype(np.float32)
    k = rng.random((4, 3, 5)).astype(np.float32)
    g = rng.uniform(0.5, 2, (4, 3)).astype(np.float32)
    o = rng.uniform(-0.1, 0.1, (4, 3)).astype(np.float32)
    w = rng.uniform(0, 2, 4).astype(np.float32)
    a, ad = local_weighted_restate(s, k, 0 * k, g, o, w, 1.0, 1)
    # (W = w * kappa there, so den = sum w kappa^2: not the weighted combine's den; with kappa = 1 it is)
    b, bd = weighted_restate(s, np.ones_like(k), g, o, w)
    a1, ad1 = local_weighted_restate(s, np.ones_like(k), 0 * k, g, o, w, 1.0, 1)
    assert np.array_equal(a1, b) and np.array_equal(ad1, bd) and a.dtype == np.float32 and ad.dtype == np.float32


# ---- the interface ------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_and_symbols():
    p = LocalParameters(radius=3, threshold=20, power=4, floor=0.5)._c()
    assert (p.radius, p.threshold, p.power, p.floor, list(p.reserved)) == (3, 20, 4, 0.5, [0, 0])
    assert ctypes.sizeof(_ffi.LocalParams) == 24
    d = LocalParameters()._c()
    assert (d.radius, d.threshold, d.power, d.floor) == (4, 16, 2, 1.0)
    lib = _ffi.load()
    for name in ("stk_local_sharpness", "stk_local_weighted_stack", "stk_ecc_match_local_weighted",
                 "stk_keypoint_match_local_weighted"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)

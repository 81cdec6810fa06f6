"""numpy restatement of the bicubic fold (include/stacker.h, "Bicubic fold"): the destination -> source map as the engine
builds it, the four weights, one sample from its 4 x 4 taps, and a whole warped frame. Two paths: f32 with every
operation rounded on its own and `fma` emulated as an f64 product and sum rounded once to f32 (the engine's operations,
up to that double rounding), and f64 (the definition's mathematics, the yardstick for error bounds)."""
import numpy as np

F = np.float32
A = -0.75


def invert(M, is_affine):
    """The engine's inverse of the forward matrix, in double (cv::invert on a 3x3 by the adjugate; invertAffineTransform),
    then cast to f32: the matrix whose fma chains give (X, Y). Returned as float64 holding the f32 values."""
    m = np.asarray(M, np.float64).reshape(-1)
    if m.size == 6:
        m = np.concatenate([m, [0.0, 0.0, 1.0]])
    if is_affine:
        D = m[0] * m[4] - m[1] * m[3]
        D = 1.0 / D if D != 0 else 0.0
        a11, a22, a12, a21 = m[4] * D, m[0] * D, -m[1] * D, -m[3] * D
        o = [a11, a12, -a11 * m[2] - a12 * m[5], a21, a22, -a21 * m[2] - a22 * m[5], 0.0, 0.0, 1.0]
    else:
        d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
        if d == 0.0:
            return np.zeros(9)
        d = 1.0 / d
        o = [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
             (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
             (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]
    return np.asarray(o, np.float64).astype(F).astype(np.float64)


def coords64(inv, h, w, is_affine):
    """(X, Y) of every destination pixel in f64 from the f32 inverse matrix."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    X = inv[0] * x + inv[1] * y + inv[2]
    Y = inv[3] * x + inv[4] * y + inv[5]
    if not is_affine:
        W = inv[6] * x + inv[7] * y + inv[8]
        with np.errstate(divide="ignore", invalid="ignore"):
            X, Y = X / W, Y / W
    return X, Y


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def weights(t, dtype=np.float64):
    """(w0, w1, w2, w3) for the fraction t (array), in `dtype`."""
    if dtype == np.float64:
        t = np.asarray(t, np.float64)
        u = 1.0 - t
        tt, uu = t * t, u * u
        return (A * t) * uu, (1.25 * t - 2.25) * tt + 1.0, (1.25 * u - 2.25) * uu + 1.0, (A * u) * tt
    t = np.asarray(t, F)
    u = F(1) - t
    tt, uu = t * t, u * u
    return ((F(A) * t) * uu, fma32(fma32(F(1.25), t, F(-2.25)), tt, F(1)),
            fma32(fma32(F(1.25), u, F(-2.25)), uu, F(1)), (F(A) * u) * tt)


def sample(taps, tx, ty, alpha, dtype=np.float64):
    """One sample per leading index from taps[..., r, k] (r, k = 0 .. 3: rows iy - 1 .., columns ix - 1 ..; raw source
    values), fractions tx, ty and the convert scale alpha (its f32 value)."""
    wx, wy = weights(tx, dtype), weights(ty, dtype)
    if dtype == np.float64:
        p = np.asarray(taps, np.float64) * float(F(alpha))
        hr = [wx[0] * p[..., r, 0] + wx[1] * p[..., r, 1] + wx[2] * p[..., r, 2] + wx[3] * p[..., r, 3] for r in range(4)]
        return wy[0] * hr[0] + wy[1] * hr[1] + wy[2] * hr[2] + wy[3] * hr[3]
    p = np.asarray(taps).astype(F) * F(alpha)
    hr = [fma32(wx[3], p[..., r, 3], fma32(wx[2], p[..., r, 2], fma32(wx[1], p[..., r, 1], wx[0] * p[..., r, 0]))) for r in range(4)]
    return fma32(wy[3], hr[3], fma32(wy[2], hr[2], fma32(wy[1], hr[1], wy[0] * hr[0])))


def footprint(X, Y, sh, sw):
    """(inside, ix, iy, tx, ty) from f64 coordinates: the footprint test and the tap origin of the pixels that pass it."""
    with np.errstate(invalid="ignore"):
        finite = (np.abs(X) < 1e9) & (np.abs(Y) < 1e9)
    Xs, Ys = np.where(finite, X, -1e5), np.where(finite, Y, -1e5)
    ix, iy = np.floor(Xs).astype(np.int64), np.floor(Ys).astype(np.int64)
    inside = finite & (ix >= 1) & (ix + 2 <= sw - 1) & (iy >= 1) & (iy + 2 <= sh - 1)
    return inside, ix, iy, Xs - ix, Ys - iy


def gather(frame, ix, iy):
    """taps[n, c, r, k] of the footprints whose origin pixel is (ix[n], iy[n]) (all inside the frame)."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    r = np.arange(-1, 3)
    rows = (iy[:, None] + r[None, :])[:, :, None]
    cols = (ix[:, None] + r[None, :])[:, None, :]
    return np.moveaxis(f[rows, cols], 3, 1)           # n x 4 x 4 x c -> n x c x 4 x 4


def warp(frame, M, is_affine, alpha, linear, dtype=np.float64):
    """The cubic fold's sample of every destination pixel: the restated cubic sample where the footprint (from f64
    coordinates) is inside, `linear` (the linear fold's image, which the definition falls back to) elsewhere. Returns
    (image, inside, V, X, Y); V: per pixel the largest |tap * alpha| of its footprint (0 outside)."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    h, w, cn = f.shape
    inv = invert(M, is_affine)
    X, Y = coords64(inv, h, w, is_affine)
    inside, ix, iy, tx, ty = footprint(X, Y, h, w)
    out = np.array(linear, dtype).reshape(h, w, cn)
    V = np.zeros((h, w))
    if inside.any():
        taps = gather(f, ix[inside], iy[inside])
        s = sample(taps, tx[inside][:, None], ty[inside][:, None], alpha, dtype)
        out[inside] = s
        V[inside] = np.abs(taps.astype(np.float64)).max(axis=(1, 2, 3)) * float(F(alpha))
    return out, inside, V, X, Y


def quality_scene(seed, h=48, w=64, n_cos=12, fmax=0.3):
    """A scene of n_cos cosines with |fx|, |fy| <= fmax cycles/px as a function scene(x, y) -> grey levels in [28, 228]."""
    rng = np.random.default_rng(seed)
    fx, fy = rng.uniform(-fmax, fmax, n_cos), rng.uniform(-fmax, fmax, n_cos)
    ph = rng.uniform(0, 2 * np.pi, n_cos)
    am = rng.uniform(0.2, 1.0, n_cos)

    def scene(x, y):
        v = np.zeros(np.broadcast(x, y).shape)
        for k in range(n_cos):
            v = v + am[k] * np.cos(2 * np.pi * (fx[k] * x + fy[k] * y) + ph[k])
        return 128.0 + (100.0 / am.sum()) * v
    return scene, h, w


def quality_stack(seed, n=8):
    """(frames u8 n x h x w x 1, forward warps, scene on the destination grid): frame k sees the scene shifted by k/8 px
    along both axes, rounded to u8; its warp brings it back onto frame 0's grid."""
    scene, h, w = quality_scene(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames, warps = [], []
    for k in range(n):
        s = k / 8.0
        # frame k's pixel (x, y) shows the scene at (x - s, y - s); the forward warp moves it back by (-s, -s):
        # destination (x, y) samples source (x + s, y + s), which shows the scene at (x, y)
        frames.append(np.clip(np.rint(scene(x - s, y - s)), 0, 255).astype(np.uint8)[..., None])
        M = np.eye(3)
        M[0, 2] = M[1, 2] = -s
        warps.append(M)
    return np.stack(frames), warps, scene(x, y)


def bilinear64(frame, X, Y):
    """f64 bilinear sample at interior coordinates (the quality test's linear yardstick)."""
    f = np.asarray(frame, np.float64)
    ix, iy = np.floor(X).astype(int), np.floor(Y).astype(int)
    ax, ay = X - ix, Y - iy
    t0 = f[iy, ix] + ax * (f[iy, ix + 1] - f[iy, ix])
    t1 = f[iy + 1, ix] + ax * (f[iy + 1, ix + 1] - f[iy + 1, ix])
    return t0 + ay * (t1 - t0)

"""numpy restatement of drizzle integration (include/stacker.h, stk_drizzle_params): the output -> source matrix as the
engine composes it, the local coordinates, the footprint, the nine tap weights and the combine. Two paths: f32 with every
operation rounded on its own and the coordinate chain through interp_restate.fma32 (the engine's operations), and f64 (the
definition's mathematics from the same f32 matrix, the yardstick for error bounds). Also the quality experiment the CPU and
the GPU test share: a dithered, undersampled stack of a scene with detail beyond one frame's Nyquist limit."""
import numpy as np

from interp_restate import F, fma32, invert

U = 2.0 ** -24


def inverse64(M, is_affine):
    """interp_restate.invert before its cast to f32: the fold's inverse of the forward matrix, in double."""
    m = np.asarray(M, np.float64).reshape(-1)
    if m.size == 6:
        m = np.concatenate([m, [0.0, 0.0, 1.0]])
    m = [float(v) for v in m]
    if is_affine:
        D = m[0] * m[4] - m[1] * m[3]
        D = 1.0 / D if D != 0 else 0.0
        a11, a22, a12, a21 = m[4] * D, m[0] * D, -m[1] * D, -m[3] * D
        return [a11, a12, -a11 * m[2] - a12 * m[5], a21, a22, -a21 * m[2] - a22 * m[5], 0.0, 0.0, 1.0]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    if d == 0.0:
        return [0.0] * 9
    d = 1.0 / d
    return [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def grid_matrix(M, is_affine, scale, origin_x=0.0, origin_y=0.0):
    """A = inv(M) . G, composed in double in the header's order, rounded to f32 (returned as float64 holding f32 values)."""
    inv = inverse64(M, is_affine)
    g = 1.0 / float(F(scale))
    tx = (0.5 * g - 0.5) + float(F(origin_x))
    ty = (0.5 * g - 0.5) + float(F(origin_y))
    A = []
    for r in range(3):
        A += [inv[3 * r] * g, inv[3 * r + 1] * g, (inv[3 * r] * tx + inv[3 * r + 1] * ty) + inv[3 * r + 2]]
    return np.asarray(A, np.float64).astype(F).astype(np.float64)


def coords(A, oh, ow, is_affine, dtype=np.float64, du=0.0, dv=0.0):
    """(u, v, finite) of every output pixel; f64: plus the offsets (du, dv), the probe of the coordinate term."""
    Y, X = np.mgrid[0:oh, 0:ow]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if dtype == F:
            a, fx, fy = A.astype(F), X.astype(F), Y.astype(F)
            u = fma32(a[0], fx, fma32(a[1], fy, a[2]))
            v = fma32(a[3], fx, fma32(a[4], fy, a[5]))
            if not is_affine:
                W = fma32(a[6], fx, fma32(a[7], fy, a[8]))
                u, v = u / W, v / W
        else:
            fx, fy = X.astype(np.float64), Y.astype(np.float64)
            u = A[0] * fx + A[1] * fy + A[2]
            v = A[3] * fx + A[4] * fy + A[5]
            if not is_affine:
                W = A[6] * fx + A[7] * fy + A[8]
                u, v = u / W, v / W
            u, v = u + du, v + dv
        finite = (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
    return u, v, finite


def _local(u, finite, dtype):
    """(jn, d): the nearest source pixel and the offset from it."""
    us = np.where(finite, u, dtype(-1e5))
    if dtype == F:
        fl = np.floor(us)
        ax = us - fl
        up = ax >= F(0.5)
        return fl.astype(np.int64) + up, np.where(up, ax - F(1), ax)
    jn = np.floor(us + 0.5)
    return jn.astype(np.int64), us - jn


def _overlaps(d, hh, jn, n, finite, hp, dtype):
    lo, hi = d - hh, d + hh
    out = []
    for a in (-1, 0, 1):
        c = dtype(a)
        o = np.fmax(dtype(0), np.fmin(hi, c + hp) - np.fmax(lo, c - hp))
        out.append(np.where(finite & (jn + a >= 0) & (jn + a < n), o, dtype(0)))
    return out


def drizzle(frames, As, is_affine, alpha, scale, pixfrac, fill, oh, ow, gain=None, offset=None, weights=None, maps=None,
            dtype=np.float64, du=0.0, dv=0.0):
    """(out oh x ow x cn, den oh x ow) in `dtype` over the entries (frames[i], As[i]); As from grid_matrix. gain / offset:
    n x cn, weights: n, maps: n planes or None entries. `scale` only documents the call: As carry it. du, dv (f64 path):
    offsets added to the coordinates, one number for every entry or one per entry."""
    del scale
    dt = dtype
    n = len(frames)
    f0 = np.asarray(frames[0])
    sh, sw = f0.shape[:2]
    cn = 1 if f0.ndim == 2 else f0.shape[2]
    p = F(pixfrac)
    if dt == F:
        hp, hmax, al = F(0.5) * p, F(1.5) - F(0.5) * p, F(alpha)
    else:
        hp, hmax, al = 0.5 * float(p), 1.5 - 0.5 * float(p), float(F(alpha))
    num, den = np.zeros((oh, ow, cn), dt), np.zeros((oh, ow), dt)
    Y, X = np.mgrid[0:oh, 0:ow]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(n):
            w = dt(F(1.0 if weights is None else weights[i]))
            if not w > 0:
                continue
            g = np.ones(cn, dt) if gain is None else np.asarray(gain[i], F).astype(dt)
            o = np.zeros(cn, dt) if offset is None else np.asarray(offset[i], F).astype(dt)
            src = np.asarray(frames[i]).reshape(sh, sw, cn)
            A = np.asarray(As[i], np.float64)
            u, v, finite = coords(A, oh, ow, is_affine, dt, du[i] if np.ndim(du) else du, dv[i] if np.ndim(dv) else dv)
            jn, d = _local(u, finite, dt)
            kn, e = _local(v, finite, dt)
            if is_affine:
                if dt == F:
                    hx = np.fmin(F(0.5 * (abs(A[0]) + abs(A[1]))), hmax)
                    hy = np.fmin(F(0.5 * (abs(A[3]) + abs(A[4]))), hmax)
                else:
                    hx, hy = min(0.5 * (abs(A[0]) + abs(A[1])), hmax), min(0.5 * (abs(A[3]) + abs(A[4])), hmax)
            elif dt == F:
                a = A.astype(F)
                uu, vv = jn.astype(F) + d, kn.astype(F) + e
                W = (a[6] * X.astype(F) + a[7] * Y.astype(F)) + a[8]
                rw = F(1) / np.abs(W)
                hx = np.fmin(((np.abs(a[0] - uu * a[6]) + np.abs(a[1] - uu * a[7])) * rw) * F(0.5), hmax)
                hy = np.fmin(((np.abs(a[3] - vv * a[6]) + np.abs(a[4] - vv * a[7])) * rw) * F(0.5), hmax)
            else:
                uu, vv = np.where(finite, u, 0.0), np.where(finite, v, 0.0)
                rw = 1.0 / np.abs(A[6] * X + A[7] * Y + A[8])
                hx = np.fmin((np.abs(A[0] - uu * A[6]) + np.abs(A[1] - uu * A[7])) * rw * 0.5, hmax)
                hy = np.fmin((np.abs(A[3] - vv * A[6]) + np.abs(A[4] - vv * A[7])) * rw * 0.5, hmax)
            ox = _overlaps(d, hx, jn, sw, finite, hp, dt)
            oy = _overlaps(e, hy, kn, sh, finite, hp, dt)
            mp = None if maps is None or maps[i] is None else np.asarray(maps[i], F)
            s, k = np.zeros((oh, ow, cn), dt), np.zeros((oh, ow), dt)
            for b in range(3):
                yy = np.clip(kn + b - 1, 0, sh - 1)
                for a_ in range(3):
                    xx = np.clip(jn + a_ - 1, 0, sw - 1)
                    live = (ox[a_] > 0) & (oy[b] > 0)
                    wgt = ox[a_] * oy[b]
                    if mp is not None:
                        mv = mp[yy, xx].astype(dt)
                        live = live & (mv > 0)
                        wgt = wgt * mv
                    t = src[yy, xx, :].astype(dt) * al
                    s = np.where(live[..., None], s + wgt[..., None] * t, s)
                    k = np.where(live, k + wgt, k)
            upd = k > 0
            num = np.where(upd[..., None], num + w * (s * g + o * k[..., None]), num)
            den = np.where(upd, den + w * k, den)
        out = np.where(den[..., None] > 0, num / den[..., None], dt(F(fill)))
    return out, den


def max_coordinate(As, oh, ow, is_affine):
    """The largest finite |u| or |v| any entry gives any output pixel (f64)."""
    m = 1.0
    for A in As:
        u, v, finite = coords(np.asarray(A, np.float64), oh, ow, is_affine)
        if finite.any():
            m = max(m, float(np.abs(u[finite]).max()), float(np.abs(v[finite]).max()))
    return m


def coordinate_term(call, As, oh, ow, is_affine):
    """The allowance for the engine's f32 coordinates: the largest change of the f64 restatement (out, den) when its
    coordinates move by +- 3 ulp (f32) of the largest coordinate magnitude. Every entry's coordinates come from their own
    fma chain and division, so their errors are independent: two entries that share a pixel may move in opposite
    directions, which changes their ratio of weights, and the image, more than any common move does. So each entry is
    moved on its own, along either axis or both (eight directions), the others held; an entry's term is its largest
    change, and the allowance is the sum of the entries' terms (the joint worst case to first order). call(du, dv) ->
    (out, den) in f64, du and dv one offset per entry."""
    delta = 3.0 * float(np.spacing(F(max_coordinate(As, oh, ow, is_affine))))
    n = len(As)
    zero = np.zeros(n)
    o0, d0 = call(zero, zero)
    eo, ed = np.zeros(o0.shape[:2]), np.zeros(d0.shape)
    for i in range(n):
        eo_i, ed_i = np.zeros_like(eo), np.zeros_like(ed)
        for su, sv in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)):
            du, dv = zero.copy(), zero.copy()
            du[i], dv[i] = su * delta, sv * delta
            o1, d1 = call(du, dv)
            eo_i = np.maximum(eo_i, np.abs(o1 - o0).max(axis=2))
            ed_i = np.maximum(ed_i, np.abs(d1 - d0))
        eo, ed = eo + eo_i, ed + ed_i
    return o0, d0, eo, ed


# ---- the quality experiment -------------------------------------------------------------------------------------------
QH, QW, QN = 24, 32, 16


def quality_scene(seed, n_cos=12, fmax=0.6):
    """12 cosines with radial frequencies up to fmax cycles per pixel (one frame's Nyquist limit is 0.5). Returns
    scene(x, y, box): the point-sampled scene in grey levels within [28, 228], or with box = True its integral over the
    unit pixel centred at (x, y) — a sinc factor per component."""
    rng = np.random.default_rng(seed)
    r, th = rng.uniform(0.05, fmax, n_cos), rng.uniform(0, 2 * np.pi, n_cos)
    fx, fy = r * np.cos(th), r * np.sin(th)
    ph = rng.uniform(0, 2 * np.pi, n_cos)
    am = rng.uniform(0.2, 1.0, n_cos)

    def scene(x, y, box=False):
        v = np.zeros(np.broadcast(x, y).shape)
        for k in range(n_cos):
            att = np.sinc(fx[k]) * np.sinc(fy[k]) if box else 1.0
            v = v + am[k] * att * np.cos(2 * np.pi * (fx[k] * x + fy[k] * y) + ph[k])
        return 128.0 + (100.0 / am.sum()) * v
    return scene


def quality_stack(seed):
    """(frames u8 16 x 24 x 32 x 1, forward warps, scene): frame k's pixel (x, y) integrates the scene over the unit pixel
    centred at frame-0 coordinate (x + sx, y + sy), (sx, sy) on the 4 x 4 grid of quarter-pixel offsets, rounded to u8; its
    forward warp is that translation."""
    scene = quality_scene(seed)
    y, x = np.mgrid[0:QH, 0:QW].astype(np.float64)
    frames, warps = [], []
    for k in range(QN):
        sx, sy = (k % 4) / 4.0, (k // 4) / 4.0
        frames.append(np.clip(np.rint(scene(x + sx, y + sy, box=True)), 0, 255).astype(np.uint8)[..., None])
        M = np.eye(3)
        M[0, 2], M[1, 2] = sx, sy
        warps.append(M)
    return np.stack(frames), warps, scene


def quality_truth(scene, s):
    """The point-sampled scene on the output grid of scale s over frame 0, and the mask three coarse pixels in."""
    oh, ow = int(round(QH * s)), int(round(QW * s))
    Y, X = np.mgrid[0:oh, 0:ow].astype(np.float64)
    truth = scene((X + 0.5) / s - 0.5, (Y + 0.5) / s - 0.5)
    m = int(round(3 * s))
    inner = np.zeros((oh, ow), bool)
    inner[m:oh - m, m:ow - m] = True
    return truth, inner


def bilinear_mean64(frames, warps, s):
    """The yardstick: the f64 bilinear, coverage-weighted mean of the frames resampled onto the output grid of scale s
    (translations only). Returns (image in the frames' units, summed coverage)."""
    oh, ow = int(round(QH * s)), int(round(QW * s))
    Y, X = np.mgrid[0:oh, 0:ow].astype(np.float64)
    num, den = np.zeros((oh, ow)), np.zeros((oh, ow))
    for f, M in zip(frames, warps):
        f = np.asarray(f, np.float64)[..., 0]
        u, v = (X + 0.5) / s - 0.5 - M[0, 2], (Y + 0.5) / s - 0.5 - M[1, 2]
        ix, iy = np.floor(u).astype(int), np.floor(v).astype(int)
        ax, ay = u - ix, v - iy
        for dy, wy in ((0, 1 - ay), (1, ay)):
            for dx, wx in ((0, 1 - ax), (1, ax)):
                ok = (ix + dx >= 0) & (ix + dx < QW) & (iy + dy >= 0) & (iy + dy < QH)
                wgt = np.where(ok, wx * wy, 0.0)
                num += wgt * f[np.clip(iy + dy, 0, QH - 1), np.clip(ix + dx, 0, QW - 1)]
                den += wgt
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, 0.0), den


def rms(img, truth, inner):
    return float(np.sqrt(np.mean((np.asarray(img, np.float64)[inner] - truth[inner]) ** 2)))


__all__ = ["F", "U", "invert", "inverse64", "grid_matrix", "coords", "drizzle", "max_coordinate", "coordinate_term",
           "quality_scene", "quality_stack", "quality_truth", "bilinear_mean64", "rms", "QH", "QW", "QN"]

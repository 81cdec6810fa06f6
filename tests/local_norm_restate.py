"""numpy restatement of local normalisation (include/stacker.h, "local normalisation"): the cell moments (float64,
math.fsum), the node estimator with its fill, and the two folds through the planes (f32, operation by operation). The
folds take the fold's samples and coverage weights as inputs (N x H x W x C and N x H x W, fold order), as the restatements
of the weighted combine and of the participation quantile do, so they restate what this feature adds and nothing else.
`fma32` is interp_restate.fma32 made exact: that helper rounds the f64 sum to f32, a double rounding in rare cases; here the
f64 sum is first rounded to odd (from the two-sum's error term), after which the rounding to f32 is the fused one's."""
import math

import numpy as np

from test_cpu_robust import robust_quantile_restate
from test_cpu_weighted import estimate

F = np.float32
NONE, OFFSET, GAIN, LINEAR = 0, 1, 2, 3


def fma32(a, b, c):
    """fma(a, b, c) on f32 operands, correctly rounded to f32."""
    a64, b64, c64 = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    a64, b64, c64 = np.broadcast_arrays(a64, b64, c64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a64 * b64                                   # exact: 24 x 24 bits
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)               # exact error of the sum (two-sum)
        even = (np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)   # the inexact sum, rounded to odd
    return s.astype(F)


def grids(w, h, step):
    """(gw, gh, cw, ch): nodes as stk_mesh_grid, cells."""
    return (w - 1 + step - 1) // step + 1, (h - 1 + step - 1) // step + 1, (w + step - 1) // step, (h + step - 1) // step


# ---- cell moments --------------------------------------------------------------------------------------------------
def cell_moments_restate(samples, kappa, step, stat_step):
    """N x ch x cw x C x 6 by math.fsum over each cell's stepped pixels with kappa_i == 1 (products of f32 values are exact
    in f64), and the sums of the absolute terms in the same shape. Entry 0: zeros."""
    s = np.asarray(samples, F)
    k = np.asarray(kappa, F)
    n, h, w, cn = s.shape
    _, _, cw, ch = grids(w, h, step)
    exact = np.zeros((n, ch, cw, cn, 6))
    mag = np.zeros((n, ch, cw, cn, 6))
    stepped = np.zeros((h, w), bool)
    stepped[::stat_step, ::stat_step] = True
    for i in range(1, n):
        m = stepped & (k[i] == F(1))
        for J in range(ch):
            for K in range(cw):
                sl = (slice(J * step, min((J + 1) * step, h)), slice(K * step, min((K + 1) * step, w)))
                mm = m[sl]
                for c in range(cn):
                    X = s[i][sl][..., c][mm].astype(np.float64)
                    Y = s[0][sl][..., c][mm].astype(np.float64)
                    terms = [np.ones_like(X), X, Y, X * X, Y * Y, X * Y]
                    exact[i, J, K, c] = [math.fsum(t.tolist()) for t in terms]
                    mag[i, J, K, c] = [math.fsum(np.abs(t).tolist()) for t in terms]
    return exact, mag


# ---- estimator and fill --------------------------------------------------------------------------------------------
def fill_restate(g, o, valid, passes):
    """`passes` Jacobi passes on one channel's (g, o) planes (gh x gw f32) with validity `valid`: the mesh fill's arithmetic.
    Returns (g, o, valid)."""
    g, o, m = np.array(g, F), np.array(o, F), np.array(valid, bool)
    gh, gw = m.shape
    for _ in range(passes):
        ng, no, nm = g.copy(), o.copy(), m.copy()
        for j in range(gh):
            for k in range(gw):
                if m[j, k]:
                    continue
                den, n0, n1 = F(0), F(0), F(0)
                for dj in (-1, 0, 1):
                    for dk in (-1, 0, 1):
                        jj, kk = j + dj, k + dk
                        if 0 <= jj < gh and 0 <= kk < gw and m[jj, kk]:
                            wgt = F((2 - abs(dj)) * (2 - abs(dk)))
                            den = F(den + wgt)
                            n0 = F(n0 + F(wgt * g[jj, kk]))
                            n1 = F(n1 + F(wgt * o[jj, kk]))
                if den > 0:
                    ng[j, k], no[j, k], nm[j, k] = F(n0 / den), F(n1 / den), True
        g, o, m = ng, no, nm
    return g, o, m


def estimate_restate(cells, w, h, step, normalize=LINEAR, min_count=16, fill=4):
    """One frame's plane from its cell moments (ch x cw x C x 6): (plane gh x gw x 2C f32, valid gh x gw int32 bit masks
    before the fill, (global gain C, global offset C, global fell_back C))."""
    cells = np.asarray(cells, np.float64)
    gw, gh, cw, ch = grids(w, h, step)
    cn = cells.shape[2]
    assert cells.shape == (ch, cw, cn, 6)
    glob = np.zeros((cn, 6))
    for J in range(ch):
        for K in range(cw):
            glob = glob + cells[J, K]
    gg, go, gfb = estimate(glob, normalize)
    node = np.zeros((gh, gw, cn, 6))
    for j in range(gh):
        for k in range(gw):
            acc = np.zeros((cn, 6))
            for J, K in ((j - 1, k - 1), (j - 1, k), (j, k - 1), (j, k)):
                if 0 <= J < ch and 0 <= K < cw:
                    acc = acc + cells[J, K]
            node[j, k] = acc
    g, o, fb = estimate(node, normalize)
    ok = (node[..., 0] >= min_count) & ~fb & (g >= F(0.25)) & (g <= F(4))
    valid = np.zeros((gh, gw), np.int32)
    plane = np.zeros((gh, gw, 2 * cn), F)
    for c in range(cn):
        valid |= ok[..., c].astype(np.int32) << c
        fg, fo, fm = fill_restate(g[..., c], o[..., c], ok[..., c], fill)
        plane[..., c] = np.where(fm, fg, gg[c])
        plane[..., cn + c] = np.where(fm, fo, go[c])
    return plane, valid, (gg, go, gfb)


# ---- the folds -------------------------------------------------------------------------------------------------------
def plane_at_pixels(plane, w, h, step):
    """(G, O), each h x w x C f32: the plane's bilinear interpolation at every destination pixel, the mesh fold's chain."""
    P = np.asarray(plane, F)
    gh, gw = P.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    k, j = x // step, y // step
    k1, j1 = np.minimum(k + 1, gw - 1), np.minimum(j + 1, gh - 1)
    u = ((x - k * step).astype(F) * F(1.0 / step))[..., None]
    v = ((y - j * step).astype(F) * F(1.0 / step))[..., None]
    t0 = fma32(u, P[j, k1] - P[j, k], P[j, k])
    t1 = fma32(u, P[j1, k1] - P[j1, k], P[j1, k])
    val = fma32(v, t1 - t0, t0)
    cn = P.shape[2] // 2
    return val[..., :cn], val[..., cn:]


def _fields(samples, planes, g, o, step):
    s = np.asarray(samples, F)
    n, h, w, cn = s.shape
    g = np.ones((n, cn), F) if g is None else np.asarray(g, F).reshape(n, cn)
    o = np.zeros((n, cn), F) if o is None else np.asarray(o, F).reshape(n, cn)
    G, O = np.empty(s.shape, F), np.empty(s.shape, F)
    for i in range(n):
        if planes is not None and planes[i] is not None:
            G[i], O[i] = plane_at_pixels(planes[i], w, h, step)
        else:
            G[i], O[i] = g[i], o[i]
    return s, G, O


def norm_mean_restate(samples, kappa, planes, step, g=None, o=None, wt=None):
    """The locally normalised mean: (out H x W x C, den H x W). planes: N planes or None entries (then g / o, N x C); kappa:
    the coverage weights, or ones for coverage = 0."""
    s, G, O = _fields(samples, planes, g, o, step)
    n = s.shape[0]
    k = np.asarray(kappa, F)
    wt = np.ones(n, F) if wt is None else np.asarray(wt, F).reshape(n)
    num = np.zeros(s.shape[1:], F)
    den = np.zeros(s.shape[1:3], F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(n):
            v = s[i] * G[i] + O[i] * k[i][..., None]
            num = num + wt[i] * v
            den = den + wt[i] * k[i]
        out = np.where(den[..., None] > 0, num / den[..., None], F(0)).astype(F)
    assert num.dtype == F and den.dtype == F
    return out, den


def norm_quantile_restate(samples, participates, planes, step, q, g=None, o=None, wt=None):
    """The locally normalised quantile: (out H x W x C, counts H x W). participates: N x H x W (kappa == 1 under coverage =
    1, all true otherwise); w enters through w > 0 only."""
    s, G, O = _fields(samples, planes, g, o, step)
    n, cn = s.shape[0], s.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        u = (s * G + O).astype(F)
    wt = np.ones(n, F) if wt is None else np.asarray(wt, F).reshape(n)
    # u * 1 + 0 == u (a -0 becomes +0, which sorts and compares as the same value)
    return robust_quantile_restate(u, participates, np.ones((n, cn), F), np.zeros((n, cn), F), wt, q)


# ---- the quality stack of the issue's prototype ------------------------------------------------------------------------
def quality_stack(seed):
    """8 frames of 128 x 96 (u8, one channel) of one scene under integer dithers, each moving frame with its own gain,
    offset, linear gradient, one slow sinusoid and noise; frame 3 carries a faint trail. Returns (frames N x H x W u8,
    forward warps N x 3 x 3, truth H x W float64 in grey levels)."""
    rng = np.random.default_rng(seed); big = 160; N, H, W = 8, 96, 128
    yy, xx = np.mgrid[0:big, 0:big].astype(float); scene = np.full((big, big), 60.0)
    for _ in range(60):
        cx, cy, a, s = rng.uniform(0, big), rng.uniform(0, big), rng.uniform(20, 150), rng.uniform(0.8, 1.6)
        scene += a * np.exp(-((xx - cx)**2 + (yy - cy)**2) / (2 * s * s))
    scene += 12 * np.exp(-((xx - 80)**2 + (yy - 70)**2) / (2 * 25.0**2))
    offs = [(16, 16)] + [(16 + int(rng.integers(-10, 11)), 16 + int(rng.integers(-10, 11))) for _ in range(N - 1)]
    y, x = np.mgrid[0:H, 0:W].astype(float)
    frames, warps = [], []
    for i, (ox, oy) in enumerate(offs):
        f = scene[oy:oy + H, ox:ox + W].copy()
        if i > 0:
            gx, gy, c = rng.uniform(-12, 12) / W, rng.uniform(-12, 12) / H, rng.uniform(-6, 6); gain = rng.uniform(0.85, 1.15)
            f = gain * f + c + gx * (x - W / 2) + gy * (y - H / 2) + 5 * np.sin(2 * np.pi * (x / W * rng.uniform(.3, .8) + y / H * rng.uniform(.3, .8)) + rng.uniform(0, 6))
        if i == 3: f = f + 7 * (np.abs((y - 20) - 0.4 * (x - 10)) < 1.5)
        f = f + rng.normal(0, 1.5, f.shape); frame_i = np.clip(np.rint(f), 0, 255)
        frames.append(frame_i.astype(np.uint8))
        # frame i maps destination (x, y) to source (x + 16 - ox, y + 16 - oy): the forward warp is the opposite shift
        M = np.eye(3); M[0, 2], M[1, 2] = ox - 16, oy - 16
        warps.append(M)
    return np.stack(frames), np.stack(warps), scene[16:16 + H, 16:16 + W]


def integer_shift_samples(frames, warps, alpha=1.0 / 255.0):
    """The fold's samples and kappa for pure integer translations (ax = ay = 0: the lerp chain returns tap (ix, iy), kappa
    is 1 where that tap is inside and 0 elsewhere): N x H x W x 1 f32 and N x H x W f32."""
    fr = np.asarray(frames)
    n, h, w = fr.shape
    s = np.zeros((n, h, w, 1), F)
    k = np.zeros((n, h, w), F)
    y, x = np.mgrid[0:h, 0:w]
    for i in range(n):
        dx, dy = int(round(-warps[i][0, 2])), int(round(-warps[i][1, 2]))       # destination -> source
        sx, sy = x + dx, y + dy
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        v = fr[i][np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(F) * F(alpha)
        s[i, ..., 0] = np.where(inside, v, F(0))
        k[i] = inside.astype(F)
    return s, k


def global_records(cells_all, normalize=LINEAR):
    """Per entry the global (gain, offset) from the sum of its cells in row-major order: N x C each; entry 0: (1, 0)."""
    n, ch, cw, cn, _ = cells_all.shape
    g, o = np.ones((n, cn), F), np.zeros((n, cn), F)
    for i in range(1, n):
        glob = np.zeros((cn, 6))
        for J in range(ch):
            for K in range(cw):
                glob = glob + cells_all[i, J, K]
        g[i], o[i], _ = estimate(glob, normalize)
    return g, o


def quality_rms(out, truth, alpha=1.0 / 255.0, border=4):
    """RMS error in grey levels, `border` px in from the edge."""
    d = np.asarray(out, np.float64)[..., 0] / alpha - truth
    d = d[border:-border, border:-border]
    return float(np.sqrt(np.mean(d * d)))

"""numpy restatement of the background model (include/stacker.h, "background model"): the window records (integers, by
sorting), the estimator (float64 and float32, operation by operation, in plain loops over the small node grid), the level
plane's interpolation (local_norm_restate.fma32) and the subtraction. Nothing here is shared with the engine: the records
come from np.sort, where the kernel selects by radix histograms. Also the scene generator of the quality test."""
import math

import numpy as np

from libstacker_rs_amd import BG_CELL_DTYPE, BG_MEAN, BG_MEDIAN, BG_MODE, BackgroundParameters
from local_norm_restate import fma32

F = np.float32


def grid(w, h, step):
    """(gw, gh): the nodes of stk_mesh_grid."""
    return (w - 1 + step - 1) // step + 1, (h - 1 + step - 1) // step + 1


def window(k, step, size):
    """(a, b): the inclusive pixel range of node k along one axis; empty when a > b."""
    q = k * step
    return max(q - step // 2, 0), min(q + step // 2, size - 1)


def keys_of(frame, f32_scale=1.0):
    """H x W x C int64 keys of a frame (u8, u16: the sample; f32: key_f32)."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    if f.dtype != F:
        return f.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((f * F(f32_scale)).astype(F))
        r = np.where(np.isnan(r), F(0), r)                      # fmaxf(NaN, 0) = 0
        return np.minimum(np.maximum(r, F(0)), F(65535)).astype(np.int64)


def clip_distance(kappa, mad):
    ks = F(np.float64(F(kappa)) * 1.4826)
    return max(int(min(math.ceil(float(F(ks * F(mad)))), 65536)), 1)


def window_record(K, clip_iters, kappa):
    """One stk_bg_cell from the window's unmasked keys (a 1-D int array)."""
    rec = np.zeros((), BG_CELL_DTYPE)
    n = int(K.size)
    if n == 0:
        return rec
    K = np.sort(K.astype(np.int64))
    lo, hi = 0, 65535
    for t in range(clip_iters + 1):
        S = K[(K >= lo) & (K <= hi)]
        m = (S.size + 1) // 2
        med = int(S[m - 1])
        mad = int(np.sort(np.abs(S - med))[m - 1])
        if t < clip_iters:
            d = clip_distance(kappa, mad)
            lo, hi = max(lo, med - d), min(hi, med + d)
    rec["n"], rec["kept"], rec["med"], rec["mad"], rec["lo"], rec["hi"] = n, S.size, med, mad, lo, hi
    rec["sum"] = int(S.sum())
    rec["sum2"] = int(sum(int(v) * int(v) for v in S.tolist()))
    return rec


def cells_restate(frame, params=None, mask=None):
    """gh x gw x min(C, 3) records of one frame."""
    p = params or BackgroundParameters()
    K = keys_of(frame, p.f32_scale)
    h, w, cn = K.shape
    cc = min(cn, 3)
    gw, gh = grid(w, h, p.step)
    keep = np.ones((h, w), bool) if mask is None else np.asarray(mask) == 0
    out = np.zeros((gh, gw, cc), BG_CELL_DTYPE)
    for j in range(gh):
        ay, by = window(j, p.step, h)
        for k in range(gw):
            ax, bx = window(k, p.step, w)
            if ay > by or ax > bx:
                continue
            sl = (slice(ay, by + 1), slice(ax, bx + 1))
            for c in range(cc):
                out[j, k, c] = window_record(K[sl][..., c][keep[sl]], p.clip_iters, p.kappa)
    return out


def _fill(A, m, passes):
    """The mesh section's Fill on one value plane (gh x gw f32) with validity m."""
    A, m = np.array(A, F), np.array(m, bool)
    gh, gw = m.shape
    for _ in range(passes):
        nA, nm = A.copy(), m.copy()
        for j in range(gh):
            for k in range(gw):
                if m[j, k]:
                    continue
                den, num = F(0), F(0)
                for dj in (-1, 0, 1):
                    for dk in (-1, 0, 1):
                        jj, kk = j + dj, k + dk
                        if 0 <= jj < gh and 0 <= kk < gw and m[jj, kk]:
                            wgt = F((2 - abs(dj)) * (2 - abs(dk)))
                            den = F(den + wgt)
                            num = F(num + F(wgt * A[jj, kk]))
                if den > 0:
                    nA[j, k], nm[j, k] = F(num / den), True
        A, m = nA, nm
    return A, m


def _lower_median(A, m):
    v = np.sort(A[m])
    return None if v.size == 0 else v[(v.size + 1) // 2 - 1]


def estimate_restate(cells, w, h, depth, params=None):
    """(level gh x gw x C f32, rms likewise, valid gh x gw int32 before the edge extrapolation, flags)."""
    p = params or BackgroundParameters()
    step = p.step
    gw, gh = grid(w, h, step)
    cells = np.asarray(cells).reshape(gh, gw, -1)
    cc = cells.shape[2]
    min_count = p.min_count or 64
    px = [sum(window(k, step, w)) / 2.0 for k in range(gw)]
    py = [sum(window(j, step, h)) / 2.0 for j in range(gh)]
    level, rms_out = np.zeros((gh, gw, cc), F), np.zeros((gh, gw, cc), F)
    valid, flags = np.zeros((gh, gw), np.int32), 0
    for c in range(cc):
        L = [[0.0] * gw for _ in range(gh)]
        R = [[0.0] * gw for _ in range(gh)]
        ok = np.zeros((gh, gw), bool)
        for j in range(gh):
            for k in range(gw):
                r = cells[j, k, c]
                n, kept, med, mad = int(r["n"]), int(r["kept"]), int(r["med"]), int(r["mad"])
                if kept > 0:
                    mean = float(int(r["sum"])) / float(kept)
                    lev = float(med)
                    if p.estimator == BG_MEAN:
                        lev = mean
                    elif p.estimator == BG_MODE:
                        s = 1.4826 * float(max(mad, 1))
                        if abs(mean - med) <= 0.3 * s:
                            lev = 2.5 * med - 1.5 * mean
                    L[j][k] = lev
                    R[j][k] = math.sqrt(max(float(int(r["sum2"])) / float(kept) - mean * mean, 0.0))
                ok[j, k] = kept >= min_count and float(n - kept) <= float(F(p.max_reject)) * float(n)
        valid |= ok.astype(np.int32) << c
        if p.recentre:
            L1 = [row[:] for row in L]
            for j in range(gh):
                for k in range(gw):
                    q = float(k * step)
                    if not ok[j, k] or px[k] == q:
                        continue
                    kn = k + 1 if px[k] > q else k - 1
                    if 0 <= kn < gw and ok[j, kn] and px[kn] != px[k]:
                        L1[j][k] = L[j][k] + ((L[j][k] - L[j][kn]) * (q - px[k])) / (px[k] - px[kn])
            L = [row[:] for row in L1]
            for j in range(gh):
                for k in range(gw):
                    q = float(j * step)
                    if not ok[j, k] or py[j] == q:
                        continue
                    jn = j + 1 if py[j] > q else j - 1
                    if 0 <= jn < gh and ok[jn, k] and py[jn] != py[j]:
                        L[j][k] = L1[j][k] + ((L1[j][k] - L1[jn][k]) * (q - py[j])) / (py[j] - py[jn])
        A, RA = np.array(L, np.float64), np.array(R, np.float64)
        if depth == 32:
            A, RA = A / np.float64(F(p.f32_scale)), RA / np.float64(F(p.f32_scale))
        A, RA = A.astype(F), RA.astype(F)
        okr = ok.copy()
        if p.filter:
            B = A.copy()
            for j in range(1, gh - 1):
                for k in range(1, gw - 1):
                    if ok[j - 1:j + 2, k - 1:k + 2].all():
                        B[j, k] = np.sort(A[j - 1:j + 2, k - 1:k + 2].reshape(-1))[4]
            A = B
        if gw >= 3:
            for j in range(gh):
                if not ok[j, gw - 1] and ok[j, gw - 2] and ok[j, gw - 3]:
                    A[j, gw - 1] = F(F(A[j, gw - 2] + A[j, gw - 2]) - A[j, gw - 3])
                    ok[j, gw - 1] = True
        if gh >= 3:
            for k in range(gw):
                if not ok[gh - 1, k] and ok[gh - 2, k] and ok[gh - 3, k]:
                    A[gh - 1, k] = F(F(A[gh - 2, k] + A[gh - 2, k]) - A[gh - 3, k])
                    ok[gh - 1, k] = True
        fall, rfall = _lower_median(A, ok), _lower_median(RA, okr)
        if fall is None:
            flags |= 1 << c
        A, ok = _fill(A, ok, p.fill)
        RA, okr = _fill(RA, okr, p.fill)
        level[..., c] = np.where(ok, A, F(0) if fall is None else fall)
        rms_out[..., c] = np.where(okr, RA, F(0) if rfall is None else rfall)
    return level, rms_out, valid, flags


def level_at_pixels(plane, w, h, step):
    """h x w x C f32: the level plane's bilinear interpolation at every pixel, the local-normalisation chain."""
    P = np.asarray(plane, F)
    gh, gw = P.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    k, j = x // step, y // step
    k1, j1 = np.minimum(k + 1, gw - 1), np.minimum(j + 1, gh - 1)
    u = ((x - k * step).astype(F) * F(1.0 / step))[..., None]
    v = ((y - j * step).astype(F) * F(1.0 / step))[..., None]
    t0 = fma32(u, P[j, k1] - P[j, k], P[j, k])
    t1 = fma32(u, P[j1, k1] - P[j1, k], P[j1, k])
    return fma32(v, t1 - t0, t0)


def apply_restate(frame, plane, step, target, out_depth):
    """One flattened frame: ((float)raw - B) + target per colour channel, channel 3 as it is; rounding and saturation as
    stk_calibrate's. plane None: B = 0."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    h, w, cn = f.shape
    cc = min(cn, 3)
    v = f.astype(F)
    B = np.zeros((h, w, cc), F) if plane is None else level_at_pixels(np.asarray(plane, F).reshape(grid(w, h, step)[1], grid(w, h, step)[0], cc), w, h, step)
    t = np.asarray(target, F).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        v[..., :cc] = (v[..., :cc] - B).astype(F) + t[:cc]
        if out_depth == 32:
            return v
        r = np.rint(v)
        r = np.where(np.isnan(r), F(0), r)
        return np.minimum(np.maximum(r, F(0)), F(255 if out_depth == 8 else 65535)).astype(np.uint8 if out_depth == 8 else np.uint16)


def flatten_restate(frame, params, mask=None):
    """(flattened frame, level plane, rms plane, records): the three parts in sequence."""
    f = np.asarray(frame)
    depth = 8 * f.dtype.itemsize
    h, w = f.shape[:2]
    cells = cells_restate(f, params, mask)
    level, rms, _, _ = estimate_restate(cells, w, h, depth, params)
    return apply_restate(f, level, params.step, params.target, params.out_depth or depth), level, rms, cells


# ---- the scene of the quality test ---------------------------------------------------------------------------------
def sky(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return 2000 + 300 * x / w + 150 * y / h + 200 * (((x - 0.3 * w) / w) ** 2 + ((y - 0.6 * h) / h) ** 2)


def scene(w, h, seed):
    """(u16 frame, the true background): the sky above, 40 Gaussian stars, Gaussian noise of sigma 40."""
    r = np.random.default_rng(seed)
    bg = sky(w, h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = bg.copy()
    for _ in range(40):
        sx = r.uniform(0, w)
        sy = r.uniform(0, h)
        amp = 10 ** r.uniform(2.3, 3.8)
        sig = r.uniform(1.2, 2.0)
        f += amp * np.exp(-((x - sx) ** 2 + (y - sy) ** 2) / (2 * sig * sig))
    f += r.normal(0, 40, f.shape)
    return np.clip(np.rint(f), 0, 65535).astype(np.uint16), bg


def level_error(B, bg):
    """RMS(B - bg) / RMS(bg - mean bg)."""
    B, bg = np.asarray(B, np.float64), np.asarray(bg, np.float64)
    return float(np.sqrt(np.mean((B - bg) ** 2)) / np.sqrt(np.mean((bg - bg.mean()) ** 2)))

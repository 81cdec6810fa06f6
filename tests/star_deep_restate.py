"""Numpy restatement of star detection on the 16-bit key (include/stacker.h, stk_star_deep_params): the key of a u8, u16 or
f32 frame, and steps 1 - 5 of "Detection" on it with that section's changes (exact order statistics by sorting, the clamp of
d_T at 65536). Written from the header's definition, not from the engine's code: whole-image array arithmetic. Records to
stars, the matching and the pipeline are star_restate's, unchanged."""
import numpy as np

import star_restate as sr
from libstacker_rs_amd import StarDeepParameters, StarParameters

TILE = sr.TILE
TILE_CAP = sr.TILE_CAP


def key(frame, deep=None):
    """K(p) of a frame, int32 in 0 .. 65535, by the frame's dtype."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    cn = f.shape[2]
    if f.dtype == np.uint8:
        return sr.grey_u8(f)
    if f.dtype == np.uint16:
        if cn == 1:
            return f[..., 0].astype(np.int32)
        b, g, r = (f[..., k].astype(np.int64) for k in range(3))
        return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.int32)
    if f.dtype != np.float32:
        raise ValueError("u8, u16 or f32 frames")
    scale = np.float32((deep or StarDeepParameters()).f32_scale)
    with np.errstate(all="ignore"):
        if cn == 1:
            gf = f[..., 0]
        else:                                                              # every product and every sum rounded to f32
            gf = (f[..., 0] * np.float32(0.114) + f[..., 1] * np.float32(0.587)).astype(np.float32) + f[..., 2] * np.float32(0.299)
        v = np.rint((gf * scale).astype(np.float32))
    v = np.where(np.isnan(v), np.float32(0), v)                            # fmaxf(NaN, 0) = 0
    return np.clip(v, np.float32(0), np.float32(65535)).astype(np.int32)


def tile_stats(K, p):
    """Per tile (rows of tiles, columns of tiles): med, mad, thr."""
    h, w = K.shape
    ty, tx = (h + TILE - 1) // TILE, (w + TILE - 1) // TILE
    med, mad, thr = (np.zeros((ty, tx), np.int64) for _ in range(3))
    ks = np.float32(np.float64(np.float32(p.kappa)) * 1.4826)
    for j in range(ty):
        for i in range(tx):
            t = K[j * TILE:(j + 1) * TILE, i * TILE:(i + 1) * TILE].ravel().astype(np.int64)
            k = (t.size + 1) // 2
            m = int(np.sort(t)[k - 1])
            a = int(np.sort(np.abs(t - m))[k - 1])
            d = max(int(min(np.ceil(np.float32(ks * np.float32(a))), np.float32(65536.0))), int(p.min_contrast))
            med[j, i], mad[j, i], thr[j, i] = m, a, m + d
    return med, mad, thr


def detect_records(frame, p, deep=None):
    """(records, n_peaks) as star_restate.detect_records, on the key."""
    K = key(frame, deep).astype(np.int64)
    h, w = K.shape
    r = int(p.radius)
    med, _, thr = tile_stats(K, p)
    MED = np.repeat(np.repeat(med, TILE, 0), TILE, 1)[:h, :w]
    THR = np.repeat(np.repeat(thr, TILE, 0), TILE, 1)[:h, :w]
    Kp = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    Kp[r:r + h, r:r + w] = K
    ys, xs = np.mgrid[0:h, 0:w]
    peak = (K >= THR) & (xs >= r) & (xs < w - r) & (ys >= r) & (ys < h - r)
    npix, S, Sx, Sy = (np.zeros((h, w), np.int64) for _ in range(4))
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            Q = Kp[r + dy:r + dy + h, r + dx:r + dx + w]
            if (dy, dx) != (0, 0):
                peak &= (Q < K) if (dy, dx) < (0, 0) else (Q <= K)          # raster order: (dy, dx) lexicographic
            npix += Q >= THR
            V = np.maximum(Q - MED, 0)
            S += V
            Sx += V * dx
            Sy += V * dy
    peak &= npix >= int(p.min_pixels)
    py, px = np.nonzero(peak)
    rec = np.stack([px, py, S[py, px], Sx[py, px], Sy[py, px], K[py, px], npix[py, px]], 1).astype(np.int64).reshape(-1, 7)
    n_peaks = len(rec)
    if n_peaks:
        assert rec[:, 2].max() <= 225 * 65535 and np.abs(rec[:, 3:5]).max() <= 840 * 65535       # the header's int32 bound
        rec = rec[np.lexsort((rec[:, 0], rec[:, 1], -rec[:, 2]))]         # S descending, py ascending, px ascending
        tile = (rec[:, 1] // TILE) * ((w + TILE - 1) // TILE) + rec[:, 0] // TILE
        keep = np.zeros(len(rec), bool)
        seen = {}
        for k, t in enumerate(tile):                                      # the first TILE_CAP of every tile, in key order
            seen[t] = seen.get(t, 0) + 1
            keep[k] = seen[t] <= TILE_CAP
        rec = rec[keep][:int(p.max_stars)]
    return rec, n_peaks


def detect(frame, p, deep=None):
    rec, n_peaks = detect_records(frame, p, deep)
    return sr.stars_from_records(rec), n_peaks


def align(frames, p=None, deep=None):
    """The restated stk_star_align_deep: (stats, lists), as star_restate.align. star_restate takes a one-channel integer
    image as its own grey, so its pipeline runs on the keys; its detection lacks only the clamp of d_T, which no tile of
    these frames reaches — checked, list by list, against this module's detection."""
    p = p or StarParameters()
    stats, lists = sr.align([key(f, deep) for f in frames], p)
    for f, got in zip(frames, lists):
        assert got.tobytes() == detect(f, p, deep)[0].tobytes()
    return stats, lists

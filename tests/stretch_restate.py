"""Numpy restatement of the display stretch (include/stacker.h, "display stretch"), written from the header's definition, not
from the engine's code: ranks by np.sort, whole-image array arithmetic in f32, one numpy operation per rounded operation,
np.fmax / np.fmin (the IEEE ones: a NaN loses), every fma through local_norm_restate.fma32; the auto rule and the tables in
float64. And the scene of the quality measurements."""
import math

import numpy as np

from local_norm_restate import fma32

F = np.float32
LINEAR, MTF, TABLE = 0, 1, 2
ASINH, GAMMA, SRGB = 0, 1, 2
STAT = np.dtype([("count", np.int64), ("min", F), ("max", F), ("median", F), ("mad", F), ("q", F, 4)])


# ---- 1. statistics ------------------------------------------------------------------------------------------------------
def kth(sorted_values, k):
    return sorted_values[k - 1]


def stats(d, mask=None, quantiles=()):
    """min(C, 3) records: finite samples (where the mask is > 0), -0 counted as +0"""
    d = np.asarray(d, F)
    img = d[..., None] if d.ndim == 2 else d
    cc = min(img.shape[2], 3)
    out = np.zeros(cc, STAT)
    for c in range(cc):
        v = img[..., c]
        ok = np.isfinite(v)
        if mask is not None:
            with np.errstate(invalid="ignore"):
                ok &= np.asarray(mask, F) > 0
        v = v[ok].copy()
        bits = v.view(np.uint32)
        bits[bits == 0x80000000] = 0
        n = v.size
        if n == 0:
            continue
        s = np.sort(v)
        med = kth(s, (n + 1) // 2)
        with np.errstate(over="ignore"):
            dev = np.abs((v - med).astype(F))
        rec = out[c]
        rec["count"], rec["min"], rec["max"], rec["median"] = n, s[0], s[-1], med
        rec["mad"] = kth(np.sort(dev), (n + 1) // 2)
        for i, p in enumerate(quantiles):
            rec["q"][i] = kth(s, min(n, max(1, int(math.ceil(float(p) * float(n))))))
    return out


# ---- 2. the auto rule, float64 ------------------------------------------------------------------------------------------
def mtf64(t, x):
    return ((t - 1.0) * x) / ((2.0 * t - 1.0) * x - t)


def _rule(median, mad, mn, w, clip, target):
    lo = median + (clip * 1.4826) * mad
    c0 = mn if mn > lo else lo
    if w <= c0:
        w = c0 + 1.0
    x0 = (median - c0) / (w - c0)
    m = 0.5
    if x0 != 0.0:
        m = min(max(mtf64(target, x0), 1e-6), 1.0 - 1e-6)
    return F(c0), F(w), F(m)


def auto(st, shadows_clip=-2.8, target_background=0.25, linked=0, white_mode=0, white=1.0):
    """(black, white, midtone): three float32 arrays of 4; entries from the colour channels on are 0, 1, 0.5"""
    cc = min(len(st), 3)
    black, wh, mid = np.zeros(4, F), np.ones(4, F), np.full(4, 0.5, F)
    w = [float(white) if white_mode == 0 else float(st[c]["max"]) if white_mode == 1 else float(st[c]["q"][0]) for c in range(cc)]
    if linked:
        med = mad = mn = ww = 0.0
        for c in range(cc):
            med, mad, mn, ww = med + float(st[c]["median"]), mad + float(st[c]["mad"]), mn + float(st[c]["min"]), ww + w[c]
        vals = [(med / cc, mad / cc, mn / cc, ww / cc)] * cc
    else:
        vals = [(float(st[c]["median"]), float(st[c]["mad"]), float(st[c]["min"]), w[c]) for c in range(cc)]
    for c in range(cc):
        black[c], wh[c], mid[c] = _rule(*vals[c], float(shadows_clip), float(target_background))
    return black, wh, mid


def table(kind, param, knots):
    x = np.arange(knots + 1, dtype=np.float64) / float(knots)
    if kind == ASINH:
        t = np.arcsinh(param * x) / np.arcsinh(param)
    elif kind == GAMMA:
        t = np.power(x, 1.0 / param)
    else:
        t = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
    t = np.clip(t.astype(F), F(0), F(1))
    t[0], t[-1] = 0.0, 1.0
    return t


# ---- 3. the stretch -----------------------------------------------------------------------------------------------------
def curve_f32(x, curve, m=0.5, tab=None):
    x = np.asarray(x, F)
    if curve == MTF:
        m = F(m)
        mm1, k = F(m - F(1)), F(F(F(2) * m) - F(1))
        with np.errstate(all="ignore"):
            return np.fmin(np.fmax(((mm1 * x).astype(F) / fma32(k, x, F(-m))).astype(F), F(0)), F(1))
    if curve == TABLE:
        T = np.asarray(tab, F)
        K = T.size - 1
        t = (x * F(K)).astype(F)
        i = np.minimum(t.astype(np.int32), K - 1)
        fr = (t - i.astype(F)).astype(F)
        return fma32((T[i + 1] - T[i]).astype(F), fr, T[i])
    return x


def stretch(d, curve=MTF, colour=0, out_depth=32, black=0.0, white=1.0, midtone=0.5, out_scale=1.0, tab=None):
    d = np.asarray(d, F)
    img = d[..., None] if d.ndim == 2 else d
    cn = img.shape[2]
    cc = min(cn, 3)
    black, white, midtone = (np.broadcast_to(np.asarray(v, F).reshape(-1), (4,)) if np.size(v) == 1 else np.asarray(v, F) for v in (black, white, midtone))
    xs = []
    with np.errstate(all="ignore"):
        for c in range(cc):
            r = F(white[c] - black[c])
            xs.append(np.fmin(np.fmax(((img[..., c] - black[c]).astype(F) / r).astype(F), F(0)), F(1)))
        if colour and cc == 3:
            L = (((xs[0] + xs[1]).astype(F) + xs[2]).astype(F) / F(3)).astype(F)
            g = curve_f32(L, curve, midtone[0], tab)
            s = np.where(L > 0, (g / np.where(L > 0, L, F(1))).astype(F), F(0)).astype(F)
            ys = [np.fmin((x * s).astype(F), F(1)) for x in xs]
        else:
            ys = [curve_f32(xs[c], curve, midtone[c], tab) for c in range(cc)]
        if cn == 4:
            ys.append(np.fmin(np.fmax(img[..., 3], F(0)), F(1)))
    y = np.stack(ys, 2)
    if out_depth == 32:
        return (y * F(out_scale)).astype(F)
    full = F(255.0) if out_depth == 8 else F(65535.0)
    r = np.clip(np.rint((y * full).astype(F)), 0, full)
    return r.astype(np.uint8 if out_depth == 8 else np.uint16)


def auto_stretch(d, mask=None, curve=MTF, colour=0, out_depth=32, out_scale=1.0, tab=None, white_quantile=0.999, **rule):
    st = stats(d, mask, (white_quantile,) if rule.get("white_mode", 0) == 2 else ())
    b, w, m = auto(st, **rule)
    return stretch(d, curve, colour, out_depth, b, w, m, out_scale, tab), st, (b, w, m)


# ---- the scene of the quality measurements ------------------------------------------------------------------------------
SKY = (0.020, 0.031, 0.012)
NOISE = (0.002, 0.0025, 0.0015)


def scene(seed, h=96, w=128):
    """a linear deep-sky stack: per channel a sky level with a small gradient, white noise, 15 Gaussian stars"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 3))
    stars = [(rng.uniform(4, w - 4), rng.uniform(4, h - 4), rng.uniform(1.0, 1.8), 10 ** rng.uniform(-1.5, -0.1)) for _ in range(15)]
    for c in range(3):
        img[..., c] = SKY[c] * (1.0 + 0.1 * x / w + 0.05 * y / h) + rng.normal(0.0, NOISE[c], (h, w))
        for sx, sy, sg, amp in stars:
            img[..., c] += amp * (1.0 - 0.1 * c) * np.exp(-((x - sx) ** 2 + (y - sy) ** 2) / (2 * sg * sg))
    return img.astype(F)

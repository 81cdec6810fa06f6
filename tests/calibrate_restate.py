"""Frame calibration restated in numpy (include/stacker.h, "frame calibration"): what test_cpu_calibrate.py checks against a
scalar loop and planted answers, and what test_gpu_calibrate.py compares the engine against bit for bit. Every operation is
f32 and rounded on its own, in the order the definition states; fmaxf / fminf are numpy's fmax / fmin.

`master_stack_restate` reuses the restatements the weighted and median / MAD clip tests already have (the estimator of
test_cpu_weighted.py, the participation form of test_cpu_robust_clip.py). Its moments are numpy f64 sums: exact, and so equal
to the engine's whatever the order, whenever the frames hold integers or dyadic values, which is what the tests feed it."""
import numpy as np

from test_cpu_robust_clip import robust_clip_restate_weighted
from test_cpu_weighted import GAIN, estimate

F = np.float32
ABSENT = np.uint32(0xFFFFFFFF)
NAN_KEY = np.uint32(0xFFFFFFFE)
OFFSETS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]       # (dx, dy), raster order


def same_bits(a, b):
    """Bit equality of two arrays, with every NaN equal to every NaN (the definition names no payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def order_key(v):
    """The definition's total order as unsigned integers: -inf < .. < -0 < +0 < .. < +inf < every NaN."""
    v = np.ascontiguousarray(v, F)
    b = v.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), NAN_KEY, k).astype(np.uint32)


def from_key(k):
    k = np.asarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == NAN_KEY, np.uint32(0x7FC00000), b).astype(np.uint32).view(F)


def median_rule(values, present):
    """values, present: 8 x ... (f32, bool). Returns (the median rule's value, m); where m == 0 the value is unspecified."""
    keys = np.where(present, order_key(values), ABSENT)
    keys = np.sort(keys, axis=0)
    m = present.sum(axis=0)
    jl = np.clip((m - 1) // 2, 0, 7)
    jh = np.clip(m // 2, 0, 7)
    lo = from_key(np.take_along_axis(keys, jl[None], axis=0)[0])
    hi = from_key(np.take_along_axis(keys, jh[None], axis=0)[0])
    with np.errstate(invalid="ignore", over="ignore"):
        even = ((lo + hi) * F(0.5)).astype(F)
    return np.where(m % 2 == 1, lo, even).astype(F), m


def shifted(a, dx, dy):
    """a[..., y + dy, x + dx, :] for an array whose axes -3, -2 are (y, x), and the plane of positions where that exists."""
    h, w = a.shape[-3], a.shape[-2]
    out = np.zeros_like(a)
    ok = np.zeros((h, w), bool)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    yd, xd = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[..., ys, xs, :] = a[..., yd, xd, :]
        ok[ys, xs] = True
    return out, ok


def calibrated_values(frames, bias=None, dark=None, flat=None, dark_scale=None, flat_mean=None, flat_min=None, pedestal=0.0):
    """v of the definition, unrepaired: n x H x W x C f32; channel 3 is (float)raw."""
    fr = np.asarray(frames)
    n, h, w, cn = fr.shape
    cc = min(cn, 3)
    v = fr.astype(F)
    s = np.ones(n, F) if dark_scale is None else np.asarray(dark_scale, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = v[..., :cc]
        if bias is not None:
            u = u - np.asarray(bias, F)[..., :cc]
        if dark is not None:
            u = u - (s[:, None, None, None] * np.asarray(dark, F)[None, ..., :cc]).astype(F)
        if flat is not None:
            t = (u * np.asarray(flat_mean, F)[:cc]).astype(F)
            u = t / np.fmax(np.asarray(flat, F)[..., :cc], F(flat_min))
        u = (u + F(pedestal)).astype(F)
    v = v.copy()
    v[..., :cc] = u
    return v


def to_depth(v, out_depth):
    if out_depth == 32:
        return v.astype(F)
    hi = F(255.0) if out_depth == 8 else F(65535.0)
    with np.errstate(invalid="ignore"):
        r = np.fmin(np.fmax(np.rint(v.astype(F)), F(0)), hi)
    return r.astype(np.uint8 if out_depth == 8 else np.uint16)


def calibrate_restate(frames, bias=None, dark=None, flat=None, dark_scale=None, flat_mean=None, flat_min=None, pedestal=0.0,
                      defects=None, step=1, out_depth=None):
    fr = np.asarray(frames)
    cn = fr.shape[-1]
    cc = min(cn, 3)
    v = calibrated_values(fr, bias, dark, flat, dark_scale, flat_mean, flat_min, pedestal)
    if defects is not None:
        bits = ((np.asarray(defects, np.uint8)[..., None] >> np.arange(cc, dtype=np.uint8)) & 1).astype(bool)     # H x W x cc
        vals, pres = [], []
        for dx, dy in OFFSETS:
            sv, ok = shifted(v[..., :cc], dx * step, dy * step)
            sb, _ = shifted(bits, dx * step, dy * step)
            vals.append(sv)
            pres.append(np.broadcast_to(ok[..., None] & ~sb, sv.shape))
        med, m = median_rule(np.stack(vals), np.stack(pres))
        fix = bits[None] & (m > 0)
        v[..., :cc] = np.where(fix, med, v[..., :cc])
    depth = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(np.float32): 32}[fr.dtype]
    return to_depth(v, depth if out_depth is None else out_depth)


def defect_map_restate(master, high=True, low=False, high_abs=0.0, low_ratio=0.5, step=1, previous=None):
    """(map H x W uint8, counts 4 int64)."""
    x = np.asarray(master, F)
    if x.ndim == 2:
        x = x[..., None]
    cc = min(x.shape[-1], 3)
    x = np.ascontiguousarray(x[..., :cc])
    vals, pres = [], []
    for dx, dy in OFFSETS:
        sv, ok = shifted(x, dx * step, dy * step)
        vals.append(sv)
        pres.append(np.broadcast_to(ok[..., None], sv.shape))
    med, m = median_rule(np.stack(vals), np.stack(pres))
    with np.errstate(invalid="ignore", over="ignore"):
        flag = ~np.isfinite(x)
        if high:
            flag = flag | ((m > 0) & ((x - med).astype(F) > F(high_abs)))
        if low:
            flag = flag | ((m > 0) & (x < (F(low_ratio) * med).astype(F)))
    out = (flag.astype(np.uint8) << np.arange(cc, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)
    if previous is not None:
        out = out | np.asarray(previous, np.uint8)
    counts = np.array([int(((out >> c) & 1).sum()) for c in range(4)], np.int64)
    return out, counts


def image_mean_restate(image):
    a = np.asarray(image, F)
    if a.ndim == 2:
        a = a[..., None]
    return a.astype(np.float64).sum(axis=(0, 1)) / float(a.shape[0] * a.shape[1])


def master_stack_restate(frames, normalize=0, stat_step=4, kappa_low=3.0, kappa_high=3.0, sigma_floor=0.5, iterations=2):
    """(out, counts): the identity fold's samples are the frames' values as f32 (alpha = 1)."""
    s = np.asarray(frames).astype(F)
    n, h, w, cn = s.shape
    g = np.ones((n, cn), F)
    if normalize == 2 and n > 1:
        sub = s[:, ::stat_step, ::stat_step].astype(np.float64)
        y = sub[0]
        mom = np.zeros((n, cn, 6))
        for i in range(1, n):
            x = sub[i]
            mom[i] = np.stack([np.full(cn, float(x.shape[0] * x.shape[1])), x.sum((0, 1)), y.sum((0, 1)), (x * x).sum((0, 1)),
                               (y * y).sum((0, 1)), (x * y).sum((0, 1))], axis=-1)
        gi, _, _ = estimate(mom[1:], GAIN)
        g[1:] = gi
    out, k, _ = robust_clip_restate_weighted(s, np.ones((n, h, w), bool), g, np.zeros((n, cn), F), np.ones(n, F), kappa_low, kappa_high,
                                             sigma_floor, iterations)
    return out, k


# ---- the planted stack: arithmetic that is exact in f32 ------------------------------------------------------------------
BLOCK = 8
FLAT_LEVEL = 32.0


def planted(h=24, w=40, cn=3, n_lights=6, seed=5):
    """A scene of integer multiples of 8 that is constant on 8 x 8 blocks; an integer bias; an integer dark, constant on
    blocks, with hot pixels; a flat of {1/2, 1, 2} x FLAT_LEVEL by block column (neighbouring blocks a factor 2 apart at
    most) with dead pixels at FLAT_LEVEL / 8; dark scales in {1, 2}. Defects sit inside the blocks (not on their rims), so a
    defect's good neighbours all show the block's scene value; in the lights a defective pixel holds a frame-dependent
    value unrelated to the scene, so that only repair brings the scene back there. Returns a dict of arrays."""
    rng = np.random.default_rng(seed)
    by, bx = (h + BLOCK - 1) // BLOCK, (w + BLOCK - 1) // BLOCK
    up = lambda a: np.repeat(np.repeat(a, BLOCK, axis=0), BLOCK, axis=1)[:h, :w]
    scene = up(8.0 * rng.integers(2, 13, (by, bx, cn))).astype(F)
    bias = rng.integers(8, 13, (h, w, cn)).astype(F)
    dark = up(rng.integers(2, 5, (by, bx, cn))).astype(F)
    ratio = np.array([0.5, 1.0, 2.0, 1.0])[np.arange(bx) % 4]
    flat = (FLAT_LEVEL * up(np.broadcast_to(ratio[None, :, None], (by, bx, cn)))).astype(F)
    hot = np.zeros((h, w, cn), bool)
    dead = np.zeros((h, w, cn), bool)
    spots = [(2, 3, 0), (2, 4, 0), (3, 3, 1), (10, 12, 2), (11, 13, 2), (19, 34, 1), (13, 21, 0), (14, 21, 0), (13, 22, 0), (20, 5, 2)]
    for k, (y, x, c) in enumerate(spots):
        if y < h and x < w:
            (hot if k % 2 == 0 else dead)[y, x, c % cn] = True
    dark = np.where(hot, dark + F(50), dark).astype(F)
    flat = np.where(dead, F(FLAT_LEVEL / 8), flat).astype(F)
    scale = np.array([1.0, 2.0] * n_lights, F)[:n_lights]
    lights = scene[None] * (flat / F(FLAT_LEVEL))[None] + scale[:, None, None, None] * dark[None] + bias[None]
    lights = np.minimum(lights, 255).astype(np.uint8)
    junk = ((200 + 17 * np.arange(n_lights)) % 256).astype(np.uint8)            # a defective pixel carries no usable signal
    lights = np.where((hot | dead)[None], junk[:, None, None, None], lights)
    defects = ((hot | dead).astype(np.uint8) << np.arange(cn, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)
    return dict(scene=scene, bias=bias, dark=dark, flat=flat, hot=hot, dead=dead, scale=scale, lights=lights, defects=defects)


def planted_calibration_frames(p, n=5):
    """Raw bias, dark and flat frames (u8, n each) whose masters are exactly p's: identical frames but for one cosmic-ray
    hit per stack, at odd coordinates (outside the flats' moments at stat_step 2 or 4); the flats at levels 1, 2, 1, 1/2, 1."""
    bias = np.repeat(p["bias"][None], n, 0).astype(np.uint8)
    dark = np.repeat((p["dark"] + p["bias"])[None], n, 0).astype(np.uint8)
    level = np.array([1.0, 2.0, 1.0, 0.5, 1.0] * n, F)[:n]
    flat = (p["flat"][None] * level[:, None, None, None] + p["bias"][None]).astype(np.uint8)
    bias[1, 5, 7] = 250
    dark[2, 3, 9] = 240
    flat[3, 7, 11] = 255
    return bias, dark, flat

"""Numpy restatement of the wavelet layers (include/stacker.h, "wavelet layers"), written from the header's definition, not
from the engine's code: whole-image array arithmetic in f32, every fma through local_norm_restate.fma32, one numpy operation
per rounded operation. The image planes carry a leading channel axis: every operation acts on the last two. The median is
np.partition on the restated first layer. The noise table is restated independently of the closed form the engine uses: as
the norm of the 2-D impulse response of layer j, built by running the cascade on a unit impulse in float64. And the scene of
the quality measurements."""
import math

import numpy as np

from local_norm_restate import fma32

F = np.float32
HARD, SOFT = 0, 1
B3 = (0.0625, 0.25, 0.375, 0.25, 0.0625)


# ---- the noise table --------------------------------------------------------------------------------------------------
def noise_table(levels=8):
    """e_j = |psi_j|_2, psi_j the 2-D impulse response of layer j: the cascade run on a unit impulse, in float64, on a grid
    wide enough that nothing reaches its border."""
    half = 2 * (2 ** levels - 1)
    n = 2 * half + 1
    c = np.zeros((n, n))
    c[half, half] = 1.0
    e = []
    for j in range(levels):
        s = 2 ** j
        hx = np.zeros_like(c)
        for k, b in zip(range(-2, 3), B3):
            hx += b * np.roll(c, k * s, axis=1)                                   # (zero beyond the reach: the roll wraps zeros)
        nxt = np.zeros_like(c)
        for k, b in zip(range(-2, 3), B3):
            nxt += b * np.roll(hx, k * s, axis=0)
        e.append(math.sqrt(float(((c - nxt) ** 2).sum())))
        c = nxt
    return np.array(e)


# ---- steps 1 - 2 --------------------------------------------------------------------------------------------------------
def sanitise(d):
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(d) & (np.abs(d) <= F(1e30)), d, F(0)).astype(F)


def _chain(v):
    a = (F(0.0625) * v[0]).astype(F)
    a = fma32(F(0.25), v[1], a)
    a = fma32(F(0.375), v[2], a)
    a = fma32(F(0.25), v[3], a)
    return fma32(F(0.0625), v[4], a)


def smooth(c, s):
    """c_{j+1} from c_j (..., h, w) at spacing s, BORDER_REFLECT_101"""
    h, w = c.shape[-2:]
    assert min(h, w) >= 2 * s + 1
    P = np.pad(c, [(0, 0)] * (c.ndim - 2) + [(0, 0), (2 * s, 2 * s)], mode="reflect")
    hx = _chain([P[..., :, k * s:k * s + w] for k in range(5)])
    P = np.pad(hx, [(0, 0)] * (c.ndim - 2) + [(2 * s, 2 * s), (0, 0)], mode="reflect")
    return _chain([P[..., k * s:k * s + h, :] for k in range(5)])


def _planes(d):
    d = np.asarray(d, F)
    img = d[..., None] if d.ndim == 2 else d
    cc = min(img.shape[2], 3)
    return img, cc, sanitise(np.moveaxis(img[..., :cc], 2, 0))


def layers(d, levels):
    """[w_0, .., w_{J-1}, c_J], each with the image's shape; C = 4: alpha is the input's in every one"""
    img, cc, c = _planes(d)
    out = []
    for j in range(levels):
        nxt = smooth(c, 2 ** j)
        out.append((c - nxt).astype(F))
        c = nxt
    out.append(c)
    res = []
    for pl in out:
        r = img.copy()
        r[..., :cc] = np.moveaxis(pl, 0, 2)
        res.append(r.reshape(np.shape(d)))
    return res


def lower_median(v):
    v = np.asarray(v).reshape(-1)
    k = (v.size + 1) // 2 - 1
    return np.partition(v, k)[k]


def sigma(d, e0=None):
    """(sigma, median) per colour channel, f32"""
    _, cc, c = _planes(d)
    e0 = noise_table(1)[0] if e0 is None else e0
    w0 = np.abs((c - smooth(c, 1)).astype(F))
    med = np.array([lower_median(w0[k]) for k in range(cc)], F)
    return np.array([F(1.4826 * float(m) / e0) for m in med], F), med


# ---- steps 3 - 5 --------------------------------------------------------------------------------------------------------
def _table(v, n, fill):
    a = np.asarray(v, np.float64).reshape(-1)
    a = np.repeat(a, n) if a.size == 1 else a
    return np.concatenate([a, np.full(n - a.size, fill)]).astype(F)


def thresholds(thr, sig, e, levels):
    """t[c][j] = (float)(threshold_j * sigma_c * e_j) in f64"""
    return np.array([[F(float(thr[j]) * float(s) * float(e[j])) for j in range(levels)] for s in sig], F)


def layer_op(w, t, la, gain, mode):
    """gain * w' of one layer; w: (cc, h, w); t: (cc,) thresholds"""
    t = np.asarray(t, F).reshape(-1, 1, 1)
    la = F(la)
    m = np.abs(w)
    if mode == HARD:
        keep = F(F(1.0) - la)
        wp = np.where(m < t, (w * keep).astype(F), w)
    else:
        z = np.copysign(np.fmax((m - t).astype(F), F(0)), w).astype(F)
        wp = fma32(la, (z - w).astype(F), w)
    return (F(gain) * wp).astype(F)


def combine(ws, cJ, D, t, la, gain, mode, residual_gain=1.0, amount=1.0, mask=None):
    """steps 3 - 4 from planes (cc, h, w): ws = [w_0 ..], cJ, D = c_0; t: (cc, J)"""
    acc = None
    for j, w in enumerate(ws):
        g = layer_op(w, t[:, j], la[j], gain[j], mode)
        acc = g if acc is None else (acc + g).astype(F)
    res = fma32(F(residual_gain), cJ, acc)
    mm = F(amount) if mask is None else (F(amount) * np.asarray(mask, F)).astype(F)
    blend = fma32(mm, (res - D).astype(F), D)
    return np.where(np.broadcast_to(mm == F(1.0), res.shape), res, blend).astype(F)


def process(d, levels=4, mode=HARD, gains=1.0, thresholds_=0.0, layer_amounts=1.0, residual_gain=1.0, amount=1.0, sigma_=None, mask=None,
            e=None, return_sigma=False, want_sigma=False):
    """The definition on an H x W x C (or H x W) f32 image; C = 4: alpha copied through. e: the noise table (default: this
    file's). sigma_: given per channel (a scalar or a list), None: estimated where a threshold of a used level is > 0 or
    want_sigma. return_sigma adds the sigma per colour channel as used."""
    img, cc, D = _planes(d)
    e = noise_table(8) if e is None else np.asarray(e, np.float64)
    gain, thr, la = _table(gains, 8, 1.0), _table(thresholds_, 8, 0.0), _table(layer_amounts, 8, 1.0)
    if sigma_ is not None:
        sig = _table(sigma_, 4, 0.0)[:cc]
    elif want_sigma or (thr[:levels] > 0).any():
        sig = sigma(d, e[0])[0]
    else:
        sig = np.zeros(cc, F)
    t = thresholds(thr, sig, e, levels)
    ws, c = [], D
    for j in range(levels):
        nxt = smooth(c, 2 ** j)
        ws.append((c - nxt).astype(F))
        c = nxt
    o = combine(ws, c, D, t, la, gain, mode, residual_gain, amount, mask)
    res = img.copy()
    res[..., :cc] = np.moveaxis(o, 0, 2)
    res = res.reshape(np.shape(d))
    return (res, sig) if return_sigma else res


# ---- the scene of the denoising measurement -----------------------------------------------------------------------------
SCENE_W, SCENE_H, SCENE_SIGMA = 128, 96, 8.0


def scene(seed, w=SCENE_W, h=SCENE_H, n_stars=15, noise=SCENE_SIGMA):
    """(truth, noisy): a sinusoidal sky plus 15 Gaussian stars of sigma 1 .. 1.8, white noise of sigma 8; f32"""
    rng = np.random.default_rng(2000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = 500.0 + 40.0 * np.sin(2 * np.pi * x / 97.0) + 30.0 * np.cos(2 * np.pi * y / 71.0)
    for _ in range(n_stars):
        cx, cy = rng.uniform(6, w - 6), rng.uniform(6, h - 6)
        s = rng.uniform(1.0, 1.8)
        peak = math.exp(rng.uniform(math.log(100.0), math.log(3000.0)))
        truth += peak * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))
    noisy = truth + rng.normal(0.0, noise, (h, w))
    return truth.astype(F), noisy.astype(F)


def rms_ratio(out, noisy, truth):
    e = lambda a: float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(truth, np.float64)) ** 2)))
    return e(out) / e(noisy)

"""numpy restatement of noise estimation (include/stacker.h, stk_noise_stat): the two exact histograms of a frame channel,
their reduction to the statistics, and the inverse-variance frame weights — written from the header's text, sharing no code
with the engine. All sums are exact integers (int64 within the header's bounds); the floating operations are the ones the
header names."""
import math

import numpy as np

NOISE_DTYPE = np.dtype([("median", "<i4"), ("mad", "<i4"), ("res_median", "<i4"), ("flags", "<i4"), ("sigma", "<f8"), ("kept", "<i8")])


def bins(depth):
    """(BV, BR)"""
    return (256, 2041) if depth == 8 else (65536, 65536)


def residual(plane):
    """Immerkaer's mask in integers over the interior pixels of one h x w plane: (h - 2) x (w - 2) int64"""
    v = plane.astype(np.int64)
    return (v[:-2, :-2] - 2 * v[:-2, 1:-1] + v[:-2, 2:] - 2 * v[1:-1, :-2] + 4 * v[1:-1, 1:-1] - 2 * v[1:-1, 2:]
            + v[2:, :-2] - 2 * v[2:, 1:-1] + v[2:, 2:])


def histograms(plane):
    """(HV, HR) of one u8 or u16 plane, uint32"""
    bv, br = bins(plane.dtype.itemsize * 8)
    hv = np.bincount(plane.reshape(-1).astype(np.int64), minlength=bv)
    hr = np.bincount(np.minimum(np.abs(residual(plane)), br - 1).reshape(-1), minlength=br)
    return hv.astype(np.uint32), hr.astype(np.uint32)


def frame_histograms(frame):
    """a frame h x w or h x w x c -> c x (BV + BR) uint32, HV then HR per channel"""
    f = frame if frame.ndim == 3 else frame[..., None]
    return np.stack([np.concatenate(histograms(f[..., c])) for c in range(f.shape[2])])


def kth(h, k):
    """the k-th smallest key of a histogram: the first bin whose cumulative count reaches k (k = 0: bin 0)"""
    cum = np.cumsum(h.astype(np.int64))
    return min(int(np.searchsorted(cum, k, side="left")), len(h) - 1)


def from_hist(hv, hr, overflow_bin):
    hv = np.asarray(hv).astype(np.int64)
    hr = np.asarray(hr).astype(np.int64)
    bv, br = len(hv), len(hr)
    n = int(hv.sum())
    k = (n + 1) // 2
    median = kth(hv, k)
    dev = np.zeros(bv, np.int64)                                          # the histogram of |v - median|
    np.add.at(dev, np.abs(np.arange(bv) - median), hv)
    mad = kth(dev, k)
    m = int(hr.sum())
    res_median = kth(hr, (m + 1) // 2)
    s = max(1.4826 * float(res_median), 0.5)
    top = br - 2 if overflow_bin else br - 1
    prev, cut, N, zero = -1, 0, 0, False
    b2 = np.arange(br, dtype=np.int64) ** 2
    for _ in range(16):
        cut = min(int(math.floor(3.0 * s)), top)
        if cut == prev:
            break
        prev = cut
        N = int(hr[:cut + 1].sum())
        Q = int((b2[:cut + 1] * hr[:cut + 1]).sum())                    # int64, exact: below 65535^2 x 2^27
        if N == 0 or Q == 0:
            zero = True
            break
        s = math.sqrt(float(Q) / float(N)) * 1.0136
    sigma = 0.0 if zero else s / 6.0
    flags = (1 if zero else 0) | (2 if overflow_bin and cut == top else 0)
    out = np.zeros((), NOISE_DTYPE)
    out["median"], out["mad"], out["res_median"], out["flags"], out["sigma"], out["kept"] = median, mad, res_median, flags, sigma, N
    return out


def stack_stats(frames):
    """n frames -> (stats n x 4 NOISE_DTYPE with the unused channel slots zeroed, hist n x c x (BV + BR))"""
    hist = np.stack([frame_histograms(f) for f in frames])
    depth = frames[0].dtype.itemsize * 8
    bv, _ = bins(depth)
    stats = np.zeros((len(frames), 4), NOISE_DTYPE)
    for i in range(hist.shape[0]):
        for c in range(hist.shape[1]):
            stats[i, c] = from_hist(hist[i, c, :bv], hist[i, c, bv:], depth == 16)
    return stats, hist


def weights(stats, channels, gain=None, include=None, user=None, sigma_floor=0.25):
    """n x 4 stats -> n float32 weights"""
    n = stats.shape[0]
    C = min(channels, 3)
    V = [0.0] * n
    ref = None
    for i in range(n):
        if include is not None and not include[i]:
            continue
        if ref is None:
            ref = i
        v = 0.0
        for c in range(C):
            g = 1.0 if gain is None else float(np.float32(gain[i][c]))
            t = g * max(float(stats[i, c]["sigma"]), float(sigma_floor))
            v = v + t * t
        V[i] = v
    out = np.zeros(n, np.float32)
    for i in range(n):
        if include is not None and not include[i]:
            continue
        u = 1.0 if user is None else float(np.float32(user[i]))
        out[i] = np.float32(u * V[ref] / V[i])
    return out

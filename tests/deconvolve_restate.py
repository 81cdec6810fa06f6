"""Numpy restatement of deconvolution (include/stacker.h, "deconvolution"), written from the header's definition, not from
the engine's code: whole-image array arithmetic in f32, every fma through local_norm_restate.fma32, one numpy operation per
rounded operation, taps in the definition's order. The image planes may carry leading axes (channels, seeds): every
operation acts on the last two. The PSF functions are restated per tap with math.exp / math.pow / math.log, libm's, the
functions the C++ calls, so they compare bit for bit too. And the scene of the quality measurements."""
import math

import numpy as np

from local_norm_restate import fma32

F = np.float32
GAUSSIAN, MOFFAT = 0, 1


# ---- the PSF functions ----------------------------------------------------------------------------------------------
def positive_definite(cxx, cyy, cxy):
    if not all(math.isfinite(v) for v in (cxx, cyy, cxy)):
        return False
    det = cxx * cyy - cxy * cxy
    return cxx > 0.0 and cyy > 0.0 and math.isfinite(det) and det > 0.0


def psf_model(kind, beta, radius, cxx, cyy, cxy):
    """(2 radius + 1)^2 float32, or None where stk_psf_model refuses."""
    cxx, cyy, cxy, beta = float(cxx), float(cyy), float(cxy), float(beta)
    if not 1 <= radius <= 16 or kind not in (GAUSSIAN, MOFFAT) or not positive_definite(cxx, cyy, cxy):
        return None
    if kind == MOFFAT and not (math.isfinite(beta) and beta > 1.0):
        return None
    det = cxx * cyy - cxy * cxy
    g = (math.pow(2.0, 1.0 / beta) - 1.0) / (2.0 * math.log(2.0)) if kind == MOFFAT else 0.0
    side = 2 * radius + 1
    v, total = [], 0.0
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            x, y = float(i), float(j)
            q = ((cyy * x) * x - ((2.0 * cxy) * x) * y + (cxx * y) * y) / det
            f = math.pow(1.0 + q * g, -beta) if kind == MOFFAT else math.exp(-q / 2.0)
            v.append(f)
            total += f
    return np.array([f / total for f in v], np.float64).astype(F).reshape(side, side)


def psf_from_shapes(shapes, min_snr=0.0, scale=1.0):
    """(cxx, cyy, cxy, used), or None where stk_psf_from_shapes refuses."""
    s = np.asarray(shapes).reshape(-1)
    good = s[(s["flags"] == 0) & (s["snr"] >= min_snr)]
    if not len(good):
        return None
    k = (len(good) + 1) // 2 - 1
    s2 = float(scale) * float(scale)
    r = [float(np.sort(good[f].astype(np.float64))[k]) * s2 for f in ("cxx", "cyy", "cxy")]
    return tuple(r) + (len(good),) if positive_definite(*r) else None


def covariance(sigma_a, sigma_b, theta):
    """The covariance of a Gaussian with axes sigma_a, sigma_b, the first rotated by theta from x."""
    c, s = math.cos(theta), math.sin(theta)
    a, b = sigma_a * sigma_a, sigma_b * sigma_b
    return a * c * c + b * s * s, a * s * s + b * c * c, (a - b) * c * s


# ---- the iteration ----------------------------------------------------------------------------------------------------
def _pad(u, R):
    return np.pad(u, [(0, 0)] * (u.ndim - 2) + [(R, R), (R, R)], mode="reflect")          # BORDER_REFLECT_101


def tap_sum(P, u, R, convolve):
    """sum_j sum_i P[j+R][i+R] u(x - i, y - j) (convolve) or u(x + i, y + j), j outermost, acc = fmaf(P, u, acc) from 0.0f"""
    h, w = u.shape[-2:]
    U = _pad(u, R)
    acc = np.zeros(u.shape, F)
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            oy, ox = (R - j, R - i) if convolve else (R + j, R + i)
            acc = fma32(P[j + R, i + R], U[..., oy:oy + h, ox:ox + w], acc)
    return acc


def tv_divisor(u, lam, e2):
    gx, gy = np.zeros(u.shape, F), np.zeros(u.shape, F)
    with np.errstate(all="ignore"):
        gx[..., :, :-1] = u[..., :, 1:] - u[..., :, :-1]
        gy[..., :-1, :] = u[..., 1:, :] - u[..., :-1, :]
        n = np.sqrt(fma32(gx, gx, fma32(gy, gy, e2)))
        px, py = (gx / n).astype(F), (gy / n).astype(F)
        pl, pu = np.zeros(u.shape, F), np.zeros(u.shape, F)
        pl[..., :, 1:] = px[..., :, :-1]
        pu[..., 1:, :] = py[..., :-1, :]
        div = ((px - pl).astype(F) + (py - pu).astype(F)).astype(F)
        return np.fmax(fma32(F(-lam), div, F(1.0)), F(0.5))


def deconvolve(d, P, iterations=30, floor=1e-6, pedestal=0.0, lam=0.0, tv_eps=1e-3, amount=1.0, mask=None, force_tv=False, keep=()):
    """The definition on an H x W x C (or H x W) f32 image; C = 4: alpha copied through. keep: iteration counts whose outputs
    are returned too, as a dict {count: image}, next to the final one."""
    d = np.asarray(d, F)
    img = d[..., None] if d.ndim == 2 else d
    cc = min(img.shape[2], 3)
    P = np.asarray(P, F)
    R = (P.shape[0] - 1) // 2
    floor, pedestal, lam, amount = F(floor), F(pedestal), F(lam), F(amount)
    e2 = F(F(tv_eps) * F(tv_eps))
    with np.errstate(all="ignore"):
        D = (np.moveaxis(img[..., :cc], 2, 0) + pedestal).astype(F)
        D = np.where(np.isfinite(D) & (D >= 0), D, F(0)).astype(F)

        def output(u):
            m = amount if mask is None else (amount * np.asarray(mask, F)).astype(F)
            blend = (fma32(m, (u - D).astype(F), D) - pedestal).astype(F)
            o = np.where(np.broadcast_to(m == F(1.0), u.shape), (u - pedestal).astype(F), blend)
            res = img.copy()
            res[..., :cc] = np.moveaxis(o, 0, 2)
            return res.reshape(d.shape)
        u, kept = D, {}
        for k in range(iterations):
            A = tap_sum(P, u, R, True)
            r = (D / np.fmax(A, floor)).astype(F)
            C = tap_sum(P, r, R, False)
            v = (u * C).astype(F)
            u = (v / tv_divisor(u, lam, e2)).astype(F) if (lam > 0 or force_tv) else v
            if k + 1 in keep:
                kept[k + 1] = output(u)
        return (output(u), kept) if keep else output(u)


# ---- the scene of the quality measurements --------------------------------------------------------------------------------
SCENE_W, SCENE_H, SCENE_R = 96, 72, 6
SCENE_COV = covariance(2.0, 1.4, 0.5)


def scene(seed, w=SCENE_W, h=SCENE_H, n_stars=12, star_sigma=0.8):
    """(truth, blurred, psf, stars): 12 stars of sigma 0.8 on a slowly varying sky, blurred by an elliptical Gaussian
    (sigma 2.0 x 1.4, rotated 0.5 rad, R = 6) with mild shot noise; f32 in 16-bit counts; stars: the integer positions."""
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = 300.0 + 0.6 * x + 0.4 * y
    pos = []
    while len(pos) < n_stars:
        cx, cy = rng.uniform(14, w - 14), rng.uniform(14, h - 14)
        if all((cx - a) ** 2 + (cy - b) ** 2 >= 15 ** 2 for a, b in pos):
            pos.append((cx, cy))
    for cx, cy in pos:
        peak = math.exp(rng.uniform(math.log(4000.0), math.log(30000.0)))
        truth += peak * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * star_sigma ** 2))
    psf = psf_model(GAUSSIAN, 0.0, SCENE_R, *SCENE_COV)
    P, R = psf.astype(np.float64), SCENE_R
    T = np.pad(truth, R, mode="reflect")
    blurred = np.zeros((h, w))
    for j in range(-R, R + 1):
        for i in range(-R, R + 1):
            blurred += P[j + R, i + R] * T[R - j:R - j + h, R - i:R - i + w]
    blurred += rng.normal(0.0, 1.0, (h, w)) * np.sqrt(blurred / 8.0)
    stars = np.array([(int(round(cx)), int(round(cy))) for cx, cy in pos], np.int64)
    return truth.astype(F), blurred.astype(F), psf, stars


def rms_ratio(out, blurred, truth):
    e = lambda a: float(np.sqrt(np.mean((np.asarray(a, np.float64) - truth) ** 2)))
    return e(out) / e(blurred)


def flux_ratio(out, blurred):
    return float(np.asarray(out, np.float64).sum() / np.asarray(blurred, np.float64).sum())

"""Numpy restatement of star measurement (include/stacker.h, stk_star_measure_params): the measurement of one star on the
16-bit key (exact order statistics by sorting, the aperture sums as Python integers), the derived values, a frame's quality,
the scores and the quality weights, each written from the header's definition, not from the engine's code; and a generator of
star fields with a per-frame elliptical Gaussian PSF on a 16-bit sky. Every f64 operation is one numpy scalar operation, so
the engine's values can be compared bit for bit."""
import numpy as np

import star_deep_restate as sd
from libstacker_rs_amd import QUALITY_DTYPE, SHAPE_DTYPE, StarMeasureParameters, StarQualityParameters

F = np.float64
FWHM_PER_SIGMA = F(2.3548200450309493)
INTS = ("S", "Sx", "Sy", "Sxx", "Syy", "Sxy", "px", "py", "bg", "mad", "thr", "npix", "peak", "n_ring", "flags", "reserved")
DOUBLES = ("x", "y", "cxx", "cyy", "cxy", "fwhm", "ecc", "snr")


# ---- 1. the measurement ---------------------------------------------------------------------------------------------
def measure_one(K, px, py, mp):
    """One star's integers on the key plane K (h x w integers): a SHAPE_DTYPE record with the doubles 0."""
    h, w = K.shape
    R, Ri, Ro = int(mp.radius), int(mp.ring_inner), int(mp.ring_outer)
    o = np.zeros((), SHAPE_DTYPE)
    o["px"], o["py"] = px, py
    if px - R < 0 or py - R < 0 or px + R > w - 1 or py + R > h - 1:
        o["flags"] = 1
        return o
    dy, dx = np.mgrid[-Ro:Ro + 1, -Ro:Ro + 1]
    d2 = dx * dx + dy * dy
    yy, xx = py + dy, px + dx
    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    ring = inside & (d2 >= Ri * Ri) & (d2 <= Ro * Ro)
    vals = K[yy[ring], xx[ring]].astype(np.int64)
    n_ring = int(vals.size)
    bg = mad = 0
    if n_ring:
        k = (n_ring + 1) // 2
        bg = int(np.sort(vals)[k - 1])
        mad = int(np.sort(np.abs(vals - bg))[k - 1])
    ks = np.float32(np.float64(np.float32(mp.kappa)) * 1.4826)
    thr = max(int(min(np.ceil(np.float32(ks * np.float32(mad))), np.float32(65536.0))), int(mp.min_contrast))
    ap = d2 <= R * R
    q = [int(v) for v in K[yy[ap], xx[ap]]]
    ax, ay = [int(v) for v in dx[ap]], [int(v) for v in dy[ap]]
    v = [(g - bg) if (g - bg) >= thr else 0 for g in q]
    npix = sum(1 for t in v if t > 0)
    S = sum(v)
    o["S"], o["Sx"], o["Sy"] = S, sum(t * x for t, x in zip(v, ax)), sum(t * y for t, y in zip(v, ay))
    o["Sxx"], o["Syy"] = sum(t * x * x for t, x in zip(v, ax)), sum(t * y * y for t, y in zip(v, ay))
    o["Sxy"] = sum(t * x * y for t, x, y in zip(v, ax, ay))
    peak = max(q)
    o["bg"], o["mad"], o["thr"], o["npix"], o["peak"], o["n_ring"] = bg, mad, thr, npix, peak, n_ring
    o["flags"] = (2 if int(mp.saturation) > 0 and peak >= int(mp.saturation) else 0) | (4 if npix < int(mp.min_pixels) or S == 0 else 0)
    return o


def measure(frame, stars, mp=None, deep=None):
    """The shapes of `stars` (anything with px and py fields, or k x 2 integers) on one frame, derived values filled."""
    mp = mp or StarMeasureParameters()
    K = sd.key(frame, deep).astype(np.int64)
    s = np.asarray(stars)
    pxy = np.stack([s["px"], s["py"]], 1) if s.dtype.names else s.reshape(-1, 2)
    out = np.zeros(len(pxy), SHAPE_DTYPE)
    for k, (px, py) in enumerate(pxy):
        out[k] = measure_one(K, int(px), int(py), mp)
    return derive(out)


# ---- 2. the derived values ------------------------------------------------------------------------------------------
def derive(shapes):
    s = np.array(shapes, SHAPE_DTYPE, copy=True)
    flat = s.reshape(-1)
    for o in flat:
        for f in DOUBLES:
            o[f] = 0.0
        o["flags"] &= ~8
        if o["flags"] != 0 or o["S"] == 0:
            continue
        S = F(int(o["S"]))
        mx, my = F(int(o["Sx"])) / S, F(int(o["Sy"])) / S
        o["x"], o["y"] = F(int(o["px"])) + mx, F(int(o["py"])) + my
        cxx = F(int(o["Sxx"])) / S - mx * mx
        cyy = F(int(o["Syy"])) / S - my * my
        cxy = F(int(o["Sxy"])) / S - mx * my
        o["cxx"], o["cyy"], o["cxy"] = cxx, cyy, cxy
        tr, dd = cxx + cyy, cxx - cyy
        df = np.sqrt(dd * dd + F(4.0) * (cxy * cxy))
        l1, l2 = (tr + df) / F(2.0), (tr - df) / F(2.0)
        if not l2 > 0.0:
            o["flags"] |= 8
            continue
        o["fwhm"] = FWHM_PER_SIGMA * np.sqrt(tr / F(2.0))
        o["ecc"] = np.sqrt(max(F(1.0) - l2 / l1, F(0.0)))
        with np.errstate(divide="ignore"):
            o["snr"] = S / (max(F(1.4826) * F(int(o["mad"])), F(0.5)) * np.sqrt(F(int(o["npix"]))))
    return s


# ---- 3. frame quality, scores, weights ------------------------------------------------------------------------------
def lower_median(v):
    v = np.sort(np.asarray(v, F))
    return v[(len(v) + 1) // 2 - 1]


def frame_quality(lists):
    """One QUALITY_DTYPE record per frame from the frames' shape lists."""
    out = np.zeros(len(lists), QUALITY_DTYPE)
    for i, s in enumerate(lists):
        s = np.asarray(s, SHAPE_DTYPE).reshape(-1)
        good = s[s["flags"] == 0]
        out[i]["n_stars"], out[i]["n_measured"] = len(s), len(good)
        if len(good):
            out[i]["fwhm"], out[i]["ecc"], out[i]["snr"] = lower_median(good["fwhm"]), lower_median(good["ecc"]), lower_median(good["snr"])
            out[i]["bg"], out[i]["noise"] = lower_median(good["bg"].astype(F)), lower_median(F(1.4826) * good["mad"].astype(F))
    return out


def quality_scores(q):
    q = np.asarray(q, QUALITY_DTYPE).reshape(-1)
    out = np.zeros((len(q), 4), F)
    for i, r in enumerate(q):
        m = r["n_measured"] > 0
        out[i] = (F(1.0) / r["fwhm"] if m else 0.0, F(1.0) - r["ecc"] if m else 0.0, r["snr"], F(int(r["n_measured"])))
    return out


def quality_weights(q, p=None, reference=-1, include=None, weights=None):
    """(weights f32, include int32, rejected), or None where the header says STK_INVALID_PARAMS."""
    p = p or StarQualityParameters()
    q = np.asarray(q, QUALITY_DTYPE).reshape(-1)
    n = len(q)
    inc = np.ones(n, bool) if include is None else np.asarray(include).astype(bool)
    u = np.ones(n, np.float32) if weights is None else np.asarray(weights, np.float32)
    powers = (int(p.fwhm_power), int(p.ecc_power), int(p.snr_power))
    if n < 1 or any(k < 0 or k > 4 for k in powers) or int(p.min_measured) < 1:
        return None
    if not (np.isfinite(p.fwhm_max) and p.fwhm_max >= 0 and np.isfinite(p.ecc_max) and p.ecc_max >= 0):
        return None
    if reference < -1 or reference >= n or (reference >= 0 and (not inc[reference] or q[reference]["n_measured"] <= 0)):
        return None
    for f in ("fwhm", "ecc", "snr"):
        if not np.isfinite(q[f]).all() or (q[f] < 0).any():
            return None
    if not np.isfinite(u).all() or (u < 0).any():
        return None
    ok = np.zeros(n, bool)
    for i in range(n):
        ok[i] = inc[i] and (i == reference or (q[i]["n_measured"] >= int(p.min_measured) and (p.fwhm_max == 0 or q[i]["fwhm"] <= p.fwhm_max)
                                               and (p.ecc_max == 0 or q[i]["ecc"] <= p.ecc_max)))
    if not ok.any():
        return None
    Fm = min(F(q[i]["fwhm"]) for i in range(n) if ok[i])
    E = max(F(1.0) - F(q[i]["ecc"]) for i in range(n) if ok[i])
    Z = max(F(q[i]["snr"]) for i in range(n) if ok[i])
    out = np.zeros(n, np.float32)
    for i in range(n):
        if not ok[i]:
            continue
        w = F(u[i])
        ff = F(1.0) if q[i]["fwhm"] == 0 else Fm / F(q[i]["fwhm"])
        fe = F(1.0) if E == 0 else (F(1.0) - F(q[i]["ecc"])) / E
        fz = F(1.0) if Z == 0 else F(q[i]["snr"]) / Z
        for f, k in zip((ff, fe, fz), powers):
            for _ in range(k):
                w = w * f
        out[i] = np.float32(w)
    return out, ok.astype(np.int32), int((inc & ~ok).sum())


# ---- the generator --------------------------------------------------------------------------------------------------
def make_field(w, h, n_stars, psf, seed=0, noise_seed=None, sky=2000.0, noise_sigma=40.0, peaks=(400.0, 20000.0), channels=1, margin=16,
               shift=(0.0, 0.0)):
    """One u16 frame of a star field: n_stars elliptical Gaussians exp(-(u^2 / sa^2 + v^2 / sb^2) / 2) sampled at the pixel
    centres, (u, v) the offset from the star turned by `angle` radians, psf = (sa, sb, angle) or one circular sigma; peaks
    log-uniform in `peaks` ADU over a sky of `sky` ADU with Gaussian noise. `seed` fixes the positions and peaks,
    `noise_seed` (default: seed) the noise: frames of one field with fresh noise share `seed`. `shift` moves every star.
    Returns (frame h x w [x channels], truth k x 3 of x, y, peak)."""
    sa, sb, ang = (float(psf), float(psf), 0.0) if np.isscalar(psf) else (float(psf[0]), float(psf[1]), float(psf[2]))
    rng = np.random.default_rng(seed)
    x = rng.uniform(margin, w - 1 - margin, n_stars) + shift[0]
    y = rng.uniform(margin, h - 1 - margin, n_stars) + shift[1]
    pk = np.exp(rng.uniform(np.log(peaks[0]), np.log(peaks[1]), n_stars))
    img = np.full((h, w), float(sky))
    c, s = np.cos(ang), np.sin(ang)
    r = int(np.ceil(5.0 * max(sa, sb))) + 1
    for xs, ys, p in zip(x, y, pk):
        x0, y0 = int(round(xs)), int(round(ys))
        ya, yb, xa, xb = max(y0 - r, 0), min(y0 + r + 1, h), max(x0 - r, 0), min(x0 + r + 1, w)
        gy, gx = np.mgrid[ya:yb, xa:xb]
        du, dv = (gx - xs) * c + (gy - ys) * s, -(gx - xs) * s + (gy - ys) * c
        img[ya:yb, xa:xb] += p * np.exp(-0.5 * (du * du / (sa * sa) + dv * dv / (sb * sb)))
    nrng = np.random.default_rng(seed if noise_seed is None else noise_seed + 7919)
    img = img + nrng.normal(0.0, noise_sigma, img.shape) if noise_sigma > 0 else img
    f = np.clip(np.rint(img), 0, 65535).astype(np.uint16)
    if channels > 1:
        f = np.stack([f] * 3 + ([np.full_like(f, 65535)] if channels == 4 else []), -1)
    return f, np.stack([x, y, pk], 1)


def true_ecc(sa, sb):
    return float(np.sqrt(1.0 - (min(sa, sb) / max(sa, sb)) ** 2))

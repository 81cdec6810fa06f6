"""numpy restatement of the blot-and-compare rejection maps (include/stacker.h, stk_reject_params): the blot coordinate
under the FORWARD matrix, valid, the bilinear model, its gradient, the sample, the noise, the two tests, the grow step and
the counts. Two paths: f32 with every operation rounded on its own and the coordinate fragment and the lerp chain through
interp_restate.fma32 (the engine's operations: its maps are compared with these exactly), and f64 (the definition's
mathematics from the same f32 matrix, for reasoning). Also the quality experiment the CPU and the GPU test share: a dithered
stack with a planted trail and hot pixels, and the defect-free stack with the same noise."""
import numpy as np

import drizzle_restate as dr
from interp_restate import F, fma32


def forward_matrix(M):
    """The nine doubles of the forward matrix cast to f32 (returned as float64 holding the f32 values)."""
    m = np.asarray(M, np.float64).reshape(-1)
    if m.size == 6:
        m = np.concatenate([m, [0.0, 0.0, 1.0]])
    return m.astype(F).astype(np.float64)


def blot(clean, M, is_affine, counts=None, min_count=0, dtype=F, halo=1):
    """(B, valid) on the lattice [-halo, sw + halo) x [-halo, sh + halo): B (.. x cn, `dtype`, 0 where not valid) is the
    clean image blotted through the forward matrix M; lattice point (x, y) is at index [y + halo][x + halo]."""
    Cl = np.asarray(clean, F)
    if Cl.ndim == 2:
        Cl = Cl[..., None]
    sh, sw, cn = Cl.shape
    m = forward_matrix(M)
    y, x = np.mgrid[-halo:sh + halo, -halo:sw + halo]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if dtype == F:
            a, fx, fy = m.astype(F), x.astype(F), y.astype(F)
            X = fma32(a[0], fx, fma32(a[1], fy, a[2]))
            Y = fma32(a[3], fx, fma32(a[4], fy, a[5]))
            if not is_affine:
                W = fma32(a[6], fx, fma32(a[7], fy, a[8]))
                X, Y = X / W, Y / W
        else:
            fx, fy = x.astype(np.float64), y.astype(np.float64)
            X = m[0] * fx + m[1] * fy + m[2]
            Y = m[3] * fx + m[4] * fy + m[5]
            if not is_affine:
                W = m[6] * fx + m[7] * fy + m[8]
                X, Y = X / W, Y / W
        finite = (np.abs(X) < 1e9) & (np.abs(Y) < 1e9)
    Xs, Ys = np.where(finite, X, dtype(-1e5)), np.where(finite, Y, dtype(-1e5))
    flx, fly = np.floor(Xs), np.floor(Ys)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    ax, ay = (Xs - flx).astype(dtype), (Ys - fly).astype(dtype)
    valid = finite & (ix >= 0) & (ix + 1 <= sw - 1) & (iy >= 0) & (iy + 1 <= sh - 1)
    jx, jy = np.clip(ix, 0, max(sw - 2, 0)), np.clip(iy, 0, max(sh - 2, 0))
    if sw < 2 or sh < 2:
        return np.zeros(valid.shape + (cn,), dtype), np.zeros(valid.shape, bool)
    if counts is not None:
        cnt = np.asarray(counts)
        mc = int(min_count)
        valid = valid & (cnt[jy, jx] >= mc) & (cnt[jy, jx + 1] >= mc) & (cnt[jy + 1, jx] >= mc) & (cnt[jy + 1, jx + 1] >= mc)
    c00, c01 = Cl[jy, jx].astype(dtype), Cl[jy, jx + 1].astype(dtype)
    c10, c11 = Cl[jy + 1, jx].astype(dtype), Cl[jy + 1, jx + 1].astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == F:
            t0 = fma32(ax[..., None], c01 - c00, c00)
            t1 = fma32(ax[..., None], c11 - c10, c10)
            B = fma32(ay[..., None], t1 - t0, t0)
        else:
            t0 = c00 + ax[..., None] * (c01 - c00)
            t1 = c10 + ax[..., None] * (c11 - c10)
            B = t0 + ay[..., None] * (t1 - t0)
    return np.where(valid[..., None], B, dtype(0)).astype(dtype), valid


def gradient(B, valid):
    """D on the lattice without its outermost ring: the largest |B(n) - B| over the valid ones of the four neighbours, in
    the header's order, from 0, by fmax."""
    Bc = B[1:-1, 1:-1]
    D = np.zeros_like(Bc)
    with np.errstate(invalid="ignore", over="ignore"):
        for sl in ((slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None)), (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1))):
            D = np.where(valid[sl][..., None], np.fmax(D, np.abs(B[sl] - Bc)), D)
    return np.where(valid[1:-1, 1:-1][..., None], D, B.dtype.type(0))            # (a point that is not valid has no D: 0)


def reject_frame(frame, M, is_affine, alpha, clean, p, counts=None, gain=None, offset=None, map_in=None, dtype=F):
    """One frame: (map sh x sw float32, rejected, judged, details). p: an object with snr1, snr2, scale1, scale2, read_noise,
    poisson_gain, min_count (libstacker_rs_amd.RejectParameters). details: dict of B, D, valid, judged, f1, f2, u."""
    dt = dtype
    src = np.asarray(frame)
    if src.ndim == 2:
        src = src[..., None]
    sh, sw, cn = src.shape
    B1, valid1 = blot(clean, M, is_affine, counts, p.min_count, dt, halo=1)
    D = gradient(B1, valid1)
    B, valid = B1[1:-1, 1:-1], valid1[1:-1, 1:-1]
    g = np.ones(cn, dt) if gain is None else np.asarray(gain, F).reshape(cn).astype(dt)
    o = np.zeros(cn, dt) if offset is None else np.asarray(offset, F).reshape(cn).astype(dt)
    mi = None if map_in is None else np.asarray(map_in, F)
    judged = valid.copy()
    if mi is not None:
        judged &= mi > 0
    with np.errstate(invalid="ignore", over="ignore"):
        u = (src.astype(dt) * dt(F(alpha))) * g + o
        e = np.abs(u - B)
        rn, pg = dt(F(p.read_noise)), dt(F(p.poisson_gain))
        sigma = np.sqrt(rn * rn + pg * np.fmax(B, dt(0)))
        t1 = (e > dt(F(p.scale1)) * D + dt(F(p.snr1)) * sigma).any(axis=2)
        t2 = (e > dt(F(p.scale2)) * D + dt(F(p.snr2)) * sigma).any(axis=2)
    f1 = judged & t1
    pad = np.zeros((sh + 2, sw + 2), bool)
    pad[1:-1, 1:-1] = f1
    around = np.zeros((sh, sw), bool)
    for dy in range(3):
        for dx in range(3):
            around |= pad[dy:dy + sh, dx:dx + sw]
    f2 = judged & around & t2
    rej = f1 | f2
    keep = np.ones((sh, sw), F) if mi is None else mi
    out = np.where(rej, F(0), keep).astype(F)
    return out, int(rej.sum()), int(judged.sum()), dict(B=B, D=D, valid=valid, judged=judged, f1=f1, f2=f2, u=u)


def reject_maps(frames, warps, is_affine, alpha, clean, p, counts=None, gain=None, offset=None, maps_in=None, include=None, dtype=F):
    """The whole call: (maps n x sh x sw float32, rejected n int64, judged n int64). An excluded frame's plane is all ones
    and its counts 0 (the engine does not write the plane)."""
    n = len(frames)
    f0 = np.asarray(frames[0])
    sh, sw = f0.shape[:2]
    maps = np.ones((n, sh, sw), F)
    rej, jud = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        if include is not None and not include[i]:
            continue
        maps[i], rej[i], jud[i], _ = reject_frame(frames[i], warps[i], is_affine, alpha, clean, p, counts,
                                                  None if gain is None else gain[i], None if offset is None else offset[i],
                                                  None if maps_in is None else maps_in[i], dtype)
    return maps, rej, jud


# ---- the clean image of the CPU experiments ---------------------------------------------------------------------------
def warped_samples(frames, warps, alpha):
    """(samples n x sh x sw x cn f64, participates n x sh x sw) of translated frames on frame 0's grid: the f64 bilinear
    sample at (x - sx, y - sy); a frame participates where every tap that carries weight is inside it (coverage = 1)."""
    n = len(frames)
    f0 = np.asarray(frames[0])
    sh, sw = f0.shape[:2]
    y, x = np.mgrid[0:sh, 0:sw].astype(np.float64)
    S, P = [], []
    for f, M in zip(frames, warps):
        f = np.asarray(f, np.float64).reshape(sh, sw, -1) * float(F(alpha))
        M = np.asarray(M, np.float64).reshape(3, 3)
        u, v = x - M[0, 2], y - M[1, 2]
        ix, iy = np.floor(u).astype(int), np.floor(v).astype(int)
        ax, ay = u - ix, v - iy
        s, part = np.zeros(f.shape), np.ones((sh, sw), bool)
        for dy, wy in ((0, 1 - ay), (1, ay)):
            for dx, wx in ((0, 1 - ax), (1, ax)):
                wgt = wx * wy
                ok = (ix + dx >= 0) & (ix + dx < sw) & (iy + dy >= 0) & (iy + dy < sh)
                part &= ok | (wgt == 0)
                s += np.where(ok, wgt, 0.0)[..., None] * f[np.clip(iy + dy, 0, sh - 1), np.clip(ix + dx, 0, sw - 1)]
        S.append(s)
        P.append(part)
    return np.stack(S), np.stack(P)


def median_clean(frames, warps, alpha):
    """(clean sh x sw x cn f32, counts sh x sw int32): the coverage-aware median of translated frames, the restated
    stk_quantile_stack_weighted at 0.5 with unit records (test_cpu_robust.robust_quantile_restate) over f64 samples."""
    from test_cpu_robust import robust_quantile_restate
    S, P = warped_samples(frames, warps, alpha)
    n, cn = S.shape[0], S.shape[-1]
    out, cnt = robust_quantile_restate(S, P, np.ones((n, cn), F), np.zeros((n, cn), F), np.ones(n, F), 0.5)
    return out, cnt.astype(np.int32)


# ---- the quality experiment -------------------------------------------------------------------------------------------
RH, RW, RN = 40, 48, 8
TRAIL_FRAME, HOT_FRAMES, N_HOT = 5, (2, 7), 6


def trail_profile(h=RH, w=RW):
    """60 exp(-0.5 (d / 0.7)^2), d the distance from the line y = 3 + 0.55 x, in grey levels."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.abs(y - 3.0 - 0.55 * x) / np.sqrt(1.0 + 0.55 ** 2)
    return 60.0 * np.exp(-0.5 * (d / 0.7) ** 2)


def reject_stack(seed):
    """(frames u8 8 x 40 x 48 x 1 with the planted defects, the defect-free frames with the same noise, forward warps,
    planted: n x h x w grey levels added). Scene drizzle_restate.quality_scene(seed, fmax = 0.25), box-integrated; frame k at
    offset sx = (k % 4) / 4 + 2 (k // 8), sy = ((k // 4) % 4) / 4 - (k % 3) with that translation as its forward warp; a
    trail in frame 5, six hot pixels of +60 at random interior places in each of frames 2 and 7; Gaussian noise of sigma = 2
    grey levels from one seeded generator; rounded and clipped to u8."""
    scene = dr.quality_scene(seed, fmax=0.25)
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:RH, 0:RW].astype(np.float64)
    bad, good, warps = [], [], []
    planted = np.zeros((RN, RH, RW))
    planted[TRAIL_FRAME] = trail_profile()
    for k in HOT_FRAMES:
        ys, xs = rng.integers(4, RH - 4, N_HOT), rng.integers(4, RW - 4, N_HOT)
        planted[k, ys, xs] = 60.0
    for k in range(RN):
        sx, sy = (k % 4) / 4.0 + 2 * (k // 8), ((k // 4) % 4) / 4.0 - (k % 3)
        img = scene(x + sx, y + sy, box=True) + rng.normal(0.0, 2.0, (RH, RW))
        good.append(np.clip(np.rint(img), 0, 255).astype(np.uint8)[..., None])
        bad.append(np.clip(np.rint(img + planted[k]), 0, 255).astype(np.uint8)[..., None])
        M = np.eye(3)
        M[0, 2], M[1, 2] = sx, sy
        warps.append(M)
    return np.stack(bad), np.stack(good), warps, planted


def quality_params():
    from libstacker_rs_amd import RejectParameters
    return RejectParameters(snr1=4.0, snr2=3.0, scale1=1.2, scale2=0.7, read_noise=2.0 / 255.0, poisson_gain=0.0, min_count=3)


def quality_measures(maps, judged, planted, with_maps, without_maps, reference, border=8):
    """The three measures of the experiment: (share of the judged planted core pixels (profile >= 15 grey levels, and the
    hot pixels) that were rejected; share of the judged pixels outside the trail's wings (profile < 1.2) and not planted
    that were rejected; RMS error of the drizzle with the maps / RMS error of the drizzle without them, both against the
    drizzle of the defect-free stack, `border` output pixels in)."""
    maps, judged = np.asarray(maps), np.asarray(judged, bool)
    rej = (maps == 0) & judged
    core = (planted >= 15.0) & judged
    cleanpix = (planted < 1.2) & judged
    inner = (slice(border, -border), slice(border, -border))
    ref = np.asarray(reference, np.float64)[..., 0][inner]
    e_with = float(np.sqrt(np.mean((np.asarray(with_maps, np.float64)[..., 0][inner] - ref) ** 2)))
    e_without = float(np.sqrt(np.mean((np.asarray(without_maps, np.float64)[..., 0][inner] - ref) ** 2)))
    return float(rej[core].sum()) / max(int(core.sum()), 1), float(rej[cleanpix].sum()) / max(int(cleanpix.sum()), 1), \
        e_with / e_without, e_with, e_without


__all__ = ["F", "forward_matrix", "blot", "gradient", "reject_frame", "reject_maps", "warped_samples", "median_clean",
           "trail_profile", "reject_stack", "quality_params", "quality_measures", "RH", "RW", "RN", "TRAIL_FRAME", "HOT_FRAMES"]

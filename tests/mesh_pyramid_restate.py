"""Coarse-to-fine local alignment, restated in numpy (include/stacker.h, "coarse-to-fine local alignment"): the box pyramid
of the integer grey, the level matrices, the seeded estimation of one level (f32 steps emulated as in
interp_restate.fma32, sums in f64: test_cpu_mesh.local_align_restate's arithmetic with a seed, a level shift and the
level's max_shift) and the fill on the carried validity. `pyramid_align_restate` returns every level's result, not only
the last. Checked in test_cpu_mesh_pyramid.py; the GPU tests (test_gpu_mesh_pyramid.py) compare the engine against it."""
import numpy as np

from interp_restate import F, invert
from test_cpu_local import grey_restate
from test_cpu_mesh import _lerp, _near, coords32, grid_restate, mesh_fill_restate


def box_pyramid_restate(g, levels):
    """[g^0, .., g^(levels-1)] of an integer grey plane: (a + b + c + d + 2) >> 2 over 2 x 2, an odd last column or row dropped."""
    out = [np.asarray(g, np.int64)]
    for _ in range(1, levels):
        a = out[-1]
        h, w = a.shape[0] >> 1, a.shape[1] >> 1
        a = a[:2 * h, :2 * w]
        out.append((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2)
    return out


def invert64(M, is_affine):
    """interp_restate.invert before its cast to f32: the double inverse the level matrices are formed from (the CPU tests
    hold its f32 cast to `invert`)."""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(-1)]
    if len(m) == 6:
        m += [0.0, 0.0, 1.0]
    if is_affine:
        D = m[0] * m[4] - m[1] * m[3]
        D = 1.0 / D if D != 0 else 0.0
        a11, a22, a12, a21 = m[4] * D, m[0] * D, -m[1] * D, -m[3] * D
        return [a11, a12, -a11 * m[2] - a12 * m[5], a21, a22, -a21 * m[2] - a22 * m[5], 0.0, 0.0, 1.0]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    if d == 0.0:
        return [0.0] * 9
    d = 1.0 / d
    return [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def level_matrix64(inv, level):
    """C_l^-1 inv C_l in double (Python floats: every operation rounded on its own), in the header's order of operations."""
    s = float(1 << level)
    c, i_s = 0.5 * (s - 1.0), 1.0 / s
    cs = c * i_s
    A = []
    for r in range(3):
        A += [inv[3 * r] * s, inv[3 * r + 1] * s, (inv[3 * r] * c + inv[3 * r + 1] * c) + inv[3 * r + 2]]
    o = [0.0] * 9
    for j in range(3):
        o[j] = A[j] * i_s - cs * A[6 + j]
        o[3 + j] = A[3 + j] * i_s - cs * A[6 + j]
        o[6 + j] = A[6 + j]
    return o


def level_matrix_restate(M, is_affine, level):
    """The f32 destination -> source matrix of level `level` (as float64 holding the f32 values); level 0 is `invert`."""
    if level == 0:
        return invert(M, is_affine)
    return np.asarray(level_matrix64(invert64(M, is_affine), level), np.float64).astype(F).astype(np.float64)


def level_estimate_restate(g0, gi, inv, is_affine, p, level, gw, gh, seed, m_seed):
    """Steps 1 - 7 on the level images g0, gi (int64) from the seeds: (d gh x gw x 2 f32, status, m bool, near bool). A node
    that fails keeps its seed and its m_seed."""
    h, w = g0.shape
    sh, sw = gi.shape
    Tx, Ty = np.zeros_like(g0), np.zeros_like(g0)
    Tx[:, 1:-1] = g0[:, 2:] - g0[:, :-2]
    Ty[1:-1, :] = g0[2:, :] - g0[:-2, :]
    gf = gi.astype(F)
    d = np.array(seed, F)
    m = np.array(m_seed, bool)
    status = np.zeros((gh, gw), np.int32)
    near = np.zeros((gh, gw), bool)
    eps2 = float(F(p.epsilon)) ** 2
    ms2 = float(F(p.max_shift) * F(2.0 ** -level)) ** 2
    me4 = 4.0 * float(F(p.min_eig))
    for j in range(gh):
        for k in range(gw):
            cx, cy, r = (k * p.step) >> level, (j * p.step) >> level, p.radius
            xa, xb, ya, yb = max(cx - r, 1), min(cx + r, w - 2), max(cy - r, 1), min(cy + r, h - 2)
            if xa > xb or ya > yb:
                status[j, k] = -1
                continue
            ys, xs = [a.reshape(-1) for a in np.mgrid[ya:yb + 1, xa:xb + 1]]
            T, tx, ty = g0[ys, xs].astype(F), Tx[ys, xs], Ty[ys, xs]
            dx, dy = F(seed[j, k, 0]), F(seed[j, k, 1])
            st = 0
            for it in range(1, p.max_iters + 1):
                ix, iy, ax, ay, finite = coords32(inv, xs.astype(F) + dx, ys.astype(F) + dy, is_affine)
                live = finite & (ix >= 0) & (ix + 1 <= sw - 1) & (iy >= 0) & (iy + 1 <= sh - 1)
                n = int(live.sum())
                if 2 * n < xs.size:
                    st = -2
                    break
                x0, y0, a_x, a_y = ix[live], iy[live], ax[live], ay[live]
                I = _lerp(a_x, a_y, gf[y0, x0], gf[y0, x0 + 1], gf[y0 + 1, x0], gf[y0 + 1, x0 + 1])
                e = (I - T[live]).astype(F).astype(np.float64)
                lx, ly = tx[live], ty[live]
                Sxx, Sxy, Syy = float((lx * lx).sum()), float((lx * ly).sum()), float((ly * ly).sum())
                bx, by = float((lx * e).sum()), float((ly * e).sum())
                dif = Sxx - Syy
                lam = 0.5 * ((Sxx + Syy) - np.sqrt(dif * dif + 4.0 * (Sxy * Sxy)))
                det = Sxx * Syy - Sxy * Sxy
                near[j, k] |= _near(lam, me4 * n) or (det != 0 and _near(Sxx * Syy, Sxy * Sxy))
                if det <= 0 or lam < me4 * n:
                    st = -3
                    break
                Dx = 2.0 * (Syy * bx - Sxy * by) / det
                Dy = 2.0 * (Sxx * by - Sxy * bx) / det
                dx, dy = F(float(dx) - Dx), F(float(dy) - Dy)
                d2 = float(dx) * float(dx) + float(dy) * float(dy)
                near[j, k] |= _near(d2, ms2)
                if not d2 <= ms2:
                    st = -4
                    break
                st = it
                D2 = Dx * Dx + Dy * Dy
                near[j, k] |= _near(D2, eps2) and eps2 > 0
                if D2 < eps2:
                    break
            status[j, k] = st
            if st > 0:
                d[j, k] = (dx, dy)
                m[j, k] = True
    return d, status, m, near


def carried_fill_restate(d, m, passes):
    """The fill on (d, m): mesh_fill_restate's arithmetic with m in place of status > 0; a hole with a valid in-grid 3 x 3
    neighbour counts as valid from the next pass on. Returns (d, m)."""
    m = np.array(m, bool)
    out = mesh_fill_restate(d, m.astype(np.int32), passes)
    gh, gw = m.shape
    for _ in range(passes):
        pad = np.zeros((gh + 2, gw + 2), bool)
        pad[1:-1, 1:-1] = m
        m = np.logical_or.reduce([pad[1 + dj:1 + dj + gh, 1 + dk:1 + dk + gw] for dj in (-1, 0, 1) for dk in (-1, 0, 1)])
    return out, m


def pyramid_align_restate(frame0, frame, M, is_affine, p, levels, seed_shift=None):
    """stk_local_align_pyramid for one frame: a list indexed by level of dicts with the estimation's `d_est`, `status`,
    `m_est`, `near`, the level's `seed` and the carried `d`, `m` after the fill. The call's field is [0]["d"], its status
    plane [0]["status"]. seed_shift: {level: (sx, sy)} added to every seed of that level (the perturbation check)."""
    p0, pi = box_pyramid_restate(grey_restate(frame0), levels), box_pyramid_restate(grey_restate(frame), levels)
    h, w = p0[0].shape
    gw, gh = grid_restate(w, h, p.step)
    out = [None] * levels
    seed, m_seed = np.zeros((gh, gw, 2), F), np.zeros((gh, gw), bool)
    for l in range(levels - 1, -1, -1):
        if seed_shift and l in seed_shift:
            seed = (seed + np.asarray(seed_shift[l], F)).astype(F)
        inv = level_matrix_restate(M, is_affine, l)
        d_est, status, m_est, near = level_estimate_restate(p0[l], pi[l], inv, is_affine, p, l, gw, gh, seed, m_seed)
        d, m = carried_fill_restate(d_est, m_est, p.fill)
        out[l] = dict(seed=seed, d_est=d_est, status=status, m_est=m_est, near=near, d=d, m=m)
        seed, m_seed = (F(2) * d).astype(F), m
    return out


def pyramid_refusal_restate(w, h, step, levels):
    """The quantity stk_local_align_pyramid refuses first among its own three checks, or None: "levels", "step", "size"."""
    if not 1 <= levels <= 4:
        return "levels"
    if (step >> (levels - 1)) < 4:
        return "step"
    if (min(w, h) >> (levels - 1)) < 16:
        return "size"
    return None


def gpu_tolerance(levels):
    """|d - d_restated| in px: each level adds the single-level test's 1e-5 (the order of the f64 additions) and a seed's
    error doubles on the way down: 1e-5 (2^levels - 1)."""
    return 1e-5 * (2 ** levels - 1)


def seed_bound(levels, level):
    """The error a seed of `level` may carry under gpu_tolerance: twice the level above's, 1e-5 (2^(levels - level) - 2)."""
    return 1e-5 * (2 ** (levels - level) - 2)


# ---- the cases the GPU tests run and the CPU perturbation check qualifies ----------------------------------------------
def log_cosines(rng, n_cos, fmin, fmax):
    """A texture of n_cos cosines with |f| log-uniform in [fmin, fmax] cycles/px and uniform direction, values in [-1, 1]."""
    f = np.exp(rng.uniform(np.log(fmin), np.log(fmax), n_cos))
    th = rng.uniform(0, 2 * np.pi, n_cos)
    fx, fy = f * np.cos(th), f * np.sin(th)
    ph, am = rng.uniform(0, 2 * np.pi, n_cos), rng.uniform(0.2, 1.0, n_cos)

    def fn(x, y):
        v = np.zeros(np.broadcast(x, y).shape)
        for k in range(n_cos):
            v = v + am[k] * np.cos(2 * np.pi * (fx[k] * x + fy[k] * y) + ph[k])
        return v / am.sum()
    return fn


def smooth_field(rng, x, y, amp, wavelength):
    """One cosine per axis of amplitude amp[0] .. amp[1] px and wavelength[0] .. wavelength[1] px: H x W x 2."""
    u = np.zeros(x.shape + (2,))
    for c in range(2):
        a = rng.uniform(*amp)
        lam = rng.uniform(*wavelength, 2)
        th, ph = rng.uniform(0, 2 * np.pi, 2)
        u[..., c] = a * np.cos(2 * np.pi * (np.cos(th) * x / lam[0] + np.sin(th) * y / lam[1]) + ph)
    return u


GPU_CASES = {            # name: (w, h, channels, is_affine, levels, frames, seed)
    "bgr-homography-3": (96, 80, 3, False, 3, 4, 11),
    "grey-affine-2-odd": (101, 77, 1, True, 2, 4, 12),
    "bgra-homography-3-odd": (101, 77, 4, False, 3, 3, 13),
    "grey-affine-3": (96, 80, 1, True, 3, 3, 14),
}


def gpu_case(name):
    """(frames n x H x W x C u8, warps n x 3 x 3, is_affine, MeshParameters, levels): frame 0 is the scene; frame i shows it
    through a rotation of up to 3 degrees with a few pixels of shift and a planted smooth field of 4 .. 6 px."""
    from libstacker_rs_amd import MeshParameters
    w, h, cn, affine, levels, n, seed = GPU_CASES[name]
    rng = np.random.default_rng(seed)
    tex = log_cosines(rng, 20, 0.006, 0.12)
    chan = [log_cosines(rng, 6, 0.01, 0.1) for _ in range(cn)]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames, warps = [], []
    for i in range(n):
        M = np.eye(3)
        u = np.zeros((h, w, 2))
        if i:
            a = np.radians(rng.uniform(-3, 3))
            c, s = np.cos(a), np.sin(a)
            cx, cy = w / 2, h / 2
            M = np.array([[c, -s, cx - c * cx + s * cy + rng.uniform(-3, 3)], [s, c, cy - s * cx - c * cy + rng.uniform(-3, 3)], [0, 0, 1.0]])
            if not affine:
                M[2, :2] = rng.uniform(-2e-5, 2e-5, 2)
        # source pixel q of frame i sits at destination P = M q; it shows the scene at P + u(P)
        P = M @ np.stack([x.ravel(), y.ravel(), np.ones(x.size)])
        X, Y = (P[0] / P[2]).reshape(h, w), (P[1] / P[2]).reshape(h, w)
        if i:
            u = smooth_field(rng, X, Y, (4.0, 6.0), (150.0, 220.0))
        X, Y = X + u[..., 0], Y + u[..., 1]
        f = np.stack([128.0 + 80.0 * tex(X, Y) + 25.0 * ch(X, Y) for ch in chan], axis=-1)
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        warps.append(M)
    p = MeshParameters(step=16, radius=6, max_iters=10, epsilon=0.01, max_shift=16.0, min_eig=1.0, fill=2)
    return np.stack(frames), np.stack(warps), affine, p, levels


_RESTATED = {}


def gpu_case_restated(name):
    """gpu_case(name) + the restatement of every moving frame (a list by frame index, entry 0 None), computed once."""
    if name not in _RESTATED:
        frames, warps, affine, p, levels = gpu_case(name)
        res = [None] + [pyramid_align_restate(frames[0], frames[i], warps[i], affine, p, levels) for i in range(1, len(frames))]
        _RESTATED[name] = (frames, warps, affine, p, levels, res)
    return _RESTATED[name]

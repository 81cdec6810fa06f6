"""Local alignment, CPU side: the numpy restatements of the definition (include/stacker.h, stk_mesh_params) that the GPU
tests (test_gpu_mesh.py) compare the engine against — `local_align_restate` (the estimation: f32 steps emulated as in
interp_restate.fma32, sums in f64), `mesh_fill_restate`, `mesh_field_restate` (the field's interpolation) and
`mesh_fold_restate` (the fold's sample at displaced coordinates) — checked here against closed forms, the four invalid
codes by construction, the quality stack that shows what the feature buys, and the ctypes mirrors."""
import ctypes

import numpy as np
import pytest

from interp_restate import F, fma32, invert
from libstacker_rs_amd import MeshParameters, _ffi, mesh_grid
from test_cpu_local import grey_restate

BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = 0, 1, 2, 3, 4
NEAR = 1e-9                      # a decision quantity within this relative distance of its threshold is "near"


def grid_restate(w, h, step):
    return (w - 1 + step - 1) // step + 1, (h - 1 + step - 1) // step + 1


def coords32(inv, fx, fy, is_affine):
    """The fold's coordinates at (fx, fy) (f32 arrays) under warp_subpixel_bits = 0: (ix, iy, ax, ay, finite)."""
    m = np.asarray(inv, np.float64).astype(F)
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    X = fma32(m[0], fx, fma32(m[1], fy, m[2]))
    Y = fma32(m[3], fx, fma32(m[4], fy, m[5]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if not is_affine:
            W = fma32(m[6], fx, fma32(m[7], fy, m[8]))
            X, Y = (X / W).astype(F), (Y / W).astype(F)
        finite = (np.abs(X) < F(1e9)) & (np.abs(Y) < F(1e9))
    Xs, Ys = np.where(finite, X, F(0)), np.where(finite, Y, F(0))
    flx, fly = np.floor(Xs), np.floor(Ys)
    ix = np.where(finite, flx, -100000).astype(np.int64)
    iy = np.where(finite, fly, -100000).astype(np.int64)
    ax = np.where(finite, Xs - flx, F(0)).astype(F)
    ay = np.where(finite, Ys - fly, F(0)).astype(F)
    return ix, iy, ax, ay, finite


def _lerp(ax, ay, p00, p01, p10, p11):
    t0 = fma32(ax, p01 - p00, p00)
    t1 = fma32(ax, p11 - p10, p10)
    return fma32(ay, t1 - t0, t0)


def _near(a, b):
    return abs(a - b) <= NEAR * max(abs(a), abs(b))


def local_align_restate(frame0, frame, M, is_affine, p: MeshParameters):
    """The estimation of the definition for one frame: (field gh x gw x 2 f32, status gh x gw int32, near gh x gw bool).
    near: some decision of the node (texture, shift, convergence) lay within a relative 1e-9 of its threshold."""
    g0, gi = grey_restate(frame0), grey_restate(frame)
    h, w = g0.shape
    sh, sw = gi.shape
    inv = invert(M, is_affine)
    gw, gh = grid_restate(w, h, p.step)
    Tx, Ty = np.zeros_like(g0), np.zeros_like(g0)
    Tx[:, 1:-1] = g0[:, 2:] - g0[:, :-2]
    Ty[1:-1, :] = g0[2:, :] - g0[:-2, :]
    gf = gi.astype(F)
    field = np.zeros((gh, gw, 2), F)
    status = np.zeros((gh, gw), np.int32)
    near = np.zeros((gh, gw), bool)
    eps2 = float(F(p.epsilon)) ** 2
    ms2 = float(F(p.max_shift)) ** 2
    me4 = 4.0 * float(F(p.min_eig))
    for j in range(gh):
        for k in range(gw):
            cx, cy, r = k * p.step, j * p.step, p.radius
            xa, xb, ya, yb = max(cx - r, 1), min(cx + r, w - 2), max(cy - r, 1), min(cy + r, h - 2)
            if xa > xb or ya > yb:
                status[j, k] = -1
                continue
            ys, xs = [a.reshape(-1) for a in np.mgrid[ya:yb + 1, xa:xb + 1]]
            T, tx, ty = g0[ys, xs].astype(F), Tx[ys, xs], Ty[ys, xs]
            dx, dy = F(0), F(0)
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
                field[j, k] = (dx, dy)
    return field, status, near


def mesh_fill_restate(field, status, passes):
    """`passes` Jacobi hole-filling passes: f32, valid in-grid neighbours in row-major order, kernel [1 2 1]^T [1 2 1]."""
    d = np.array(field, F)
    m = np.asarray(status) > 0
    gh, gw = m.shape
    for _ in range(passes):
        nd, nm = d.copy(), m.copy()
        for j in range(gh):
            for k in range(gw):
                if m[j, k]:
                    continue
                den, num = F(0), np.zeros(2, F)
                for dj in (-1, 0, 1):
                    for dk in (-1, 0, 1):
                        jj, kk = j + dj, k + dk
                        if 0 <= jj < gh and 0 <= kk < gw and m[jj, kk]:
                            wgt = F((2 - abs(dj)) * (2 - abs(dk)))
                            den = F(den + wgt)
                            num = (num + wgt * d[jj, kk]).astype(F)
                if den > 0:
                    nd[j, k] = (num / den).astype(F)
                    nm[j, k] = True
        d, m = nd, nm
    return d


def mesh_field_restate(field, w, h, step):
    """The displaced coordinates (fx, fy) of every destination pixel, f32; field None: the pixel's own."""
    y, x = np.mgrid[0:h, 0:w]
    if field is None:
        return x.astype(F), y.astype(F)
    D = np.asarray(field, F)
    gh, gw = D.shape[:2]
    k, j = x // step, y // step
    k1, j1 = np.minimum(k + 1, gw - 1), np.minimum(j + 1, gh - 1)
    u = (x - k * step).astype(F) * F(1.0 / step)
    v = (y - j * step).astype(F) * F(1.0 / step)
    d = []
    for c in range(2):
        t0 = fma32(u, D[j, k1, c] - D[j, k, c], D[j, k, c])
        t1 = fma32(u, D[j1, k1, c] - D[j1, k, c], D[j1, k, c])
        d.append(fma32(v, t1 - t0, t0))
    return (x.astype(F) + d[0]).astype(F), (y.astype(F) + d[1]).astype(F)


def _border(p, n, mode):
    """border_interp of the fold on an index array: the index inside, -1 for a BORDER_CONSTANT tap outside."""
    p = np.asarray(p, np.int64).copy()
    out = (p < 0) | (p >= n)
    if mode == BORDER_CONSTANT:
        return np.where(out, -1, p)
    if mode == BORDER_REPLICATE:
        return np.clip(p, 0, n - 1)
    if mode in (BORDER_REFLECT, BORDER_REFLECT_101):
        if n == 1:
            return np.zeros_like(p)
        delta = 1 if mode == BORDER_REFLECT_101 else 0
        while ((p < 0) | (p >= n)).any():
            p = np.where(p < 0, -p - 1 + delta, np.where(p >= n, n - 1 - (p - n) - delta, p))
        return p
    return np.mod(p, n)         # BORDER_WRAP


def mesh_fold_restate(frame, M, is_affine, alpha, field, step, border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), dsize=None):
    """The linear fold's sample of every destination pixel at the coordinates displaced by `field` (None: the plain
    fold's): H x W x C f32, every operation rounded on its own."""
    f = np.asarray(frame)
    if f.ndim == 2:
        f = f[..., None]
    sh, sw, cn = f.shape
    h, w = dsize or (sh, sw)
    fx, fy = mesh_field_restate(field, w, h, step)
    ix, iy, ax, ay, finite = coords32(invert(M, is_affine), fx, fy, is_affine)
    x0, x1 = _border(ix, sw, border_mode), _border(ix + 1, sw, border_mode)
    y0, y1 = _border(iy, sh, border_mode), _border(iy + 1, sh, border_mode)
    if border_mode == BORDER_CONSTANT:
        x0, x1, y0, y1 = (np.where(finite, a, -1) for a in (x0, x1, y0, y1))
    else:
        x0, x1, y0, y1 = (np.where(finite, a, 0) for a in (x0, x1, y0, y1))
    out = np.empty((h, w, cn), F)
    for c in range(cn):
        bv = F(border_value[c])

        def tap(yy, xx):
            ok = (xx >= 0) & (yy >= 0)
            v = f[np.maximum(yy, 0), np.maximum(xx, 0), c].astype(F) * F(alpha)
            return np.where(ok, v, bv).astype(F)
        out[..., c] = _lerp(ax, ay, tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1))
    return out


def mesh_mean_restate(frames, warps, is_affine, alpha, fields, step, border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0)):
    """stk_mesh_stack: the samples summed in fold order in f32, x (float)(1.0 / N). fields[i] None: no displacement."""
    acc = None
    for fr, M, D in zip(frames, warps, fields):
        s = mesh_fold_restate(fr, M, is_affine, alpha, D, step, border_mode, border_value)
        acc = s if acc is None else (acc + s).astype(F)
    return (acc * F(1.0 / len(frames))).astype(F)


# ---- the quality stack: a cosine scene seen through a smooth displacement field per frame -----------------------------
QM = dict(h=120, w=157, n=8, seed=3, n_cos=14, fmax=0.12, amp=(1.0, 2.5), wavelength=(130.0, 170.0), noise=2.0, margin=12,
          mesh=MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=2))


def _cosines(rng, n_cos, fmax):
    fx, fy = rng.uniform(-fmax, fmax, n_cos), rng.uniform(-fmax, fmax, n_cos)
    ph, am = rng.uniform(0, 2 * np.pi, n_cos), rng.uniform(0.2, 1.0, n_cos)

    def fn(x, y):
        v = np.zeros(np.broadcast(x, y).shape)
        for k in range(n_cos):
            v = v + am[k] * np.cos(2 * np.pi * (fx[k] * x + fy[k] * y) + ph[k])
        return v / am.sum()
    return fn


def quality_mesh_stack():
    """(scene H x W f64 in grey levels, frames n x H x W u8, true fields n x H x W x 2). Frame 0 is the scene; frame i shows
    the scene at (x, y) + u_i(x, y), u_i two cosines per axis of 1 .. 2.5 px and 130 .. 170 px wavelength; noise, rounded."""
    rng = np.random.default_rng(QM["seed"])
    h, w, n = QM["h"], QM["w"], QM["n"]
    tex = _cosines(rng, QM["n_cos"], QM["fmax"])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def scene(xx, yy):
        return 128.0 + 90.0 * tex(xx, yy)
    frames, truth = [], []
    for i in range(n):
        u = np.zeros((h, w, 2))
        if i:
            for c in range(2):
                a = rng.uniform(*QM["amp"])
                lam = rng.uniform(*QM["wavelength"], 2)
                th, ph = rng.uniform(0, 2 * np.pi, 2)
                u[..., c] = a * np.cos(2 * np.pi * (np.cos(th) * x / lam[0] + np.sin(th) * y / lam[1]) + ph)
        f = scene(x + u[..., 0], y + u[..., 1]) + rng.normal(0.0, QM["noise"], (h, w))
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        truth.append(u)
    return scene(x, y), np.stack(frames), np.stack(truth)


def interior_rms(img, scene, margin=None):
    m = QM["margin"] if margin is None else margin
    d = np.asarray(img, np.float64)[m:-m, m:-m] - scene[m:-m, m:-m]
    return float(np.sqrt((d * d).mean()))


def quality_mesh_restated(frames):
    """The definition on the quality stack under identity warps: (mesh mean, plain mean, fields, statuses), grey levels."""
    p = QM["mesh"]
    I3 = np.eye(3)
    fields, stats = [None], [None]
    for f in frames[1:]:
        d, s, _ = local_align_restate(frames[0], f, I3, False, p)
        fields.append(mesh_fill_restate(d, s, p.fill))
        stats.append(s)
    warps = [I3] * len(frames)
    mesh = mesh_mean_restate(frames, warps, False, 1.0 / 255.0, fields, p.step)[..., 0] * 255.0
    mean = mesh_mean_restate(frames, warps, False, 1.0 / 255.0, [None] * len(frames), p.step)[..., 0] * 255.0
    return mesh, mean, fields, stats


@pytest.fixture(scope="module")
def quality():
    scene, frames, truth = quality_mesh_stack()
    return (scene, frames, truth) + quality_mesh_restated(frames)


def test_quality_stack_mesh_beats_the_mean(quality):
    scene, frames, truth, mesh, mean, fields, stats = quality
    r_mesh, r_mean, r_0 = interior_rms(mesh, scene), interior_rms(mean, scene), interior_rms(frames[0], scene)
    # the folded field undoes the frame's own: d = -u at the nodes inside the frame
    p = QM["mesh"]
    errs, its = [], []
    for i in range(1, len(frames)):
        nodes = -truth[i][::p.step, ::p.step]
        gh, gw = nodes.shape[:2]
        errs.append(float(np.sqrt(((fields[i][:gh, :gw] - nodes)[1:-1, 1:-1] ** 2).sum(axis=-1).mean())))
        its.append(stats[i][stats[i] > 0].mean())
    print("quality stack: RMS mesh", r_mesh, "plain mean", r_mean, "frame 0", r_0, "ratio", r_mesh / r_mean)
    print("field error per frame (px RMS, inner nodes)", np.round(errs, 3), "true field RMS",
          float(np.sqrt((truth[1:] ** 2).sum(axis=-1).mean())), "iterations per node", float(np.mean(its)))
    # the issue's bound: its f64 prototype measured 0.26
    assert r_mesh <= 0.5 * r_mean
    assert max(errs) < 0.5


# ---- the estimation ----------------------------------------------------------------------------------------------------
def _scene_u8(h, w, seed, shift=(0, 0)):
    tex = _cosines(np.random.default_rng(seed), 12, 0.1)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(128.0 + 100.0 * tex(x - shift[0], y - shift[1])), 0, 255).astype(np.uint8)


def test_integer_translation_closed_form():
    """Frame i is frame 0 moved by s = (3, -2) and the global warp moves it on by m = (-2, 1): the residual that brings it
    onto frame 0 is d = s + m = (1, -1). At d the taps are frame 0's own pixels, e = 0: a fixed point of the iteration.
    Measured on the CPU (80 x 96, step 16, radius 8, epsilon 0.01): the nodes whose patch stays inside both frames end
    within 2.6e-4 px of (1, -1) after 3 iterations; the bound asked is 1e-3 px."""
    h, w = 80, 96
    f0 = _scene_u8(h, w, 1)
    fi = _scene_u8(h, w, 1, shift=(3, -2))
    M = np.eye(3)
    M[0, 2], M[1, 2] = -2.0, 1.0
    p = MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=0)
    for affine in (False, True):
        d, s, _ = local_align_restate(f0, fi, M, affine, p)
        inner = (slice(1, -1), slice(1, -2))
        assert (s[inner] > 0).all() and s[inner].max() <= 5
        err = np.abs(d[inner] - np.array([1.0, -1.0], F)).max()
        print("closed form: max |d - (1, -1)| =", err, "iterations", s[inner].min(), "..", s[inner].max())
        assert err <= 1e-3
    # identical frames under the identity: d = 0 exactly, one iteration
    d, s, _ = local_align_restate(f0, f0, np.eye(3), False, p)
    assert (d == 0).all() and (s[s > 0] == 1).all()


def test_the_four_invalid_codes():
    p = MeshParameters(step=16, radius=2, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=0)
    # -1: w = 18 puts the last column of nodes at x = 32, its patch [30, 34] misses 1 <= x <= 16
    f0 = _scene_u8(40, 18, 2)
    d, s, _ = local_align_restate(f0, f0, np.eye(3), False, p)
    assert s.shape == (4, 3) and (s[:, 2] == -1).all() and (s[:3, :2] > 0).all() and (d[:, 2] == 0).all()
    # -2: a warp that moves the frame 20 px to the right leaves the patches of the left nodes outside the source
    f0 = _scene_u8(48, 64, 3)
    M = np.eye(3)
    M[0, 2] = 20.0
    p8 = MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=0)
    d, s, _ = local_align_restate(f0, _scene_u8(48, 64, 3, shift=(-20, 0)), M, False, p8)
    assert (s[:, :2] == -2).all() and (s[1:-1, 2:-1] > 0).all() and (d[:, :2] == 0).all()
    # -3: a flat patch has no texture; min_eig = 0 accepts everything with det > 0 and still refuses det = 0
    flat = f0.copy()
    flat[8:40, 8:40] = 77
    for me in (1.0, 0.0):
        q = MeshParameters(step=16, radius=4, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=me, fill=0)
        d, s, _ = local_align_restate(flat, f0, np.eye(3), False, q)
        assert s[1, 1] == -3 and s[2, 2] == -3 and (d[1, 1] == 0).all()
    # -4: a true shift of 2 px against max_shift = 0.5
    q = MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=0.5, min_eig=1.0, fill=0)
    d, s, _ = local_align_restate(f0, _scene_u8(48, 64, 3, shift=(2, 0)), np.eye(3), False, q)
    assert (s[1:-1, 1:-1] == -4).all() and (d == 0).all()
    # max_iters exhausted: valid, the status is the count
    q = MeshParameters(step=16, radius=8, max_iters=2, epsilon=0.0, max_shift=8.0, min_eig=1.0, fill=0)
    d, s, _ = local_align_restate(f0, _scene_u8(48, 64, 3, shift=(1, 0)), np.eye(3), False, q)
    assert (s[1:-1, 1:-1] == 2).all() and (np.abs(d[1:-1, 1:-1, 0] - 1.0) < 0.2).all()


def test_fill():
    d = np.zeros((4, 5, 2), F)
    d[..., 0], d[..., 1] = 1.5, -0.5
    s = np.full((4, 5), 3, np.int32)
    s[1, 2] = -3                                   # an isolated hole takes its neighbours' common value
    d[1, 2] = 0
    assert np.array_equal(mesh_fill_restate(d, s, 0), d)
    out = mesh_fill_restate(d, s, 1)
    assert (out[..., 0] == 1.5).all() and (out[..., 1] == -0.5).all()
    # weights: the hole at a corner sees 2, 2 and 1
    d2 = np.zeros((2, 2, 2), F)
    d2[0, 1], d2[1, 0], d2[1, 1] = (1, 0), (2, 0), (4, 0)
    s2 = np.array([[-2, 1], [1, 1]], np.int32)
    assert mesh_fill_restate(d2, s2, 1)[0, 0, 0] == F(10) / F(5)
    # no valid neighbour: one pass leaves the far hole, the second reaches it; valid nodes never change
    d3 = np.zeros((1, 4, 2), F)
    d3[0, 0] = (3, 1)
    s3 = np.array([[2, -1, -3, -4]], np.int32)
    o1, o2 = mesh_fill_restate(d3, s3, 1), mesh_fill_restate(d3, s3, 3)
    assert (o1[0, 1] == (3, 1)).all() and (o1[0, 2:] == 0).all() and (o2[0, :, 0] == 3).all() and (o2[0, 0] == d3[0, 0]).all()
    # a grid without a valid node stays zero
    assert (mesh_fill_restate(np.zeros((3, 3, 2), F), np.full((3, 3), -3), 4) == 0).all()


# ---- the fold ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101])
def test_zero_field_gives_the_plain_fold(border):
    rng = np.random.default_rng(border)
    f = rng.integers(0, 256, (37, 45, 3), dtype=np.uint8)
    M = np.array([[1.01, 0.02, 2.3], [-0.015, 0.99, -1.7], [1e-5, -2e-5, 1.0]])
    gw, gh = grid_restate(45, 37, 16)
    bv = (0.1, 0.2, 0.3, 0)
    a = mesh_fold_restate(f, M, False, 1.0 / 255.0, np.zeros((gh, gw, 2), F), 16, border, bv)
    b = mesh_fold_restate(f, M, False, 1.0 / 255.0, None, 16, border, bv)
    assert a.dtype == F and np.array_equal(a, b)


def test_field_interpolation_and_displaced_sample():
    # a constant field moves every coordinate by it; the node values come back at the nodes
    w, h, step = 45, 37, 16
    gw, gh = grid_restate(w, h, step)
    assert (gw, gh) == (4, 4) and mesh_grid(w, h, step) == (gw, gh) and mesh_grid(33, 17, 8) == (5, 3)
    D = np.zeros((gh, gw, 2), F)
    D[..., 0], D[..., 1] = 2.0, -1.0
    fx, fy = mesh_field_restate(D, w, h, step)
    y, x = np.mgrid[0:h, 0:w]
    assert np.array_equal(fx, (x + 2).astype(F)) and np.array_equal(fy, (y - 1).astype(F))
    D = np.random.default_rng(4).uniform(-3, 3, (gh, gw, 2)).astype(F)
    fx, fy = mesh_field_restate(D, w, h, step)
    assert np.array_equal(fx[::step, ::step], x[::step, ::step].astype(F) + D[:3, :3, 0])
    assert np.array_equal(fy[16, 8], F(16) + F(0.5) * (D[1, 0, 1] + D[1, 1, 1]))
    # an integer field under the identity reads the shifted frame
    f = np.random.default_rng(5).integers(0, 256, (h, w, 1), dtype=np.uint8)
    D = np.zeros((gh, gw, 2), F)
    D[..., 0], D[..., 1] = 2.0, -1.0
    s = mesh_fold_restate(f, np.eye(3), False, 1.0, D, step)
    assert np.array_equal(s[1:, :-2, 0], f[:-1, 2:, 0].astype(F)) and (s[0] == 0).all() and (s[:, -2:] == 0).all()


# ---- the interface -----------------------------------------------------------------------------------------------------
def test_ctypes_mirror_and_symbols():
    p = MeshParameters(step=32, radius=12, max_iters=7, epsilon=0.5, max_shift=4.0, min_eig=2.0, fill=3)._c()
    assert (p.step, p.radius, p.max_iters, p.epsilon, p.max_shift, p.min_eig, p.fill, p.reserved) == (32, 12, 7, 0.5, 4.0, 2.0, 3, 0)
    assert ctypes.sizeof(_ffi.MeshParams) == 32
    d = MeshParameters()._c()
    assert (d.step, d.radius, d.max_iters, d.fill) == (16, 8, 10, 2)
    lib = _ffi.load()
    for name in ("stk_mesh_grid", "stk_local_align", "stk_mesh_stack", "stk_mesh_local_weighted_stack",
                 "stk_ecc_match_local_aligned", "stk_keypoint_match_local_aligned"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    gw, gh = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.stk_mesh_grid(157, 120, 16, ctypes.byref(gw), ctypes.byref(gh)) == 0 and (gw.value, gh.value) == (11, 9)
    for bad in ((157, 120, 12), (157, 120, 4), (157, 120, 512), (0, 120, 16), (157, 0, 16)):
        assert lib.stk_mesh_grid(*bad, ctypes.byref(gw), ctypes.byref(gh)) == 2
    assert lib.stk_mesh_grid(157, 120, 16, None, ctypes.byref(gh)) == 2
    with pytest.raises(Exception):
        mesh_grid(10, 10, 3)

"""numpy restatement of mesh-displaced drizzle (include/stacker.h, the block after stk_drizzle_params): the field sample at
the output pixel's frame-0 coordinate, its slopes, the displaced output coordinate, the footprint from the product of the
two Jacobians, then drizzle_restate's local coordinates, overlaps and combine. Two paths, as in drizzle_restate: f32 with
every operation rounded on its own (the engine's operations) and f64 (the definition's mathematics from the same f32
inputs, the yardstick for error bounds). The f64 path takes the probes the bounds are built from: offsets on the source
coordinates (du, dv), on the footprint (dhx, dhy), and a bias on the two decisions the field sample makes from x0 (which
cell, clamped or not), which an f32 x0 one ulp away may make differently."""
import numpy as np

import drizzle_restate as dr
from drizzle_restate import _local, _overlaps
from interp_restate import F, fma32

U = 2.0 ** -24


def grid_map(scale, origin_x=0.0, origin_y=0.0):
    """((float)g, (float)tx, (float)ty, (float)s) of the header, as Python floats holding f32 values."""
    g = 1.0 / float(F(scale))
    tx = (0.5 * g - 0.5) + float(F(origin_x))
    ty = (0.5 * g - 0.5) + float(F(origin_y))
    return float(F(g)), float(F(tx)), float(F(ty)), float(F(scale))


def frame0_coords(oh, ow, scale, origin_x=0.0, origin_y=0.0, dtype=np.float64):
    """(x0, y0) of every output pixel."""
    g, tx, ty, _ = grid_map(scale, origin_x, origin_y)
    Y, X = np.mgrid[0:oh, 0:ow]
    if dtype == F:
        return X.astype(F) * F(g) + F(tx), Y.astype(F) * F(g) + F(ty)
    return X.astype(np.float64) * g + tx, Y.astype(np.float64) * g + ty


def x0_inexact(oh, ow, scale, origin_x=0.0, origin_y=0.0):
    """Per axis, the output columns and rows whose f32 x0 = X g + tx is rounded at all: where the product and the sum are
    both f32 numbers the engine's x0 is the exact one and takes the decisions the f64 path takes."""
    g, tx, ty, _ = grid_map(scale, origin_x, origin_y)
    res = []
    for n, t in ((ow, tx), (oh, ty)):
        prod = np.arange(n, dtype=np.float64) * g                    # exact in f64: 24 x 24 bits
        p32 = prod.astype(F).astype(np.float64)
        total = p32 + t
        res.append((p32 != prod) | (total.astype(F).astype(np.float64) != total))
    return res[0][None, :], res[1][:, None]


def _axis(x0, n, step, gn, dtype, bias, inexact=None):
    """(k, k1, u, clamped) along one axis from the frame-0 coordinate. bias (f64 only) moves the coordinate the two
    decisions are taken from, where the f32 coordinate is rounded at all; u always comes from the coordinate itself."""
    shift = step.bit_length() - 1
    lim = dtype(n - 1)
    xc = np.fmin(np.fmax(x0, dtype(0)), lim)
    xb, xcb = x0, xc
    if bias:
        xb = x0 + np.where(inexact, bias, 0.0)
        xcb = np.fmin(np.fmax(xb, 0.0), lim)
    k = xcb.astype(np.int64) >> shift
    k1 = np.minimum(k + 1, gn - 1)
    if dtype == F:
        u = (xc - (k << shift).astype(F)) * F(1.0 / step)
    else:
        u = (xc - (k << shift)) * (1.0 / step)
    return k, k1, u, xb != xcb


def field_sample(D, oh, ow, sw, sh, step, scale, origin_x=0.0, origin_y=0.0, dtype=np.float64, bias=(0.0, 0.0)):
    """(d0, d1, e00, e01, e10, e11) of every output pixel: the field's sample and the displacement's Jacobian
    E = I + grad d. D: gh x gw x 2 f32."""
    D = np.asarray(D, F)
    gh, gw = D.shape[:2]
    x0, y0 = frame0_coords(oh, ow, scale, origin_x, origin_y, dtype)
    ix, iy = x0_inexact(oh, ow, scale, origin_x, origin_y) if (bias[0] or bias[1]) else (None, None)
    k, k1, u, cx = _axis(x0, sw, step, gw, dtype, bias[0], ix)
    j, j1, v, cy = _axis(y0, sh, step, gh, dtype, bias[1], iy)
    inv = dtype(1.0 / step)
    d, gx, gy = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(2):
            n00, n01, n10, n11 = (D[j, k, c].astype(dtype), D[j, k1, c].astype(dtype), D[j1, k, c].astype(dtype),
                                  D[j1, k1, c].astype(dtype))
            a, b, p, q = n01 - n00, n11 - n10, n10 - n00, n11 - n01
            if dtype == F:
                t0, t1 = fma32(u, a, n00), fma32(u, b, n10)
                d.append(fma32(v, t1 - t0, t0))
                sx, sy = fma32(v, b - a, a) * inv, fma32(u, q - p, p) * inv
            else:
                t0, t1 = u * a + n00, u * b + n10
                d.append(v * (t1 - t0) + t0)
                sx, sy = (v * (b - a) + a) * inv, (u * (q - p) + p) * inv
            gx.append(np.where(cx, dtype(0), sx))
            gy.append(np.where(cy, dtype(0), sy))
    one = dtype(1)
    return d[0], d[1], one + gx[0], gy[0], gx[1], one + gy[1]


def displaced_coords(D, oh, ow, sw, sh, step, scale, origin_x=0.0, origin_y=0.0, dtype=np.float64, bias=(0.0, 0.0)):
    """(Xd, Yd) of every output pixel; D None: the pixel's own."""
    Y, X = np.mgrid[0:oh, 0:ow]
    if D is None:
        return X.astype(dtype), Y.astype(dtype)
    s = dtype(grid_map(scale)[3])
    d0, d1 = field_sample(D, oh, ow, sw, sh, step, scale, origin_x, origin_y, dtype, bias)[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        return X.astype(dtype) + s * d0, Y.astype(dtype) + s * d1


def entry_terms(frame, A, is_affine, alpha, pixfrac, oh, ow, D=None, step=16, scale=1.0, origin_x=0.0, origin_y=0.0, mp=None,
                dtype=np.float64, du=0.0, dv=0.0, dhx=0.0, dhy=0.0, bias=(0.0, 0.0)):
    """(s oh x ow x cn, k oh x ow) of one table entry: the weighted sum of its live taps and the sum of their weights. A from
    drizzle_restate.grid_matrix; D: the entry's field or None (plain drizzle arithmetic). f64 only: du, dv are added to the
    source coordinates, dhx, dhy to the footprint's half-extents before the clamp, bias as in field_sample."""
    dt = dtype
    src = np.asarray(frame)
    sh, sw = src.shape[:2]
    src = src.reshape(sh, sw, -1)
    cn = src.shape[2]
    p = F(pixfrac)
    if dt == F:
        hp, hmax, al = F(0.5) * p, F(1.5) - F(0.5) * p, F(alpha)
    else:
        hp, hmax, al = 0.5 * float(p), 1.5 - 0.5 * float(p), float(F(alpha))
    A = np.asarray(A, np.float64)
    a = A.astype(dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fx, fy = displaced_coords(D, oh, ow, sw, sh, step, scale, origin_x, origin_y, dt, bias)
        if dt == F:
            u = fma32(a[0], fx, fma32(a[1], fy, a[2]))
            v = fma32(a[3], fx, fma32(a[4], fy, a[5]))
            if not is_affine:
                W = fma32(a[6], fx, fma32(a[7], fy, a[8]))
                u, v = u / W, v / W
        else:
            u = a[0] * fx + a[1] * fy + a[2]
            v = a[3] * fx + a[4] * fy + a[5]
            if not is_affine:
                W = a[6] * fx + a[7] * fy + a[8]
                u, v = u / W, v / W
            u, v = u + du, v + dv
        finite = (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
        jn, d = _local(u, finite, dt)
        kn, e = _local(v, finite, dt)
        half = dt(0.5)
        if D is None:
            if is_affine:
                if dt == F:
                    hx, hy = F(0.5 * (abs(A[0]) + abs(A[1]))), F(0.5 * (abs(A[3]) + abs(A[4])))
                else:
                    hx, hy = 0.5 * (abs(A[0]) + abs(A[1])), 0.5 * (abs(A[3]) + abs(A[4]))
            else:
                if dt == F:
                    uu, vv = jn.astype(F) + d, kn.astype(F) + e
                else:
                    uu, vv = np.where(finite, u, 0.0), np.where(finite, v, 0.0)
                rw = dt(1) / np.abs((a[6] * fx + a[7] * fy) + a[8])
                hx = ((np.abs(a[0] - uu * a[6]) + np.abs(a[1] - uu * a[7])) * rw) * half
                hy = ((np.abs(a[3] - vv * a[6]) + np.abs(a[4] - vv * a[7])) * rw) * half
        else:
            e00, e01, e10, e11 = field_sample(D, oh, ow, sw, sh, step, scale, origin_x, origin_y, dt, bias)[2:]
            if is_affine:
                j00, j01, j10, j11, rw = a[0], a[1], a[3], a[4], None
            else:
                if dt == F:
                    uu, vv = jn.astype(F) + d, kn.astype(F) + e
                else:
                    uu, vv = np.where(finite, u, 0.0), np.where(finite, v, 0.0)
                rw = dt(1) / np.abs((a[6] * fx + a[7] * fy) + a[8])
                j00, j01, j10, j11 = a[0] - uu * a[6], a[1] - uu * a[7], a[3] - vv * a[6], a[4] - vv * a[7]
            hx = np.abs(j00 * e00 + j01 * e10) + np.abs(j00 * e01 + j01 * e11)
            hy = np.abs(j10 * e00 + j11 * e10) + np.abs(j10 * e01 + j11 * e11)
            if rw is not None:
                hx, hy = hx * rw, hy * rw
            hx, hy = hx * half, hy * half
        if dt != F:
            hx, hy = np.fmax(hx + dhx, 0.0), np.fmax(hy + dhy, 0.0)
        hx, hy = np.fmin(hx, hmax), np.fmin(hy, hmax)
        ox = _overlaps(d, hx, jn, sw, finite, hp, dt)
        oy = _overlaps(e, hy, kn, sh, finite, hp, dt)
        mpl = None if mp is None else np.asarray(mp, F)
        s, k = np.zeros((oh, ow, cn), dt), np.zeros((oh, ow), dt)
        for b in range(3):
            yy = np.clip(kn + b - 1, 0, sh - 1)
            for a_ in range(3):
                xx = np.clip(jn + a_ - 1, 0, sw - 1)
                live = (ox[a_] > 0) & (oy[b] > 0)
                wgt = ox[a_] * oy[b]
                if mpl is not None:
                    mv = mpl[yy, xx].astype(dt)
                    live = live & (mv > 0)
                    wgt = wgt * mv
                t = src[yy, xx, :].astype(dt) * al
                s = np.where(live[..., None], s + wgt[..., None] * t, s)
                k = np.where(live, k + wgt, k)
    return s, k


def combine(terms, fill, gain=None, offset=None, weights=None, dtype=np.float64):
    """drizzle's combine over the entries' (s, k) in fold order: (out, den)."""
    dt = dtype
    s0, k0 = terms[0]
    cn = s0.shape[2]
    num, den = np.zeros(s0.shape, dt), np.zeros(k0.shape, dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i, (s, k) in enumerate(terms):
            w = dt(F(1.0 if weights is None else weights[i]))
            if not w > 0:
                continue
            g = np.ones(cn, dt) if gain is None else np.asarray(gain[i], F).astype(dt)
            o = np.zeros(cn, dt) if offset is None else np.asarray(offset[i], F).astype(dt)
            upd = k > 0
            num = np.where(upd[..., None], num + w * (s * g + o * k[..., None]), num)
            den = np.where(upd, den + w * k, den)
        out = np.where(den[..., None] > 0, num / den[..., None], dt(F(fill)))
    return out, den


def mesh_drizzle(frames, As, is_affine, alpha, scale, pixfrac, fill, oh, ow, fields, step, origin_x=0.0, origin_y=0.0, gain=None,
                 offset=None, weights=None, maps=None, dtype=np.float64):
    """(out oh x ow x cn, den oh x ow) in `dtype` over the entries (frames[i], As[i], fields[i]); fields[i] None: the entry
    is not displaced."""
    terms = [entry_terms(frames[i], As[i], is_affine, alpha, pixfrac, oh, ow, fields[i], step, scale, origin_x, origin_y,
                         None if maps is None else maps[i], dtype) for i in range(len(frames))]
    return combine(terms, fill, gain, offset, weights, dtype)


# ---- the error bound of the general case, from the f64 restatement alone ------------------------------------------------------
def ulp32(x):
    return float(np.spacing(F(abs(x))))


def probe_sizes(As, fields, is_affine, oh, ow, sw, sh, step, scale, origin_x, origin_y):
    """(delta, eh, bias): how far the engine's f32 source coordinates and footprint half-extents can lie from the f64 ones,
    and the distance from a cell or clamp boundary within which its f32 x0 may decide differently. Derivation (u = 2^-24,
    ulp = f32 spacing):
      x0 = X g + tx: two roundings, E_x0 = ulp(max |x0|); xc - (k << shift) is exact and 1 / step a power of two.
      d_c: three differences and three fmas on magnitudes <= 2 Dmax, 6 x 0.5 ulp(2 Dmax); the error of (u, v) enters through
        the slopes, 2 G E_x0 (G = the largest |slope|): E_d = 3 ulp(2 Dmax) + 2 G E_x0.
      Xd = X + s d: E_xd = s E_d + 0.5 ulp(s Dmax) + 0.5 ulp(max |Xd|).
      (u, v): the fragment's own 3 ulp of the largest coordinate, as in drizzle, plus the largest row sum R of the local
        Jacobian times E_xd: delta = 3 ulp(C) + R E_xd.
      slopes: a, b, b - a and the fma, each 0.5 ulp(4 Dmax), a's and b's errors passed on with weights that sum to 1: 5 x 0.5
        ulp(4 Dmax) / step; 1 + slope: u (|e| < 2). E_e = 2.5 ulp(4 Dmax) / step + u.
      footprint: j0 e00 + j1 e10 is two products and a sum below 2 (u each) on e's off by E_e: R E_e + 3 u; two of them, their
        sum below 4 (2 u), halved: R E_e + 4 u. Doubled for the perspective rows' own roundings (A - uu A2, 1 / |W| and the
        product with it, a relative u each on a value below 2): eh = 2 (R E_e + 4 u).
      bias = 2 E_x0."""
    Dmax, G = 1e-30, 0.0
    for D in fields:
        if D is None:
            continue
        D = np.asarray(D, np.float64)
        Dmax = max(Dmax, float(np.abs(D).max()))
        G = max(G, float(np.abs(np.diff(D, axis=0)).max()) / step if D.shape[0] > 1 else 0.0,
                float(np.abs(np.diff(D, axis=1)).max()) / step if D.shape[1] > 1 else 0.0)
    x0, y0 = frame0_coords(oh, ow, scale, origin_x, origin_y)
    e_x0 = ulp32(max(np.abs(x0).max(), np.abs(y0).max(), 1.0))
    s = grid_map(scale)[3]
    e_d = 3.0 * ulp32(2.0 * Dmax) + 2.0 * G * e_x0
    e_xd = s * e_d + 0.5 * ulp32(s * Dmax) + 0.5 * ulp32(max(oh, ow) + s * Dmax)
    C, R = 1.0, 0.0
    Y, X = np.mgrid[0:oh, 0:ow].astype(np.float64)
    for A, D in zip(As, fields):
        A = np.asarray(A, np.float64)
        fx, fy = displaced_coords(D, oh, ow, sw, sh, step, scale, origin_x, origin_y)
        W = np.ones_like(fx) if is_affine else A[6] * fx + A[7] * fy + A[8]
        u, v = (A[0] * fx + A[1] * fy + A[2]) / W, (A[3] * fx + A[4] * fy + A[5]) / W
        ok = (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
        if ok.any():
            C = max(C, float(np.abs(u[ok]).max()), float(np.abs(v[ok]).max()))
            rw = 1.0 / np.abs(W[ok])
            R = max(R, float(((np.abs(A[0] - u[ok] * A[6]) + np.abs(A[1] - u[ok] * A[7])) * rw).max()),
                    float(((np.abs(A[3] - v[ok] * A[6]) + np.abs(A[4] - v[ok] * A[7])) * rw).max()))
    delta = 3.0 * ulp32(C) + R * e_xd
    e_e = 2.5 * ulp32(4.0 * Dmax) / step + U
    eh = 2.0 * (R * e_e + 4.0 * U)
    return delta, eh, 2.0 * e_x0


def bound_terms(entry, n, finish, delta, eh, bias):
    """The allowance for the engine's f32 coordinates, footprints and cell decisions, per output pixel: (out0, den0, eo, ed).
    entry(i, **probe) -> (s, k) of entry i in f64, finish(terms) -> (out, den). As drizzle_restate.coordinate_term: every
    entry is moved on its own, the others held, since the entries' errors are independent; an entry's term is the sum of its
    largest change under the eight coordinate moves by delta, its largest under the four footprint moves by eh, and (only
    where a field is sampled) its largest under the four moves of the decision coordinate by bias; the allowance is the
    sum of the entries' terms."""
    base = [entry(i) for i in range(n)]
    o0, d0 = finish(base)
    eo, ed = np.zeros(d0.shape), np.zeros(d0.shape)

    def worst(i, probes):
        wo, wd = np.zeros(d0.shape), np.zeros(d0.shape)
        for kw in probes:
            t = list(base)
            t[i] = entry(i, **kw)
            o1, d1 = finish(t)
            wo = np.maximum(wo, np.abs(o1 - o0).max(axis=2))
            wd = np.maximum(wd, np.abs(d1 - d0))
        return wo, wd
    for i in range(n):
        groups = [[dict(du=a * delta, dv=b * delta) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1))],
                  [dict(dhx=a * eh, dhy=b * eh) for a, b in ((1, 1), (1, -1), (-1, 1), (-1, -1))],
                  [dict(bias=(a * bias, b * bias)) for a, b in ((1, 1), (1, -1), (-1, 1), (-1, -1))]]
        for g in groups:
            wo, wd = worst(i, g)
            eo, ed = eo + wo, ed + wd
    return o0, d0, eo, ed


__all__ = ["F", "U", "grid_map", "frame0_coords", "x0_inexact", "field_sample", "displaced_coords", "entry_terms", "combine", "mesh_drizzle",
           "ulp32", "probe_sizes", "bound_terms", "dr"]

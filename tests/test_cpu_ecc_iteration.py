"""One forward-additive ECC iteration, CPU side: a float64 numpy restatement of findTransformECC's step as
oracle/oracle_ecc.cpp states it (ecc_iteration_restate), the table of cases the GPU tests (test_gpu_ecc_iteration.py)
run the engine on, and the checks that pin the restatement to the oracle on every one of them.

The cases put the template partly outside frame 0 (`shift`), rotate it (`rot`), bend it (`persp`) and cut the frame so
that the last 64-pixel column is partial, one lane wide, or the only one: every case differs from its neighbours in one
regime of the column-walking pixel pass."""
import functools
import zlib

import numpy as np
import pytest

import oracle
from libstacker_rs_amd import synth

MOTIONS = {"translation": oracle.MOTION_TRANSLATION, "euclidean": oracle.MOTION_EUCLIDEAN,
           "affine": oracle.MOTION_AFFINE, "homography": oracle.MOTION_HOMOGRAPHY}


def _bilinear_zero(p, ix, iy, ax, ay, q):
    """Bilinear tap of plane p at (ix + ax, iy + ay), zero outside the plane; q rounds every intermediate."""
    h, w = p.shape

    def at(x, y):
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(ok, p[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0.0)
    p00, p01, p10, p11 = at(ix, iy), at(ix + 1, iy), at(ix, iy + 1), at(ix + 1, iy + 1)
    v0 = q(ax * q(p01 - p00) + p00)
    v1 = q(ax * q(p11 - p10) + p10)
    return q(ay * q(v1 - v0) + v0)


def _iteration(templ_blurred_f32, input_blurred_f32, warp3x3, motion, accumulate):
    """The pixel pass of one iteration (see ecc_iteration_restate); returns the function that finishes it."""
    assert accumulate in ("f64", "f32_columns")
    f32 = accumulate == "f32_columns"
    q = (lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, np.float64))

    def total(a):
        if f32:
            return float(np.add.accumulate(a.astype(np.float32), axis=0, dtype=np.float32)[-1].astype(np.float64).sum())
        return float(np.sum(a, dtype=np.float64))

    T = np.asarray(templ_blurred_f32, np.float32).astype(np.float64)
    I = np.asarray(input_blurred_f32, np.float32).astype(np.float64)
    th, tw = T.shape
    ih, iw = I.shape
    m = np.eye(3)
    wv = np.asarray(warp3x3, np.float32).astype(np.float64)
    m[:wv.shape[0], :] = wv
    if motion != oracle.MOTION_HOMOGRAPHY:
        m[2] = (0.0, 0.0, 1.0)
    # gradients of the input: 0.5 (I[x+1] - I[x-1]), reflect-101 borders
    Ip = np.pad(I, 1, mode="reflect")
    GX = q(0.5 * Ip[1:-1, 2:] - 0.5 * Ip[1:-1, :-2])
    GY = q(0.5 * Ip[2:, 1:-1] - 0.5 * Ip[:-2, 1:-1])

    y, x = np.mgrid[0:th, 0:tw].astype(np.float64)
    X = m[0, 0] * x + m[0, 1] * y + m[0, 2]
    Y = m[1, 0] * x + m[1, 1] * y + m[1, 2]
    if motion == oracle.MOTION_HOMOGRAPHY:
        W = m[2, 0] * x + m[2, 1] * y + m[2, 2]
        assert np.all(W != 0)
        X, Y = X / W, Y / W
        mx, my = np.rint(X), np.rint(Y)                       # the classic INTER_NEAREST test: rint of the double coordinate
    else:                                                      # ... and its 10-bit fixed-point form for warpAffine
        adx, bdx = np.rint(m[0, 0] * x * 1024), np.rint(m[1, 0] * x * 1024)
        X0 = np.rint((m[0, 1] * y + m[0, 2]) * 1024) + 512
        Y0 = np.rint((m[1, 1] * y + m[1, 2]) * 1024) + 512
        mx, my = np.floor((X0 + adx) / 1024), np.floor((Y0 + bdx) / 1024)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(Y))
    mask = (mx >= 0) & (mx < iw) & (my >= 0) & (my < ih)
    X, Y = q(X), q(Y)
    fx, fy = np.floor(X), np.floor(Y)
    ix, iy, ax, ay = fx.astype(np.int64), fy.astype(np.int64), q(X - fx), q(Y - fy)
    Iw = _bilinear_zero(I, ix, iy, ax, ay, q)
    gx = _bilinear_zero(GX, ix, iy, ax, ay, q)
    gy = _bilinear_zero(GY, ix, iy, ax, ay, q)

    n = float(mask.sum())
    assert n > 0
    mk = mask.astype(np.float64)
    sI, sII = total(Iw * mk), total(q(Iw * Iw) * mk)
    sT, sTT = total(T * mk), total(q(T * T) * mk)
    img_mean, tmp_mean = sI / n, sT / n
    img_norm = np.sqrt(n * max(sII / n - img_mean * img_mean, 0.0))
    tmp_norm = np.sqrt(n * max(sTT / n - tmp_mean * tmp_mean, 0.0))
    # pixels outside the mask keep their warped value in iz and nothing in tz: they still feed the Hessian and the image projection
    iz = np.where(mask, q(Iw - img_mean), Iw)
    tz = np.where(mask, q(T - tmp_mean), 0.0)

    h0, h1, h2, h3, h4, h5, h6, h7 = m[0, 0], m[1, 0], m[2, 0], m[0, 1], m[1, 1], m[2, 1], m[0, 2], m[1, 2]
    if motion == oracle.MOTION_HOMOGRAPHY:
        den = x * h2 + y * h5 + 1.0
        hat_x = (-x * h0 - y * h3 - h6) / den
        hat_y = (-x * h1 - y * h4 - h7) / den
        a, b = q(gx / den), q(gy / den)
        t = q(hat_x * a + hat_y * b)
        J = [a * x, b * x, t * x, a * y, b * y, t * y, a, b]
    elif motion == oracle.MOTION_AFFINE:
        J = [gx * x, gy * x, gx * y, gy * y, gx, gy]
    elif motion == oracle.MOTION_EUCLIDEAN:
        hat_x = -(x * h1) - (y * h0)
        hat_y = (x * h0) - (y * h1)
        J = [gx * hat_x + gy * hat_y, gx, gy]
    else:
        J = [gx, gy]
    J = [q(j) for j in J]
    P = len(J)
    H = np.zeros((P, P))
    for k in range(P):
        for l in range(k, P):
            H[k, l] = H[l, k] = total(q(J[k] * J[l]))
    ip = np.array([total(q(J[k] * iz)) for k in range(P)])
    tp = np.array([total(q(J[k] * tz)) for k in range(P)])
    corr = total(q(tz * iz))
    rho = corr / (img_norm * tmp_norm)

    def lambda_d():
        """The denominator of lambda, whose sign decides the "correlation is going to be minimized" exit. A Hessian with an
        exactly zero row has no inverse: Mat::inv then returns the zero matrix and the image projection drops out."""
        if not H.any(axis=0).all():
            return corr
        d = 1.0 / np.sqrt(np.diag(H))
        return corr - float(tp @ (d * np.linalg.solve(H * d[:, None] * d[None, :], d * ip)))

    def finish(solve="f64", ulp_rng=None):
        if solve == "f32":
            new, dp = _solve_f32(m, motion, H, ip, tp, corr, img_norm, lambda lam: np.array(
                [total(q(J[k] * q(float(lam) * tz - iz))) for k in range(P)]), ulp_rng)
            return new, float(rho), dp, n / (tw * th)

        d = 1.0 / np.sqrt(np.diag(H))                              # symmetric scaling: the homography's H spans 10 decades

        def solve_spd(rhs):
            return d * np.linalg.solve(H * d[:, None] * d[None, :], d * rhs)
        iph = solve_spd(ip)
        lambda_n = img_norm * img_norm - float(ip @ iph)
        lambda_d = corr - float(tp @ iph)
        assert lambda_d > 0
        lam = lambda_n / lambda_d
        e = q(q(lam) * tz - iz)
        ep = np.array([total(q(J[k] * e)) for k in range(P)])
        dp = solve_spd(ep)
        return _updated(m, dp, motion), float(rho), dp, n / (tw * th)
    finish.hessian, finish.correlation, finish.rho, finish.lambda_d = H, corr, float(rho), lambda_d
    return finish


def ecc_iteration_restate(templ_blurred_f32, input_blurred_f32, warp3x3, motion, accumulate="f64", solve="f64", ulp_rng=None):
    """One iteration of findTransformECC from `warp3x3` (template pixel -> input pixel, its f32 value is what counts).
    Returns (new warp 3x3 f64, rho, dp, mask coverage).

    accumulate = "f64": every operation in float64 — the answer the other sides are measured against.
    accumulate = "f32_columns": the precision the pixel pass is designed to have, modelled without looking at it: per-pixel
    quantities rounded to float32, every sum carried in float32 down a whole template column (one lane over the longest
    strip it can have), the column totals added in float64.
    solve = "f64": the normal equations solved in float64 (symmetrically scaled). solve = "f32": the tail as OpenCV runs
    it (_solve_f32), `ulp_rng` moving every f32 entry by one ulp first."""
    return _iteration(templ_blurred_f32, input_blurred_f32, warp3x3, motion, accumulate)(solve, ulp_rng)


def ecc_iteration_lambda(templ_blurred_f32, input_blurred_f32, warp3x3, motion):
    """(lambda_d, correlation, rho, Hessian) of the iteration's float64 sums at `warp3x3`, without the parameter update:
    defined also where the iteration ends the run (lambda_d <= 0) or moves nothing (a singular Hessian)."""
    fin = _iteration(templ_blurred_f32, input_blurred_f32, warp3x3, motion, "f64")
    return fin.lambda_d(), fin.correlation, fin.rho, fin.hessian


SOLVE_DRAWS = 16


def f32_solve_spread(templ_blurred_f32, input_blurred_f32, warp3x3, motion, draws=SOLVE_DRAWS):
    """New warps of `draws` f32 solves of the SAME float64 sums, each with every f32 entry of the Hessian and of the
    projections moved by one ulp (seeds 0 .. draws - 1). OpenCV — and with it the oracle and the engine — casts the sums
    to f32 and inverts the Hessian by f32 LU; for the homography on a thin or half-covered template that system is so
    poorly conditioned that the last bit of its entries is worth up to 1e-3 px, whoever computes them."""
    fin = _iteration(templ_blurred_f32, input_blurred_f32, warp3x3, motion, "f64")
    return [fin("f32", np.random.default_rng(k))[0] for k in range(draws)]


def _updated(m, dp, motion):
    """update_warping_matrix_ECC: m (3x3) + dp in OpenCV's parameter order, in the dtype of m."""
    new = m.copy()
    if motion == oracle.MOTION_HOMOGRAPHY:
        new[0, 0] += dp[0]; new[1, 0] += dp[1]; new[2, 0] += dp[2]; new[0, 1] += dp[3]
        new[1, 1] += dp[4]; new[2, 1] += dp[5]; new[0, 2] += dp[6]; new[1, 2] += dp[7]
    elif motion == oracle.MOTION_AFFINE:
        new[0, 0] += dp[0]; new[1, 0] += dp[1]; new[0, 1] += dp[2]; new[1, 1] += dp[3]; new[0, 2] += dp[4]; new[1, 2] += dp[5]
    elif motion == oracle.MOTION_TRANSLATION:
        new[0, 2] += dp[0]; new[1, 2] += dp[1]
    else:
        theta = float(dp[0]) + np.arcsin(float(m[1, 0]))
        new[0, 2] += dp[1]; new[1, 2] += dp[2]
        new[0, 0] = new[1, 1] = np.cos(theta)
        new[1, 0] = np.sin(theta)
        new[0, 1] = -new[1, 0]
    return new


def _invert_f32(S):
    """Mat::inv(DECOMP_LU) of an n x n CV_32F matrix: closed forms evaluated in double for n <= 3, otherwise hal::LU32f
    on [A | I] (partial pivoting, every operation rounded to f32) and back substitution."""
    n = S.shape[0]
    if n <= 3:
        return np.linalg.inv(S.astype(np.float64)).astype(np.float32)
    A = np.concatenate([S.astype(np.float32), np.eye(n, dtype=np.float32)], axis=1)
    for i in range(n):
        k = i + int(np.argmax(np.abs(A[i:, i])))
        assert abs(A[k, i]) >= np.float32(1.1920929e-06)
        if k != i:
            A[[i, k]] = A[[k, i]]
        dd = np.float32(-1) / A[i, i]
        for j in range(i + 1, n):
            A[j] = A[j] + (A[j, i] * dd) * A[i]
    X = np.zeros((n, n), np.float32)
    for i in range(n - 1, -1, -1):
        sacc = A[i, n:].copy()
        for k in range(i + 1, n):
            sacc = sacc - A[i, k] * X[k]
        X[i] = sacc / A[i, i]
    return X


def _solve_f32(m, motion, H, ip, tp, corr, img_norm, error_projection, ulp_rng):
    """The tail of the iteration as OpenCV runs it: the sums cast to f32, the Hessian inverted in f32, f32 gemms, the
    warp updated in f32. With `ulp_rng` every f32 entry is first moved one ulp up or down (seeded): what the last bit of
    sums that any two f32 implementations may round differently is worth in the result."""
    P = len(ip)

    def cast(a):
        a = np.asarray(a, np.float64).astype(np.float32)
        if ulp_rng is None:
            return a
        up = ulp_rng.integers(0, 2, a.shape) > 0
        if a.ndim == 2:
            up = np.triu(up) | np.triu(up, 1).T                # keep the Hessian symmetric
        return np.nextafter(a, np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))

    def gemv(M, v):
        s = np.zeros(P, np.float32)
        for l in range(P):
            s = s + M[:, l] * v[l]
        return s
    Hinv = _invert_f32(cast(H))
    ipf, tpf = cast(ip), cast(tp)
    iph = gemv(Hinv, ipf)
    lambda_n = img_norm * img_norm - float(ipf.astype(np.float64) @ iph.astype(np.float64))
    lambda_d = corr - float(tpf.astype(np.float64) @ iph.astype(np.float64))
    assert lambda_d > 0
    dp = gemv(Hinv, cast(error_projection(np.float32(lambda_n / lambda_d))))
    return _updated(m.astype(np.float32), dp, motion).astype(np.float64), dp.astype(np.float64)


# ---- the case table ---------------------------------------------------------------------------------------------
def truth_map(name, w, h):
    """S: template pixel -> frame-0 pixel, the warp the iteration heads for."""
    if name == "id":
        return np.eye(3)
    if name == "shift":                                        # half the template maps outside frame 0
        return np.array([[1, 0, 0.3 * w], [0, 1, -0.25 * h], [0, 0, 1.0]])
    if name == "rot":                                          # 16 degrees: outside the ring's row-rate window
        return np.array([[0.96, -0.28, 0.2 * w], [0.28, 0.96, -0.1 * h], [0, 0, 1.0]])
    if name == "persp":
        return np.array([[1.02, 0.03, -4], [-0.02, 0.97, 3], [3e-4, -2e-4, 1.0]])
    raise KeyError(name)


_ALL = ("id", "shift", "rot", "persp")
# (h, w): what the shape is there for -> truths
SHAPES = [
    ((33, 64), _ALL),                       # exactly one full column
    ((61, 67), _ALL),                       # one full column + 3 lanes
    ((128, 129), _ALL),                     # two full columns + 1 lane
    ((97, 191), _ALL),                      # two full columns + 63 lanes, odd height
    ((200, 449), _ALL),                     # strips reach 8 rows (default blocks: at some columns; ecc_blocks = 8: ~43 rows)
    ((9, 130), ("id", "shift", "persp")),   # thin: strips that never reach 8 rows
    ((130, 9), ("id", "shift", "persp")),   # thin: a single partial column
    ((8, 65), ("id", "shift", "persp")),    # fewer units than waves: some waves have nothing to do
]


def _cases():
    out = []
    for (h, w), truths in SHAPES:
        for truth in truths:
            for motion in MOTIONS:
                if truth == "persp" and motion != "homography":
                    continue
                if truth == "rot" and motion == "translation":
                    continue
                if (h, w) == (8, 65) and truth == "shift" and motion == "homography":
                    continue                                   # ill-posed: 8 parameters from half of 8 rows (a 13 px step)
                out.append((h, w, truth, motion))
    return out


CASES = _cases()


def case_id(case, gauss=5, depth=8):
    h, w, truth, motion = case
    return "%dx%d-%s-%s" % (h, w, truth, motion) + ("" if (gauss, depth) == (5, 8) else "-g%d-d%d" % (gauss, depth))


@functools.lru_cache(maxsize=None)
def scene(h, w):
    frames, _ = synth.make_stack(1, w, h)
    g0 = oracle.grey(frames[0].numpy())
    g0.setflags(write=False)
    return g0


# cases whose seeded draw leaves the admission conditions (test_cases_are_admissible) take another draw of the same
# distribution: 8 homography parameters from 8 rows are poorly determined, and one draw in a few makes a > 8 px step
RESEEDED = {"8x65-id-homography": "#1"}


def start_warp(case, cid):
    """The truth, moved by (+0.6, -0.4) px and (affine, homography) N(0, 1e-3) on its 2 x 2 block, as f32."""
    h, w, truth, motion = case
    rng = np.random.default_rng(zlib.crc32((cid + RESEEDED.get(cid, "")).encode()))
    W = truth_map(truth, w, h).copy()
    W[0, 2] += 0.6
    W[1, 2] -= 0.4
    if motion in ("affine", "homography"):
        W[:2, :2] += rng.normal(0, 1e-3, (2, 2))
    elif motion == "euclidean":
        th = np.arctan2(W[1, 0], W[0, 0])
        W[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    return W.astype(np.float32)


class Case:
    """Inputs of one case and its CPU answers; built once per process and shared (read-only) by every test that needs it."""

    def __init__(self, case, gauss=5, depth=8):
        h, w, truth, motion = case
        self.h, self.w, self.truth, self.motion = h, w, truth, motion
        self.id = case_id(case, gauss, depth)
        self.omotion = MOTIONS[motion]
        g0 = scene(h, w)
        S = truth_map(truth, w, h)
        t = oracle.warp_frame(g0, np.linalg.inv(S), alpha=1.0, border_mode=oracle.BORDER_REPLICATE)[..., 0]
        if depth == 8:
            self.templ, self.inp = np.clip(np.rint(t), 0, 255).astype(np.uint8), g0
        else:
            self.templ, self.inp = np.ascontiguousarray(t, np.float32), g0.astype(np.float32)
        self.gauss = gauss
        self.start = start_warp(case, self.id)
        self.start_arg = self.start if motion == "homography" else self.start[:2]
        tb, ib = oracle.gaussian_blur_f32(self.templ, gauss), oracle.gaussian_blur_f32(self.inp, gauss)
        self.W64, self.rho64, self.dp64, self.coverage = ecc_iteration_restate(tb, ib, self.start, self.omotion)
        self.W32c, self.rho32c, _, _ = ecc_iteration_restate(tb, ib, self.start, self.omotion, accumulate="f32_columns")
        rc, Wo, self.rho_oracle, its = oracle.find_transform_ecc(self.templ, self.inp, self.start_arg, self.omotion, 1, None, gauss)
        assert rc == 0 and its == 1, (self.id, rc, its)
        self.W_oracle = Wo.astype(np.float64)
        self.e_oracle = synth.corner_error(self.W_oracle, self.W64, w, h)
        self.e_f32col = synth.corner_error(self.W32c, self.W64, w, h)
        self.move = synth.corner_error(self.W64, self.start, w, h)
        self.e_f32solve = max(self.error(W) for W in f32_solve_spread(tb, ib, self.start, self.omotion))
        # how far from float64 a correct f32 implementation may land: the largest of the three reference-side figures
        self.floor = max(self.e_oracle, self.e_f32col, self.e_f32solve)
        self.ulp = float(np.spacing(np.float32(max(w, h))))     # the result is stored as f32

    def error(self, W):
        """Corner displacement (px) of a 3x3 result from the float64 answer."""
        W = np.asarray(W, np.float64).reshape(3, 3).copy()
        if self.motion != "homography":
            W[2] = (0.0, 0.0, 1.0)
        return synth.corner_error(W, self.W64, self.w, self.h)


@functools.lru_cache(maxsize=None)
def get_case(case, gauss=5, depth=8):
    return Case(case, gauss, depth)


# ---- CPU tests ---------------------------------------------------------------------------------------------------
def test_known_answer_translation_of_a_plane_wave():
    """A closed form, independent of the oracle: for a smooth pattern shifted by a fraction of a pixel one translation
    iteration lands on the shift to second order."""
    yy, xx = np.mgrid[0:48, 0:80].astype(np.float64)

    def pat(x, y):
        return 120 + 50 * np.sin(x / 9.0) * np.cos(y / 7.0) + 30 * np.sin((x + 2 * y) / 23.0)
    ref, mov = pat(xx, yy).astype(np.float32), pat(xx + 0.25, yy - 0.125).astype(np.float32)
    W, rho, dp, cov = ecc_iteration_restate(mov, ref, np.eye(3), oracle.MOTION_TRANSLATION)
    assert abs(W[0, 2] - 0.25) < 5e-3 and abs(W[1, 2] + 0.125) < 5e-3
    assert cov == 1.0 and rho > 0.999
    assert np.array_equal(W[:2, :2], np.eye(2)) and np.array_equal(W[2], [0, 0, 1])


def test_case_table_is_the_stated_one():
    assert len(CASES) == len(set(CASES))
    by_shape = {}
    for h, w, truth, motion in CASES:
        by_shape.setdefault((h, w), []).append((truth, motion))
    assert [s for s, _ in SHAPES] == list(by_shape)
    for (h, w), truths in SHAPES:
        got = by_shape[(h, w)]
        assert {t for t, _ in got} == set(truths)
        assert [m for t, m in got if t == "persp"] == ["homography"]
        assert "translation" not in [m for t, m in got if t == "rot"]
        assert sorted(m for t, m in got if t == "id") == sorted(MOTIONS)
    assert sorted(m for t, m in by_shape[(8, 65)] if t == "shift") == ["affine", "euclidean", "translation"]
    assert max(max(s) for s, _ in SHAPES) <= 449


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=["%dx%d" % s for s, _ in SHAPES])
def test_cases_are_admissible(shape):
    """On the float64 restatement alone: a well-posed step (no corner moves by more than 8 px), at least a quarter of the
    template inside frame 0, and a correlation worth maximising."""
    for case in CASES:
        if case[:2] != shape:
            continue
        c = get_case(case)
        print("%-34s coverage %.3f rho %.4f move %.3f px" % (c.id, c.coverage, c.rho64, c.move))
        assert c.move <= 8.0, c.id
        assert c.coverage >= 0.25, c.id
        assert c.rho64 >= 0.75, c.id
    if shape == (200, 449):                                    # `shift` is there to put half of the template outside
        assert get_case((200, 449, "shift", "homography")).coverage < 0.6


# at most this many cases may sit above 2e-4 px (none above 2e-3): the oracle solves the 8 x 8 system by f32 LU, which
# costs it up to 1e-3 px where the step is poorly conditioned (few rows, half coverage). The allowance was set as 9 of 79
# cases; the table as specified has 86, and the count of exceptions allowed stays 9 (measured: 5, all `shift` + homography,
# the largest 4.9e-4 px)
MAX_ABOVE_2E4 = 9


def test_restatement_agrees_with_the_oracle():
    """The float64 restatement against oracle.find_transform_ecc(max_count = 1) on every case: rho to 1e-6, the new
    warp to 2e-3 px at the corners everywhere and to 2e-4 px on all but a few cases. Prints the oracle's distance from
    float64 — the floor the GPU test scales its bar from — and the f32-column model's."""
    above = []
    for case in CASES:
        c = get_case(case)
        print("%-34s oracle %.2e px  f32-columns %.2e px  f32-solve %.2e px  |drho| %.1e"
              % (c.id, c.e_oracle, c.e_f32col, c.e_f32solve, abs(c.rho_oracle - c.rho64)))
        assert abs(c.rho_oracle - c.rho64) <= 1e-6, c.id
        assert c.e_oracle <= 2e-3, c.id
        if c.e_oracle > 2e-4:
            above.append((c.id, c.e_oracle))
    assert len(above) <= MAX_ABOVE_2E4, above


def test_precision_models_account_for_the_oracle():
    """The two models of f32 precision are statements about round-off, not other algorithms. Both must land where float64
    does, within the bar the oracle itself gets (2e-3 px); and between them they must explain the oracle's own distance
    from float64 under the rule the GPU test applies to the engine: no more than 3 x the larger model plus one f32 ulp of
    the frame size. (The oracle's distance IS the f32 solve: the unperturbed f32 solve of the float64 sums reproduces it
    to within a factor of two on the homography cases.)"""
    for case in CASES:
        c = get_case(case)
        assert c.e_f32col <= 2e-3 and c.e_f32solve <= 2e-3, (c.id, c.e_f32col, c.e_f32solve)
        assert c.e_oracle <= 3.0 * max(c.e_f32col, c.e_f32solve) + c.ulp, (c.id, c.e_oracle, c.e_f32col, c.e_f32solve)

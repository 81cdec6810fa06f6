"""The ways a findTransformECC run ends other than by converging, CPU side: the table of cases the GPU tests
(test_gpu_ecc_exits.py) run the engine on, and the checks that admit every case on the reference side alone — the oracle's
answer, and where a sign or an exact zero decides the exit, the float64 restatement's sums (test_cpu_ecc_iteration).

  status 2   lambda_d <= 0 at the first iteration ("the correlation is going to be minimized"): a negated template
  status 1   NaN rho: a constant template, a constant input, a start that maps the whole template outside the input
  singular   stripes: one gradient plane is exactly 0, the Hessian has exact zero rows, Mat::inv returns 0, nothing moves
  zero       no iteration at all: max_count = 0, or epsilon > 0.5 (|rho - last_rho| = |-1 + eps| < eps before iteration 1)

Every frame is 80 x 64 or 131 x 97 (a partial last 64-pixel column, row bytes no multiple of 4), 8-bit, with one float32
variant per exit."""
import functools

import numpy as np
import pytest

import oracle
from test_cpu_ecc_iteration import MOTIONS, ecc_iteration_lambda

SIZES = ((64, 80), (97, 131))                                   # (h, w)
GAUSS = 5
# what the engine reports for the oracle's return codes (OpenCV's two StsNoConv texts)
MESSAGES = {1: "findTransformECC: NaN encountered (StsNoConv)",
            2: "findTransformECC: the algorithm stopped before its convergence; the correlation is going to be minimized (StsNoConv)"}
# status 2 is in the table only where float64 puts lambda_d this far below zero, relative to the correlation: nearer to
# zero the f32 sums decide the sign and no side could be called right
LAMBDA_MARGIN = 1e-3


def smooth(h, w, dx=0.0, dy=0.0):
    """The pattern of test_gpu_ecc.py::test_translated_pattern_recovers_shift, sampled at (x + dx, y + dy)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = xx + dx, yy + dy
    return np.clip(120 + 60 * np.sin(x / 9.0) * np.cos(y / 7.0) + 40 * np.sin((x + 2 * y) / 23.0), 0, 255).astype(np.uint8)


def stripes(h, w, axis, shift=0.0):
    """120 + 80 sin(t / 5) along x (axis = "v": vertical stripes, gy == 0) or along y ("h": gx == 0)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = (xx if axis == "v" else yy) + shift
    return np.clip(120 + 80 * np.sin(t / 5.0), 0, 255).astype(np.uint8)


def _shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float32)


# a start near the (1.5, -1.0) px shift of the good pair, one per motion type, none the identity
ZERO_STARTS = {
    "translation": _shift(1.25, -0.75),
    "euclidean": np.array([[np.cos(0.01), -np.sin(0.01), 1.25], [np.sin(0.01), np.cos(0.01), -0.75], [0, 0, 1]], np.float32),
    "affine": np.array([[1.01, 0.005, 1.0], [-0.004, 0.99, -0.5], [0, 0, 1]], np.float32),
    "homography": np.array([[1.01, 0.005, 1.0], [-0.004, 0.99, -0.5], [1e-5, -2e-5, 1]], np.float32),
}
# (max_count, epsilon): four that run no iteration, and the boundary that does
ZERO_CRITERIA = ((0, None), (0, 1e-5), (50, 0.6), (None, 0.75))
BOUNDARY = (50, 0.5)


class ExitCase:
    def __init__(self, kind, name, motion, templ, inp, start, criteria=(50, 1e-5), f32=False):
        self.kind, self.name, self.motion, self.omotion = kind, name, motion, MOTIONS[motion]
        if f32:
            templ, inp = templ.astype(np.float32), inp.astype(np.float32)
        self.templ, self.inp = np.ascontiguousarray(templ), np.ascontiguousarray(inp)
        self.h, self.w = templ.shape
        self.start = np.asarray(start, np.float32)
        self.start_arg = self.start if motion == "homography" else self.start[:2]
        self.max_count, self.epsilon = criteria
        self.id = "%s-%s-%dx%d-%s%s" % (kind, name, self.w, self.h, motion, "-f32" if f32 else "")
        for a in (self.templ, self.inp, self.start):
            a.setflags(write=False)

    def oracle(self, max_count=-1, epsilon=-1):
        """(rc, warp 3x3 f32, rho, iterations) of the oracle, under the case's criteria unless others are given."""
        mc = self.max_count if max_count == -1 else max_count
        eps = self.epsilon if epsilon == -1 else epsilon
        return _oracle(self, mc, eps)

    def first_iteration_sums(self):
        """(lambda_d, correlation, rho, Hessian) of the float64 restatement at the start warp."""
        return _sums(self)


@functools.lru_cache(maxsize=None)
def _oracle(case, max_count, epsilon):
    rc, W, rho, its = oracle.find_transform_ecc(case.templ, case.inp, case.start_arg, case.omotion, max_count, epsilon, GAUSS)
    W.setflags(write=False)
    return rc, W, rho, its


@functools.lru_cache(maxsize=None)
def _sums(case):
    tb, ib = oracle.gaussian_blur_f32(case.templ, GAUSS), oracle.gaussian_blur_f32(case.inp, GAUSS)
    return ecc_iteration_lambda(tb, ib, case.start, case.omotion)


def _build():
    eye = np.eye(3, dtype=np.float32)
    cases = []
    # ---- status 2: the negated input, and the negated SHIFTED input (the template of the good pair, negated)
    for k, motion in enumerate(MOTIONS):
        h, w = SIZES[k % 2]
        cases.append(ExitCase("status2", "negated", motion, 255 - smooth(h, w), smooth(h, w), eye))
        h, w = SIZES[(k + 1) % 2]
        cases.append(ExitCase("status2", "negated-shifted", motion, 255 - smooth(h, w, 1.5, -1.0), smooth(h, w), eye))
    cases.append(ExitCase("status2", "negated", "homography", 255 - smooth(97, 131), smooth(97, 131), eye, f32=True))
    # ---- status 1
    for k, motion in enumerate(MOTIONS):
        h, w = SIZES[k % 2]
        cases.append(ExitCase("status1", "constant-template", motion, np.full((h, w), 7, np.uint8), smooth(h, w), eye))
        h, w = SIZES[(k + 1) % 2]
        cases.append(ExitCase("status1", "constant-input", motion, smooth(h, w), np.full((h, w), 7, np.uint8), eye))
    for k, motion in enumerate(("homography", "translation")):
        h, w = SIZES[k]
        cases.append(ExitCase("status1", "outside", motion, smooth(h, w, 1.5, -1.0), smooth(h, w), _shift(3.0 * w, 0)))
    for h, w in SIZES:                                          # sheared and scaled as well: still every pixel beyond the far corner
        A = np.array([[1.5, 0.2, 2.0 * w], [-0.1, 1.2, 2.0 * h], [0, 0, 1]], np.float32)
        cases.append(ExitCase("status1", "outside-affine", "affine", smooth(h, w, 1.5, -1.0), smooth(h, w), A))
    cases.append(ExitCase("status1", "constant-input", "homography", smooth(97, 131), np.full((97, 131), 7, np.uint8), eye, f32=True))
    # ---- singular: stripes against the same stripes 0.7 px on, from the identity and from that shift
    for axis in ("v", "h"):
        on = _shift(0.7, 0) if axis == "v" else _shift(0, 0.7)
        for motion in MOTIONS:
            for h, w in SIZES:
                for sname, start in (("identity", eye), ("shifted", on)):
                    cases.append(ExitCase("singular", "%sstripes-%s" % (axis, sname), motion, stripes(h, w, axis, 0.7),
                                          stripes(h, w, axis), start))
    cases.append(ExitCase("singular", "vstripes-shifted", "homography", stripes(97, 131, "v", 0.7), stripes(97, 131, "v"),
                          _shift(0.7, 0), f32=True))
    # ---- no iteration, and the boundary that iterates
    for k, motion in enumerate(MOTIONS):
        h, w = SIZES[k % 2]
        for crit in ZERO_CRITERIA + (BOUNDARY,):
            kind = "boundary" if crit == BOUNDARY else "zero"
            cases.append(ExitCase(kind, "count%s-eps%s" % crit, motion, smooth(h, w, 1.5, -1.0), smooth(h, w), ZERO_STARTS[motion], crit))
    for crit in ((0, None), (50, 0.6)):
        cases.append(ExitCase("zero", "count%s-eps%s" % crit, "homography", smooth(97, 131, 1.5, -1.0), smooth(97, 131),
                              ZERO_STARTS["homography"], crit, f32=True))
    return cases


CASES = _build()


def cases_of(kind):
    return [c for c in CASES if c.kind == kind]


@functools.lru_cache(maxsize=None)
def good_pair():
    """A pair that aligns: (template, input, criteria) of the smooth pattern and its (1.5, -1.0) px shifted copy."""
    t, i = smooth(64, 80, 1.5, -1.0), smooth(64, 80)
    t.setflags(write=False)
    i.setflags(write=False)
    return t, i


def same_values(a, b):
    """Bit for bit, except that -0.0 counts as 0.0 (a Euclidean update writes -sin(0))."""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


# ---- CPU tests ---------------------------------------------------------------------------------------------------
def test_the_table_is_the_stated_one():
    assert len({c.id for c in CASES}) == len(CASES)
    assert {(c.h, c.w) for c in CASES} == set(SIZES)
    for kind in ("status2", "status1", "singular", "zero"):
        group = cases_of(kind)
        assert sum(c.templ.dtype == np.float32 for c in group) >= 1, kind
        assert {(c.h, c.w) for c in group if c.templ.dtype == np.uint8} == set(SIZES), kind
    for name in ("negated", "negated-shifted"):
        assert sorted(c.motion for c in cases_of("status2") if c.name == name and c.templ.dtype == np.uint8) == sorted(MOTIONS)
    assert {c.name for c in cases_of("status1")} == {"constant-template", "constant-input", "outside", "outside-affine"}
    sing = cases_of("singular")
    for axis in "vh":
        for start in ("identity", "shifted"):
            got = [c for c in sing if c.name == "%sstripes-%s" % (axis, start) and c.templ.dtype == np.uint8]
            assert sorted(c.motion for c in got) == sorted(2 * list(MOTIONS))
    for c in sing:                                              # pure x or y translation starts only
        assert np.array_equal(c.start[:2, :2], np.eye(2)) and np.array_equal(c.start[2], [0, 0, 1])
    for motion in MOTIONS:
        got = [(c.max_count, c.epsilon) for c in cases_of("zero") if c.motion == motion and c.templ.dtype == np.uint8]
        assert got == list(ZERO_CRITERIA)
        assert [(c.max_count, c.epsilon) for c in cases_of("boundary") if c.motion == motion] == [BOUNDARY]
    for c in cases_of("zero") + cases_of("boundary"):
        assert not np.array_equal(c.start, np.eye(3))


def test_status2_cases_are_admissible():
    """The oracle stops at iteration 1 with rc 2, and the float64 sums put lambda_d at least LAMBDA_MARGIN x |correlation|
    below zero: the sign is no matter of round-off."""
    for c in cases_of("status2"):
        rc, W, rho, its = c.oracle()
        lam, corr, rho64, H = c.first_iteration_sums()
        print("%-52s rc %d its %d  lambda_d / |correlation| %.4f  rho64 %.5f" % (c.id, rc, its, lam / abs(corr), rho64))
        assert (rc, its) == (2, 1), c.id
        assert lam <= -LAMBDA_MARGIN * abs(corr), c.id
        assert np.linalg.matrix_rank(H) == H.shape[0], c.id


def test_status1_cases_give_nan():
    for c in cases_of("status1"):
        rc, W, rho, its = c.oracle()
        print("%-52s rc %d its %d rho %r" % (c.id, rc, its, rho))
        assert rc == 1 and np.isnan(rho), c.id
    for c in cases_of("status1"):
        if "outside" in c.id:                                   # wholly outside: every corner, hence (affine maps) every pixel
            xs, ys = np.array([0, c.w - 1, 0, c.w - 1.0]), np.array([0, 0, c.h - 1.0, c.h - 1.0])
            m = c.start.astype(np.float64)
            X, Y = m[0, 0] * xs + m[0, 1] * ys + m[0, 2], m[1, 0] * xs + m[1, 1] * ys + m[1, 2]
            assert np.all((X >= c.w + 1) | (Y >= c.h + 1)) and np.array_equal(m[2], [0, 0, 1]), c.id
            assert np.all(X >= c.w + 1) or np.all(Y >= c.h + 1), c.id


def _zero_columns(c):
    P = {"translation": 2, "euclidean": 3, "affine": 6, "homography": 8}[c.motion]
    dead = "gy" if "vstripes" in c.id else "gx"
    # parameter order of the Jacobian (test_cpu_ecc_iteration._iteration): which columns are built from the dead plane alone
    cols = {"translation": {"gx": [0], "gy": [1]}, "euclidean": {"gx": [1], "gy": [2]},
            "affine": {"gx": [0, 2, 4], "gy": [1, 3, 5]}, "homography": {"gx": [0, 3, 6], "gy": [1, 4, 7]}}[c.motion][dead]
    return P, cols


def test_singular_cases_have_exact_zero_rows_and_move_nothing():
    """float64: the rows and columns of the dead gradient plane are exactly 0 (the first zero column is column 1 for vertical
    stripes — met at the second pivot step — and column 0 for horizontal ones). The oracle returns its start bit for bit,
    after 2 iterations under epsilon = 1e-5 and after all 4 of max_count = 4."""
    worst = 0.0
    for c in cases_of("singular"):
        lam, corr, rho64, H = c.first_iteration_sums()
        P, cols = _zero_columns(c)
        assert H.shape == (P, P)
        for k in cols:
            assert not H[k].any() and not H[:, k].any(), (c.id, k)
        if P > 3:                                               # the LU branch: where the elimination meets the zero pivot
            assert min(cols) == (1 if "vstripes" in c.id else 0)
        assert lam == corr and lam > 0
        rc, W, rho, its = c.oracle()
        rc4, W4, rho4, its4 = c.oracle(4, None)
        print("%-52s rc %d its %d rho %.5f | count 4: its %d rho %.5f | rho64 %.5f" % (c.id, rc, its, rho, its4, rho4, rho64))
        assert (rc, its) == (0, 2) and (rc4, its4) == (0, 4), c.id
        assert same_values(W, c.start) and same_values(W4, c.start), c.id
        assert abs(rho - rho64) <= 1e-6 and abs(rho4 - rho64) <= 1e-6, c.id
        worst = max(worst, abs(rho - rho64), abs(rho4 - rho64))
    print("worst |rho_oracle - rho64| %.2e" % worst)


def test_zero_iteration_cases_return_the_start():
    for c in cases_of("zero"):
        rc, W, rho, its = c.oracle()
        print("%-52s rc %d its %d rho %r" % (c.id, rc, its, rho))
        assert (rc, its, rho) == (0, 0, -1.0), c.id
        assert W.tobytes() == c.start.tobytes(), c.id            # the start warp, untouched


def test_boundary_epsilon_iterates():
    """epsilon = 0.5 exactly: |-1 - (-0.5)| >= 0.5 holds, iteration 1 runs; the second is the last (rho moves by < 0.5)."""
    for c in cases_of("boundary"):
        rc, W, rho, its = c.oracle()
        print("%-52s rc %d its %d rho %.5f" % (c.id, rc, its, rho))
        assert rc == 0 and its >= 1 and rho > 0.9, c.id
        assert not np.array_equal(W, c.start), c.id


def test_good_pair_aligns():
    t, i = good_pair()
    rc, W, rho, its = oracle.find_transform_ecc(t, i, np.eye(3), oracle.MOTION_HOMOGRAPHY, 50, 1e-5, GAUSS)
    assert rc == 0 and rho > 0.99 and abs(W[0, 2] - 1.5) < 0.1 and abs(W[1, 2] + 1.0) < 0.1


# ---- the stack the GPU tests plant failing frames in -----------------------------------------------------------------
STACK_N, STACK_W, STACK_H = 6, 128, 96
STACK_CRITERIA = (50, 1e-5)


@functools.lru_cache(maxsize=None)
def good_stack():
    """synth.make_stack(6, 128, 96) as a read-only [n, h, w, 3] uint8 array."""
    from libstacker_rs_amd import synth
    frames, _ = synth.make_stack(STACK_N, STACK_W, STACK_H)
    f = frames.numpy().copy()
    f.setflags(write=False)
    return f


def planted_frame(status):
    """A frame that fails against frame 0 with the given status: its negative (2), a constant (1)."""
    f0 = good_stack()[0]
    return 255 - f0 if status == 2 else np.full_like(f0, 128)


def planted_stack(plan, bits=8):
    """The good stack with frame i replaced by planted_frame(plan[i]); bits = 16: the same stack times 257."""
    s = good_stack().copy()
    for i, status in plan.items():
        s[i] = planted_frame(status)
    return s if bits == 8 else s.astype(np.uint16) * 257


def grey8_stack_of(stack16):
    """A 3-channel 8-bit stack whose grey is EXACTLY the 8-bit reduction (grey16 + 128) // 257 the hybrid path describes
    16-bit frames on: B = G = R = g, and BGR2GRAY's integer weights sum to 1 << 14 (checked in
    test_planted_frames_fail_in_the_oracle)."""
    g8 = np.stack([((oracle.grey(f).astype(np.uint32) + 128) // 257).astype(np.uint8) for f in stack16])
    return np.ascontiguousarray(np.repeat(g8[..., None], 3, axis=3)), g8


def test_planted_frames_fail_in_the_oracle():
    f = good_stack()
    g0 = oracle.grey(f[0])
    tb0 = oracle.gaussian_blur_f32(g0, GAUSS)
    for status in (2, 1):
        g = oracle.grey(planted_frame(status))
        rc, W, rho, its = oracle.find_transform_ecc(g, g0, np.eye(3), oracle.MOTION_HOMOGRAPHY, *STACK_CRITERIA, GAUSS)
        assert (rc, its) == (status, 1)
    lam, corr, rho64, H = ecc_iteration_lambda(oracle.gaussian_blur_f32(oracle.grey(planted_frame(2)), GAUSS), tb0, np.eye(3),
                                               oracle.MOTION_HOMOGRAPHY)
    print("negated frame 0: lambda_d / |correlation| %.4f" % (lam / abs(corr)))
    assert lam <= -LAMBDA_MARGIN * abs(corr)
    # the good frames align from their ORB seeds; a planted frame fails the hybrid composition with its own status
    for bits in (8, 16):
        oracle.hybrid_match(list(planted_stack({}, bits)), max_count=STACK_CRITERIA[0], epsilon=STACK_CRITERIA[1])
        for status in (2, 1):
            with pytest.raises(RuntimeError, match="rc=%d on frame 3" % status):
                oracle.hybrid_match(list(planted_stack({3: status}, bits)), max_count=STACK_CRITERIA[0], epsilon=STACK_CRITERIA[1])
    # the 8-bit stand-in of the 16-bit stack: grey(B = G = R = g) == g
    grey3, g8 = grey8_stack_of(planted_stack({}, 16))
    assert all(np.array_equal(oracle.grey(grey3[i]), g8[i]) for i in range(STACK_N))
    # without an iteration the hybrid composition returns its seeds, and they are not the identity
    for bits in (8, 16):
        _, warps, iters, seeds = oracle.hybrid_match(list(planted_stack({}, bits)), max_count=0)
        assert not iters.any() and np.array_equal(warps, seeds)
        assert all(not np.array_equal(seeds[i], np.eye(3)) for i in range(1, STACK_N))

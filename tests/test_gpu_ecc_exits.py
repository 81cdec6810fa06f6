"""The exits of an ECC run other than convergence, on the GPU, against the table test_cpu_ecc_exits.py admits on the reference
side: a failed run (NaN rho, lambda_d <= 0) raises with the oracle's status and leaves the context as it was, a singular
Hessian moves nothing, a run without an iteration returns its start — the caller's warp at stage level, the identity in
ecc_match, the ORB seed in hybrid_match — and a failing frame inside a stack is named, whatever the entry point."""
import numpy as np
import pytest
import torch

from libstacker_rs_amd import (EccMatchParameters, KeyPointMatchParameters, MotionType, OpenCvError, RANSAC, SelectParameters,
                               synth)
from test_cpu_ecc_exits import (GAUSS, MESSAGES, STACK_CRITERIA, STACK_H, STACK_N, STACK_W, cases_of, good_pair, good_stack,
                                grey8_stack_of, planted_stack, same_values)
from test_gpu_ecc_iteration import DEFAULTS, MOTION, RHO_BAR, ROUTES

pytestmark = pytest.mark.gpu

GOOD = EccMatchParameters(MotionType.Homography, 50, 1e-5, GAUSS)
STACK = EccMatchParameters(MotionType.Homography, STACK_CRITERIA[0], STACK_CRITERIA[1], GAUSS)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)


class options:
    """Engine options for the length of a with-block, then back to their defaults."""
    ALL = dict(DEFAULTS, ecc_slots=0)

    def __init__(self, stacker, opts):
        self.stacker, self.opts = stacker, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.stacker.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.stacker.set_option(k, self.ALL[k])


def run_case(stacker, c, max_count=-1, epsilon=-1):
    p = EccMatchParameters(MOTION[c.motion], c.max_count if max_count == -1 else max_count,
                           c.epsilon if epsilon == -1 else epsilon, GAUSS)
    return stacker.find_transform_ecc(c.templ, c.inp, c.start_arg, p)


def align_good_pair(stacker):
    t, i = good_pair()
    return stacker.find_transform_ecc(t, i, np.eye(3), GOOD)


def same_result(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2]


# ---- stage level -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["status2", "status1"])
def test_failed_run_raises_the_oracles_status_and_leaves_the_context_usable(stacker, kind):
    failures = []
    for name, opts in ROUTES:
        with options(stacker, opts):
            before = align_good_pair(stacker)
            assert before[1] > 0.99
            for c in cases_of(kind):
                rc = c.oracle()[0]
                try:
                    got = run_case(stacker, c)
                    failures.append((c.id, name, "no error", got[1], got[2]))
                except OpenCvError as e:
                    print("%-52s %-15s %s" % (c.id, name, str(e)[:60]))
                    if str(e) != MESSAGES[rc]:
                        failures.append((c.id, name, str(e)))
                if not same_result(align_good_pair(stacker), before):
                    failures.append((c.id, name, "the good pair changed after the failure"))
    assert not failures, failures


@pytest.mark.parametrize("axis", ["vstripes", "hstripes"])
def test_singular_hessian_moves_nothing(stacker, axis):
    """A Hessian with exact zero rows (LU: pivot below 10 FLT_EPSILON at the first or second step; P <= 3: determinant 0)
    inverts to 0: the warp stays the start, rho is the start's, and the loop ends as the oracle's does."""
    failures, worst = [], 0.0
    for c in cases_of("singular"):
        if axis not in c.id:
            continue
        rc, Wo, rho_o, its_o = c.oracle()
        rc4, W4, rho_o4, its_o4 = c.oracle(4, None)
        for name, opts in ROUTES:
            with options(stacker, opts):
                for (mc, eps), want_its, want_rho in (((c.max_count, c.epsilon), 2, rho_o), ((4, None), 4, rho_o4)):
                    W, rho, its = run_case(stacker, c, mc, eps)
                    drho = abs(rho - want_rho)
                    worst = max(worst, drho)
                    print("%-52s %-15s count %s eps %s: its %d |rho - rho_oracle| %.2e" % (c.id, name, mc, eps, its, drho))
                    if not same_values(W, c.start):
                        failures.append((c.id, name, mc, "warp moved", W))
                    if its != want_its:
                        failures.append((c.id, name, mc, "iterations", its))
                    if not drho <= RHO_BAR:
                        failures.append((c.id, name, mc, "|drho| %.3e" % drho))
    print("worst |rho - rho_oracle| over the %s cases: %.2e" % (axis, worst))
    assert not failures, failures


def test_run_without_an_iteration_returns_the_start(stacker):
    failures = []
    for c in cases_of("zero"):
        rc, Wo, rho_o, its_o = c.oracle()
        assert (rc, its_o, rho_o) == (0, 0, -1.0) and Wo.tobytes() == c.start.tobytes()
        rows = 3 if c.motion == "homography" else 2
        for name, opts in ROUTES:
            with options(stacker, opts):
                W, rho, its = run_case(stacker, c)
            print("%-52s %-15s its %d rho %r warp == start: %s" % (c.id, name, its, rho, W[:rows].tobytes() == c.start[:rows].tobytes()))
            if W[:rows].tobytes() != c.start[:rows].tobytes():
                failures.append((c.id, name, "warp", W.tolist()))
            if (its, rho) != (0, -1.0):
                failures.append((c.id, name, "its / rho", its, rho))
    assert not failures, failures


def test_boundary_epsilon_one_half_iterates(stacker):
    """epsilon = 0.5 is the largest that still runs: compared with the oracle like test_fixed_iteration_count_no_eps."""
    for c in cases_of("boundary"):
        rc, Wo, rho_o, its_o = c.oracle()
        for name, opts in ROUTES:
            with options(stacker, opts):
                W, rho, its = run_case(stacker, c)
            e = synth.corner_error(W, Wo, c.w, c.h)
            print("%-52s %-15s its %d (oracle %d) %.2e px |drho| %.1e" % (c.id, name, its, its_o, e, abs(rho - rho_o)))
            assert its == its_o and its >= 1, (c.id, name)
            assert e <= 0.01, (c.id, name)
            np.testing.assert_allclose(W, Wo, rtol=0, atol=2e-5)
            assert abs(rho - rho_o) <= RHO_BAR


# ---- stack level -----------------------------------------------------------------------------------------------------
FEEDS = [("host", 0), ("host", 2), ("device", 0), ("device", 2)]
FEED_IDS = ["%s-slots%d" % f for f in FEEDS]


def fed(stack, feed):
    """The stack as the engine takes it: a list of host arrays, or one device tensor."""
    return list(stack) if feed == "host" else torch.from_numpy(stack.copy()).cuda()


def as_numpy(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def same_stats(a, b):
    return len(a) == len(b) and all(x["status"] == y["status"] and x["iterations"] == y["iterations"] and x["rho"] == y["rho"] and
                                    np.asarray(x["warp"]).tobytes() == np.asarray(y["warp"]).tobytes() for x, y in zip(a, b))


def expect_failure(call, frame, status):
    with pytest.raises(OpenCvError) as ei:
        call()
    msg = str(ei.value)
    assert "[frame %d]" % frame in msg and MESSAGES[status] in msg, msg


@pytest.mark.parametrize("feed,slots", FEEDS, ids=FEED_IDS)
def test_failing_frame_in_a_stack_is_named(stacker, feed, slots):
    with options(stacker, {"ecc_slots": slots}):
        good = fed(good_stack(), feed)
        out0, stats0 = stacker.ecc_match(good, STACK, return_stats=True)
        out0 = as_numpy(out0).copy()
        for plan, frame, status in (({3: 2}, 3, 2), ({3: 1}, 3, 1), ({2: 2, 4: 1}, 2, 2), ({2: 1, 4: 2}, 2, 1)):
            bad = fed(planted_stack(plan), feed)
            expect_failure(lambda: stacker.ecc_match(bad, STACK, return_stats=True), frame, status)
            out, stats = stacker.ecc_match(good, STACK, return_stats=True)
            assert np.array_equal(as_numpy(out), out0) and same_stats(stats, stats0), plan


@pytest.mark.parametrize("feed,slots", FEEDS, ids=FEED_IDS)
def test_every_entry_point_reports_the_failing_frame(stacker, feed, slots):
    """The combines run the plain call first: its error is theirs. After each failure the good stack gives, through the same
    context, the bits it gave before any of them."""
    with options(stacker, {"ecc_slots": slots}):
        good = fed(good_stack(), feed)
        out0, stats0 = stacker.ecc_match(good, STACK, return_stats=True)
        out0 = as_numpy(out0).copy()
        good16 = fed(planted_stack({}, 16), feed)
        hyb0, hstats0 = stacker.hybrid_match(good16, KP, STACK, return_stats=True)
        hyb0 = as_numpy(hyb0).copy()

        def still_good(label):
            out, stats = stacker.ecc_match(good, STACK, return_stats=True)
            assert np.array_equal(as_numpy(out), out0) and same_stats(stats, stats0), label

        for status in (2, 1):
            bad = fed(planted_stack({3: status}), feed)
            acc = torch.empty((STACK_H, STACK_W, 3), dtype=torch.float32, device="cuda")
            calls = [("shard", lambda: stacker.ecc_match_shard(bad, STACK, True, acc)),
                     ("clipped", lambda: stacker.ecc_match_clipped(bad, STACK)),
                     ("quantile", lambda: stacker.ecc_match_quantile(bad, STACK)),
                     ("weighted", lambda: stacker.ecc_match_weighted(bad, STACK))]
            for label, call in calls:
                expect_failure(call, 3, status)
                still_good((label, status))
            bad16 = fed(planted_stack({3: status}, 16), feed)
            expect_failure(lambda: stacker.hybrid_match(bad16, KP, STACK), 3, status)
            still_good(("hybrid", status))
            hyb, hstats = stacker.hybrid_match(good16, KP, STACK, return_stats=True)
            assert np.array_equal(as_numpy(hyb), hyb0) and same_stats(hstats, hstats0), status
        # ranked: the kept list is in ranked order, and the error names the failing frame's place in it. The constant frame has
        # no sharpness at all: the selection keeps it (nothing is dropped), as the last of the list.
        bad = fed(planted_stack({3: 1}), feed)
        select = SelectParameters()
        order, n_kept, _, _ = stacker.rank(bad, select)
        assert n_kept == STACK_N and int(order[-1]) == 3 and int(order[0]) != 3
        expect_failure(lambda: stacker.ecc_match_ranked(bad, STACK, select), STACK_N - 1, 1)
        still_good(("ranked", 1))


def identity_fold(stacker, stack, is_affine=False):
    """finalize_mean of the frames folded through the identity, in stack order."""
    acc = None
    M = np.eye(2, 3) if is_affine else np.eye(3)
    for f in torch.from_numpy(stack.copy()).cuda():
        acc = stacker.warp_accumulate(f, M, is_affine=is_affine, acc=acc)
    return stacker.finalize_mean(acc, len(stack)).cpu().numpy()


@pytest.mark.parametrize("criteria", [(0, 1e-5), (50, 0.6)], ids=["count0", "eps0.6"])
@pytest.mark.parametrize("feed", ["host", "device"])
def test_ecc_match_without_an_iteration_folds_through_the_identity(stacker, feed, criteria):
    stack = good_stack()
    frames = fed(stack, feed)
    want = {False: identity_fold(stacker, stack), True: identity_fold(stacker, stack, is_affine=True)}
    for motion, scale in ((MotionType.Homography, None), (MotionType.Homography, 60.0), (MotionType.Affine, None)):
        out, stats = stacker.ecc_match(frames, EccMatchParameters(motion, criteria[0], criteria[1], GAUSS), scale_down_width=scale,
                                       return_stats=True)
        for i, s in enumerate(stats[1:], 1):
            assert (s["status"], s["iterations"], s["rho"]) == (0, 0, -1.0), (motion, scale, i, s)
            assert np.array_equal(s["warp"], np.eye(3)), (motion, scale, i, s["warp"])
        assert np.array_equal(as_numpy(out), want[motion == MotionType.Affine]), (motion, scale)


@pytest.mark.parametrize("criteria", [(0, 1e-5), (50, 0.6)], ids=["count0", "eps0.6"])
@pytest.mark.parametrize("bits", [8, 16])
def test_hybrid_match_without_an_iteration_folds_through_the_orb_seeds(stacker, bits, criteria):
    """include/stacker.h: the ORB homography H / h22, cast to f32, IS findTransformECC's initial warp; with no iteration it
    is the result. The 16-bit seeds are checked through an 8-bit stand-in whose grey is exactly the 8-bit reduction ORB
    runs on (B = G = R = (grey16 + 128) // 257: test_cpu_ecc_exits.grey8_stack_of), not through a tolerance."""
    stack = planted_stack({}, bits)
    orb_stack = stack if bits == 8 else grey8_stack_of(stack)[0]
    if bits == 16:
        g8 = grey8_stack_of(stack)[1]
        assert all(np.array_equal(stacker.grey(orb_stack[i]), g8[i]) for i in range(STACK_N))
    _, _, kstats = stacker.keypoint_match(list(orb_stack), KP, return_stats=True)
    out, stats = stacker.hybrid_match(list(stack), KP, EccMatchParameters(MotionType.Homography, criteria[0], criteria[1], GAUSS),
                                      return_stats=True)
    alpha = 1.0 / 255.0 if bits == 8 else 1.0 / 65535.0
    acc = stacker.warp_accumulate(stack[0], np.eye(3), alpha=alpha)
    n_seeded = 0
    for i in range(1, STACK_N):
        k, s = kstats[i], stats[i]
        H = np.asarray(k["warp"], np.float64)
        want = np.eye(3, dtype=np.float32)
        if k["status"] == 0 and abs(H[2, 2]) > 1e-12:
            want = (H / H[2, 2]).astype(np.float32)
            n_seeded += 1
        print("frame %d: keypoints %d matches %d seed == f32(H / h22): %s" % (i, s["n_keypoints"], s["n_matches"],
                                                                              np.array_equal(s["warp"], want.astype(np.float64))))
        assert (s["status"], s["iterations"], s["rho"]) == (0, 0, -1.0), (i, s)
        assert np.array_equal(s["warp"], want.astype(np.float64)), (i, s["warp"], want)
        assert (s["n_keypoints"], s["n_matches"]) == (k["n_keypoints"], k["n_matches"]), i
        acc = stacker.warp_accumulate(stack[i], s["warp"], alpha=alpha, acc=acc)
    assert stats[0]["n_keypoints"] == kstats[0]["n_keypoints"]
    assert n_seeded == STACK_N - 1, "a frame without an ORB seed: the test would say nothing about it"
    want_img = stacker.finalize_mean(torch.from_numpy(acc).cuda(), STACK_N).cpu().numpy()
    assert np.array_equal(out, want_img)

"""The first ECC iteration of a frame that starts at the identity takes a short route through the column pass (option
ecc_first_iter, default on): the sums that do not read the template come from one evaluation per call, the 11 that do are
accumulated from the template and frame 0's own pixels. It runs the operations of the general route in the same order, so
nothing may differ in a single bit with the option on and off: warps, iteration counts, rho, the stacked image. The shapes
are the smallest at which the (column strip, row) partition changes its behaviour; the counter ecc_first_iter_slots of timing()
says which slot-iterations took the route."""
import contextlib

import numpy as np
import pytest

import oracle
from libstacker_rs_amd import EccMatchParameters, KeyPointMatchParameters, MotionType, RANSAC, synth

pytestmark = pytest.mark.gpu

PRODUCTION = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)      # examples/main.rs:107-112
ONE = EccMatchParameters(MotionType.Homography, 1, None, 5)                # the first iteration is the whole result
DEFAULTS = {"ecc_first_iter": 1, "ecc_blocks": 0, "ecc_slots": 0, "ecc_groups": 0, "ecc_variant": 3}
# (width, height, frames): a partial last column strip (the iteration tests' case); runs that straddle two columns and
# strips under 8 rows; one column and fewer row units than waves; a last column one lane wide; the general small stack
SHAPES = [(449, 200, 3), (130, 37, 3), (64, 9, 3), (65, 40, 3), (640, 480, 8)]

_stacks = {}


def stack(n, w, h):
    if (n, w, h) not in _stacks:
        _stacks[(n, w, h)] = synth.make_stack(n, w, h)[0]
    return _stacks[(n, w, h)]


@contextlib.contextmanager
def options(stacker, opts):
    try:
        for k, v in opts.items():
            stacker.set_option(k, v)
        yield
    finally:
        for k in opts:
            stacker.set_option(k, DEFAULTS[k])


def run(stacker, src, params, opts):
    """(outcome, counter): outcome = (image, iterations, rhos, warps) or the error the stack fails with."""
    with options(stacker, opts):
        try:
            out, stats = stacker.ecc_match(src, params, return_stats=True)
            res = (out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out), [s["iterations"] for s in stats],
                   [s["rho"] for s in stats], [s["warp"] for s in stats])
        except Exception as e:          # a frame too small to correlate fails the same way by both routes
            res = (type(e), str(e))
        return res, stacker.timing()["ecc_first_iter_slots"]


def assert_same(on, off, label):
    if isinstance(on[0], type) or isinstance(off[0], type):
        assert on == off, label
        return
    assert on[1] == off[1], (label, "iterations", on[1], off[1])
    assert on[2] == off[2], (label, "rho", on[2], off[2])
    assert all(np.array_equal(a, b) for a, b in zip(on[3], off[3])), (label, "warps")
    assert np.array_equal(on[0], off[0]), (label, "image")


@pytest.mark.parametrize("w,h,n", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
@pytest.mark.parametrize("blocks", [0, 8], ids=["blocks-auto", "blocks8"])
@pytest.mark.parametrize("params", [ONE, PRODUCTION], ids=["one-iteration", "production"])
def test_on_and_off_agree_bit_for_bit(stacker, w, h, n, blocks, params):
    dev = stack(n, w, h).cuda()
    on, c_on = run(stacker, dev, params, {"ecc_blocks": blocks})
    off, c_off = run(stacker, dev, params, {"ecc_blocks": blocks, "ecc_first_iter": 0})
    assert_same(on, off, (w, h, blocks))
    assert c_on == n - 1 and c_off == 0, (c_on, c_off)


def test_refills_mix_first_and_later_iterations_in_one_launch(stacker):
    """12 frames through 2 slots: a refilled slot is at its first iteration while its neighbour is not. From pinned host
    memory frames enter slots that sat idle while `ready` trailed; with two slot groups the launches alternate streams."""
    frames = stack(12, 640, 480)
    dev, pinned = frames.cuda(), frames.pin_memory()
    ref, c = run(stacker, dev, PRODUCTION, {"ecc_first_iter": 0})
    assert c == 0
    for label, src, opts in (("slots2", dev, {"ecc_slots": 2}), ("slots2-host", pinned, {"ecc_slots": 2}),
                             ("groups", dev, {"ecc_groups": 2}), ("groups-slots8", dev, {"ecc_groups": 2, "ecc_slots": 8})):
        on, c_on = run(stacker, src, PRODUCTION, opts)
        off, c_off = run(stacker, src, PRODUCTION, dict(opts, ecc_first_iter=0))
        assert_same(on, off, label)
        assert_same(on, ref, label + " vs plain")
        assert c_on == 11 and c_off == 0, (label, c_on, c_off)


def test_counter_is_zero_where_the_route_does_not_apply(stacker):
    frames = stack(3, 449, 200)
    dev = frames.cuda()
    _, c = run(stacker, dev, PRODUCTION, {"ecc_variant": 0})
    assert c == 0
    f32 = [f.astype(np.float32) for f in frames.numpy()]
    on, c_on = run(stacker, f32, PRODUCTION, {})
    off, c_off = run(stacker, f32, PRODUCTION, {"ecc_first_iter": 0})
    assert_same(on, off, "32F")
    assert c_on == 0 and c_off == 0
    g = [oracle.grey(f).astype(np.float32) for f in frames.numpy()[:2]]
    stacker.find_transform_ecc(g[1], g[0], np.eye(3), PRODUCTION)
    assert stacker.timing()["ecc_first_iter_slots"] == 0


@pytest.mark.parametrize("motion", [MotionType.Affine, MotionType.Euclidean, MotionType.Translation])
def test_other_motions_keep_the_general_route(stacker, motion):
    p = EccMatchParameters(motion, 50, 1e-4, 5)
    for n, w, h in ((3, 449, 200), (8, 640, 480)):
        dev = stack(n, w, h).cuda()
        on, c_on = run(stacker, dev, p, {})
        off, c_off = run(stacker, dev, p, {"ecc_first_iter": 0})
        assert_same(on, off, (motion, w, h))
        assert c_on == 0 and c_off == 0


def test_find_transform_ecc_starts(stacker):
    """An explicit identity start takes the route once; a start one ulp of one entry away from it does not. Both give the
    bits of the option-off run."""
    frames = stack(3, 449, 200).numpy()
    g0, g1 = oracle.grey(frames[0]), oracle.grey(frames[1])
    eye = np.eye(3, dtype=np.float32)
    near = eye.copy()
    near[0, 1] = np.nextafter(np.float32(0), np.float32(1))
    near2 = eye.copy()
    near2[1, 1] = np.nextafter(np.float32(1), np.float32(2))
    for start, want in ((eye, 1), (near, 0), (near2, 0)):
        for p in (ONE, PRODUCTION):
            W, rho, its = stacker.find_transform_ecc(g1, g0, start, p)
            assert stacker.timing()["ecc_first_iter_slots"] == want
            with options(stacker, {"ecc_first_iter": 0}):
                W0, rho0, its0 = stacker.find_transform_ecc(g1, g0, start, p)
                assert stacker.timing()["ecc_first_iter_slots"] == 0
            assert np.array_equal(W, W0) and rho == rho0 and its == its0, (start, W, W0)


def test_hybrid_seeds(stacker):
    """ORB-seeded ECC: only a frame whose seed is the identity (no homography found) may take the route."""
    frames = list(stack(4, 640, 480).numpy())
    kp = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
    ecc = EccMatchParameters(MotionType.Homography, 200, 1e-5, 5)
    out, stats = stacker.hybrid_match(frames, kp, ecc, return_stats=True)
    c_on = stacker.timing()["ecc_first_iter_slots"]
    with options(stacker, {"ecc_first_iter": 0}):
        out0, stats0 = stacker.hybrid_match(frames, kp, ecc, return_stats=True)
        assert stacker.timing()["ecc_first_iter_slots"] == 0
    # a frame for which findHomography returned nothing has no inliers: its seed is the identity
    assert c_on == sum(1 for s in stats[1:] if s["n_inliers"] == 0)
    assert [s["iterations"] for s in stats] == [s["iterations"] for s in stats0]
    assert [s["rho"] for s in stats] == [s["rho"] for s in stats0]
    assert all(np.array_equal(a["warp"], b["warp"]) for a, b in zip(stats, stats0))
    assert np.array_equal(np.asarray(out), np.asarray(out0))

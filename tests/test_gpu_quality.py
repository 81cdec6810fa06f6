"""Score and rank a whole stack on the device (include/stacker.h: stk_stack_sharpness, stk_ecc_match_ranked,
stk_keypoint_match_ranked): the first half of examples/main.rs:35-64. Every score is compared with the CPU
oracle and with the per-frame route (stk_grey + stk_sharpness) with ==, never a tolerance: the pass sums exact integers."""
import numpy as np
import pytest
import torch

import oracle
from conftest import assert_ecc_stack_close, assert_stack_close
from libstacker_rs_amd import (EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType, NotEnoughFiles,
                               NotImplementedYet, RANSAC, SelectParameters, WeightParameters, rank_frames, synth)
from libstacker_rs_amd.api import QUALITY_WEIGHT_SCORE, SHARPNESS_TENG

pytestmark = pytest.mark.gpu

TILE = 64                                   # kernels_quality.hip: QT_W = QT_H
SHAPES = [(97, 131), (240, 320), (5, 3), (1, 17), (33, 1), (479, 641),
          (TILE, TILE), (TILE - 1, TILE - 1), (TILE + 1, TILE + 1), (TILE - 1, TILE + 1), (TILE + 1, TILE - 1),
          (2 * TILE, TILE), (TILE, 2 * TILE)]


def _frames(n, shape, cn, seed=0):
    rng = np.random.default_rng(1000 * seed + 10 * shape[0] + shape[1] + cn)
    return [rng.integers(0, 256, shape if cn == 1 else shape + (cn,), dtype=np.uint8) for _ in range(n)]


def _grey(f):
    return f if f.ndim == 2 else oracle.grey(np.ascontiguousarray(f[..., :3]))


def _oracle_scores(frames, k):
    return np.array([[oracle.sharpness(g, 0), oracle.sharpness(g, 1), oracle.sharpness(g, 2, k), oracle.sharpness(g, 3)]
                     for g in map(_grey, frames)])


def _per_frame_scores(s, frames, k):
    """The route the engine offered before: stk_grey, then one stk_sharpness call per metric."""
    rows = []
    for f in frames:
        g = f if f.ndim == 2 else s.grey(f)
        rows.append([s.sharpness_modified_laplacian(g), s.sharpness_variance_of_laplacian(g), s.sharpness_tenengrad(g, k),
                     s.sharpness_normalized_gray_level_variance(g)])
    return np.array(rows)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_scores_equal_the_oracle_and_the_per_frame_route(stacker, shape, cn):
    frames = _frames(2, shape, cn)
    for k in (1, 3, 5, 7):
        got = stacker.stack_sharpness(frames, k)
        assert got.shape == (2, 4) and got.dtype == np.float64
        ref = _oracle_scores(frames, k)
        for i in range(2):
            assert tuple(got[i]) == tuple(ref[i]), (shape, cn, k, i)
        assert _same_bits(got, _per_frame_scores(stacker, frames, k))


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("shape", [(97, 131), (479, 641), (2 * TILE, 3 * TILE)])
def test_host_arrays_one_tensor_and_a_shuffled_list_of_tensors_agree(stacker, shape, cn, n):
    frames = _frames(n, shape, cn, seed=n)
    for k in (3, 7):
        ref = _oracle_scores(frames, k)
        host = stacker.stack_sharpness(frames, k)
        assert _same_bits(host, ref)
        stack = torch.from_numpy(np.stack(frames).reshape((n,) + shape + (cn,))).cuda()
        assert _same_bits(stacker.stack_sharpness(stack, k), ref)
        # separately allocated tensors handed over in another order: the pass may not assume a distance between frames
        perm = np.random.default_rng(n).permutation(n)
        spacers, tensors = [], {}
        for i in perm[::-1]:
            tensors[int(i)] = torch.from_numpy(frames[i]).cuda()
            spacers.append(torch.empty(1000 + 77 * int(i), dtype=torch.uint8, device="cuda"))
        assert _same_bits(stacker.stack_sharpness([tensors[int(i)] for i in perm], k), ref[perm])


def test_host_stacks_larger_than_one_upload_batch():
    from libstacker_rs_amd import Stacker
    frames = _frames(21, (70, 90), 3)
    s = Stacker(0)                                            # a fresh context: its frame workspace is still empty
    try:
        s.set_option("upload_batch", 2)
        got = s.stack_sharpness(frames, 5)
    finally:
        s.close()
    assert _same_bits(got, _oracle_scores(frames, 5))


def test_saturated_4k_frames_pin_the_int64_bound(stacker):
    # a one-pixel checkerboard of 0 / 255 drives every filter to its extreme at every pixel; all-255 the plain sums
    yy, xx = np.mgrid[0:2160, 0:3840]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    white = np.full((2160, 3840, 3), 255, np.uint8)
    got = stacker.stack_sharpness([board, white], 7)
    ref = _oracle_scores([board, white], 7)
    print("saturated 4K, ksize 7: engine", got.tolist(), "oracle", ref.tolist())
    assert _same_bits(got, ref)
    one = stacker.stack_sharpness([board[..., 0].copy()], 7)   # the same grey as a one-channel frame
    assert _same_bits(one, ref[:1])
    # TENG's antisymmetric derivative taps cancel on a period-2 pattern, so the board leaves its sum at 0. Stripes four
    # pixels wide bring it to its extreme instead: the row derivative takes the values 10, 10, 4, -4, -10, -10, -4, 4 (x 255)
    # over a period, gx = 64 x that, so gx^2 averages 58 x 16320^2 = 1.5e10 per pixel: above 2^32 in every product's sum
    stripes = np.repeat(np.where((xx // 4) & 1, 255, 0).astype(np.uint8)[..., None], 3, axis=2)
    rows = np.repeat(np.where((yy // 4) & 1, 255, 0).astype(np.uint8)[..., None], 3, axis=2)
    got = stacker.stack_sharpness([stripes, rows], 7)
    ref = _oracle_scores([stripes, rows], 7)
    print("4-px stripes 4K, ksize 7: engine", got.tolist(), "oracle", ref.tolist())
    assert _same_bits(got, ref)
    assert got[0, SHARPNESS_TENG] > 2.0 ** 32 and got[1, SHARPNESS_TENG] > 2.0 ** 32


def test_full_size_stack_equals_the_per_frame_route(stacker):
    frames, _ = synth.make_stack(8, 3840, 2160, device="cuda:0")
    host = frames.cpu().numpy()
    for k in (3, 7):
        got = stacker.stack_sharpness(frames, k)
        assert _same_bits(got, _per_frame_scores(stacker, list(host), k))
        for i in (0, 5):
            assert tuple(got[i]) == tuple(_oracle_scores([host[i]], k)[0])
    t = stacker.timing()
    assert t["prep_ms"] > 0 and t["align_ms"] == 0 and t["warp_ms"] == 0    # the pass reports through prep_ms


def test_two_calls_and_two_input_forms_return_the_same_bits(stacker):
    frames, _ = synth.make_stack(5, 640, 480, device="cuda:0")
    a = stacker.stack_sharpness(frames, 3)
    b = stacker.stack_sharpness(frames, 3)
    c = stacker.stack_sharpness([f.clone() for f in frames.unbind(0)], 3)
    assert _same_bits(a, b) and _same_bits(a, c)


def _example_stack():
    """The ten 800x600 frames of test_gpu_example_flow.py with the same graded blurs."""
    frames, _ = synth.make_stack(10, 800, 600)
    fr = [f.copy() for f in frames.numpy()]
    for idx, k in ((4, 7), (7, 3), (2, 3)):
        b = np.stack([np.clip(np.rint(oracle.gaussian_blur_f32(fr[idx][..., c].copy(), k)), 0, 255) for c in range(3)], -1).astype(np.uint8)
        if k == 7:
            b = np.stack([np.clip(np.rint(oracle.gaussian_blur_f32(b[..., c].copy(), 7)), 0, 255) for c in range(3)], -1).astype(np.uint8)
        fr[idx] = b
    return fr


def _restated(column, drop):
    return sorted(range(len(column)), key=lambda i: column[i])[drop:][::-1]       # main.rs:53, 64


def test_ranked_calls_are_the_plain_calls_on_the_ranked_list(stacker):
    fr = _example_stack()
    n = len(fr)
    ref_scores = _oracle_scores(fr, 3)
    teng = ref_scores[:, SHARPNESS_TENG]
    assert len(set(teng.tolist())) == n, "the oracle's TENG scores must be pairwise distinct for the order to be defined"
    want = _restated(teng, 1)
    sel = SelectParameters(metric=SHARPNESS_TENG, ksize=3, drop_worst=1)
    kp = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)               # main.rs:69-76
    ecc = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)     # main.rs:107-112

    order, n_kept, scores, weights = stacker.rank(fr, sel)
    assert _same_bits(scores, ref_scores)
    assert n_kept == n - 1 and list(order[:n_kept]) == want and order[n_kept] == 4       # frame 4 is the one dropped
    assert sorted(order.tolist()) == list(range(n))
    files = [fr[i] for i in want]

    img, kept, sc, stats = stacker.ecc_match_ranked(fr, ecc, sel, return_scores=True, return_stats=True)
    assert list(kept) == want and _same_bits(sc, ref_scores) and len(stats) == n - 1
    plain, pstats = stacker.ecc_match(files, ecc, return_stats=True)
    assert np.array_equal(img.view(np.uint32), plain.view(np.uint32))
    for a, b in zip(stats, pstats):
        assert a["iterations"] == b["iterations"] and a["rho"] == b["rho"] and np.array_equal(a["warp"], b["warp"])
    e_ref, warps, iters = oracle.ecc_match(files, max_count=5000, epsilon=1e-5, gauss_filt_size=5)
    assert_ecc_stack_close(img, e_ref, files, warps, label="ranked ecc", iters=[s["iterations"] for s in stats[1:]], iters_ref=iters[1:])

    dropped, kimg, kkept, kstats = stacker.keypoint_match_ranked(fr, kp, sel, return_stats=True)
    assert list(kkept) == want
    pdropped, kplain, kpstats = stacker.keypoint_match(files, kp, return_stats=True)
    assert dropped == pdropped == 0
    assert np.array_equal(kimg.view(np.uint32), kplain.view(np.uint32))
    for a, b in zip(kstats, kpstats):
        assert a["status"] == b["status"] and a["n_inliers"] == b["n_inliers"] and np.array_equal(a["warp"], b["warp"])
    d_o, k_ref = oracle.keypoint_match(files)
    assert d_o == 0
    assert_stack_close(kimg, k_ref, bulk=9e-6)

    # device-resident frames: the same ranking, the same bits as the plain call on the permuted tensors
    dev = [torch.from_numpy(f).cuda() for f in fr]
    dimg, dkept = stacker.ecc_match_ranked(dev, ecc, sel)
    assert list(dkept) == want
    assert torch.equal(dimg, stacker.ecc_match([dev[i] for i in want], ecc))


def test_rank_composes_with_the_weighted_combine(stacker, small_stack):
    frames, _ = small_stack
    fr = [f.copy() for f in frames]
    fr[2] = np.stack([np.clip(np.rint(oracle.gaussian_blur_f32(fr[2][..., c].copy(), 5)), 0, 255) for c in range(3)], -1).astype(np.uint8)
    sel = SelectParameters(metric=SHARPNESS_TENG, ksize=3, weight_mode=QUALITY_WEIGHT_SCORE)
    order, n_kept, scores, w = stacker.rank(fr, sel)
    teng = _oracle_scores(fr, 3)[:, SHARPNESS_TENG]
    want = _restated(teng, 0)
    assert n_kept == len(fr) and list(order) == want and order[-1] == 2
    w_ref = np.array([np.float32(teng[i] / teng[want[0]]) for i in want], np.float32)
    assert np.array_equal(w.view(np.uint32), w_ref.view(np.uint32)) and w[0] == 1.0 and 0 < w[-1] < 1
    files = [fr[i] for i in order[:n_kept]]
    ecc = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    a = stacker.ecc_match_weighted(files, ecc, WeightParameters(), weights=w[:n_kept])
    b = stacker.ecc_match_weighted(files, ecc, WeightParameters(), weights=w_ref)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the host half alone gives the same selection from the same scores
    o2, k2, w2 = rank_frames(scores, sel)
    assert list(o2) == list(order) and k2 == n_kept and np.array_equal(w2, w)


def test_errors_leave_the_context_usable(stacker):
    good = _frames(3, (40, 50), 3)
    ref = _oracle_scores(good, 3)
    ecc = EccMatchParameters(MotionType.Homography, 50, 1e-3, 5)

    def still_works():
        assert _same_bits(stacker.stack_sharpness(good, 3), ref)

    for bad in (np.zeros((2, 40, 50, 3), np.uint16), np.zeros((2, 40, 50, 3), np.float32)):
        with pytest.raises(NotImplementedYet):
            stacker.stack_sharpness(bad, 3)
        still_works()
        with pytest.raises(NotImplementedYet):
            stacker.ecc_match_ranked(list(bad), ecc, SelectParameters())
        still_works()
    with pytest.raises(InvalidParams, match="Kernel size must be 1, 3, 5, or 7"):
        stacker.stack_sharpness(good, 4)
    still_works()
    with pytest.raises(InvalidParams):
        stacker.ecc_match_ranked(good, ecc, SelectParameters(ksize=4))
    still_works()
    with pytest.raises(NotEnoughFiles):
        stacker.stack_sharpness([], 3)
    still_works()
    with pytest.raises(NotEnoughFiles):
        stacker.keypoint_match_ranked([], KeyPointMatchParameters(), SelectParameters())
    still_works()
    with pytest.raises(NotEnoughFiles):
        stacker.ecc_match_ranked(good, ecc, SelectParameters(drop_worst=3))          # nothing kept
    still_works()
    with pytest.raises(InvalidParams):
        stacker.ecc_match_ranked(good, ecc, SelectParameters(drop_worst=1, keep_fraction=0.5))
    still_works()

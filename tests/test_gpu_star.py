"""Star registration on the GPU (include/stacker.h, stk_star_params): stk_star_detect against the numpy restatement
(tests/star_restate.py) star for star — px, py, peak, npix exactly, flux (= S, an exact integer in f32) and x, y as bits, which
is as much of Sx and Sy as stk_star carries —, stk_star_align against the restated pipeline on the CPU test's stacks,
stk_star_match against its parts bit for bit, the composition with two caller-held-warps combines, and every refusal."""
import numpy as np
import pytest

import star_restate as sr
from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, DrizzleParameters, InvalidParams, NotEnoughFiles, NotImplementedYet,
                               RobustClipParameters, Stacker, StarParameters, synth)
from test_cpu_star import H, MOTIONS, W, flip_stack, motion_stack, rejects_stack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _place(frame, pad, device):
    """The frame where the call shall find it: host or device, tightly packed or as a row-strided view of a buffer whose rows
    are `pad` bytes longer."""
    f3 = frame if frame.ndim == 3 else frame[..., None]
    h, w, cn = f3.shape
    if device:
        import torch
        if not pad:
            return torch.from_numpy(np.ascontiguousarray(frame)).cuda()
        big = torch.zeros((h, w * cn + pad), dtype=torch.uint8, device="cuda")
        big[:, :w * cn] = torch.from_numpy(np.ascontiguousarray(f3).reshape(h, w * cn)).cuda()
        view = big[:, :w * cn].unflatten(1, (w, cn))
        assert h == 1 or view.stride(0) == w * cn + pad
        return view
    if not pad:
        return np.ascontiguousarray(frame)
    big = np.zeros((h, w * cn + pad), np.uint8)
    big[:, :w * cn] = f3.reshape(h, w * cn)
    view = big[:, :w * cn].reshape(h, w, cn)
    assert np.shares_memory(view, big) and view.strides[0] == w * cn + pad
    return view


def _channels(grey, cn, rng):
    """A cn-channel frame whose integer grey is NOT trivially one channel: B, G, R differ where cn >= 3."""
    if cn == 1:
        return grey
    f = np.stack([grey] * cn, -1)
    if cn == 4:
        f[..., 3] = rng.integers(0, 256, grey.shape, dtype=np.uint8)        # alpha: not read
    d = rng.integers(0, 3, grey.shape, dtype=np.uint8)
    f[..., 0] = np.minimum(f[..., 0].astype(np.int32) + d, 255).astype(np.uint8)
    f[..., 2] = np.maximum(f[..., 2].astype(np.int32) - d, 0).astype(np.uint8)
    return f


def _speckle(rng, h, w):
    """noise 0 .. 23 with one pixel in 40 raised to 40 .. 255, some of them in 2 x 2 groups: many peaks, ties and plateaus"""
    g = rng.integers(0, 24, (h, w), dtype=np.uint8)
    m = rng.random((h, w)) < 0.025
    g[m] = rng.integers(40, 256, int(m.sum()), dtype=np.uint8)
    ys, xs = np.nonzero(m & (rng.random((h, w)) < 0.3))
    for y, x in zip(ys, xs):
        g[y:y + 2, x:x + 2] = g[y, x]
    return g


def _check_detect(st, frames, p, device, pad):
    lists, peaks = st.star_detect([_place(f, pad, device) for f in frames], p, return_peaks=True)
    total = 0
    for k, f in enumerate(frames):
        want, n_peaks = sr.detect(f, p)
        assert int(peaks[k]) == n_peaks, (k, int(peaks[k]), n_peaks)
        assert len(lists[k]) == len(want), (k, len(lists[k]), len(want))
        assert lists[k].tobytes() == want.tobytes(), k
        total += len(want)
    return total


# (w, h, channels, radius, device, row padding, frames per launch)
DETECT_CASES = [
    (1, 1, 3, 4, 1, 0, 1), (1, 17, 1, 2, 0, 5, 2), (33, 1, 4, 7, 1, 5, 3), (5, 3, 3, 2, 0, 0, 1),
    (9, 9, 1, 4, 1, 0, 2),                 # exactly one admissible pixel at radius 4
    (64, 64, 3, 4, 1, 0, 3), (64, 64, 1, 7, 0, 0, 1), (64, 64, 4, 2, 1, 5, 2),
    (63, 65, 3, 7, 0, 5, 2), (63, 65, 4, 4, 1, 0, 1), (70, 130, 1, 2, 1, 5, 3), (70, 130, 3, 4, 0, 0, 2),
    (64, 128, 3, 2, 1, 0, 2), (64, 128, 1, 4, 0, 0, 3), (128, 64, 4, 7, 1, 0, 1), (128, 64, 3, 4, 1, 0, 3),   # the dword route
    (192, 70, 1, 7, 1, 0, 2), (192, 70, 4, 2, 0, 0, 1),   # dword tiles above a partial row of tiles
    (37, 641, 3, 4, 1, 0, 2), (37, 641, 4, 2, 0, 5, 1), (37, 641, 1, 7, 1, 5, 3),                              # the byte route
]


@pytest.mark.parametrize("case", DETECT_CASES, ids=["%dx%d-c%d-r%d-%s-pad%d-n%d" % (c[0], c[1], c[2], c[3], "dev" if c[4] else "host", c[5], c[6]) for c in DETECT_CASES])
def test_detect_equals_the_restatement(st, case):
    w, h, cn, r, device, pad, n = case
    rng = np.random.default_rng(1000 * w + h + cn + r)
    frames = [_channels(_speckle(rng, h, w), cn, rng) for _ in range(n)]
    found = _check_detect(st, frames, StarParameters(radius=r, min_pixels=1, max_stars=1024), device, pad)
    found += _check_detect(st, frames, StarParameters(radius=r, min_pixels=2, kappa=1.0, min_contrast=3, max_stars=50), device, pad)
    if w > 2 * r and h > 2 * r and w * h >= 64 * 64:
        assert found >= 5                                                   # the case does exercise the records
    if (w, h) == (9, 9):                                                    # the one admissible pixel, planted
        g = np.full((9, 9), 5, np.uint8)
        g[4, 4] = 90
        g[0, 0] = g[8, 8] = g[4, 3] = 80
        frames = [_channels(g, cn, rng)]
        assert _check_detect(st, frames, StarParameters(radius=4, min_pixels=1), device, pad) == 1


@pytest.mark.parametrize("cn,device", [(3, 1), (1, 0), (4, 1)])
def test_detect_on_generator_frames(st, cn, device):
    frames, _ = synth.make_star_stack([None, synth.star_motion(200, 150, 33.0, 5.0, -4.0)], 200, 150, 40, seed=5, channels=cn)
    for r in (2, 4, 7):
        assert _check_detect(st, list(frames), StarParameters(radius=r), device, 0) >= 30
    # max_stars truncation: the head of the full list; n_peaks still counts them all
    full, peaks = st.star_detect(list(frames), StarParameters(), return_peaks=True)
    cut, peaks_cut = st.star_detect(list(frames), StarParameters(max_stars=10), return_peaks=True)
    for a, b in zip(full, cut):
        assert len(a) > 10 and len(b) == 10 and a[:10].tobytes() == b.tobytes()
    assert peaks.tolist() == peaks_cut.tolist() and (peaks >= [len(a) for a in full]).all()
    assert _check_detect(st, list(frames), StarParameters(max_stars=10), device, 5) == 20
    # two calls give the same bits
    again = st.star_detect(list(frames), StarParameters())
    assert [a.tobytes() for a in again] == [a.tobytes() for a in full]


def test_constant_frame_gives_no_peak(st):
    for v in (0, 17, 255):
        lists, peaks = st.star_detect([np.full((70, 130, 3), v, np.uint8)], StarParameters(min_pixels=1), return_peaks=True)
        assert len(lists[0]) == 0 and peaks[0] == 0


def test_windows_and_plateaus_across_tile_corners(st):
    frames, want = [], []
    for (x, y) in ((63, 63), (64, 64), (63, 64)):                           # a 3 x 3 blob whose window lies in four tiles
        g = np.full((130, 130), 10, np.uint8)
        g[y - 1:y + 2, x - 1:x + 2] = 60
        g[y, x] = 120
        g[y, x + 1] = 90
        frames.append(g)
        want.append([(x, y)])
    g = np.full((130, 130), 10, np.uint8)
    g[63:65, 63:65] = 100                                                   # a plateau on the corner of four tiles
    g[20, 63] = g[20, 64] = 90                                              # a plateau across a vertical tile border
    g[63, 100] = g[64, 100] = 80                                            # and across a horizontal one
    g[100, 64] = g[100, 65] = g[101, 63] = 70                               # raster-first (64, 100): the pixel below-left comes later
    frames.append(g)
    want.append([(63, 63), (64, 100), (63, 20), (100, 63)])                 # S = 4 x 90, 3 x 60, 2 x 80, 2 x 70
    for r in (2, 4, 7):
        p = StarParameters(radius=r, min_pixels=2)
        for device in (0, 1):
            _check_detect(st, frames, p, device, 0)
        lists = st.star_detect(frames, p)
        assert [[(int(s["px"]), int(s["py"])) for s in l] for l in lists] == want


def test_more_than_32_peaks_in_a_tile(st):
    p = StarParameters(radius=2, min_pixels=1, max_stars=200)
    g = np.full((64, 64), 10, np.uint8)
    vals = 40 + np.random.default_rng(3).permutation(144)                   # 144 distinct fluxes on a lattice of spacing r + 1
    for k, v in enumerate(vals):
        g[2 + 3 * (k // 12), 2 + 3 * (k % 12)] = v
    lists, peaks = st.star_detect([g], p, return_peaks=True)
    assert peaks[0] == 144 and len(lists[0]) == 32
    assert lists[0]["peak"].tolist() == list(range(183, 151, -1))           # the 32 largest, brightest first
    # the densest lattice the tile holds, with repeated fluxes (ties go by py, then px), beside a sparse second tile
    g2 = np.full((64, 128), 10, np.uint8)
    for i in range(20):
        for j in range(20):
            g2[2 + 3 * i, 2 + 3 * j] = 40 + (7 * i + 13 * j) % 200
    g2[30, 100] = 250
    g3 = np.full((64, 128), 10, np.uint8)
    g3[:, 64:] = g                                                          # the first lattice in the second tile
    lists, peaks = st.star_detect([g2, g3], p, return_peaks=True)
    assert peaks.tolist() == [401, 144] and len(lists[0]) == 33 and len(lists[1]) == 32
    _check_detect(st, [g2, g3], p, 1, 0)
    _check_detect(st, [g2, g3], p, 0, 5)


# ---- stk_star_align against the restated pipeline -------------------------------------------------------------------
def _stats_equal(got, want, w, h):
    assert [s["status"] for s in got] == [s["status"] for s in want]
    for key in ("n_keypoints", "n_matches", "n_inliers"):
        assert [s[key] for s in got] == [s[key] for s in want], key
    for a, b in zip(got, want):
        if a["status"] == 0:
            assert synth.corner_error(a["warp"], b["warp"], w, h) <= 1e-3


@pytest.mark.parametrize("k", range(len(MOTIONS)))
def test_align_equals_the_restated_pipeline(st, k):
    frames, G = motion_stack(k)
    want, lists = sr.align(list(frames))
    import torch
    dropped, got = st.star_align(torch.from_numpy(frames).cuda() if k % 2 else list(frames))
    assert [a.tobytes() for a in st.star_detect(list(frames))] == [a.tobytes() for a in lists]
    _stats_equal(got, want, W, H)
    assert dropped == sum(s["status"] != 0 for s in got[1:])
    err = synth.corner_error(got[1]["warp"], G[1], W, H)
    print(MOTIONS[k], "stars", got[0]["n_keypoints"], got[1]["n_keypoints"], "inliers", got[1]["n_inliers"], "corner error %.3f px" % err)
    if min(len(lists[0]), len(lists[1])) >= 12:
        assert got[1]["status"] == 0 and err <= 0.5


def test_dropped_frames_are_reported_and_an_all_dropped_stack_fails(st):
    frames, G = rejects_stack()
    want, _ = sr.align(list(frames))
    dropped, got = st.star_align(list(frames))
    _stats_equal(got, want, W, H)
    assert dropped == 2 and [s["status"] for s in got] == [0, 0, 1, 1]
    with pytest.raises(InvalidParams, match="All images discarded"):        # the keypoint path's error
        st.star_align([frames[0], frames[3]])
    with pytest.raises(InvalidParams, match="All images discarded"):
        st.star_match([frames[0], frames[2], frames[3]])


# ---- stk_star_match against its parts -------------------------------------------------------------------------------
@pytest.mark.parametrize("cn,device,border", [(3, 1, BORDER_CONSTANT), (4, 0, BORDER_CONSTANT), (3, 0, BORDER_REPLICATE), (4, 1, BORDER_REPLICATE)])
def test_match_equals_its_parts(st, cn, device, border):
    import torch
    frames, G = rejects_stack()
    if cn == 4:
        frames = np.concatenate([frames, np.full(frames.shape[:3] + (1,), 200, np.uint8)], -1)
    files = [torch.from_numpy(f).cuda() for f in frames] if device else list(frames)
    p = StarParameters(border_mode=border, border_value=(0.1, 0.2, 0.3, 0.4))
    dropped, out, stats = st.star_match(files, p, return_stats=True)
    d2, stats2 = st.star_align(files, p)
    assert dropped == d2 == 2 and [s["status"] for s in stats] == [0, 0, 1, 1]
    for a, b in zip(stats, stats2):
        assert np.array_equal(a["warp"], b["warp"]) and a["n_inliers"] == b["n_inliers"]
    acc = None
    for f, s in zip(frames, stats):
        if s["status"] == 0:
            acc = st.warp_accumulate(torch.from_numpy(f).cuda(), s["warp"], border_mode=border, border_value=p.border_value, acc=acc)
    want = st.finalize_mean(acc, len(frames) - dropped)
    assert np.array_equal(_np(out), _np(want))


# ---- composition: the stats feed the caller-held-warps combines -----------------------------------------------------
def test_stats_feed_robust_clip_and_drizzle(st):
    n, w, h = 8, 240, 180
    mots = [None] + [synth.star_motion(w, h, 3.0 * i, 1.5 * i, -1.0 * i) for i in range(1, n)]
    frames, G = synth.make_star_stack(mots, w, h, 60, seed=9)
    clean, _ = synth.make_star_stack(mots, w, h, 60, seed=9, noise_sigma=0.0)
    frames = frames.copy()
    marked = np.zeros((h, w), bool)
    marked[80:83, 30:200] = True
    frames[3][marked] = np.minimum(frames[3][marked].astype(np.int32) + 128, 255).astype(np.uint8)   # a trail in one frame
    dropped, stats = st.star_align(list(frames))
    assert dropped == 0
    warps = [s["warp"] for s in stats]
    include = [s["status"] == 0 for s in stats]
    clip = RobustClipParameters(3.0, 3.0, 0.5 / 255.0, 2)
    out, cnt = st.robust_clip_stack(list(frames), warps, clip, include, return_counts=True)
    truth = st.robust_clip_stack(list(clean), warps, clip, include)
    assert out.shape == (h, w, 3) and cnt.shape == (h, w, 3)
    # where the trail lands in frame 0's coordinates, and where all eight frames cover
    import oracle
    trail = oracle.warp_frame(np.where(marked, 255, 0).astype(np.uint8), warps[3])[..., 0] >= 0.5
    cover = np.ones((h, w), bool)
    for M in warps:
        cover &= oracle.warp_frame(np.full((h, w), 255, np.uint8), M)[..., 0] >= 1.0 - 1e-6
    trail &= cover
    assert trail.sum() > 300

    def rms(e):
        return float(np.sqrt(np.mean(e.astype(np.float64) ** 2)))

    # the robust-clip ground-truth test's criterion: the trail's sample is left out, and what remains on the trail is the
    # stack's own noise — what the combine leaves off the trail (8 samples) scaled to 7, plus 4 standard errors of that RMS
    r_off, r_trail = rms((out - truth)[cover & ~trail]), rms((out - truth)[trail])
    m = int(trail.sum()) * 3
    bound = r_off * np.sqrt(8.0 / 7.0) * (1.0 + 4.0 / np.sqrt(2.0 * m))
    print("RMS error off the trail", r_off, "on the trail", r_trail, "bound", bound)
    assert (cnt[trail] <= 7).all()
    assert r_trail <= bound
    acc = None
    for f, M in zip(frames, warps):
        acc = st.warp_accumulate(f, M, acc=acc)
    assert rms((acc / np.float32(n) - truth)[trail]) > 10 * r_trail         # the plain mean keeps it
    dz = DrizzleParameters(scale=2.0)
    dout = st.drizzle_stack(list(frames), warps, dz, include=include)
    assert tuple(dout.shape) == tuple(dz.out_shape(h, w)) + (3,)
    assert np.isfinite(dout).all()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals(st):
    frames, _ = motion_stack(4)
    ok = list(frames)
    for dt in (np.uint16, np.float32):
        bad = [f.astype(dt) for f in ok]
        for call in (st.star_detect, st.star_align, st.star_match):
            with pytest.raises(NotImplementedYet):
                call(bad)
    for kw in (dict(radius=1), dict(radius=8), dict(kappa=-1.0), dict(kappa=float("nan")), dict(min_contrast=0), dict(min_contrast=256),
               dict(min_pixels=0), dict(min_pixels=82), dict(radius=2, min_pixels=26), dict(max_stars=3), dict(max_stars=1025),
               dict(match_stars=3), dict(match_stars=201), dict(neighbours=1), dict(neighbours=9), dict(tri_tolerance=0.0),
               dict(tri_tolerance=float("inf")), dict(min_votes=0), dict(refine=2), dict(min_stars=3), dict(min_inliers=3),
               dict(method=3), dict(ransac_reproj_threshold=0.0), dict(ransac_reproj_threshold=float("nan"))):
        for call in (st.star_detect, st.star_align, st.star_match):
            with pytest.raises(InvalidParams):
                call(ok, StarParameters(**kw))
    with pytest.raises(InvalidParams):
        st.star_match(ok, StarParameters(border_mode=7))
    for method in (16, 32, 38):                                             # RHO and the USAC family
        with pytest.raises(NotImplementedYet):
            st.star_align(ok, StarParameters(method=method))
    for call in (st.star_align, st.star_match):                             # n < 2 for the stack forms
        with pytest.raises(NotEnoughFiles):
            call(ok[:1])
    assert len(st.star_detect(ok[:1])) == 1                                 # detection takes one frame
    # the context is still usable
    dropped, stats = st.star_align(ok)
    assert dropped == 0 and stats[1]["status"] == 0

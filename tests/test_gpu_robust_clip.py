"""Median / MAD sigma clipping on the GPU: stk_robust_clip_stack, its participation form and the four whole-stack forms
against the numpy restatements of the definition (test_cpu_robust_clip.robust_clip_restate / robust_clip_restate_weighted),
bit for bit. As in test_gpu_quantile.py the samples come from the engine's own single-frame warp
(Stacker.warp_accumulate with the same matrices), the coverage weights from the same warp of an all-ones frame."""
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, MotionType, NotImplementedYet, RobustClipParameters, SigmaClipParameters,
                               Stacker, WeightParameters, synth)
from libstacker_rs_amd.api import INTER_CUBIC, INTER_LINEAR
from test_cpu_robust_clip import robust_clip_restate, robust_clip_restate_weighted
from test_cpu_weighted import LINEAR, estimate
from test_gpu_quantile import _ALPHA, _SCALE, CASES, noisy_frames, samples_of, small_warps
from test_gpu_robust import rim_warps
from test_gpu_weighted import _applied_equal, _dimmed, engine_kappa, engine_samples

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
F = np.float32


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, ref, what=""):
    out, cnt = (_np(v) for v in got)
    assert np.array_equal(cnt, ref[1]), what
    assert np.array_equal(out, ref[0], equal_nan=True), what


# ---- 1. the combine against the restatement, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-N{c[6]}-{c[8][0]}x{c[8][1]}{'-inc' if c[9] else ''}" for c in CASES])
def test_robust_clip_stack_matches_restatement(st, case):
    import torch
    dtype, cn, affine, border, bv, sub, n, _, (h, w), subset = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()) + 2)
    frames = noisy_frames(rng, n + (1 if subset else 0), h, w, cn, dtype)
    warps = small_warps(rng, len(frames), affine)
    include = None
    if subset:
        include = [1] * len(frames)
        include[len(frames) // 2] = 0
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype])
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    params = [RobustClipParameters(2.0, 2.5, floor, T) for T in (1, 3) for floor in (0.0, 0.5 / _SCALE[dtype])]
    st.set_option("warp_subpixel_bits", sub)
    try:
        samples = samples_of(st, frames, warps, include, **kw)
        got = [(st.robust_clip_stack(frames, warps, p, include, return_counts=True, **kw),
                st.robust_clip_stack(dframes, warps, p, include, return_counts=True, **kw),
                st.robust_clip_stack(frames, warps, p, include, **kw)) for p in params]
    finally:
        st.set_option("warp_subpixel_bits", 0)
    rejected = False
    for p, (host, dev, only) in zip(params, got):
        ref = robust_clip_restate(samples, p.kappa_low, p.kappa_high, p.sigma_floor, p.iterations)
        _same(host, ref, ("host", p))
        _same(dev, ref, ("device", p))
        assert np.array_equal(only, ref[0], equal_nan=True), p
        rejected |= bool((ref[1] < n).any())
        assert (ref[1] == n).all() if n < 3 else True
    assert rejected or n < 3                            # the test cannot pass on stacks nothing is rejected from


# the launcher's instantiations (S lanes per pixel-channel, 4G keys per lane), by N:
#   1, 2, 3, 4 -> (1, 1);  5 -> (1, 2);  11 -> (1, 4);  32 -> (1, 8);  33, 64 -> (2, 8);  65 -> (4, 8);  257 -> (16, 8);
#   1024 -> (32, 8);  2049 -> (64, 16)
LARGE_N = [1, 2, 3, 4, 5, 11, 32, 33, 64, 65, 257, 1024, 2049]


@pytest.fixture(scope="module")
def large_stack(st):
    rng = np.random.default_rng(5)
    n, h, w = max(LARGE_N), 6, 21
    frames = noisy_frames(rng, n, h, w, 1, np.uint16)
    warps = small_warps(rng, n, True)
    kw = dict(is_affine=True, border_mode=BORDER_REPLICATE, alpha=_ALPHA[np.uint16])
    return frames, warps, kw, samples_of(st, frames, warps, **kw)


@pytest.mark.parametrize("n", LARGE_N)
def test_every_launcher_instantiation(st, large_stack, n):
    frames, warps, kw, samples = large_stack
    for p in (RobustClipParameters(2.0, 2.0, 0.0, 3), RobustClipParameters(3.0, 2.5, 0.5 / 65535.0, 1)):
        ref = robust_clip_restate(samples[:n], p.kappa_low, p.kappa_high, p.sigma_floor, p.iterations)
        _same(st.robust_clip_stack(frames[:n], warps[:n], p, return_counts=True, **kw), ref, (n, p))
        assert (ref[1] < n).any() or n < 3


def test_band_rows_change_no_bit(st):
    rng = np.random.default_rng(9)
    n, h, w = 11, 37, 53                             # 37 rows: not a multiple of 3
    frames = noisy_frames(rng, n, h, w, 3, np.uint8)
    warps = small_warps(rng, n, False)
    p = RobustClipParameters(2.0, 2.0, 0.5 / 255.0, 2)
    ref = robust_clip_restate(samples_of(st, frames, warps), 2.0, 2.0, 0.5 / 255.0, 2)
    outs = []
    for rows in (1, 3, 0):
        st.set_option("quantile_band_rows", rows)
        try:
            outs.append(st.robust_clip_stack(frames, warps, p, return_counts=True))
        finally:
            st.set_option("quantile_band_rows", 0)
    for o in outs:                                   # every band's rows of the planes reached the last pass
        _same(o, ref)


def test_cubic_fold_matches_restatement(st):
    rng = np.random.default_rng(17)
    n, h, w = 9, 31, 70
    frames = noisy_frames(rng, n, h, w, 3, np.uint8)
    warps = small_warps(rng, n, False)
    p = RobustClipParameters(2.0, 2.5, 0.5 / 255.0, 2)
    st.set_option("warp_interpolation", INTER_CUBIC)
    try:
        samples = samples_of(st, frames, warps)
        got = st.robust_clip_stack(frames, warps, p, return_counts=True)
    finally:
        st.set_option("warp_interpolation", INTER_LINEAR)
    assert not np.array_equal(samples, samples_of(st, frames, warps))
    _same(got, robust_clip_restate(samples, 2.0, 2.5, 0.5 / 255.0, 2))


# ---- 2. the reason for the feature: ground truth, no restatement ---------------------------------------------------------
def test_a_short_stack_loses_its_trail_where_the_plain_clip_keeps_it(st):
    n, h, w = 8, 96, 128
    rng = np.random.default_rng(21)
    clean = (rng.random((h, w, 3)) * 200).astype(np.uint8)
    frames = [clean.copy() for _ in range(n)]
    frames[2][40:43, 10:120] = 255                     # a bright 3-pixel-wide trail in one frame
    frames[5][70, 33] = 255                            # a hot pixel in another
    marked = np.zeros((h, w), bool)
    marked[40:43, 10:120] = True
    marked[70, 33] = True
    warps = [np.eye(3)] * n
    truth = clean.astype(F) * F(1.0 / 255.0)
    out, cnt = st.robust_clip_stack(frames, warps, RobustClipParameters(3.0, 3.0, 0.5 / 255.0, 2), return_counts=True)
    np.testing.assert_array_equal(out, truth)
    assert (cnt[marked] == 7).all() and (cnt[~marked] == 8).all()
    # the plain clip: no sample of 8 is 3 standard deviations from their mean (sqrt(7) = 2.65 at most)
    pout, pcnt = st.clip_stack(frames, warps, SigmaClipParameters(3.0, 3.0, 2), return_counts=True)
    assert (pcnt == 8).all()
    assert np.abs(pout - truth)[40:43, 10:120].min() > 0.02        # (255 - 199) / 8 / 255 at least


def test_a_noisy_short_stack_beats_the_median_and_cleans_the_trail(st):
    n, h, w = 8, 120, 160
    rng = np.random.default_rng(22)
    clean = rng.uniform(0.2, 0.8, (h, w, 3)).astype(F)
    frames = [(clean + rng.normal(0, 0.02, clean.shape)).astype(F) for _ in range(n)]
    trail = np.zeros((h, w), bool)
    trail[50:53, 10:150] = True
    frames[3][trail] += F(0.5)
    warps = [np.eye(3)] * n
    out, cnt = st.robust_clip_stack(frames, warps, RobustClipParameters(3.0, 3.0, 0.0, 2), alpha=1.0, return_counts=True)
    med = st.quantile_stack(frames, warps, 0.5, alpha=1.0)

    def rms(e):
        return float(np.sqrt(np.mean(e.astype(np.float64) ** 2)))

    r_all, r_med = rms(out - clean), rms(med - clean)
    r_off, r_trail = rms((out - clean)[~trail]), rms((out - clean)[trail])
    # the bound on the trail comes from the stack's own noise: what the same combine leaves off the trail (8 samples), scaled
    # to the 7 samples a trail pixel keeps, plus 4 standard errors of an RMS over the trail's values (1 / sqrt(2 m) each)
    m = int(trail.sum()) * 3
    bound = r_off * np.sqrt(8.0 / 7.0) * (1.0 + 4.0 / np.sqrt(2.0 * m))
    print("RMS error: robust clip", r_all, "median", r_med, "| off the trail", r_off, "on the trail", r_trail, "bound", bound)
    assert (cnt[trail] <= 7).all()
    assert r_all < r_med
    assert r_trail <= bound


# ---- 3. whole-stack forms equal their parts --------------------------------------------------------------------------------
def test_ecc_match_robust_clipped_equals_robust_clip_stack_on_its_warps(st):
    frames, _ = synth.make_stack(6, 256, 192, device="cuda")
    p = RobustClipParameters(2.5, 2.5, 0.5 / 255.0, 2)
    out, cnt, stats = st.ecc_match_robust_clipped(frames, ECC, p, return_stats=True, return_counts=True)
    t = st.timing()
    assert t["finalize_ms"] > 0 and 0 < t["robust_select_us"] <= t["finalize_ms"] * 1000.0 + 1
    _, pstats = st.ecc_match(frames, ECC, return_stats=True)
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["rho"] == b["rho"]
        assert np.array_equal(a["warp"], b["warp"])
    ref, rcnt = st.robust_clip_stack(frames, [s["warp"] for s in stats], p, return_counts=True)
    assert np.array_equal(_np(out), _np(ref)) and np.array_equal(_np(cnt), _np(rcnt))
    assert int(_np(cnt).min()) < 6
    # host-fed: the same bits, outputs on the host
    hout, hcnt = st.ecc_match_robust_clipped(frames.cpu().numpy(), ECC, p, return_counts=True)
    assert np.array_equal(hout, _np(out)) and np.array_equal(hcnt, _np(cnt))


def test_keypoint_match_robust_clipped_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 640, 480)
    frames = frames.numpy()
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    p = RobustClipParameters(2.5, 2.5, 0.5 / 255.0, 2)
    dropped, out, cnt, stats = st.keypoint_match_robust_clipped(stack, KP, p, return_stats=True, return_counts=True)
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["n_matches"] == b["n_matches"] and np.array_equal(a["warp"], b["warp"])
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] for s in stats]
    _same(st.robust_clip_stack(stack, warps, p, include, return_counts=True), (out, cnt))
    assert cnt.max() == 4                               # the dropped frame is no sample
    samples = samples_of(st, stack, warps, include)
    assert samples.shape[0] == 4
    _same((out, cnt), robust_clip_restate(samples, 2.5, 2.5, 0.5 / 255.0, 2))


# ---- 4. the participation form --------------------------------------------------------------------------------------------
# (depth, channels, affine, border, border value, subpixel bits, iterations, (h, w))
PCASES = [
    (np.uint8, 3, False, BORDER_CONSTANT, (0.25, 0.5, 0.75, 0), 0, 2, (45, 131)),     # u8 BGR fast kernel
    (np.uint16, 1, True, BORDER_REPLICATE, (0, 0, 0, 0), 5, 1, (30, 61)),
    (np.float32, 4, False, BORDER_CONSTANT, (0.1, 0.2, 0.3, 0.4), 0, 3, (23, 69)),
]


@pytest.mark.parametrize("coverage", [0, 1])
@pytest.mark.parametrize("case", PCASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-T{c[6]}" for c in PCASES])
def test_participation_form_matches_restatement(st, case, coverage):
    import torch
    dtype, cn, affine, border, bv, sub, T, (h, w) = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()) + 3)
    n = 9
    base = rng.random((h, w, cn))
    frames = []
    for _ in range(n):                                  # one scene, noise and outliers: the clip has something to reject
        f = np.clip(base + rng.normal(0, 0.03, base.shape), 0, 1)
        f[rng.random((h, w)) < 0.03] = 1.0
        f = f * _SCALE[dtype]
        frames.append(np.rint(f).astype(dtype) if dtype != np.float32 else f.astype(F))
    warps = rim_warps(rng, n, affine, h)                # every frame 1 .. 6 px right and down: a rim of 0, 1, 2 ... covers
    include = [1] * n
    include[4] = 0
    idx = [i for i in range(n) if include[i]]
    g = rng.uniform(0.9, 1.1, (n, cn)).astype(F)
    o = rng.uniform(-0.02, 0.02, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[2] = 0.0
    p = RobustClipParameters(2.0, 2.5, 0.5 / 255.0, T)      # the samples are in [0, 1] at every depth
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype], coverage=bool(coverage))
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    st.set_option("warp_subpixel_bits", sub)
    try:
        samples = engine_samples(st, frames, warps, idx, is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype])
        kappa = engine_kappa(st, (h, w), warps, idx, affine)
        host = st.robust_clip_stack_weighted(frames, warps, p, g, o, wt, include, return_counts=True, return_kept_weight=True, **kw)
        dev = st.robust_clip_stack_weighted(dframes, warps, p, g, o, wt, include, return_counts=True, return_kept_weight=True, **kw)
        st.set_option("quantile_band_rows", 3)
        only = st.robust_clip_stack_weighted(frames, warps, p, g, o, wt, include, **kw)
    finally:
        st.set_option("warp_subpixel_bits", 0)
        st.set_option("quantile_band_rows", 0)
    full = kappa == F(1.0)
    live = np.array([wt[i] > 0 for i in idx])
    n_cov = (full & live[:, None, None]).sum(axis=0)
    assert (n_cov == 0).any() and ((n_cov >= 1) & (n_cov <= 2)).any() and (n_cov >= 3).any()
    part = full if coverage else np.ones_like(full)
    ref, ref_k, ref_sw = robust_clip_restate_weighted(samples, part, g[idx], o[idx], wt[idx], 2.0, 2.5, p.sigma_floor, T)
    for got in (host, dev):
        out, cnt, kept = (_np(v) for v in got)
        assert np.array_equal(cnt, ref_k) and np.array_equal(kept, ref_sw)
        assert np.array_equal(out, ref, equal_nan=True)
    assert np.array_equal(only, ref, equal_nan=True)
    n_part = n_cov if coverage else np.full_like(n_cov, live.sum())
    assert (ref_k < n_part[..., None]).any()            # something was rejected
    if coverage:                                        # a pixel nobody covers: 0 / 0 / 0
        none = n_cov == 0
        assert (ref[none] == 0).all() and (ref_k[none] == 0).all() and (ref_sw[none] == 0).all()


def test_unit_records_give_the_plain_form(st):
    frames, _ = synth.make_stack(8, 320, 240)
    frames = frames.numpy()
    _, stats = st.ecc_match(frames, ECC, return_stats=True)
    warps = [s["warp"] for s in stats]
    p = RobustClipParameters(2.0, 2.5, 0.5 / 255.0, 2)
    a, ak, aw = st.robust_clip_stack_weighted(frames, warps, p, coverage=False, return_counts=True, return_kept_weight=True)
    b, bk = st.robust_clip_stack(frames, warps, p, return_counts=True)
    assert np.array_equal(a, b) and np.array_equal(ak, bk) and np.array_equal(aw, bk.astype(F))
    assert (bk < 8).any()
    # coverage = 1 puts no condition on the border mode or value: a border tap never reaches a participating sample
    c1 = st.robust_clip_stack_weighted(frames, warps, p, coverage=True, return_counts=True)
    c2 = st.robust_clip_stack_weighted(frames, warps, p, coverage=True, border_mode=BORDER_REPLICATE, return_counts=True)
    c3 = st.robust_clip_stack_weighted(frames, warps, p, coverage=True, border_value=(0.5, 0.5, 0.5, 0), return_counts=True)
    assert np.array_equal(c1[1], c2[1]) and np.array_equal(c1[0], c2[0])
    assert np.array_equal(c1[1], c3[1]) and np.array_equal(c1[0], c3[0])
    assert (c1[1] < ak).any()


def test_weighted_whole_stack_forms_equal_their_parts(st):
    import torch
    frames, _ = synth.make_stack(6, 256, 192)
    host = _dimmed(frames.numpy(), [1.0, 0.8, 0.9, 1.0, 0.7, 0.85])
    dev = torch.from_numpy(host).cuda()
    weights = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0]
    wp = WeightParameters(LINEAR, True, 0)
    p = RobustClipParameters(2.5, 2.5, 0.5 / 255.0, 2)
    out, cnt, kept, applied, stats = st.ecc_match_robust_clipped_weighted(dev, ECC, p, wp, weights, return_stats=True, return_counts=True,
                                                                         return_kept_weight=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and np.array_equal(a["warp"], b["warp"])
    warps = [s["warp"] for s in stats]
    g, o, fb = estimate(st.overlap_moments(dev, warps, stat_step=4), LINEAR)
    g[0], o[0], fb[0] = 1, 0, False
    _applied_equal(applied, g, o, fb, weights)
    ref, rk, rw = st.robust_clip_stack_weighted(dev, warps, p, applied=applied, coverage=True, return_counts=True, return_kept_weight=True)
    assert np.array_equal(_np(out), _np(ref)) and np.array_equal(_np(cnt), _np(rk)) and np.array_equal(_np(kept), _np(rw))
    assert int(_np(cnt).max()) == 5 and int(_np(cnt).min()) < 5                 # frame 3 has weight 0
    hout, hcnt, hkept = st.ecc_match_robust_clipped_weighted(host, ECC, p, wp, weights, return_counts=True, return_kept_weight=True)
    assert np.array_equal(hout, _np(out)) and np.array_equal(hcnt, _np(cnt)) and np.array_equal(hkept, _np(kept))


def test_weighted_keypoint_form_equals_its_parts(st):
    frames, _ = synth.make_stack(4, 640, 480)
    frames = _dimmed(frames.numpy(), [1.0, 0.8, 0.9, 0.75])
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    weights = [1.0, 2.0, 3.0, 0.5, 1.0]
    wp = WeightParameters(LINEAR, True, 2)
    p = RobustClipParameters(2.5, 2.5, 0.5 / 255.0, 1)
    dropped, out, cnt, kept, applied, stats = st.keypoint_match_robust_clipped_weighted(stack, KP, p, wp, weights, return_stats=True,
                                                                                        return_counts=True, return_kept_weight=True,
                                                                                        return_applied=True)
    assert dropped == 1 and stats[2]["status"] == 1 and applied[2]["weight"] == 0
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    ref, rk, rw = st.robust_clip_stack_weighted(stack, warps, p, applied=applied, include=include, coverage=True, return_counts=True,
                                                return_kept_weight=True)
    assert np.array_equal(out, ref) and np.array_equal(cnt, rk) and np.array_equal(kept, rw)
    assert cnt.max() == 4 and kept.max() == F(1.0 + 2.0 + 0.5 + 1.0)


# ---- 5. infinities and NaNs ---------------------------------------------------------------------------------------------
def test_infinities_and_nans(st):
    rng = np.random.default_rng(13)
    n, h, w = 11, 20, 40
    frames = noisy_frames(rng, n, h, w, 3, np.float32)
    # identity warps go through the classic 4-weight path below (weights 1, 0, 0, 0): a planted inf stays an inf sample
    # there, and is NaN (0 * inf) at the pixels that have it as a zero-weight tap (test_gpu_quantile). So the infs sit on
    # the lattice of even rows and columns, whose forward neighbours are never planted
    yy, xx = np.mgrid[0:h, 0:w]
    lattice = ((yy % 2 == 0) & (xx % 2 == 0))[..., None]
    rows = lambda lo, hi: lattice & ((yy >= lo) & (yy < hi))[..., None]
    one = rows(5, 12) & (rng.random((h, w, 3)) < 0.7)   # rows 5 .. 11: one inf per pixel-channel among 11
    which = rng.integers(0, n, (h, w, 3))
    sign = np.where(rng.random((h, w, 3)) < 0.5, np.inf, -np.inf).astype(F)
    for i in range(n):
        sel = one & (which == i)
        frames[i][sel] = sign[sel]
    for i in range(6):
        frames[i][np.broadcast_to(rows(0, 4), (h, w, 3))] = np.inf          # rows 0 .. 3: a majority of +inf
    for i in range(3):
        frames[i][np.broadcast_to(rows(14, 16), (h, w, 3))] = -np.inf       # row 14: three -inf among 11 (a minority)
    frames[9][rng.integers(17, h, 20), rng.integers(0, w, 20), rng.integers(0, 3, 20)] = np.nan
    warps = [np.eye(3)] * n
    st.set_option("warp_subpixel_bits", 5)
    try:
        samples = samples_of(st, frames, warps, alpha=1.0)
        got = {(T, fl): st.robust_clip_stack(frames, warps, RobustClipParameters(3.0, 3.0, fl, T), alpha=1.0, return_counts=True)
               for T in (1, 3) for fl in (0.0, 0.01)}
    finally:
        st.set_option("warp_subpixel_bits", 0)
    nan = np.isnan(samples).any(axis=0)
    ninf = np.isinf(samples).sum(axis=0)
    assert nan.any() and (ninf == 1).any() and (ninf == 6).any() and (ninf == 3).any()
    for (T, fl), g in got.items():
        _same(g, robust_clip_restate(samples, 3.0, 3.0, fl, T), (T, fl))       # NaN positions included
        out, cnt = g
        assert np.isnan(out[nan]).all()
        lone = (ninf == 1) & ~nan
        assert np.isfinite(out[lone]).all() and (cnt[lone] <= n - 1).all()      # one inf hot pixel is rejected
        few = (ninf == 3) & ~nan
        assert np.isfinite(out[few]).all() and (cnt[few] <= n - 3).all()
        assert np.isnan(out[(ninf == 6) & ~nan]).all()                          # an infinite median: NaN


# ---- 6. errors ------------------------------------------------------------------------------------------------------------
def test_invalid_parameters_are_rejected(st):
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    I = [np.eye(3)] * 3
    inf, nan = float("inf"), float("nan")
    bad = [RobustClipParameters(0.0, 3.0), RobustClipParameters(3.0, -1.0), RobustClipParameters(inf, 3.0), RobustClipParameters(3.0, nan),
           RobustClipParameters(3.0, 3.0, -1e-6), RobustClipParameters(3.0, 3.0, nan), RobustClipParameters(3.0, 3.0, 0.0, 0),
           RobustClipParameters(3.0, 3.0, 0.0, 17)]
    for p in bad:
        for call in (lambda: st.robust_clip_stack(frames, I, p), lambda: st.robust_clip_stack_weighted(frames, I, p),
                     lambda: st.ecc_match_robust_clipped(frames, ECC, p), lambda: st.keypoint_match_robust_clipped(frames, KP, p),
                     lambda: st.ecc_match_robust_clipped_weighted(frames, ECC, p),
                     lambda: st.keypoint_match_robust_clipped_weighted(frames, KP, p)):
            with pytest.raises(InvalidParams, match="robust clipping"):
                call()
    st.robust_clip_stack(frames, I, RobustClipParameters(3.0, 3.0, 0.0, 16))    # sigma_floor = 0 and 16 rounds are allowed
    with pytest.raises(InvalidParams, match="no frame"):
        st.robust_clip_stack(frames, I, include=[0, 0, 0])
    with pytest.raises(NotImplementedYet):
        st.robust_clip_stack(frames, I, border_mode=5)                          # BORDER_TRANSPARENT
    with pytest.raises(InvalidParams, match="weight"):
        st.robust_clip_stack_weighted(frames, I, weights=[1, -1, 1])


def test_strided_output_and_null_parameters_are_rejected(st):
    import ctypes as C
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    frames, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(frames.numpy())
    ep, kp, cp, wp = ECC._c(), KP._c(), RobustClipParameters()._c(), WeightParameters()._c()
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    rec = (_ffi.FrameWeight * 3)()
    for r in rec:
        r.gain[:] = [1, 1, 1, 1]
        r.weight = 1.0
    out = np.empty((96, 128, 3), F)
    img = _ffi.ImageF32(out.ctypes.data, 128, 96, 3, HOST, 0)
    wide = np.empty((96, 160, 3), F)
    loose = _ffi.ImageF32(wide.ctypes.data, 128, 96, 3, HOST, 160 * 3 * 4)
    lib, h, fr, a = st._lib, st._h, C.byref(m.c_frames), 1.0 / 255
    dropped = C.c_int32(0)

    def calls(cpp, im):
        return [lib.stk_robust_clip_stack(h, fr, Mp, None, 0, 0, None, a, cpp, im, None),
                lib.stk_robust_clip_stack_weighted(h, fr, Mp, None, 0, 0, None, a, cpp, rec, 1, im, None, None),
                lib.stk_ecc_match_robust_clipped(h, fr, C.byref(ep), 0.0, cpp, im, None, None),
                lib.stk_keypoint_match_robust_clipped(h, fr, C.byref(kp), 0.0, cpp, im, C.byref(dropped), None, None),
                lib.stk_ecc_match_robust_clipped_weighted(h, fr, C.byref(ep), 0.0, cpp, C.byref(wp), None, im, None, None, None, None),
                lib.stk_keypoint_match_robust_clipped_weighted(h, fr, C.byref(kp), 0.0, cpp, C.byref(wp), None, im, C.byref(dropped), None,
                                                               None, None, None)]

    assert calls(C.byref(cp), C.byref(loose)) == [2] * 6                        # STK_INVALID_PARAMS
    assert b"tightly" in lib.stk_last_error(h)
    assert calls(None, C.byref(img)) == [2] * 6
    assert b"robust clip" in lib.stk_last_error(h)
    assert calls(C.byref(cp), C.byref(img))[:2] == [0, 0]                       # and the good calls


def test_too_many_samples(st):
    n = 4097
    frames = np.zeros((n, 2, 4, 3), np.uint8)
    with pytest.raises(NotImplementedYet, match="4096"):
        st.robust_clip_stack(frames, [np.eye(3)] * n)
    with pytest.raises(NotImplementedYet, match="4096"):
        st.robust_clip_stack_weighted(frames, [np.eye(3)] * n)


# ---- 7. stability -----------------------------------------------------------------------------------------------------------
def test_options_and_repetition_change_no_bit(st):
    frames, _ = synth.make_stack(12, 320, 240, device="cuda")
    p = RobustClipParameters(2.5, 2.5, 0.5 / 255.0, 2)
    base, bcnt = (_np(v) for v in st.ecc_match_robust_clipped(frames, ECC, p, return_counts=True))
    again, acnt = (_np(v) for v in st.ecc_match_robust_clipped(frames, ECC, p, return_counts=True))
    assert np.array_equal(again, base) and np.array_equal(acnt, bcnt)
    for name, val, back in (("ecc_slots", 4, 0), ("quantile_band_rows", 7, 0)):
        st.set_option(name, val)
        try:
            o = st.ecc_match_robust_clipped(frames, ECC, p)
        finally:
            st.set_option(name, back)
        assert np.array_equal(_np(o), base), name
    kres = []
    for lanes in (1, 3):
        st.set_option("kp_lanes", lanes)
        try:
            kres.append(st.keypoint_match_robust_clipped(frames, KP, p))
        finally:
            st.set_option("kp_lanes", 3)
    assert kres[0][0] == kres[1][0] and np.array_equal(_np(kres[0][1]), _np(kres[1][1]))
    multi = Stacker(devices=[0, 0])                   # a multi-device context runs these calls on its first device
    try:
        mo = multi.ecc_match_robust_clipped(frames, ECC, p)
    finally:
        multi.close()
    assert np.array_equal(_np(mo), base)

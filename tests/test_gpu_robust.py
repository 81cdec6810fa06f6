"""Normalised, coverage-aware sigma-clip and quantile stacking on the GPU: stk_clip_stack_weighted /
stk_quantile_stack_weighted and the four whole-stack forms against the numpy restatements of the definition
(test_cpu_robust.robust_clip_restate / robust_quantile_restate). As in test_gpu_weighted.py the samples come from the
engine's own single-frame warp and the coverage weights kappa from the same warp of an all-ones f32 frame."""
import ctypes as C
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, MotionType, NotImplementedYet, SigmaClipParameters, Stacker,
                               WeightParameters, synth)
from test_cpu_robust import dyadic_stack, robust_clip_restate, robust_quantile_restate
from test_cpu_weighted import LINEAR, NONE, OFFSET, estimate
from test_gpu_clip import CASES
from test_gpu_weighted import _ALPHA, _applied_equal, _dimmed, engine_kappa, engine_samples, random_frames, shifted_warps

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
F = np.float32


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def rim_warps(rng, n, affine, h):
    """shifted_warps with every frame moved right and down by 1 .. 6 px, so that the first rows and columns are covered by
    none, one, two ... of the frames. A one-row frame is covered only where y maps onto the row exactly: translations along
    x alone."""
    Ms = shifted_warps(rng, n, affine)
    for M in Ms:
        M[:2, 2] = rng.uniform(1.0, 6.0, 2)
        if h == 1:
            M[:] = np.eye(3)
            M[0, 2] = rng.uniform(1.0, 6.0)
    return Ms


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ---- 6. the two combines against the restatements, bit for bit ----------------------------------------------------
@pytest.mark.parametrize("coverage", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-T{c[6]}-{c[8][0]}x{c[8][1]}" for c in CASES])
def test_robust_stacks_match_restatement(st, case, coverage):
    import torch
    dtype, cn, affine, border, bv, sub, T, (kl, kh), (h, w) = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()) + 1)
    n = 9
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = rim_warps(rng, n, affine, h)
    include = [1] * n
    include[4] = 0
    idx = [i for i in range(n) if include[i]]
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[2] = 0.0
    clip = SigmaClipParameters(kl, kh, T)
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype])
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    qs = (0.5, 0.3)
    got = {}
    st.set_option("warp_subpixel_bits", sub)
    try:
        samples = engine_samples(st, frames, warps, idx, **kw)
        kappa = engine_kappa(st, (h, w), warps, idx, affine)
        cov = dict(coverage=bool(coverage), **kw)
        got["clip"] = st.clip_stack_weighted(frames, warps, clip, g, o, wt, include, return_counts=True, return_kept_weight=True, **cov)
        got["dclip"] = st.clip_stack_weighted(dframes, warps, clip, g, o, wt, include, return_counts=True, return_kept_weight=True, **cov)
        got["only"] = st.clip_stack_weighted(frames, warps, clip, g, o, wt, include, **cov)
        for q in qs:
            for rows in (0, 1, 3):
                st.set_option("quantile_band_rows", rows)
                got["q", q, rows] = st.quantile_stack_weighted(frames, warps, q, g, o, wt, include, return_counts=True, **cov)
            st.set_option("quantile_band_rows", 0)
            got["dq", q] = st.quantile_stack_weighted(dframes, warps, q, g, o, wt, include, return_counts=True, **cov)
            got["qonly", q] = st.quantile_stack_weighted(frames, warps, q, g, o, wt, include, **cov)
    finally:
        st.set_option("warp_subpixel_bits", 0)
        st.set_option("quantile_band_rows", 0)
    full = kappa == F(1.0)
    # conditions on the inputs: the test cannot pass on interiors alone
    assert (~full).mean() >= 0.03, (~full).mean()
    live = np.array([wt[i] > 0 for i in idx])
    n_cov = (full & live[:, None, None]).sum(axis=0)
    assert (n_cov == 0).any() and ((n_cov >= 1) & (n_cov <= 2)).any() and (n_cov >= 3).any()
    part = full if coverage else np.ones_like(full)
    ref, ref_k, ref_sw = robust_clip_restate(samples, part, g[idx], o[idx], wt[idx], kl, kh, T)
    for key in ("clip", "dclip"):
        out, cnt, kept = (_np(v) for v in got[key])
        assert np.array_equal(cnt, ref_k), key
        assert np.array_equal(kept, ref_sw), key
        assert np.array_equal(out, ref, equal_nan=True), key
    assert np.array_equal(got["only"], ref, equal_nan=True)
    if coverage:
        assert (ref_k == 0).any() and (ref_k >= 3).any()
    for q in qs:
        qref, qn = robust_quantile_restate(samples, part, g[idx], o[idx], wt[idx], q)
        assert np.array_equal(qn, n_cov if coverage else np.full_like(n_cov, live.sum()))
        for key in [("q", q, rows) for rows in (0, 1, 3)] + [("dq", q)]:
            out, cnt = (_np(v) for v in got[key])
            assert np.array_equal(cnt, qn), key
            assert np.array_equal(out, qref, equal_nan=True), key
        assert np.array_equal(got["qonly", q], qref, equal_nan=True)


def test_nan_infinite_and_mark_like_samples(st):
    """A float stack with NaN, +-inf and the NaN bit patterns the band uses as marks (all ones, and signalling NaNs) among
    its pixels: a genuine NaN of any payload is a sample, never an absent entry."""
    rng = np.random.default_rng(21)
    n, h, w = 7, 24, 40
    frames = random_frames(rng, n, h, w, 3, F)
    bits = [0x7fc00000, 0xffffffff, 0x7fa00000, 0xffa00000, 0x7f800001, 0x7f800000, 0xff800000]     # NaNs, then +inf, -inf
    for i, bpat in enumerate(bits):
        ys, xs = rng.integers(6, h - 1, 12), rng.integers(6, w - 1, 12)
        frames[i].view(np.uint32)[ys, xs, i % 3] = bpat
    warps = rim_warps(rng, n, True, h)
    g = rng.uniform(0.5, 2.0, (n, 3)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, 3)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    idx = list(range(n))
    kw = dict(is_affine=True, alpha=1.0)
    samples = engine_samples(st, frames, warps, idx, **kw)
    kappa = engine_kappa(st, (h, w), warps, idx, True)
    assert np.isnan(samples).any() and np.isinf(samples).any()
    for coverage in (0, 1):
        part = kappa == F(1.0) if coverage else np.ones_like(kappa, bool)
        for q in (0.5, 0.3, 1.0):
            ref, rn = robust_quantile_restate(samples, part, g, o, wt, q)
            out, cnt = st.quantile_stack_weighted(frames, warps, q, g, o, wt, coverage=bool(coverage), return_counts=True, **kw)
            assert np.array_equal(cnt, rn) and np.array_equal(out, ref, equal_nan=True), (coverage, q)
            assert np.isnan(ref).any() and (rn[np.isnan(ref).any(axis=-1)] > 0).all()
        clip = SigmaClipParameters(2.0, 2.5, 2)
        ref, rk, rsw = robust_clip_restate(samples, part, g, o, wt, 2.0, 2.5, 2)
        out, cnt, kept = st.clip_stack_weighted(frames, warps, clip, g, o, wt, coverage=bool(coverage), return_counts=True,
                                                return_kept_weight=True, **kw)
        assert np.array_equal(cnt, rk) and np.array_equal(kept, rsw, equal_nan=True) and np.array_equal(out, ref, equal_nan=True)
        assert np.isnan(ref).any() and not np.isnan(ref).all()


# ---- 7. rim ground truth on the engine, independent of the restatement ------------------------------------------------
def test_coverage_restores_a_constant_scene_on_the_rim(st):
    rng = np.random.default_rng(11)
    n, h, w = 9, 48, 80
    frames = [np.full((h, w, 3), 153, np.uint8) for _ in range(n)]
    v = F(153) * F(1.0 / 255.0)
    warps = []
    for _ in range(n):
        M = np.eye(3)
        M[:2, 2] = rng.uniform(1.0, 6.0, 2)
        warps.append(M)
    clip = SigmaClipParameters(2.0, 2.0, 2)
    out, cnt = st.clip_stack_weighted(frames, warps, clip, coverage=True, return_counts=True)
    assert (cnt == 0).any() and ((cnt > 0) & (cnt < n)).any() and (cnt == n).any()
    assert (out[cnt > 0] == v).all() and (out[cnt == 0] == 0).all()
    med, n_p = st.quantile_stack_weighted(frames, warps, 0.5, coverage=True, return_counts=True)
    assert np.array_equal(n_p, cnt[..., 0])
    assert (med[n_p > 0] == v).all() and (med[n_p == 0] == 0).all()
    # the defect: the plain rejection combines take the border value for a sample
    covered = n_p > 0
    plain_clip = st.clip_stack(frames, warps, clip)
    plain_med = st.quantile_stack(frames, warps, 0.5)
    assert plain_clip[covered].min() < 0.9 * v and plain_med[covered].min() < 0.9 * v


# ---- 8. dyadic ground truth through the engine, at integer shifts ----------------------------------------------------
def test_normalisation_lets_the_clip_see_a_faint_trail(st):
    n, t, h, w = 12, 5, 24, 40
    rng = np.random.default_rng(8)
    big = (rng.integers(256, 769, (h + 12, w + 12, 1)) * 2.0 ** -10).astype(F)
    _, b, trail, mask = dyadic_stack(n, h, w, t)                   # the offsets and the trail (inside every frame's cover)
    shifts = [(0, 0)] + [tuple(int(v) for v in rng.integers(-6, 7, 2)) for _ in range(1, n)]
    scene = big[6:6 + h, 6:6 + w]
    frames, warps = [], []
    for i, (ox, oy) in enumerate(shifts):
        f = (big[6 + oy:6 + oy + h, 6 + ox:6 + ox + w] + b[i]).astype(F)
        if i == t:
            ys, xs = np.nonzero(mask)                              # the trail at frame 0's pixels `mask`
            f[ys - oy, xs - ox] += trail
        frames.append(f)
        M = np.eye(3)
        M[:2, 2] = (ox, oy)
        warps.append(M)
    clip = SigmaClipParameters(2.0, 2.0, 2)
    g = np.ones((n, 1), F)
    kw = dict(coverage=True, alpha=1.0)
    out, cnt, kept = st.clip_stack_weighted(frames, warps, clip, g, -b.reshape(n, 1), return_counts=True, return_kept_weight=True, **kw)
    assert (cnt > 0).all() and (cnt < n).any()
    assert np.array_equal(out, scene)
    assert (cnt[mask] == n - 1).all() and np.array_equal(kept, cnt.astype(F))
    med, n_p = st.quantile_stack_weighted(frames, warps, 0.5, g, -b.reshape(n, 1), return_counts=True, **kw)
    assert np.array_equal(med, scene) and (n_p[mask] == n).all() and np.array_equal(n_p[~mask], cnt[..., 0][~mask])
    raw, rk = st.clip_stack_weighted(frames, warps, clip, return_counts=True, **kw)
    assert (rk[mask] == n).all()
    assert np.abs(raw - scene)[mask].max() > 1e-3


# ---- 9. all weights 1, no normalisation, no coverage: the plain combines' samples ------------------------------------
def test_unit_records_give_the_plain_quantile_and_nearly_the_plain_clip(st):
    frames, _ = synth.make_stack(8, 320, 240)
    frames = frames.numpy()
    _, stats = st.ecc_match(frames, ECC, return_stats=True)
    warps = [s["warp"] for s in stats]
    for q in (0.5, 0.3):
        a = st.quantile_stack_weighted(frames, warps, q, coverage=False)
        assert np.array_equal(a, st.quantile_stack(frames, warps, q))
    clip = SigmaClipParameters(2.0, 2.5, 2)
    a, ak = st.clip_stack_weighted(frames, warps, clip, coverage=False, return_counts=True)
    p, pk = st.clip_stack(frames, warps, clip, return_counts=True)
    print("weighted clip with unit records against clip_stack: counts equal on", (ak == pk).mean(), "of the pixels, largest difference",
          np.abs(a - p).max())


# ---- 10. whole-stack forms equal their parts --------------------------------------------------------------------------
def _same_stats(stats, pstats):
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["rho"] == b["rho"]
        assert a["n_matches"] == b["n_matches"] and np.array_equal(a["warp"], b["warp"])


@pytest.mark.parametrize("mode,step", [(LINEAR, 0), (OFFSET, 3), (NONE, 0)])
def test_ecc_forms_equal_their_parts(st, mode, step):
    import torch
    frames, _ = synth.make_stack(6, 256, 192)
    host = _dimmed(frames.numpy(), [1.0, 0.8, 0.9, 1.0, 0.7, 0.85])
    dev = torch.from_numpy(host).cuda()
    weights = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0]
    wp = WeightParameters(mode, True, step)
    clip = SigmaClipParameters(2.0, 2.5, 2)
    out, cnt, kept, applied, stats = st.ecc_match_clipped_weighted(dev, ECC, clip, wp, weights, return_stats=True, return_counts=True,
                                                                  return_kept_weight=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    qout, qcnt, qapplied, qstats = st.ecc_match_quantile_weighted(dev, ECC, 0.5, wp, weights, return_stats=True, return_counts=True,
                                                                  return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    plain, pstats = st.ecc_match(dev, ECC, return_stats=True)
    _same_stats(stats, pstats)
    _same_stats(qstats, pstats)
    warps = [s["warp"] for s in stats]
    mom = st.overlap_moments(dev, warps, stat_step=step or 4)
    g, o, fb = estimate(mom, mode)
    g[0], o[0], fb[0] = 1, 0, False
    _applied_equal(applied, g, o, fb, weights)
    _applied_equal(qapplied, g, o, fb, weights)
    wapplied = st.ecc_match_weighted(dev, ECC, wp, weights, return_applied=True)[1]
    for a, b in zip(applied, wapplied):
        assert np.array_equal(a["gain"], b["gain"]) and np.array_equal(a["offset"], b["offset"]) and a["weight"] == b["weight"] and a["flags"] == b["flags"]
    ref, rk, rw = st.clip_stack_weighted(dev, warps, clip, applied=applied, coverage=True, return_counts=True, return_kept_weight=True)
    assert np.array_equal(_np(out), _np(ref)) and np.array_equal(_np(cnt), _np(rk)) and np.array_equal(_np(kept), _np(rw))
    qref, qrk = st.quantile_stack_weighted(dev, warps, 0.5, applied=applied, coverage=True, return_counts=True)
    assert np.array_equal(_np(qout), _np(qref)) and np.array_equal(_np(qcnt), _np(qrk))
    assert int(_np(qcnt).max()) == 5 and int(_np(qcnt).min()) < 5               # frame 3 has weight 0; the rim is covered by fewer
    # host-fed: the same bits, outputs on the host
    hout, hcnt, hkept = st.ecc_match_clipped_weighted(host, ECC, clip, wp, weights, return_counts=True, return_kept_weight=True)
    assert np.array_equal(hout, _np(out)) and np.array_equal(hcnt, _np(cnt)) and np.array_equal(hkept, _np(kept))
    hq, hqc = st.ecc_match_quantile_weighted(host, ECC, 0.5, wp, weights, return_counts=True)
    assert np.array_equal(hq, _np(qout)) and np.array_equal(hqc, _np(qcnt))
    if mode != LINEAR:
        return
    # options change no bit; a two-"device" context runs on device 0
    for name, val, back in (("ecc_slots", 4, 0), ("prep_overlap", 0, 1), ("kp_lanes", 1, 3)):
        st.set_option(name, val)
        try:
            o2 = st.ecc_match_clipped_weighted(dev, ECC, clip, wp, weights)
            q2 = st.ecc_match_quantile_weighted(dev, ECC, 0.5, wp, weights)
        finally:
            st.set_option(name, back)
        assert np.array_equal(_np(o2), _np(out)) and np.array_equal(_np(q2), _np(qout)), name
    multi = Stacker(devices=[0, 0])
    try:
        mo = multi.ecc_match_clipped_weighted(dev, ECC, clip, wp, weights)
        mq = multi.ecc_match_quantile_weighted(dev, ECC, 0.5, wp, weights)
    finally:
        multi.close()
    assert np.array_equal(_np(mo), _np(out)) and np.array_equal(_np(mq), _np(qout))


def test_keypoint_forms_with_a_dropped_frame(st):
    import torch
    frames, _ = synth.make_stack(4, 640, 480)
    frames = _dimmed(frames.numpy(), [1.0, 0.8, 0.9, 0.75])
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    weights = [1.0, 2.0, 3.0, 0.5, 1.0]
    wp = WeightParameters(LINEAR, True, 2)
    clip = SigmaClipParameters(2.0, 2.0, 1)
    dropped, out, cnt, kept, applied, stats = st.keypoint_match_clipped_weighted(stack, KP, clip, wp, weights, return_stats=True,
                                                                                 return_counts=True, return_kept_weight=True,
                                                                                 return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    qd, qout, qcnt, qapplied, qstats = st.keypoint_match_quantile_weighted(stack, KP, 0.5, wp, weights, return_stats=True,
                                                                            return_counts=True, return_applied=True)
    pd, plain, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == qd == pd == 1 and stats[2]["status"] == 1
    _same_stats(stats, pstats)
    _same_stats(qstats, pstats)
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    mom = st.overlap_moments(stack, warps, include, stat_step=2)
    g, o, fb = estimate(mom, LINEAR)
    g[0], o[0], fb[0] = 1, 0, False
    g[2], o[2], fb[2] = 1, 0, False                     # the dropped frame: weight 0, gains 1, not a sample
    w_applied = list(weights)
    w_applied[2] = 0.0
    _applied_equal(applied, g, o, fb, w_applied)
    _applied_equal(qapplied, g, o, fb, w_applied)
    wapplied = st.keypoint_match_weighted(stack, KP, wp, weights, return_applied=True)[2]
    for a, b in zip(applied, wapplied):
        assert np.array_equal(a["gain"], b["gain"]) and np.array_equal(a["offset"], b["offset"]) and a["weight"] == b["weight"]
    ref, rk, rw = st.clip_stack_weighted(stack, warps, clip, applied=applied, include=include, coverage=True, return_counts=True,
                                         return_kept_weight=True)
    assert np.array_equal(out, ref) and np.array_equal(cnt, rk) and np.array_equal(kept, rw)
    assert cnt.max() == 4 and kept.max() == F(1.0 + 2.0 + 0.5 + 1.0)
    qref, qrk = st.quantile_stack_weighted(stack, warps, 0.5, applied=applied, include=include, coverage=True, return_counts=True)
    assert np.array_equal(qout, qref) and np.array_equal(qcnt, qrk) and qcnt.max() == 4
    dstack = torch.from_numpy(np.stack(stack)).cuda()
    for lanes in (1, 3):
        st.set_option("kp_lanes", lanes)
        try:
            dd, dout = st.keypoint_match_clipped_weighted(dstack, KP, clip, wp, weights)
            dq, dqout = st.keypoint_match_quantile_weighted(dstack, KP, 0.5, wp, weights)
        finally:
            st.set_option("kp_lanes", 3)
        assert dd == dq == 1 and np.array_equal(_np(dout), out) and np.array_equal(_np(dqout), qout)
    # coverage = 1 puts no condition on the border mode
    st.keypoint_match_clipped_weighted(stack, KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9, BORDER_REPLICATE), clip, wp, weights)


# ---- 11. errors, and the other calls are left alone -----------------------------------------------------------------
def test_invalid_arguments_are_rejected(st):
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    I = [np.eye(3)] * 3
    for wts in ([1, -1, 1], [1, float("nan"), 1], [1, float("inf"), 1], [0, 0, 0]):
        with pytest.raises(InvalidParams, match="weight"):
            st.clip_stack_weighted(frames, I, weights=wts)
        with pytest.raises(InvalidParams, match="weight"):
            st.quantile_stack_weighted(frames, I, weights=wts)
    with pytest.raises(InvalidParams, match="weight"):
        st.clip_stack_weighted(frames, I, weights=[0, 5, 0], include=[1, 0, 1])      # every INCLUDED weight is 0
    with pytest.raises(InvalidParams, match="finite"):
        st.clip_stack_weighted(frames, I, gain=np.full((3, 3), np.inf))
    with pytest.raises(InvalidParams, match="finite"):
        st.quantile_stack_weighted(frames, I, offset=np.full((3, 3), np.nan))
    with pytest.raises(InvalidParams, match="no frame"):
        st.clip_stack_weighted(frames, I, include=[0, 0, 0])
    # coverage = 1 with any border mode or value
    st.clip_stack_weighted(frames, I, coverage=True, border_mode=BORDER_REPLICATE)
    st.quantile_stack_weighted(frames, I, coverage=True, border_value=(0, 0.5, 0, 0))
    with pytest.raises(NotImplementedYet):
        st.clip_stack_weighted(frames, I, border_mode=5)                             # BORDER_TRANSPARENT
    with pytest.raises(InvalidParams):
        st.quantile_stack_weighted(frames, I, border_mode=6)
    for clip in (SigmaClipParameters(0.0, 3.0, 2), SigmaClipParameters(3.0, float("inf"), 2), SigmaClipParameters(3.0, 3.0, 0),
                 SigmaClipParameters(3.0, 3.0, 17)):
        with pytest.raises(InvalidParams, match="sigma clipping"):
            st.clip_stack_weighted(frames, I, clip)
        with pytest.raises(InvalidParams, match="sigma clipping"):
            st.ecc_match_clipped_weighted(frames, ECC, clip)
        with pytest.raises(InvalidParams, match="sigma clipping"):
            st.keypoint_match_clipped_weighted(frames, KP, clip)
    for q in (-0.1, 1.5, float("nan")):
        with pytest.raises(InvalidParams, match="quantile"):
            st.quantile_stack_weighted(frames, I, q)
        with pytest.raises(InvalidParams, match="quantile"):
            st.ecc_match_quantile_weighted(frames, ECC, q)
        with pytest.raises(InvalidParams, match="quantile"):
            st.keypoint_match_quantile_weighted(frames, KP, q)
    for wp in (WeightParameters(4), WeightParameters(-1), WeightParameters(LINEAR, True, 65), WeightParameters(NONE, 2)):
        for call in (st.ecc_match_clipped_weighted, st.ecc_match_quantile_weighted):
            with pytest.raises(InvalidParams, match="weighted"):
                call(frames, ECC, None, wp)
        for call in (st.keypoint_match_clipped_weighted, st.keypoint_match_quantile_weighted):
            with pytest.raises(InvalidParams, match="weighted"):
                call(frames, KP, None, wp)
    for wts in ([1, -1, 1], [0, 0, 0]):
        with pytest.raises(InvalidParams, match="weight"):
            st.ecc_match_clipped_weighted(frames, ECC, None, WeightParameters(), wts)
        with pytest.raises(InvalidParams, match="weight"):
            st.ecc_match_quantile_weighted(frames, ECC, None, WeightParameters(), wts)


def test_null_pointers_reserved_and_output_geometry_are_rejected(st):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    frames, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(frames.numpy())
    out = np.empty((96, 128, 3), F)
    img = _ffi.ImageF32(out.ctypes.data, 128, 96, 3, HOST, 0)
    ep = ECC._c()
    wp, cp, qp = WeightParameters()._c(), SigmaClipParameters()._c(), _ffi.QuantileParams(0.5, 0)
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    rec = (_ffi.FrameWeight * 3)()
    for r in rec:
        r.gain[:] = [1, 1, 1, 1]
        r.weight = 1.0
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    a = 1.0 / 255
    assert lib.stk_clip_stack_weighted(h, fr, None, None, 0, 0, None, a, C.byref(cp), rec, 1, C.byref(img), None, None) == 2
    assert lib.stk_clip_stack_weighted(h, fr, Mp, None, 0, 0, None, a, None, rec, 1, C.byref(img), None, None) == 2
    assert lib.stk_clip_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(cp), None, 1, C.byref(img), None, None) == 2
    assert lib.stk_clip_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(cp), rec, 2, C.byref(img), None, None) == 2
    assert b"coverage" in lib.stk_last_error(h)
    assert lib.stk_quantile_stack_weighted(h, fr, Mp, None, 0, 0, None, a, None, rec, 1, C.byref(img), None) == 2
    assert lib.stk_quantile_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(qp), None, 1, C.byref(img), None) == 2
    assert lib.stk_ecc_match_clipped_weighted(h, fr, C.byref(ep), 0.0, None, C.byref(wp), None, C.byref(img), None, None, None, None) == 2
    assert lib.stk_ecc_match_clipped_weighted(h, fr, C.byref(ep), 0.0, C.byref(cp), None, None, C.byref(img), None, None, None, None) == 2
    assert lib.stk_ecc_match_quantile_weighted(h, fr, C.byref(ep), 0.0, None, C.byref(wp), None, C.byref(img), None, None, None) == 2
    bad = WeightParameters()._c()
    bad.reserved = 1
    assert lib.stk_ecc_match_clipped_weighted(h, fr, C.byref(ep), 0.0, C.byref(cp), C.byref(bad), None, C.byref(img), None, None, None, None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    badq = _ffi.QuantileParams(0.5, 1)
    assert lib.stk_ecc_match_quantile_weighted(h, fr, C.byref(ep), 0.0, C.byref(badq), C.byref(wp), None, C.byref(img), None, None, None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    narrow = np.empty((96, 127, 3), F)
    nimg = _ffi.ImageF32(narrow.ctypes.data, 127, 96, 3, HOST, 0)
    assert lib.stk_ecc_match_clipped_weighted(h, fr, C.byref(ep), 0.0, C.byref(cp), C.byref(wp), None, C.byref(nimg), None, None, None, None) == 2
    assert b"geometry" in lib.stk_last_error(h)
    assert lib.stk_quantile_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(qp), rec, 1, C.byref(nimg), None) == 2
    assert b"geometry" in lib.stk_last_error(h)
    wide = np.empty((96, 160, 3), F)
    loose = _ffi.ImageF32(wide.ctypes.data, 128, 96, 3, HOST, 160 * 3 * 4)
    assert lib.stk_clip_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(cp), rec, 1, C.byref(loose), None, None) == 2
    assert b"tightly" in lib.stk_last_error(h)
    assert lib.stk_clip_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(cp), rec, 1, C.byref(img), None, None) == 0      # and the good calls
    assert lib.stk_quantile_stack_weighted(h, fr, Mp, None, 0, 0, None, a, C.byref(qp), rec, 1, C.byref(img), None) == 0


def test_too_many_samples_for_the_quantile(st):
    n = 4097
    frames = np.zeros((n, 2, 4, 3), np.uint8)
    with pytest.raises(NotImplementedYet, match="4096"):
        st.quantile_stack_weighted(frames, [np.eye(3)] * n)


def test_other_calls_are_unchanged_around_the_new_ones(st):
    frames, _ = synth.make_stack(5, 256, 192, device="cuda")
    clip = SigmaClipParameters(2.0, 2.5, 2)
    wp = WeightParameters(LINEAR, True, 1)
    wts = [1, 2, 0.5, 1, 1]

    def others():
        plain, stats = st.ecc_match(frames, ECC, return_stats=True)
        kd, kout = st.keypoint_match(frames, KP)
        return [_np(plain), np.stack([s["warp"] for s in stats]), np.array(kd), _np(kout)] + \
            [_np(v) for v in st.ecc_match_clipped(frames, ECC, clip, return_counts=True)] + \
            [_np(st.ecc_match_quantile(frames, ECC, 0.5))] + \
            [_np(v) for v in st.ecc_match_weighted(frames, ECC, wp, wts, return_coverage=True)]

    before = others()
    st.ecc_match_clipped_weighted(frames, ECC, clip, wp, wts)
    st.ecc_match_quantile_weighted(frames, ECC, 0.5, wp, wts)
    st.keypoint_match_clipped_weighted(frames, KP, clip, wp, wts)
    st.keypoint_match_quantile_weighted(frames, KP, 0.3, wp, wts)
    after = others()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- 12. full size ----------------------------------------------------------------------------------------------------
def test_fullsize_u8_ecc_clipped_weighted(st):
    frames, _ = synth.make_stack(64, 3840, 2160, device="cuda")
    wp = WeightParameters(LINEAR, True, 0)
    out, cnt, kept = st.ecc_match_clipped_weighted(frames, ECC, SigmaClipParameters(3.0, 3.0, 2), wp, return_counts=True,
                                                   return_kept_weight=True)
    assert int(cnt.max()) == 64 and int(cnt.min()) < 64 and int(cnt.min()) >= 0
    assert float(kept.max()) == 64.0 and bool((kept == cnt.float()).all())
    assert bool(out.isfinite().all())


def test_fullsize_u8_ecc_quantile_weighted(st):
    frames, _ = synth.make_stack(64, 3840, 2160, device="cuda")
    wp = WeightParameters(LINEAR, True, 0)
    out, cnt = st.ecc_match_quantile_weighted(frames, ECC, 0.5, wp, return_counts=True)
    assert int(cnt.max()) == 64 and int(cnt.min()) < 64 and int(cnt.min()) >= 0
    assert bool(out.isfinite().all())

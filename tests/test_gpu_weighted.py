"""Weighted, coverage-aware stacking on the GPU: stk_weighted_stack / stk_overlap_moments / stk_ecc_match_weighted /
stk_keypoint_match_weighted against the numpy restatements of the definition (test_cpu_weighted.weighted_restate and
estimate). The samples come from the engine's own single-frame warp (Stacker.warp_accumulate with the same matrices), the
coverage weights kappa from the same warp of an all-ones f32 frame under BORDER_CONSTANT 0 with alpha = 1."""
import ctypes as C
import math
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, MotionType, NotImplementedYet, Stacker, WeightParameters, synth)
from test_cpu_weighted import GAIN, LINEAR, NONE, OFFSET, estimate, weighted_restate
from test_gpu_clip import CASES

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
_ALPHA = {np.uint8: 1.0 / 255.0, np.uint16: 1.0 / 65535.0, np.float32: 1.0}
_SCALE = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def random_frames(rng, n, h, w, cn, dtype):
    out = []
    for _ in range(n):
        f = rng.random((h, w, cn)) * _SCALE[dtype]
        out.append(np.rint(f).astype(dtype) if dtype != np.float32 else f.astype(np.float32))
    return out


def shifted_warps(rng, n, affine, reach=6.0):
    """Small warps with translations of up to +-reach px (frame 0's included), so that the rim is exercised."""
    Ms = []
    for _ in range(n):
        M = np.eye(3)
        M[:2, :2] += rng.normal(0, 4e-3, (2, 2))
        M[:2, 2] = rng.uniform(-reach, reach, 2)
        if not affine:
            M[2, :2] = rng.normal(0, 2e-5, 2)
        Ms.append(M)
    return Ms


def engine_samples(st, frames, warps, idx, **kw):
    return np.stack([np.asarray(st.warp_accumulate(frames[i], warps[i], acc=None, **kw)) for i in idx])


def engine_kappa(st, shape_hw, warps, idx, is_affine):
    """kappa_i: channel 0 of the engine's sample of an all-ones three-channel f32 frame, BORDER_CONSTANT 0, alpha = 1."""
    ones = np.ones((shape_hw[0], shape_hw[1], 3), np.float32)
    return np.stack([np.asarray(st.warp_accumulate(ones, warps[i], acc=None, is_affine=is_affine, border_mode=BORDER_CONSTANT,
                                                   border_value=(0, 0, 0, 0), alpha=1.0))[..., 0] for i in idx])


# ---- 1. weighted_stack against the restatement, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("coverage", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-{c[8][0]}x{c[8][1]}" for c in CASES])
def test_weighted_stack_matches_restatement(st, case, coverage):
    import torch
    dtype, cn, affine, border, bv, sub, _, _, (h, w) = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    n = 9
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine)
    include = [1] * n
    include[4] = 0
    idx = [i for i in range(n) if include[i]]
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(np.float32)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(np.float32)
    wt = rng.uniform(0.0, 2.0, n).astype(np.float32)
    wt[2] = 0.0
    if coverage:
        bv = (0, 0, 0, 0)                        # coverage = 1 needs BORDER_CONSTANT 0
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype])
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    st.set_option("warp_subpixel_bits", sub)
    try:
        if coverage and border != BORDER_CONSTANT:
            with pytest.raises(InvalidParams, match="coverage"):
                st.weighted_stack(frames, warps, g, o, wt, include, coverage=True, **kw)
            return
        samples = engine_samples(st, frames, warps, idx, **kw)
        kappa = engine_kappa(st, (h, w), warps, idx, affine)
        out, den = st.weighted_stack(frames, warps, g, o, wt, include, coverage=bool(coverage), return_coverage=True, **kw)
        dout, dden = st.weighted_stack(dframes, warps, g, o, wt, include, coverage=bool(coverage), return_coverage=True, **kw)
        only = st.weighted_stack(frames, warps, g, o, wt, include, coverage=bool(coverage), **kw)
    finally:
        st.set_option("warp_subpixel_bits", 0)
    # the test cannot pass on interiors alone: the rim is a real share of the (pixel, entry) pairs
    rim = ((kappa >= 0) & (kappa < 1)).mean()
    assert rim >= 0.03, rim
    assert ((kappa >= 0) & (kappa <= 1)).all()
    ref, ref_den = weighted_restate(samples, kappa if coverage else np.ones_like(kappa), g[idx], o[idx], wt[idx])
    assert np.array_equal(den, ref_den) and np.array_equal(out, ref, equal_nan=True)
    assert np.array_equal(dden.cpu().numpy(), ref_den) and np.array_equal(dout.cpu().numpy(), ref, equal_nan=True)
    assert np.array_equal(only, out, equal_nan=True)
    if coverage:
        assert (den < np.float32(wt[idx].sum()) * 0.999).any()


# ---- 2. coverage ground truth, independent of the restatement ---------------------------------------------------------
def test_coverage_restores_a_constant_scene_on_the_rim(st):
    rng = np.random.default_rng(11)
    n, h, w = 9, 48, 80
    frames = [np.full((h, w, 3), 153, np.uint8) for _ in range(n)]
    v = np.float32(153) * np.float32(1.0 / 255.0)
    # every frame is shifted right and down by 1 .. 6 px: the first column and row are covered by no frame
    warps = []
    for _ in range(n):
        M = np.eye(3)
        M[:2, 2] = rng.uniform(1.0, 6.0, 2)
        warps.append(M)
    out, den = st.weighted_stack(frames, warps, coverage=True, return_coverage=True)
    cov = den > 0
    assert (~cov).any() and (den[cov] < n).any() and (den == n).any()
    rel = np.abs(out[cov].astype(np.float64) - float(v)) / float(v)
    print("coverage ground truth: max relative error", rel.max() / 2.0 ** -24, "x 2^-24")
    # one division and two running sums of a few terms each: a few 2^-24; the bound is the issue's (twice its prototype's 4)
    assert rel.max() <= 8 * 2.0 ** -24
    assert (out[~cov] == 0).all()
    # the defect this fixes: the plain mean darkens the rim by the share of frames that miss it
    acc = None
    for f, M in zip(frames, warps):
        acc = st.warp_accumulate(f, M, acc=acc)
    mean = np.asarray(acc) / n
    assert mean[cov].min() < 0.9 * v


# ---- 3. overlap moments against math.fsum ---------------------------------------------------------------------
def _exact_moments(samples, kappa, step):
    """n x cn x 6 by math.fsum over the stepped pixels with kappa_i == 1 (products of f32 values are exact in f64), and the
    sums of the absolute terms."""
    n, h, w, cn = samples.shape
    exact = np.zeros((n, cn, 6))
    mag = np.zeros((n, cn, 6))
    for i in range(1, n):
        m = np.zeros((h, w), bool)
        m[::step, ::step] = True
        m &= kappa[i] == np.float32(1.0)
        for c in range(cn):
            X = samples[i][..., c][m].astype(np.float64)
            Y = samples[0][..., c][m].astype(np.float64)
            terms = [np.ones_like(X), X, Y, X * X, Y * Y, X * Y]
            exact[i, c] = [math.fsum(t.tolist()) for t in terms]
            mag[i, c] = [math.fsum(np.abs(t).tolist()) for t in terms]
    return exact, mag


@pytest.mark.parametrize("dtype,cn,border", [(np.uint8, 3, BORDER_CONSTANT), (np.uint8, 4, BORDER_CONSTANT),
                                             (np.float32, 3, BORDER_REPLICATE), (np.uint16, 1, BORDER_CONSTANT)])
@pytest.mark.parametrize("step", [1, 3, 4])
def test_overlap_moments_match_exact_sums(st, dtype, cn, border, step):
    rng = np.random.default_rng(zlib.crc32(f"{dtype}{cn}{border}{step}".encode()))
    n, h, w = 7, 48, 80
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, False)
    warps[0] = np.eye(3)
    warps[3][:2, 2] = (200.0, -150.0)                      # shifted fully out of view: n = 0
    include = [1] * n
    include[5] = 0
    idx = [i for i in range(n) if include[i]]
    kw = dict(border_mode=border, border_value=(0, 0, 0, 0), alpha=_ALPHA[dtype])
    mom = st.overlap_moments(frames, warps, include, stat_step=step, **kw)
    samples = engine_samples(st, frames, warps, idx, **kw)
    kappa = engine_kappa(st, (h, w), warps, idx, False)      # the BORDER_CONSTANT one, whatever the fold's border mode
    exact, mag = _exact_moments(samples, kappa, step)
    assert (mom[0] == 0).all() and (mom[5] == 0).all() and (mom[3] == 0).all()
    u = 2.0 ** -53
    for k, i in enumerate(idx):
        if i == 0:
            continue
        cnt = exact[k, 0, 0]
        assert (mom[i, :, 0] == cnt).all(), (i, mom[i, :, 0], cnt)          # n exactly
        gamma = (cnt - 1) * u / (1 - (cnt - 1) * u) if cnt > 1 else 0.0
        assert (np.abs(mom[i] - exact[k]) <= gamma * mag[k]).all(), (i, np.abs(mom[i] - exact[k]).max())
    assert any(exact[k, 0, 0] > 50 for k in range(1, len(idx)))
    # the same bits on every call, host-fed or device-resident
    assert np.array_equal(st.overlap_moments(frames, warps, include, stat_step=step, **kw), mom)


def test_overlap_moments_do_not_depend_on_options(st):
    rng = np.random.default_rng(5)
    frames = random_frames(rng, 6, 96, 160, 3, np.uint8)
    warps = shifted_warps(rng, 6, False)
    base = st.overlap_moments(frames, warps, stat_step=2)
    for name, val, back in (("kp_lanes", 1, 3), ("ecc_slots", 4, 0), ("prep_overlap", 0, 1)):
        st.set_option(name, val)
        try:
            again = st.overlap_moments(frames, warps, stat_step=2)
        finally:
            st.set_option(name, back)
        assert np.array_equal(again, base), name
    other = Stacker(0)
    try:
        assert np.array_equal(other.overlap_moments(frames, warps, stat_step=2), base)
    finally:
        other.close()


# ---- 4. whole-stack forms -----------------------------------------------------------------------------------------
def _dimmed(frames, gains):
    """u8 frames scaled frame by frame (a session whose transparency drifts)."""
    f = frames.astype(np.float32) * np.asarray(gains, np.float32)[:, None, None, None]
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _applied_equal(applied, g, o, fb, weights):
    for i, a in enumerate(applied):
        assert np.array_equal(a["gain"], g[i]) and np.array_equal(a["offset"], o[i]), (i, a, g[i], o[i])
        assert a["weight"] == np.float32(weights[i])
        assert a["flags"] == sum(1 << c for c in range(len(fb[i])) if fb[i][c])


@pytest.mark.parametrize("mode,step", [(LINEAR, 0), (GAIN, 3), (OFFSET, 1), (NONE, 0)])
def test_ecc_match_weighted_equals_its_parts(st, mode, step):
    import torch
    frames, _ = synth.make_stack(6, 256, 192)
    host = _dimmed(frames.numpy(), [1.0, 0.8, 0.9, 1.0, 0.7, 0.85])
    dev = torch.from_numpy(host).cuda()
    weights = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0]
    wp = WeightParameters(mode, True, step)
    out, cov, applied, stats = st.ecc_match_weighted(dev, ECC, wp, weights, return_stats=True, return_coverage=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    plain, pstats = st.ecc_match(dev, ECC, return_stats=True)
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["rho"] == b["rho"]
        assert np.array_equal(a["warp"], b["warp"])
    warps = [s["warp"] for s in stats]
    mom = st.overlap_moments(dev, warps, stat_step=step or 4)
    g, o, fb = estimate(mom, mode)
    g[0], o[0], fb[0] = 1, 0, False
    _applied_equal(applied, g, o, fb, weights)
    if mode in (GAIN, LINEAR):
        assert abs(applied[4]["gain"][0] - 1 / 0.7) < 0.05          # the normalisation did something
    ref, ref_cov = st.weighted_stack(dev, warps, applied=applied, coverage=True, return_coverage=True)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(cov.cpu().numpy(), ref_cov.cpu().numpy())
    # host-fed: the same bits, outputs on the host
    hout, hcov, happlied = st.ecc_match_weighted(host, ECC, wp, weights, return_coverage=True, return_applied=True)
    assert np.array_equal(hout, out.cpu().numpy()) and np.array_equal(hcov, cov.cpu().numpy())
    _applied_equal(happlied, g, o, fb, weights)
    # a multi-device context runs the weighted calls on its first device: the single-device bits
    if mode == LINEAR:
        multi = Stacker(devices=[0, 0])
        try:
            mo = multi.ecc_match_weighted(dev, ECC, wp, weights)
        finally:
            multi.close()
        assert np.array_equal(mo.cpu().numpy(), out.cpu().numpy())


def test_keypoint_match_weighted_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 640, 480)
    frames = _dimmed(frames.numpy(), [1.0, 0.8, 0.9, 0.75])
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    weights = [1.0, 2.0, 3.0, 0.5, 1.0]
    wp = WeightParameters(LINEAR, True, 2)
    dropped, out, cov, applied, stats = st.keypoint_match_weighted(stack, KP, wp, weights, return_stats=True, return_coverage=True,
                                                                   return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    pd, plain, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["n_matches"] == b["n_matches"] and np.array_equal(a["warp"], b["warp"])
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    mom = st.overlap_moments(stack, warps, include, stat_step=2)
    g, o, fb = estimate(mom, LINEAR)
    g[0], o[0], fb[0] = 1, 0, False
    g[2], o[2], fb[2] = 1, 0, False                     # the dropped frame: weight 0, gains 1, not a sample
    w_applied = list(weights)
    w_applied[2] = 0.0
    _applied_equal(applied, g, o, fb, w_applied)
    ref, ref_cov = st.weighted_stack(stack, warps, applied=applied, include=include, coverage=True, return_coverage=True)
    assert np.array_equal(out, ref) and np.array_equal(cov, ref_cov)
    assert cov.max() == np.float32(1.0 + 2.0 + 0.5 + 1.0)
    import torch
    dd, dout = st.keypoint_match_weighted(torch.from_numpy(np.stack(stack)).cuda(), KP, wp, weights)
    assert dd == 1 and np.array_equal(dout.cpu().numpy(), out)


# ---- 5. normalisation ground truth ----------------------------------------------------------------------------------
def _cut_stack(rng, n, h, w, a, b):
    """Frame i = a_i * scene + b_i cut at integer shifts of up to +-6 px (frame 0: none): the samples are exact."""
    scene = rng.random((h + 12, w + 12, 3)).astype(np.float32)
    shifts = [(0, 0)] + [tuple(int(v) for v in rng.integers(-6, 7, 2)) for _ in range(1, n)]
    frames, warps = [], []
    for i, (ox, oy) in enumerate(shifts):
        cut = scene[6 + oy:6 + oy + h, 6 + ox:6 + ox + w]
        frames.append((np.float32(a[i]) * cut + np.float32(b[i])).astype(np.float32))
        M = np.eye(3)
        M[:2, 2] = (ox, oy)           # frame i's pixel (x, y) is frame 0's (x + ox, y + oy)
        warps.append(M)
    return frames, warps


def test_linear_normalisation_reproduces_frame_0(st):
    rng = np.random.default_rng(3)
    n, h, w = 9, 48, 80
    a = np.concatenate([[1.0], rng.uniform(0.6, 1.5, n - 1)]).astype(np.float32)
    b = np.concatenate([[0.0], rng.uniform(-0.1, 0.2, n - 1)]).astype(np.float32)
    frames, warps = _cut_stack(rng, n, h, w, a, b)
    mom = st.overlap_moments(frames, warps, stat_step=1, alpha=1.0)
    g, o, fb = estimate(mom, LINEAR)
    g[0], o[0] = 1, 0
    assert not fb[1:].any()
    out, den = st.weighted_stack(frames, warps, g, o, coverage=True, alpha=1.0, return_coverage=True)
    raw = st.weighted_stack(frames, warps, coverage=True, alpha=1.0)
    assert (den > 0).all() and (den < n).any()
    err = np.abs(out - frames[0]).max()
    raw_err = np.abs(raw - frames[0]).max()
    print("LINEAR normalisation: max abs error", err, "un-normalised", raw_err)
    assert raw_err > 0.05
    # measured on the MI355X: 1.19e-7 = 2^-23, two ulps of a value below 1 (the f32 gains and offsets carry 2^-24 relative
    # each, then a nine-term weighted sum and one division) against 0.139 un-normalised; asserted at four times the
    # measured value, far below 1e-3 of the un-normalised error
    assert err <= 4 * 2.0 ** -23
    assert err < 1e-3 * raw_err


def test_offset_and_gain_recover_the_frames_levels(st):
    """`applied` of the whole-stack forms is estimate(overlap_moments) bit for bit (test_ecc_match_weighted_equals_its_parts),
    so the levels are checked on that pair, where the samples are exact."""
    rng = np.random.default_rng(4)
    n, h, w = 7, 48, 80
    one, zero = np.ones(n, np.float32), np.zeros(n, np.float32)
    b = np.concatenate([[0.0], rng.uniform(-0.1, 0.2, n - 1)]).astype(np.float32)
    frames, warps = _cut_stack(rng, n, h, w, one, b)
    g, o, fb = estimate(st.overlap_moments(frames, warps, stat_step=1, alpha=1.0), OFFSET)
    assert (g == 1).all() and not fb[1:].any()
    # X = f32(scene + b) is within 2^-24 of scene + b (values below 2), so is the mean; rounding o to f32 adds 2^-26
    assert np.abs(o[1:] + b[1:, None]).max() <= 2.0 ** -23
    a = np.concatenate([[1.0], rng.uniform(0.6, 1.5, n - 1)]).astype(np.float32)
    frames, warps = _cut_stack(rng, n, h, w, a, zero)
    g, o, fb = estimate(st.overlap_moments(frames, warps, stat_step=1, alpha=1.0), GAIN)
    assert (o == 0).all() and not fb[1:].any()
    # X = f32(a scene) is within 2^-24 relative of a scene, so is the mean; rounding g to f32 adds another 2^-24
    assert np.abs(g[1:].astype(np.float64) * a[1:, None].astype(np.float64) - 1).max() <= 2.0 ** -23


# ---- 6. errors, and the plain call is left alone ---------------------------------------------------------------------
def test_invalid_arguments_are_rejected(st):
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    I = [np.eye(3)] * 3
    for wts in ([1, -1, 1], [1, float("nan"), 1], [1, float("inf"), 1], [0, 0, 0]):
        with pytest.raises(InvalidParams, match="weight"):
            st.weighted_stack(frames, I, weights=wts)
    with pytest.raises(InvalidParams, match="weight"):
        st.weighted_stack(frames, I, weights=[0, 5, 0], include=[1, 0, 1])      # every INCLUDED weight is 0
    with pytest.raises(InvalidParams, match="finite"):
        st.weighted_stack(frames, I, gain=np.full((3, 3), np.inf))
    with pytest.raises(InvalidParams, match="finite"):
        st.weighted_stack(frames, I, offset=np.full((3, 3), np.nan))
    with pytest.raises(InvalidParams, match="coverage"):
        st.weighted_stack(frames, I, coverage=True, border_mode=BORDER_REPLICATE)
    with pytest.raises(InvalidParams, match="coverage"):
        st.weighted_stack(frames, I, coverage=True, border_value=(0, 0.5, 0, 0))
    st.weighted_stack(frames, I, coverage=False, border_mode=BORDER_REPLICATE)
    st.weighted_stack(frames, I, coverage=False, border_value=(0, 0.5, 0, 0))
    with pytest.raises(NotImplementedYet):
        st.weighted_stack(frames, I, coverage=False, border_mode=5)             # BORDER_TRANSPARENT
    with pytest.raises(NotImplementedYet):
        st.overlap_moments(frames, I, border_mode=5)
    with pytest.raises(InvalidParams):
        st.weighted_stack(frames, I, coverage=False, border_mode=6)
    for step in (0, 65, -1):
        with pytest.raises(InvalidParams, match="stat_step"):
            st.overlap_moments(frames, I, stat_step=step)
    with pytest.raises(InvalidParams, match="frame 0"):
        st.overlap_moments(frames, I, include=[0, 1, 1])
    for wp in (WeightParameters(4), WeightParameters(-1), WeightParameters(LINEAR, True, 65), WeightParameters(LINEAR, True, -1),
               WeightParameters(NONE, 2)):
        with pytest.raises(InvalidParams, match="weighted"):
            st.ecc_match_weighted(frames, ECC, wp)
        with pytest.raises(InvalidParams, match="weighted"):
            st.keypoint_match_weighted(frames, KP, wp)
    for wts in ([1, -1, 1], [0, 0, 0], [1, float("nan"), 1]):
        with pytest.raises(InvalidParams, match="weight"):
            st.ecc_match_weighted(frames, ECC, WeightParameters(), wts)
    with pytest.raises(InvalidParams, match="coverage"):
        st.keypoint_match_weighted(frames, KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9, BORDER_REPLICATE), WeightParameters())
    st.keypoint_match_weighted(frames, KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9, BORDER_REPLICATE), WeightParameters(NONE, False))


def test_null_pointers_reserved_and_untight_output_are_rejected(st):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    frames, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(frames.numpy())
    out = np.empty((96, 128, 3), np.float32)
    img = _ffi.ImageF32(out.ctypes.data, 128, 96, 3, HOST, 0)
    ep, kp = ECC._c(), KP._c()
    wp = WeightParameters()._c()
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    rec = (_ffi.FrameWeight * 3)()
    for r in rec:
        r.gain[:] = [1, 1, 1, 1]
        r.weight = 1.0
    mom = np.zeros((3, 3, 6))
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    dropped = C.c_int32(0)
    assert lib.stk_ecc_match_weighted(h, fr, C.byref(ep), 0.0, None, None, C.byref(img), None, None, None) == 2        # null params
    assert lib.stk_keypoint_match_weighted(h, fr, C.byref(kp), 0.0, None, None, C.byref(img), C.byref(dropped), None, None, None) == 2
    assert lib.stk_weighted_stack(h, fr, None, None, 0, 0, None, 1.0 / 255, rec, 1, C.byref(img), None) == 2             # null matrices
    assert lib.stk_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, 1, C.byref(img), None) == 2              # null records
    assert lib.stk_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, rec, 2, C.byref(img), None) == 2               # coverage enum
    assert lib.stk_overlap_moments(h, fr, None, None, 0, 0, None, 1.0 / 255, 4, C.c_void_p(mom.ctypes.data)) == 2
    assert lib.stk_overlap_moments(h, fr, Mp, None, 0, 0, None, 1.0 / 255, 4, None) == 2
    bad = WeightParameters()._c()
    bad.reserved = 1
    assert lib.stk_ecc_match_weighted(h, fr, C.byref(ep), 0.0, C.byref(bad), None, C.byref(img), None, None, None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    wide = np.empty((96, 160, 3), np.float32)
    loose = _ffi.ImageF32(wide.ctypes.data, 128, 96, 3, HOST, 160 * 3 * 4)
    assert lib.stk_ecc_match_weighted(h, fr, C.byref(ep), 0.0, C.byref(wp), None, C.byref(loose), None, None, None) == 2
    assert b"tightly" in lib.stk_last_error(h)
    assert lib.stk_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, rec, 1, C.byref(loose), None) == 2
    assert b"tightly" in lib.stk_last_error(h)
    assert lib.stk_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, rec, 1, C.byref(img), None) == 0               # and the good call


def test_plain_calls_are_unchanged_around_a_weighted_call(st):
    frames, _ = synth.make_stack(5, 256, 192, device="cuda")
    before, bstats = st.ecc_match(frames, ECC, return_stats=True)
    kd, kbefore = st.keypoint_match(frames, KP)
    st.ecc_match_weighted(frames, ECC, WeightParameters(LINEAR, True, 1), [1, 2, 0.5, 1, 1])
    after, astats = st.ecc_match(frames, ECC, return_stats=True)
    kd2, kafter = st.keypoint_match(frames, KP)
    assert np.array_equal(before.cpu().numpy(), after.cpu().numpy())
    assert all(np.array_equal(a["warp"], b["warp"]) for a, b in zip(astats, bstats))
    assert kd == kd2 and np.array_equal(kbefore.cpu().numpy(), kafter.cpu().numpy())
    # all weights 1, no normalisation, no coverage: the plain mean's samples, sum / N instead of sum * (1 / N)
    same = st.ecc_match_weighted(frames, ECC, WeightParameters(NONE, False))
    assert (same - before).abs().max().item() <= 1e-6


# ---- 7. full size -------------------------------------------------------------------------------------------------------
def test_fullsize_u8_ecc_weighted(st):
    frames, _ = synth.make_stack(64, 3840, 2160, device="cuda")
    wp = WeightParameters(LINEAR, True, 0)
    out, cov, applied, stats = st.ecc_match_weighted(frames, ECC, wp, return_stats=True, return_coverage=True, return_applied=True)
    for a in applied:
        assert np.isfinite(a["gain"]).all() and np.isfinite(a["offset"]).all() and a["flags"] == 0 and a["weight"] == 1.0
        assert np.abs(a["gain"] - 1).max() < 0.05 and np.abs(a["offset"]).max() < 0.05     # one scene, one exposure
    warps = [s["warp"] for s in stats]
    ref, ref_cov = st.weighted_stack(frames, warps, applied=applied, coverage=True, return_coverage=True)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(cov.cpu().numpy(), ref_cov.cpu().numpy())
    assert float(cov.max()) == 64.0 and float(cov.min()) < 64.0
    assert np.isfinite(out.cpu().numpy()).all()

"""The two clip combines through local-normalisation planes on the GPU: NULL and constant planes against the weighted clips
bit for bit, random planes against the numpy restatements (local_norm_clip_restate.py) bit for bit, the u8 BGR fast state
against the generic one, the whole-stack forms against their parts, and the refusals. As in test_gpu_local_norm.py the
fold's samples come from the engine's own single-frame warp and kappa from the same warp of an all-ones frame.
Shapes: 150 x 45 has three waves per row with the last one partial, h no multiple of 4 and at step 16 an 11 x 4 grid;
200 x 70 at step 64 gives a 5 x 3 grid, where a wave shares its four nodes; 193 x 65 at step 64 puts the last column and
row on the last node, where k1 and j1 clamp."""
import ctypes as C
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, INTER_CUBIC, INTER_LINEAR, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, LocalNormParameters, MotionType, NotImplementedYet, RobustClipParameters,
                               SigmaClipParameters, Stacker, local_norm_estimate, local_norm_grid, synth)
from local_norm_clip_restate import norm_clip_restate, norm_robust_clip_restate, planted_stack
from local_norm_restate import LINEAR, quality_rms
from test_cpu_local_norm import quality_restated
from test_gpu_local_norm import _graded_stack, _same_stats
from test_gpu_robust import rim_warps
from test_gpu_weighted import _ALPHA, engine_kappa, engine_samples, random_frames, shifted_warps

pytestmark = pytest.mark.gpu

F = np.float32
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
FLOOR = 0.5 / 255.0
SHAPE = {16: (45, 150), 64: (70, 200)}                 # (h, w) by step
RET = dict(return_counts=True, return_kept_weight=True)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _same(got, ref, what=""):
    """(out, counts, kept) bit for bit."""
    out, cnt, kept = (_np(v) for v in got)
    assert np.array_equal(cnt, _np(ref[1])), what
    assert np.array_equal(kept, _np(ref[2])), what
    assert np.array_equal(out, _np(ref[0]), equal_nan=True), what


def _planes(rng, n, h, w, cn, step, none=()):
    """Gains 0.8 .. 1.25 and offsets +-0.05 per node."""
    gh, gw, _, _ = local_norm_grid(w, h, step)
    return [None if i in none else
            np.concatenate([rng.uniform(0.8, 1.25, (gh, gw, cn)), rng.uniform(-0.05, 0.05, (gh, gw, cn))], axis=-1).astype(F)
            for i in range(n)]


# ---- 1. NULL and constant planes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_null_and_constant_planes_give_the_weighted_clips_bits(st, dtype, cn):
    """u8 cn 3 under BORDER_CONSTANT: both sides run the u8 BGR fast kernels."""
    rng = np.random.default_rng(10 * cn + np.dtype(dtype).itemsize)
    n, step = 5, 16
    h, w = SHAPE[step]
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = rim_warps(rng, n, False, h)
    g = rng.uniform(0.8, 1.25, (n, cn)).astype(F)
    o = rng.uniform(-0.05, 0.05, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[3] = 0.0
    gh, gw, _, _ = local_norm_grid(w, h, step)
    const = [np.broadcast_to(np.concatenate([g[i], o[i]]), (gh, gw, 2 * cn)).copy() for i in range(n)]
    clip, mad = SigmaClipParameters(1.5, 2.0, 2), RobustClipParameters(2.0, 2.5, FLOOR, 2)
    kw = dict(alpha=_ALPHA[dtype])
    for cov in (True, False):
        ref = st.clip_stack_weighted(frames, warps, clip, g, o, wt, coverage=cov, **RET, **kw)
        rref = st.robust_clip_stack_weighted(frames, warps, mad, g, o, wt, coverage=cov, **RET, **kw)
        for planes, rec in (([None] * n, (g, o)), (None, (g, o)), (const, (None, None)), (const[:2] + [None] * 3, (g, o))):
            _same(st.clip_stack_local_norm(frames, warps, planes, step, clip, rec[0], rec[1], wt, coverage=cov, **RET, **kw), ref)
            _same(st.robust_clip_stack_local_norm(frames, warps, planes, step, mad, rec[0], rec[1], wt, coverage=cov, **RET, **kw), rref)
        assert (ref[1] < n - 1).any()                           # something is rejected or uncovered


# ---- 2. random planes against the restatement ----------------------------------------------------------------------------
CASES = [
    # n, dtype, cn, border, step, iterations, planes that are None, entry of weight 0
    (1, np.uint8, 3, BORDER_CONSTANT, 16, 1, (), None),                 # centre only
    (2, np.uint8, 3, BORDER_CONSTANT, 64, 3, (), None),                 # no update below k = 3
    (3, np.uint8, 3, BORDER_CONSTANT, 16, 3, (), None),                 # the first update
    (5, np.uint8, 3, BORDER_CONSTANT, 64, 1, (2,), 1),
    (5, np.uint8, 3, BORDER_CONSTANT, 16, 3, (0,), 3),
    (5, np.uint8, 3, BORDER_REPLICATE, 16, 1, (3,), 1),                 # the generic state
    (5, np.uint8, 3, BORDER_REPLICATE, 64, 3, (), None),
    (3, np.uint16, 1, BORDER_CONSTANT, 64, 1, (), None),
    (5, np.uint16, 1, BORDER_CONSTANT, 16, 3, (4,), 2),
    (2, np.float32, 4, BORDER_CONSTANT, 16, 1, (), None),
    (5, np.float32, 4, BORDER_CONSTANT, 64, 3, (1,), 0),
    (5, np.uint8, 3, BORDER_CONSTANT, 64, 1, (), None, (65, 193)),      # the last pixel sits on the last node: k1, j1 clamp
]


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}-{np.dtype(c[1]).name}c{c[2]}-b{c[3]}-s{c[4]}-T{c[5]}" + ("-clamp" if len(c) > 8 else "") for c in CASES])
def test_random_planes_match_the_restatement(st, case):
    import torch
    n, dtype, cn, border, step, T, none, zero = case[:8]
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    h, w = case[8] if len(case) > 8 else SHAPE[step]
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = rim_warps(rng, n, False, h)
    planes = _planes(rng, n, h, w, cn, step, none)
    g = rng.uniform(0.8, 1.25, (n, cn)).astype(F)
    o = rng.uniform(-0.05, 0.05, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    if zero is not None:
        wt[zero] = 0.0
    kw = dict(border_mode=border, border_value=(0, 0, 0, 0), alpha=_ALPHA[dtype])
    samples = engine_samples(st, frames, warps, range(n), **kw)
    kappa = engine_kappa(st, (h, w), warps, range(n), False)
    assert (kappa < 1).mean() >= 0.03
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    kl, kh = 1.5, 2.0
    for cov in (1, 0):
        part = kappa == F(1) if cov else np.ones(kappa.shape, bool)
        ref = norm_clip_restate(samples, part, planes, step, kl, kh, T, g, o, wt)
        for fr in (frames, dframes):
            _same(st.clip_stack_local_norm(fr, warps, planes, step, SigmaClipParameters(kl, kh, T), g, o, wt, coverage=bool(cov), **RET, **kw),
                  ref, ("clip", cov))
        for floor in (0.0, FLOOR):
            rref = norm_robust_clip_restate(samples, part, planes, step, kl, kh, floor, T, g, o, wt)
            _same(st.robust_clip_stack_local_norm(frames, warps, planes, step, RobustClipParameters(kl, kh, floor, T), g, o, wt,
                                                  coverage=bool(cov), **RET, **kw), rref, ("mad", cov, floor))
        if n >= 5:
            assert (ref[1] < ref[1].max()).any()
        if cov and len(none) < n and n > 1:
            # the planes matter: the restatement with the records instead is something else
            assert not np.array_equal(norm_clip_restate(samples, part, None, step, kl, kh, T, g, o, wt)[0], ref[0])


# ---- 3. fast against generic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [16, 64])
def test_fast_state_equals_the_generic_state(st, step):
    """coverage = 1: a participating sample has no weighted tap outside the frame, so the border mode cannot show; under
    BORDER_CONSTANT u8 BGR runs the fast kernels, under BORDER_REPLICATE the generic one."""
    rng = np.random.default_rng(step)
    n = 6
    h, w = SHAPE[step]
    frames = random_frames(rng, n, h, w, 3, np.uint8)
    warps = rim_warps(rng, n, False, h)
    planes = _planes(rng, n, h, w, 3, step, (4,))
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    for affine in (False, True):
        Ms = warps if not affine else [np.vstack([M[:2], [0, 0, 1]]) for M in warps]
        fast = st.clip_stack_local_norm(frames, Ms, planes, step, SigmaClipParameters(1.5, 2.0, 2), weights=wt, is_affine=affine, **RET)
        slow = st.clip_stack_local_norm(frames, Ms, planes, step, SigmaClipParameters(1.5, 2.0, 2), weights=wt, is_affine=affine,
                                        border_mode=BORDER_REPLICATE, **RET)
        _same(fast, slow)
        mfast = st.robust_clip_stack_local_norm(frames, Ms, planes, step, RobustClipParameters(2.0, 2.5, FLOOR, 2), weights=wt,
                                                is_affine=affine, **RET)
        mslow = st.robust_clip_stack_local_norm(frames, Ms, planes, step, RobustClipParameters(2.0, 2.5, FLOOR, 2), weights=wt,
                                                is_affine=affine, border_mode=BORDER_REPLICATE, **RET)
        _same(mfast, mslow)
        assert (fast[1] == 0).any() and (fast[1] >= 3).any()


# ---- 4. cubic and classic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,value,back,border", [("warp_interpolation", INTER_CUBIC, INTER_LINEAR, BORDER_CONSTANT),
                                                      ("warp_interpolation", INTER_CUBIC, INTER_LINEAR, BORDER_REPLICATE),
                                                      ("warp_subpixel_bits", 5, 0, BORDER_CONSTANT)])
def test_cubic_and_classic_clips_match_the_restatement(st, option, value, back, border):
    rng = np.random.default_rng(value + border)
    n, cn, step = 4, 3, 16
    h, w = SHAPE[step]
    frames = random_frames(rng, n, h, w, cn, np.uint8)
    warps = shifted_warps(rng, n, False)
    planes = _planes(rng, n, h, w, cn, step, (2,))
    g = rng.uniform(0.8, 1.25, (n, cn)).astype(F)
    o = rng.uniform(-0.05, 0.05, (n, cn)).astype(F)
    kw = dict(border_mode=border)
    # kappa is the linear fold's under the cubic fold too (the exact-coordinate one); under the classic path it is that path's
    if option == "warp_subpixel_bits":
        st.set_option(option, value)
    try:
        kappa = engine_kappa(st, (h, w), warps, range(n), False)
        st.set_option(option, value)
        samples = engine_samples(st, frames, warps, range(n), **kw)
        got = st.clip_stack_local_norm(frames, warps, planes, step, SigmaClipParameters(1.5, 2.0, 2), g, o, **RET, **kw)
        mgot = st.robust_clip_stack_local_norm(frames, warps, planes, step, RobustClipParameters(2.0, 2.5, FLOOR, 1), g, o, **RET, **kw)
    finally:
        st.set_option(option, back)
    assert not np.array_equal(engine_samples(st, frames, warps, range(n), **kw), samples)       # the option is in force
    part = kappa == F(1)
    _same(got, norm_clip_restate(samples, part, planes, step, 1.5, 2.0, 2, g, o))
    _same(mgot, norm_robust_clip_restate(samples, part, planes, step, 2.0, 2.5, FLOOR, 1, g, o))


# The cubic clip pass at every depth and channel count (ClipNorm through the generic cubic kernel, and for u8 BGR under an
# affine table the cubic u8 BGR kernel with ClipNormU8C3; the perspective one runs above): 70 x 6 destinations, a ragged
# second 64-wide and 4-row tile; 5 frames, so that a clip still has k >= 3 after one rejection; step 8, a 10 x 2 grid.
CUBIC_FORMATS = [(dt, cn) for dt in (np.uint8, np.uint16, np.float32) for cn in (1, 3, 4)]


@pytest.mark.parametrize("dtype,cn", CUBIC_FORMATS, ids=[f"{np.dtype(dt).name}c{cn}" for dt, cn in CUBIC_FORMATS])
def test_cubic_clips_match_the_restatement_at_every_depth_and_channel_count(st, dtype, cn):
    idx = CUBIC_FORMATS.index((dtype, cn))
    rng = np.random.default_rng(950 + idx)
    n, h, w, step = 5, 6, 70, 8
    affine = (dtype, cn) == (np.uint8, 3) or bool(idx % 2)
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine, reach=1.5)
    planes = _planes(rng, n, h, w, cn, step, (2,))
    g = rng.uniform(0.8, 1.25, (n, cn)).astype(F)
    o = rng.uniform(-0.05, 0.05, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    kw = dict(is_affine=affine, alpha=_ALPHA[dtype])
    # kappa is the linear fold's under the cubic fold too (the exact-coordinate one)
    kappa = engine_kappa(st, (h, w), warps, range(n), affine)
    plain = engine_samples(st, frames, warps, range(n), **kw)
    st.set_option("warp_interpolation", INTER_CUBIC)
    try:
        samples = engine_samples(st, frames, warps, range(n), **kw)
        got = st.clip_stack_local_norm(frames, warps, planes, step, SigmaClipParameters(1.5, 2.0, 2), g, o, wt, **RET, **kw)
        mgot = st.robust_clip_stack_local_norm(frames, warps, planes, step, RobustClipParameters(2.0, 2.5, FLOOR, 1), g, o, wt, **RET, **kw)
    finally:
        st.set_option("warp_interpolation", INTER_LINEAR)
    assert not np.array_equal(plain, samples)                       # the option is in force
    part = kappa == F(1)
    assert (~part).mean() >= 0.03 and part.mean() >= 0.3
    ref = norm_clip_restate(samples, part, planes, step, 1.5, 2.0, 2, g, o, wt)
    _same(got, ref)
    _same(mgot, norm_robust_clip_restate(samples, part, planes, step, 2.0, 2.5, FLOOR, 1, g, o, wt))
    assert (ref[1] < ref[1].max()).any()                            # something is rejected or uncovered
    # the planes matter: the restatement with the records instead is something else
    assert not np.array_equal(norm_clip_restate(samples, part, None, step, 1.5, 2.0, 2, g, o, wt)[0], ref[0])


# ---- 5. bands ------------------------------------------------------------------------------------------------------------------
def test_banded_median_mad_clip_addresses_the_grid_by_the_pixels_own_row(st):
    """quantile_band_rows = 7 on h = 45: bands start at rows that are no multiple of the step; the store launch must address
    the grid by the pixel's own row, and the last pass is a whole-frame launch."""
    rng = np.random.default_rng(7)
    n, cn, step = 5, 3, 16
    h, w = SHAPE[step]
    frames = random_frames(rng, n, h, w, cn, np.uint8)
    warps = rim_warps(rng, n, False, h)
    planes = _planes(rng, n, h, w, cn, step)
    for P in planes:                                          # planes that vary down the rows, so that a wrong row shows
        P[..., :cn] *= np.linspace(0.8, 1.2, P.shape[0], dtype=F)[:, None, None]
    mad = RobustClipParameters(2.0, 2.5, FLOOR, 2)
    whole = st.robust_clip_stack_local_norm(frames, warps, planes, step, mad, **RET)
    st.set_option("quantile_band_rows", 7)
    try:
        banded = st.robust_clip_stack_local_norm(frames, warps, planes, step, mad, **RET)
    finally:
        st.set_option("quantile_band_rows", 0)
    _same(banded, whole)
    samples = engine_samples(st, frames, warps, range(n))
    kappa = engine_kappa(st, (h, w), warps, range(n), False)
    _same(banded, norm_robust_clip_restate(samples, kappa == F(1), planes, step, 2.0, 2.5, FLOOR, 2))


# ---- 6. the planted exact case ----------------------------------------------------------------------------------------------
def test_planted_ramps_are_undone_exactly_on_the_device(st):
    frames, planes, scene, mask = planted_stack()
    n = len(frames)
    stack = list(frames)
    warps = [np.eye(3)] * n
    want = np.where(mask, n - 1, n)[..., None].astype(np.int32)
    kw = dict(alpha=1.0, coverage=True)
    for call, clip in ((st.robust_clip_stack_local_norm, RobustClipParameters(3.0, 3.0, 0.25, 1)),
                       (st.clip_stack_local_norm, SigmaClipParameters(2.0, 2.0, 2))):
        out, cnt, kept = call(stack, warps, planes, 16, clip, **RET, **kw)
        assert np.array_equal(out, scene)
        assert np.array_equal(cnt, want) and np.array_equal(kept, cnt.astype(F))
        unit = call(stack, warps, None, 16, clip, **kw)
        assert (unit == scene).mean() < 0.01


# ---- 7. whole-stack forms ---------------------------------------------------------------------------------------------------
CLIPS = [SigmaClipParameters(2.0, 2.5, 2), RobustClipParameters(2.5, 3.0, FLOOR, 2)]


def _check_parts(st, stack, stats, include, np_, weights, clip, res):
    """A whole-stack result against the parts on the stats' warps: moments, estimator, the caller-held clip."""
    out, cnt, kept, planes, applied = res
    n, (h, w, cn) = len(stack), stack[0].shape
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    mom = st.local_moments(stack, warps, np_.step, include, stat_step=np_.stat_step or 4)
    want = [None] * n
    for i in range(1, n):
        if not include[i]:
            assert planes[i] is None and applied[i]["weight"] == 0 and (applied[i]["gain"] == 1).all()
            continue
        want[i], glob = local_norm_estimate(w, h, cn, mom[i], np_, return_global=True)
        assert np.array_equal(planes[i], want[i])
        assert np.array_equal(applied[i]["gain"], glob["gain"]) and np.array_equal(applied[i]["offset"], glob["offset"])
        assert applied[i]["flags"] == glob["flags"] and applied[i]["weight"] == F(weights[i])
    assert planes[0] is None and (applied[0]["gain"] == 1).all() and applied[0]["weight"] == F(weights[0])
    call = st.clip_stack_local_norm if isinstance(clip, SigmaClipParameters) else st.robust_clip_stack_local_norm
    _same((out, cnt, kept), call(stack, warps, want, np_.step, clip, weights=weights, include=include, coverage=bool(np_.coverage), **RET))


ALL = dict(return_stats=True, return_norm=True, return_applied=True, **RET)


@pytest.mark.parametrize("clip", CLIPS, ids=["sigma", "mad"])
def test_ecc_form_equals_its_parts(st, clip):
    import torch
    host = _graded_stack()
    dev = torch.from_numpy(host).cuda()
    weights = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0]
    np_ = LocalNormParameters(step=32, stat_step=2, normalize=LINEAR, coverage=True, min_count=16, fill=4)
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    out, cnt, kept, planes, applied, stats = st.ecc_match_local_normalized_clipped(dev, ECC, np_, clip, weights, **ALL)
    assert st.timing()["finalize_ms"] > 0
    assert hasattr(out, "cpu")                                  # `out` on the device
    _same_stats(stats, pstats)
    _check_parts(st, list(host), stats, [1] * 6, np_, weights, clip, (out, cnt, kept, planes, applied))
    assert int(_np(cnt).max()) == 5                             # frame 3 has weight 0
    hout, hcnt, hkept = st.ecc_match_local_normalized_clipped(host, ECC, np_, clip, weights, **RET)      # host-fed, outputs on the host
    assert isinstance(hout, np.ndarray)
    _same((hout, hcnt, hkept), (out, cnt, kept))


@pytest.mark.parametrize("clip", CLIPS, ids=["sigma", "mad"])
def test_keypoint_form_equals_its_parts_with_a_dropped_frame(st, clip):
    import torch
    host = _graded_stack()
    host[2] = 128                                               # featureless: dropped
    stack = list(host)
    weights = [1.0, 2.0, 3.0, 0.5, 1.0, 1.5]
    np_ = LocalNormParameters(step=64, stat_step=0, normalize=LINEAR, coverage=True, min_count=0, fill=2)
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    d, out, cnt, kept, planes, applied, stats = st.keypoint_match_local_normalized_clipped(stack, KP, np_, clip, weights, **ALL)
    assert st.timing()["finalize_ms"] > 0
    assert d == pd == 1 and stats[2]["status"] == 1
    _same_stats(stats, pstats)
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    _check_parts(st, stack, stats, include, np_, weights, clip, (out, cnt, kept, planes, applied))
    dd, dout, dcnt, dkept = st.keypoint_match_local_normalized_clipped(torch.from_numpy(host).cuda(), KP, np_, clip, weights, **RET)
    assert dd == 1 and hasattr(dout, "cpu")
    _same((dout, dcnt, dkept), (out, cnt, kept))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(st):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import _Marshalled
    rng = np.random.default_rng(9)
    frames = random_frames(rng, 3, 45, 70, 3, np.uint8)
    warps = shifted_warps(rng, 3, False)
    for call in (st.clip_stack_local_norm, st.robust_clip_stack_local_norm):
        for step in (0, 12, 512):
            with pytest.raises(InvalidParams, match="step"):
                call(frames, warps, None, step)
        with pytest.raises(InvalidParams, match="coverage"):
            call(frames, warps, None, 16, coverage=2)
        with pytest.raises(InvalidParams):
            call(frames, warps, None, 16, weights=[0, 0, 0])
        with pytest.raises(InvalidParams):
            call(frames, warps, None, 16, include=[0, 0, 0])
        call(frames, warps, None, 16, border_mode=BORDER_REPLICATE, border_value=(0.5, 0, 0, 0))      # coverage = 1: no condition on the border
    with pytest.raises(InvalidParams, match="iterations"):
        st.clip_stack_local_norm(frames, warps, None, 16, SigmaClipParameters(2, 2, 0))
    with pytest.raises(InvalidParams, match="sigma_floor"):
        st.robust_clip_stack_local_norm(frames, warps, None, 16, RobustClipParameters(2, 2, -1.0, 1))
    # through the C interface: both clips or neither, a NULL out, a reserved field
    small, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(small.numpy())
    out = np.zeros((96, 128, 3), F)
    img = _ffi.ImageF32(C.c_void_p(out.ctypes.data), 128, 96, 3, 0, 0)
    p, ecc, kp = LocalNormParameters(step=16)._c(), ECC._c(), KP._c()
    sc, rc = SigmaClipParameters()._c(), RobustClipParameters()._c()
    dropped = C.c_int32(0)
    lib, fr = st._lib, C.byref(m.c_frames)
    for a, b in ((C.byref(sc), C.byref(rc)), (None, None)):
        assert lib.stk_ecc_match_local_normalized_clipped(st._h, fr, C.byref(ecc), 0.0, C.byref(p), a, b, None, C.byref(img), None, None,
                                                          None, None, None) == 2
        assert b"exactly one" in lib.stk_last_error(st._h)
        assert lib.stk_keypoint_match_local_normalized_clipped(st._h, fr, C.byref(kp), 0.0, C.byref(p), a, b, None, C.byref(img),
                                                               C.byref(dropped), None, None, None, None, None) == 2
    assert lib.stk_ecc_match_local_normalized_clipped(st._h, fr, C.byref(ecc), 0.0, C.byref(p), C.byref(sc), None, None, None, None, None,
                                                      None, None, None) == 2                       # NULL out
    assert lib.stk_ecc_match_local_normalized_clipped(st._h, fr, C.byref(ecc), 0.0, None, C.byref(sc), None, None, C.byref(img), None,
                                                      None, None, None, None) == 2                 # NULL norm
    for k in (0, 1):
        p.reserved[k] = 1
        assert lib.stk_ecc_match_local_normalized_clipped(st._h, fr, C.byref(ecc), 0.0, C.byref(p), None, C.byref(rc), None, C.byref(img),
                                                          None, None, None, None, None) == 2
        p.reserved[k] = 0
    Md = np.stack([np.eye(3)] * 3)
    bv = np.zeros(4)
    assert lib.stk_clip_stack_local_norm(st._h, fr, C.c_void_p(Md.ctypes.data), None, 0, BORDER_CONSTANT, C.c_void_p(bv.ctypes.data),
                                         1.0 / 255.0, C.byref(sc), None, None, 16, 1, None, None, None) == 2      # NULL out
    for bad in (dict(step=12), dict(stat_step=65), dict(normalize=4), dict(fill=17)):
        q = LocalNormParameters(**{**dict(step=16), **bad})
        with pytest.raises(InvalidParams):
            st.ecc_match_local_normalized_clipped(small, ECC, q, SigmaClipParameters())
        with pytest.raises(InvalidParams):
            st.keypoint_match_local_normalized_clipped(small, KP, q, RobustClipParameters())
    # N > 4096 for the median / MAD form: refused before anything is allocated or read; the sigma clip has no such limit
    n = 4097
    with pytest.raises(NotImplementedYet, match="4096"):
        st.robust_clip_stack_local_norm(np.zeros((n, 8, 8, 1), np.uint8), [np.eye(3)] * n, None, 8)
    with pytest.raises(NotImplementedYet, match="4096"):
        st.ecc_match_local_normalized_clipped(np.zeros((n, 8, 8, 3), np.uint8), ECC, LocalNormParameters(step=8), RobustClipParameters())


# ---- 9. neighbours ------------------------------------------------------------------------------------------------------------
def test_other_calls_are_unchanged_around_the_new_ones(st):
    frames, _ = synth.make_stack(5, 256, 192, device="cuda")
    clip, mad = SigmaClipParameters(2.0, 2.5, 2), RobustClipParameters(2.0, 2.5, FLOOR, 2)
    np_ = LocalNormParameters(step=32)
    wts = [1, 2, 0.5, 1, 1]

    def others():
        plain, stats = st.ecc_match(frames, ECC, return_stats=True)
        kd, kout = st.keypoint_match(frames, KP)
        return [_np(plain), np.stack([s["warp"] for s in stats]), np.array(kd), _np(kout)] + \
            [_np(v) for v in st.ecc_match_clipped(frames, ECC, clip, return_counts=True)] + \
            [_np(v) for v in st.ecc_match_robust_clipped(frames, ECC, mad, return_counts=True)] + \
            [_np(v) for v in st.ecc_match_local_normalized(frames, ECC, np_, None, wts, return_den=True)] + \
            [_np(v) for v in st.ecc_match_local_normalized(frames, ECC, np_, 0.5, wts, return_counts=True)]

    before = others()
    st.ecc_match_local_normalized_clipped(frames, ECC, np_, clip, wts)
    st.ecc_match_local_normalized_clipped(frames, ECC, np_, mad, wts)
    st.keypoint_match_local_normalized_clipped(frames, KP, np_, clip, wts)
    st.keypoint_match_local_normalized_clipped(frames, KP, np_, mad, wts)
    after = others()
    assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after))


# ---- 10. quality on the device -------------------------------------------------------------------------------------------
def test_device_quality_is_the_restatements(st):
    """The device's RMS error against the scene on quality_stack(1) (step 16, stat_step 2, LINEAR, min_count 16, fill 4,
    coverage 1; caller-held integer warps) lies within 1 % of the restatement's, for both clips."""
    from local_norm_restate import integer_shift_samples
    q = quality_restated(1)
    rplanes, frames, warps, truth = q[4], q[7], q[8], q[9]
    s, k = integer_shift_samples(frames, warps)
    part = k == 1
    rmad = quality_rms(norm_robust_clip_restate(s, part, rplanes, 16, 3, 3, FLOOR, 2)[0], truth)
    rsig = quality_rms(norm_clip_restate(s, part, rplanes, 16, 2, 2, 2)[0], truth)
    stack = [f[..., None] for f in frames]
    np_ = LocalNormParameters(step=16, stat_step=2, normalize=LINEAR, coverage=True, min_count=16, fill=4)
    mom = st.local_moments(stack, list(warps), 16, stat_step=2)
    h, w = frames[0].shape
    planes = [None] + [local_norm_estimate(w, h, 1, mom[i], np_) for i in range(1, len(stack))]
    dmad = quality_rms(st.robust_clip_stack_local_norm(stack, list(warps), planes, 16, RobustClipParameters(3, 3, FLOOR, 2)), truth)
    dsig = quality_rms(st.clip_stack_local_norm(stack, list(warps), planes, 16, SigmaClipParameters(2, 2, 2)), truth)
    print(f"quality_stack(1): median/MAD clip device {dmad:.4f} restatement {rmad:.4f}; sigma clip device {dsig:.4f} restatement {rsig:.4f}")
    assert abs(dmad - rmad) <= 0.01 * rmad
    assert abs(dsig - rsig) <= 0.01 * rsig

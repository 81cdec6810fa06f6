"""The bicubic fold (option "warp_interpolation" = INTER_CUBIC; definition: include/stacker.h, "Bicubic fold") on the GPU:
the option, exact known answers, the f64 restatement (interp_restate.py), u8 BGR against the same values as float
frames, every combine fed with the cubic sample, the whole-stack calls against their parts, and the quality gain the
feature exists for. Two frame shapes: 37 x 131 (row bytes no multiple of 4, width no multiple of 64, height no multiple
of 4) and 36 x 132 (dword-aligned rows)."""
import contextlib
import zlib

import numpy as np
import pytest

import interp_restate as ir
from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_WRAP, RANSAC,
                               EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType, SigmaClipParameters,
                               Stacker, WeightParameters, synth)
from libstacker_rs_amd.api import INTER_CUBIC, INTER_LINEAR
from test_cpu_clip import clip_restate
from test_cpu_interp import restated_quality
from test_cpu_quantile import quantile_restate
from test_cpu_robust import robust_clip_restate, robust_quantile_restate
from test_cpu_weighted import LINEAR, weighted_restate
from test_gpu_weighted import _exact_moments, engine_kappa, engine_samples, random_frames, shifted_warps

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(37, 131), (36, 132)]
BORDERS = [BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101]
ALPHA = {np.uint8: 1.0 / 255.0, np.uint16: 1.0 / 65535.0, np.float32: 1.0}
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
# test_gpu_stages.H_CASES, restated
H_CASES = {
    "projective": np.array([[1.01, 0.02, -3.3], [-0.015, 0.99, 4.1], [2e-5, -1e-5, 1.0]]),
    "big_rotation": np.array([[0.8, -0.6, 40.0], [0.6, 0.8, -30.0], [0, 0, 1.0]]),
}
# (dtype, channels, border mode, border value): the u8 BGR BORDER_CONSTANT configuration and two generic ones
KINDS = [(np.uint8, 3, BORDER_CONSTANT, (0, 0, 0, 0)), (np.float32, 4, BORDER_REPLICATE, (0, 0, 0, 0)),
         (np.uint16, 1, BORDER_REFLECT_101, (0, 0, 0, 0))]
KIND_IDS = ["u8c3-constant", "f32c4-replicate", "u16c1-reflect101"]


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


@contextlib.contextmanager
def cubic(st):
    st.set_option("warp_interpolation", INTER_CUBIC)
    try:
        yield
    finally:
        st.set_option("warp_interpolation", INTER_LINEAR)


def shift(sx, sy):
    M = np.eye(3)
    M[0, 2], M[1, 2] = sx, sy
    return M


def both(st, frame, M, **kw):
    lin = np.asarray(st.warp_accumulate(frame, M, **kw))
    with cubic(st):
        cub = np.asarray(st.warp_accumulate(frame, M, **kw))
    return lin, cub


# ---- 1. the option ----------------------------------------------------------------------------------------------------
def test_option_values_default_and_the_subpixel_conflict(st):
    rng = np.random.default_rng(1)
    h, w = SHAPES[0]
    frame = random_frames(rng, 1, h, w, 3, np.uint8)[0]
    M = H_CASES["projective"]
    fresh = Stacker(0)
    try:
        never = np.asarray(fresh.warp_accumulate(frame, M))
        fresh.set_option("warp_interpolation", INTER_LINEAR)
        one = np.asarray(fresh.warp_accumulate(frame, M))
        fresh.set_option("warp_interpolation", INTER_CUBIC)
        two = np.asarray(fresh.warp_accumulate(frame, M))
        fresh.set_option("warp_interpolation", INTER_LINEAR)
        back = np.asarray(fresh.warp_accumulate(frame, M))
        for v in (0, 3, 4):
            with pytest.raises(InvalidParams, match="warp_interpolation"):
                fresh.set_option("warp_interpolation", v)
        assert np.array_equal(np.asarray(fresh.warp_accumulate(frame, M)), never)      # a refused value changes nothing
    finally:
        fresh.close()
    assert np.array_equal(never, one) and np.array_equal(never, back)
    assert not np.array_equal(never, two)
    # cubic is defined on exact coordinates only; the pair is checked at the call, in either order of setting
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    warps = [np.eye(3)] * 3
    calls = {"warp_accumulate": lambda: st.warp_accumulate(frame, M), "clip_stack": lambda: st.clip_stack(frames, warps),
             "quantile_stack": lambda: st.quantile_stack(frames, warps), "weighted_stack": lambda: st.weighted_stack(frames, warps),
             "ecc_match": lambda: st.ecc_match(frames, ECC)}
    for order in ((("warp_interpolation", INTER_CUBIC), ("warp_subpixel_bits", 5)), (("warp_subpixel_bits", 5), ("warp_interpolation", INTER_CUBIC))):
        try:
            for name, v in order:
                st.set_option(name, v)
            for what, call in calls.items():
                with pytest.raises(InvalidParams, match="warp_interpolation.*warp_subpixel_bits"):
                    call()
            st.grey(frame)                                   # a call that does not fold is not concerned
        finally:
            st.set_option("warp_subpixel_bits", 0)
            st.set_option("warp_interpolation", INTER_LINEAR)
    for call in calls.values():
        call()


# ---- 2. integer translations: the linear fold's bits on every pixel ---------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_integer_translations_give_the_linear_bits(st, dtype):
    rng = np.random.default_rng(2)
    h, w = SHAPES[0]
    for cn in (1, 3, 4):
        frame = random_frames(rng, 1, h, w, cn, dtype)[0]
        for border in BORDERS:
            for affine in (False, True):
                for sx, sy in ((5, -3), (-2, 4)):
                    M = shift(sx, sy)[:2] if affine else shift(sx, sy)
                    lin, cub = both(st, frame, M, is_affine=affine, border_mode=border, border_value=(0.25, 0.5, 0.75, 0.125),
                                    alpha=ALPHA[dtype])
                    assert np.array_equal(lin, cub), (cn, border, affine, sx, sy)
                    assert np.isfinite(cub).all()


# ---- 3. half-pixel translations: the exact known answer ---------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["37x131", "36x132"])
@pytest.mark.parametrize("dtype,cn,top", [(np.uint8, 3, 255), (np.uint8, 1, 255), (np.uint16, 3, 4095), (np.uint16, 1, 4095)])
def test_half_pixel_translations_are_exact(st, shape, dtype, cn, top):
    h, w = shape
    rng = np.random.default_rng(3)
    frame = rng.integers(0, top + 1, (h, w, cn)).astype(dtype)        # top * 44^2 < 2^24: every partial sum is exact in f32
    half, whole = np.array([-3, 19, 19, -3], np.int64), np.array([0, 32, 0, 0], np.int64)
    for sx, sy in ((0.5, 0.5), (0.5, 0.0), (0.0, 0.5), (2.5, -1.5)):
        lin, cub = both(st, frame, shift(sx, sy), alpha=1.0)
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        inside, ix, iy, tx, ty = ir.footprint(x - sx, y - sy, h, w)
        assert inside.mean() > 0.8
        taps = ir.gather(frame, ix[inside], iy[inside]).astype(np.int64)
        exact = np.einsum("r,k,ncrk->nc", half if sy % 1 else whole, half if sx % 1 else whole, taps)
        assert np.array_equal(cub[inside].astype(np.float64) * 1024.0, exact.astype(np.float64)), (sx, sy)
        assert np.array_equal(cub[~inside], lin[~inside]), (sx, sy)
        assert (cub[inside] != lin[inside]).any()


# ---- 4. against the f64 restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["37x131", "36x132"])
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_eighth_pixel_translations_against_the_f64_restatement(st, kind, shape):
    """Coordinates that are exact in f32: nothing is excluded. Footprint inside: within 2^-19 V of the definition in f64
    (<= 27 roundings of 2^-24 * 1.375^2 V; V: the footprint's largest |tap * alpha|). Elsewhere: the linear bits."""
    dtype, cn, border, bv = kind
    h, w = shape
    rng = np.random.default_rng(4)
    frame = random_frames(rng, 1, h, w, cn, dtype)[0]
    worst = 0.0
    for sx, sy in ((2.125, -1.375), (0.875, 3.5), (-4.25, 0.625), (-0.125, -0.125)):
        kw = dict(border_mode=border, border_value=bv, alpha=ALPHA[dtype])
        lin, cub = both(st, frame, shift(sx, sy), **kw)
        ref, inside, V, _, _ = ir.warp(frame, shift(sx, sy), False, F(ALPHA[dtype]), lin)
        err = np.abs(cub.astype(np.float64) - ref)[inside] / V[inside][:, None]
        worst = max(worst, err.max())
        assert err.max() <= 2.0 ** -19, (sx, sy, err.max())
        assert np.array_equal(cub[~inside], lin[~inside]), (sx, sy)
        assert inside.mean() > 0.6 and (~inside).any()
    print("eighth-pixel translations: worst", worst / 2.0 ** -24, "x 2^-24 V")


@pytest.mark.parametrize("shape", SHAPES, ids=["37x131", "36x132"])
@pytest.mark.parametrize("name", list(H_CASES))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_projective_maps_against_the_f64_restatement(st, kind, name, shape):
    """The engine's f32 coordinates differ from the f64 ones by <= 3 ulp of 256 (4.6e-5 px), so pixels within 1e-3 px of
    a line where the footprint test switches the formula (X = 1, X = sw - 2, Y = 1, Y = sh - 2) are left out: at most
    1 % of the pixels. (The rotation's entries 0.8 / 0.6 put whole families of pixels ON such lines: 0.65 % here. The
    frame's own edge lines need no exclusion: on both sides of them the cubic fold is the engine's linear sample, which
    is compared bit for bit.) The slope of the kernel is <= 3 V per px and axis."""
    dtype, cn, border, bv = kind
    h, w = shape
    rng = np.random.default_rng(5)
    frame = random_frames(rng, 1, h, w, cn, dtype)[0]
    M = H_CASES[name]
    kw = dict(border_mode=border, border_value=bv, alpha=ALPHA[dtype])
    lin, cub = both(st, frame, M, **kw)
    ref, inside, V, X, Y = ir.warp(frame, M, False, F(ALPHA[dtype]), lin)     # V: per pixel, the footprint's largest |tap * alpha|
    near = np.zeros((h, w), bool)
    for C_, n_ in ((X, w), (Y, h)):
        for line in (1, n_ - 2):
            near |= np.abs(C_ - line) < 1e-3
    assert near.mean() <= 0.01, near.mean()
    m = inside & ~near
    assert m.mean() > 0.15, m.mean()
    err = np.abs(cub.astype(np.float64) - ref)[m] / V[m][:, None]
    print(name, "worst", err.max(), "V; share inside", m.mean(), "left out", near.mean())
    assert err.max() <= 2.0 ** -19 + 6 * 4.6e-5
    o = ~inside & ~near
    assert np.array_equal(cub[o], lin[o])


# ---- 5. u8 BGR BORDER_CONSTANT against the same values as a float frame, every pixel ------------------------------------
def _matrices(rng, w, h):
    return [(np.eye(3), False), (synth.random_homography(rng, w, h, 8.0), False), (synth.random_homography(rng, w, h, 30.0), False),
            (np.array([[0.7, 0.2, 15.3], [-0.25, 0.9, 40.1], [4e-4, -3e-4, 1.0]]), False),          # strong perspective
            (np.array([[1e-3, 0, 0], [0, 1e-3, 0], [0, 0, 1e-3]]), False),                            # tiny W
            (np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1e-20]]), False),                                 # leaves the shared reciprocal chain
            (np.array([[1, 0, 0], [0, 1, 0], [-0.02, 0, 1.0]]), False),                               # W changes sign inside the image
            (np.diag([1e-39, 1.0, 1.0]), False),                                                      # inf * 0 = NaN coordinates
            (np.array([[1, 0, 1e30], [0, 1, 0], [0, 0, 1.0]]), False),                                # huge finite coordinates
            (np.array([[1.0, 0.01, np.nan], [0.0, 1.0, 3.0]]), True),                                 # affine, NaN translation
            (np.array([[1.0, 0.01, 2.5], [0.02, 1.0, -3.25]]), True)]


@pytest.mark.parametrize("shape", SHAPES, ids=["37x131", "36x132"])
def test_u8_bgr_equals_the_float_frame_everywhere(st, shape):
    h, w = shape
    rng = np.random.default_rng(6)
    frame = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    as_f32 = frame.astype(np.float32)
    with cubic(st):
        for M, aff in _matrices(rng, w, h):
            for value in ((0, 0, 0, 0), (0.25, 0.5, 0.75, 0.0)):
                a = np.asarray(st.warp_accumulate(frame, M, is_affine=aff, border_value=value))
                b = np.asarray(st.warp_accumulate(as_f32, M, is_affine=aff, border_value=value))
                assert np.array_equal(a, b), (M, value)
                assert np.isfinite(a).all()


@pytest.mark.parametrize("shape", SHAPES, ids=["37x131", "36x132"])
def test_seven_frame_folds_u8_equal_float_and_padded_equals_tight(st, shape):
    import torch
    h, w = shape
    rng = np.random.default_rng(7)
    n = 7
    frames = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    floats = frames.astype(np.float32)
    warps = shifted_warps(rng, n, False)
    # a padded, misaligned device stack: row stride = row bytes + 5, every frame's base at an odd offset
    rs = w * 3 + 5
    buf = torch.from_numpy(rng.integers(0, 256, n * h * rs + 16, dtype=np.uint8)).cuda()
    padded = []
    for i in range(n):
        v = torch.as_strided(buf, (h, w, 3), (rs, 3, 1), 1 + i * h * rs)
        v.copy_(torch.from_numpy(frames[i]).cuda())
        assert v.data_ptr() % 2 == (buf.data_ptr() + 1 + i * h * rs) % 2
        padded.append(v)
    tight = torch.from_numpy(frames).cuda()
    clip = SigmaClipParameters(2.0, 2.5, 2)
    with cubic(st):
        # the accumulating mean fold
        acc8 = accf = accp = None
        for i in range(n):
            acc8 = st.warp_accumulate(frames[i], warps[i], acc=acc8)
            accf = st.warp_accumulate(floats[i], warps[i], acc=accf)
            accp = st.warp_accumulate(padded[i], warps[i], acc=accp)
        assert np.array_equal(np.asarray(acc8), np.asarray(accf))
        assert np.array_equal(accp.cpu().numpy(), np.asarray(acc8))
        # seven frames in one launch, through three states
        for call in (lambda f: st.weighted_stack(f, warps, coverage=False), lambda f: st.weighted_stack(f, warps, coverage=True),
                     lambda f: st.clip_stack(f, warps, clip), lambda f: st.quantile_stack(f, warps, 0.5)):
            a, b = np.asarray(call(frames)), np.asarray(call(floats))
            assert np.array_equal(a, b)
            assert np.array_equal(call(tight).cpu().numpy(), a)
            assert np.array_equal(call(padded).cpu().numpy(), a)


# ---- 6. every combine sees the cubic sample ------------------------------------------------------------------------------
def _every_combine(st, kind, shape, n, affine, interp, reach, steps, seed):
    """Every combine built on the fold with a u8 BGR fast state (the clip, the weighted mean, the moments, the two quantile
    stores; with and without normalisation) under `interp`, each against its restatement on the engine's own samples."""
    dtype, cn, border, bv = kind
    h, w = shape
    rng = np.random.default_rng(zlib.crc32(seed.encode()))
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine, reach=reach)
    idx = list(range(n))
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[2] = 0.0
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=ALPHA[dtype])
    clip = SigmaClipParameters(2.0, 2.5, 2)
    # kappa is the linear fold's by definition (a cubic sample of an all-ones frame need not round to 1.0f)
    kappa = engine_kappa(st, (h, w), warps, idx, affine)
    linear_samples = engine_samples(st, frames, warps, idx, **kw)
    covs = (False, True) if border == BORDER_CONSTANT else (False,)
    got = {}
    with (cubic(st) if interp == INTER_CUBIC else contextlib.nullcontext()):
        samples = engine_samples(st, frames, warps, idx, **kw)
        got["clip"] = st.clip_stack(frames, warps, clip, return_counts=True, **kw)
        for q in (0.5, 0.9):
            got["q", q] = st.quantile_stack(frames, warps, q, **kw)
        for cov in covs:
            got["w", cov] = st.weighted_stack(frames, warps, g, o, wt, coverage=cov, return_coverage=True, **kw)
            got["cw", cov] = st.clip_stack_weighted(frames, warps, clip, g, o, wt, coverage=cov, return_counts=True,
                                                    return_kept_weight=True, **kw)
            got["qw", cov] = st.quantile_stack_weighted(frames, warps, 0.5, g, o, wt, coverage=cov, return_counts=True, **kw)
        for step in steps:
            got["m", step] = st.overlap_moments(frames, warps, stat_step=step, **kw)
    full = kappa == F(1.0)
    assert (~full).mean() >= 0.03, (~full).mean()            # the rim is a real share of the (pixel, entry) pairs
    assert np.array_equal(samples, linear_samples) == (interp == INTER_LINEAR)
    ref, ref_k = clip_restate(samples, clip.kappa_low, clip.kappa_high, clip.iterations)
    assert np.array_equal(got["clip"][0], ref, equal_nan=True) and np.array_equal(got["clip"][1], ref_k)
    for q in (0.5, 0.9):
        assert np.array_equal(got["q", q], quantile_restate(samples, q), equal_nan=True), q
    for cov in covs:
        ref, ref_den = weighted_restate(samples, kappa if cov else np.ones_like(kappa), g, o, wt)
        assert np.array_equal(got["w", cov][1], ref_den) and np.array_equal(got["w", cov][0], ref, equal_nan=True), cov
        part = full if cov else np.ones_like(full)
        ref, ref_k, ref_sw = robust_clip_restate(samples, part, g, o, wt, clip.kappa_low, clip.kappa_high, clip.iterations)
        out, cnt, kept = got["cw", cov]
        assert np.array_equal(cnt, ref_k) and np.array_equal(kept, ref_sw) and np.array_equal(out, ref, equal_nan=True), cov
        qref, qn = robust_quantile_restate(samples, part, g, o, wt, 0.5)
        assert np.array_equal(got["qw", cov][1], qn) and np.array_equal(got["qw", cov][0], qref, equal_nan=True), cov
    u = 2.0 ** -53
    for step in steps:
        exact, mag = _exact_moments(samples, kappa, step)
        mom = got["m", step]
        for i in range(1, n):
            cnt = exact[i, 0, 0]
            assert (mom[i, :, 0] == cnt).all(), (step, i)
            gamma = (cnt - 1) * u / (1 - (cnt - 1) * u) if cnt > 1 else 0.0
            assert (np.abs(mom[i] - exact[i]) <= gamma * mag[i]).all(), (step, i)
        assert any(exact[i, 0, 0] > 50 for i in range(1, n))


@pytest.mark.parametrize("kind", KINDS[:2], ids=KIND_IDS[:2])
def test_every_combine_sees_the_cubic_sample(st, kind):
    _every_combine(st, kind, SHAPES[0], 7, False, INTER_CUBIC, 6.0, (1, 3), str(kind))


# Which kernel a combine runs is decided by one launcher (fold_launch.h) and one (depth, cn) ladder: every cell of
# depth x channels x interpolation x motion model, for all six combines at once. 70 x 6: the 64-wide and the 4-row tile both
# have a ragged second tile; 5 frames: a clip still has k >= 3 after one rejection. (DESIGN.md 4.19 has the table.)
@pytest.mark.parametrize("interp", [INTER_LINEAR, INTER_CUBIC], ids=["linear", "cubic"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "persp"])
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_every_combine_at_every_launcher_cell(st, dtype, cn, affine, interp):
    kind = (dtype, cn, BORDER_CONSTANT, (0, 0, 0, 0))
    _every_combine(st, kind, (6, 70), 5, affine, interp, 2.0, (1, 2), f"cell {np.dtype(dtype).name} {cn} {affine} {interp}")


# u8 BGR where the fast state does not apply (any border mode but BORDER_CONSTANT): the launcher then takes the generic cubic
# kernel at <uint8_t, 3> with the combine's generic state, which the cells above (BORDER_CONSTANT: the cubic u8 BGR kernel)
# never reach. The same 70 x 6 destinations and 5 frames.
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "persp"])
def test_every_combine_under_cubic_where_u8_bgr_takes_the_generic_kernel(st, affine):
    kind = (np.uint8, 3, BORDER_REPLICATE, (0, 0, 0, 0))
    _every_combine(st, kind, (6, 70), 5, affine, INTER_CUBIC, 2.0, (1, 2), f"generic u8 bgr cubic {affine}")


# ---- 7. whole-stack calls equal their parts ----------------------------------------------------------------------------
def _mean_of_parts(st, frames, stats, n_total, **kw):
    """The mean fold in fold order (frame 0, then the kept frames in ascending index) by single-frame accumulates."""
    acc, count = None, 0
    for i in range(n_total):
        if i == 0 or stats[i]["status"] == 0:
            acc = st.warp_accumulate(frames[i], stats[i]["warp"], acc=acc, **kw)
            count += 1
    return st.finalize_mean(acc, count), count


def _same_alignment(a, b, keys):
    for x, y in zip(a, b):
        for k in keys:
            assert x[k] == y[k], k
        assert np.array_equal(x["warp"], y["warp"])


def test_ecc_calls_equal_their_parts_under_cubic(st):
    frames, _ = synth.make_stack(6, 128, 96, device="cuda")
    n = frames.shape[0]
    clip = SigmaClipParameters(2.0, 2.5, 2)
    wp = WeightParameters(LINEAR, True, 2)
    lin, lstats = st.ecc_match(frames, ECC, return_stats=True)
    with cubic(st):
        cub, cstats = st.ecc_match(frames, ECC, return_stats=True)
        parts, count = _mean_of_parts(st, list(frames.unbind(0)), cstats, n)
        cout, ccnt, clstats = st.ecc_match_clipped(frames, ECC, clip, return_stats=True, return_counts=True)
        warps = [s["warp"] for s in cstats]
        cref, cref_k = st.clip_stack(frames, warps, clip, return_counts=True)
        wout, wcov, applied, wstats = st.ecc_match_weighted(frames, ECC, wp, return_stats=True, return_coverage=True, return_applied=True)
        wref, wref_cov = st.weighted_stack(frames, warps, applied=applied, coverage=True, return_coverage=True)
    keys = ("status", "iterations", "rho")
    _same_alignment(cstats, lstats, keys)
    _same_alignment(clstats, lstats, keys)
    _same_alignment(wstats, lstats, keys)
    assert count >= 2                                       # at least one moving frame converged and was folded
    assert np.array_equal(cub.cpu().numpy(), parts.cpu().numpy())
    assert not np.array_equal(cub.cpu().numpy(), lin.cpu().numpy())
    assert np.array_equal(cout.cpu().numpy(), cref.cpu().numpy()) and np.array_equal(ccnt.cpu().numpy(), cref_k.cpu().numpy())
    assert np.array_equal(wout.cpu().numpy(), wref.cpu().numpy()) and np.array_equal(wcov.cpu().numpy(), wref_cov.cpu().numpy())
    assert not np.array_equal(cref.cpu().numpy(), st.clip_stack(frames, warps, clip).cpu().numpy())      # (linear again)


def test_keypoint_match_equals_its_parts_under_cubic(st):
    frames, _ = synth.make_stack(6, 128, 96)
    stack = list(frames.numpy())
    stack[3] = np.full_like(stack[0], 128)                  # featureless: dropped
    n = len(stack)
    ldrop, lin, lstats = st.keypoint_match(stack, KP, return_stats=True)
    with cubic(st):
        cdrop, cub, cstats = st.keypoint_match(stack, KP, return_stats=True)
        kept = [i for i in range(n) if i == 0 or cstats[i]["status"] == 0]
        acc = None
        for i in kept:
            acc = st.warp_accumulate(stack[i], cstats[i]["warp"], acc=acc)
    _same_alignment(cstats, lstats, ("status", "n_matches"))
    assert cdrop == ldrop == n - len(kept) and cstats[3]["status"] != 0
    assert len(kept) >= 2                                   # at least one moving frame was folded
    parts = np.asarray(acc) * F(1.0 / len(kept))
    assert np.array_equal(np.asarray(cub), parts)
    assert not np.array_equal(np.asarray(cub), np.asarray(lin))


# ---- 8. it does what it is for ---------------------------------------------------------------------------------------------
def test_cubic_stack_is_closer_to_the_scene(st):
    seed = 7
    frames, warps, scene = ir.quality_stack(seed)
    n, h, w, _ = frames.shape
    m = np.zeros((h, w), bool)
    m[5:h - 5, 5:w - 5] = True
    lin = np.asarray(st.weighted_stack(frames, warps, coverage=False, alpha=1.0))[..., 0]
    with cubic(st):
        cub = np.asarray(st.weighted_stack(frames, warps, coverage=False, alpha=1.0))[..., 0]
    rms = lambda img: float(np.sqrt(np.mean((img[m].astype(np.float64) - scene[m]) ** 2)))
    rl, rc = restated_quality(seed)
    print("quality: engine linear", rms(lin), "cubic", rms(cub), "restated", rl, rc, "ratio", rc / rl)
    assert rc / rl < 0.25
    assert abs(rms(lin) - rl) <= 0.01 * rl and abs(rms(cub) - rc) <= 0.01 * rc

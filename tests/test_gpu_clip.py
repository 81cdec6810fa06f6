"""Sigma-clipped stacking on the GPU: stk_clip_stack / stk_ecc_match_clipped / stk_keypoint_match_clipped against the numpy
restatement of the definition (test_cpu_clip.clip_restate), whose samples come from the engine's own single-frame warp
(Stacker.warp_accumulate with the same matrices)."""
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, MotionType, SigmaClipParameters, Stacker, synth)
from test_cpu_clip import clip_restate

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


_ALPHA = {np.uint8: 1.0 / 255.0, np.uint16: 1.0 / 65535.0, np.float32: 1.0}
_SCALE = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}


def outlier_frames(rng, n, h, w, cn, dtype):
    """n noisy copies of one random scene, each with ~3 % of its pixels replaced by bright or dark outliers."""
    base = rng.random((h, w, cn))
    frames = []
    for _ in range(n):
        f = base + rng.normal(0, 0.02, base.shape)
        hot = rng.random((h, w)) < 0.03
        f[hot] = rng.choice([0.0, 1.0], size=(int(hot.sum()), 1))
        f = np.clip(f, 0, 1) * _SCALE[dtype]
        frames.append(np.rint(f).astype(dtype) if dtype != np.float32 else f.astype(np.float32))
    return frames


def small_warps(rng, n, affine):
    Ms = [np.eye(3)]
    for _ in range(1, n):
        M = np.eye(3)
        M[:2, :2] += rng.normal(0, 4e-3, (2, 2))
        M[:2, 2] = rng.uniform(-1.5, 1.5, 2)
        if not affine:
            M[2, :2] = rng.normal(0, 2e-5, 2)
        Ms.append(M)
    return Ms


def restated(st, frames, warps, include, clip, **kw):
    idx = [i for i in range(len(frames)) if include is None or include[i]]
    samples = np.stack([np.asarray(st.warp_accumulate(frames[i], warps[i], acc=None, **kw)) for i in idx])
    return clip_restate(samples, clip.kappa_low, clip.kappa_high, clip.iterations)


# (depth, channels, affine, border, border value, subpixel bits, iterations, kappas, (h, w))
CASES = [
    (np.uint8, 3, False, BORDER_CONSTANT, (0.25, 0.5, 0.75, 0), 0, 1, (2.0, 2.5), (45, 131)),    # u8 BGR fast kernel
    (np.uint8, 3, True, BORDER_CONSTANT, (0, 0, 0, 0), 0, 3, (1.5, 3.0), (40, 200)),             # fast kernel, affine
    (np.uint8, 3, False, BORDER_CONSTANT, (0, 0, 0, 0), 0, 3, (2.0, 2.0), (1, 65)),              # one-row frame: generic
    (np.uint8, 3, False, BORDER_REPLICATE, (0, 0, 0, 0), 0, 3, (2.5, 1.5), (33, 97)),
    (np.uint8, 4, True, BORDER_CONSTANT, (0.1, 0.2, 0.3, 0.4), 5, 1, (2.0, 3.0), (31, 77)),
    (np.uint16, 3, False, BORDER_CONSTANT, (0.5, 0.5, 0.5, 0), 5, 3, (2.0, 2.5), (29, 67)),
    (np.uint16, 4, True, BORDER_REPLICATE, (0, 0, 0, 0), 0, 1, (3.0, 2.0), (27, 63)),
    (np.float32, 3, True, BORDER_CONSTANT, (0.3, 0.6, 0.9, 0), 0, 3, (1.5, 2.0), (25, 71)),
    (np.float32, 4, False, BORDER_REPLICATE, (0, 0, 0, 0), 5, 1, (2.0, 2.0), (23, 69)),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-T{c[6]}-{c[8][0]}x{c[8][1]}" for c in CASES])
def test_clip_stack_matches_restatement(st, case):
    dtype, cn, affine, border, bv, sub, T, (kl, kh), (h, w) = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    n = 11
    frames = outlier_frames(rng, n, h, w, cn, dtype)
    warps = small_warps(rng, n, affine)
    include = [1] * n
    include[4] = 0
    clip = SigmaClipParameters(kl, kh, T)
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype])
    st.set_option("warp_subpixel_bits", sub)
    try:
        ref, ref_k = restated(st, frames, warps, include, clip, **kw)
        out, cnt = st.clip_stack(frames, warps, clip, include, return_counts=True, **kw)
        import torch
        dframes = torch.from_numpy(np.stack(frames)).cuda()
        dout, dcnt = st.clip_stack(dframes, warps, clip, include, return_counts=True, **kw)
    finally:
        st.set_option("warp_subpixel_bits", 0)
    assert np.array_equal(out, ref) and np.array_equal(cnt, ref_k)
    assert np.array_equal(dout.cpu().numpy(), ref) and np.array_equal(dcnt.cpu().numpy(), ref_k)
    assert cnt.min() < n - 1 and (cnt < n - 1).mean() > 0.01      # rejection happened


def _clip_of(st, frames, stats, clip, include=None, **kw):
    warps = [s["warp"] for s in stats]
    return st.clip_stack(frames, warps, clip, include, return_counts=True, **kw)


def test_ecc_match_clipped_equals_clip_stack_on_its_warps(st):
    frames, _ = synth.make_stack(6, 256, 192, device="cuda")
    clip = SigmaClipParameters(2.0, 2.5, 2)
    out, cnt, stats = st.ecc_match_clipped(frames, ECC, clip, return_stats=True, return_counts=True)
    plain, pstats = st.ecc_match(frames, ECC, return_stats=True)
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["rho"] == b["rho"]
        assert np.array_equal(a["warp"], b["warp"])
    ref, ref_k = _clip_of(st, frames, stats, clip)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(cnt.cpu().numpy(), ref_k.cpu().numpy())
    # host-fed: the same bits, outputs on the host
    hout, hcnt = st.ecc_match_clipped(frames.cpu().numpy(), ECC, clip, return_counts=True)
    assert np.array_equal(hout, out.cpu().numpy()) and np.array_equal(hcnt, cnt.cpu().numpy())
    # the clip passes' device time is reported
    assert st.timing()["finalize_ms"] > 0


def test_keypoint_match_clipped_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 640, 480)
    frames = frames.numpy()
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    clip = SigmaClipParameters(2.0, 2.0, 1)
    dropped, out, cnt, stats = st.keypoint_match_clipped(stack, KP, clip, return_stats=True, return_counts=True)
    pd, plain, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["n_matches"] == b["n_matches"] and np.array_equal(a["warp"], b["warp"])
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    ref, ref_k = _clip_of(st, stack, stats, clip, include)
    assert np.array_equal(out, ref) and np.array_equal(cnt, ref_k)
    assert cnt.max() == 4


def test_huge_kappas_give_the_plain_mean(st):
    frames, _ = synth.make_stack(5, 256, 192, device="cuda")
    clip = SigmaClipParameters(1e30, 1e30, 2)
    out, cnt = st.ecc_match_clipped(frames, ECC, clip, return_counts=True)
    plain = st.ecc_match(frames, ECC)
    assert (cnt == 5).all()
    assert (out - plain).abs().max().item() <= 1e-6


def test_streaks_and_hot_pixels_are_rejected(st):
    n, w, h = 24, 320, 240
    frames, _ = synth.make_stack(n, w, h)
    clean = frames.numpy()
    dirty = clean.copy()
    dirty[5, 100:103, 40:280] = 255                   # a satellite trail in two frames
    dirty[17, 100:103, 40:280] = 255
    rng = np.random.default_rng(7)
    for i in (3, 9, 20):                              # and a few hot pixels (away from the trail)
        dirty[i, rng.integers(150, 200, 20), rng.integers(60, 260, 20)] = 255
    clip = SigmaClipParameters(3.0, 3.0, 2)
    _, stats = st.ecc_match(clean, ECC, return_stats=True)      # the same warps for every combine below
    warps = [s["warp"] for s in stats]
    got, cnt = st.clip_stack(dirty, warps, clip, return_counts=True)
    without = [0 if i in (5, 17) else 1 for i in range(n)]
    ref, ref_cnt = st.clip_stack(clean, warps, clip, without, return_counts=True)   # the clean stack without the two frames
    mean_dirty = st.clip_stack(dirty, warps, SigmaClipParameters(1e30, 1e30, 1))
    # streak pixels: the destination pixels whose footprint in frames 5 and 17 lies inside the streak
    inside = np.ones((h, w), bool)
    for i in (5, 17):
        ones = np.zeros((h, w, 3), np.uint8)
        ones[100:103, 40:280] = 255
        inside &= st.warp_accumulate(ones, warps[i])[..., 0] >= 1.0 - 1e-6
    # (and no sample of the clean frames rejected there; and a scene darker than the trail by more than the noise: on a
    # near-white pixel a white trail is no outlier)
    sel = inside[..., None] & (ref_cnt == n - 2) & (ref < 0.7)
    assert sel.sum() > 300
    assert (cnt[sel] == n - 2).all()
    assert np.max(np.abs(got[sel] - ref[sel])) <= 2e-6
    err = np.abs(mean_dirty[sel] - ref[sel])
    assert err.max() > 0.05 and err.mean() > 0.02


def test_options_do_not_change_a_clipped_bit(st):
    frames, _ = synth.make_stack(20, 640, 480, device="cuda")
    clip = SigmaClipParameters(2.0, 2.0, 2)
    base, bcnt = st.ecc_match_clipped(frames, ECC, clip, return_counts=True)
    for name, val in (("ecc_slots", 4), ("prep_overlap", 0)):
        st.set_option(name, val)
        try:
            o, c = st.ecc_match_clipped(frames, ECC, clip, return_counts=True)
        finally:
            st.set_option(name, 0 if name == "ecc_slots" else 1)
        assert np.array_equal(o.cpu().numpy(), base.cpu().numpy()) and np.array_equal(c.cpu().numpy(), bcnt.cpu().numpy()), name
    kres = []
    for lanes in (1, 3):
        st.set_option("kp_lanes", lanes)
        try:
            kres.append(st.keypoint_match_clipped(frames, KP, clip, return_counts=True))
        finally:
            st.set_option("kp_lanes", 3)
    assert kres[0][0] == kres[1][0]
    assert np.array_equal(kres[0][1].cpu().numpy(), kres[1][1].cpu().numpy()) and np.array_equal(kres[0][2].cpu().numpy(), kres[1][2].cpu().numpy())
    # a multi-device context runs the clipped calls on its first device: the single-device bits
    multi = Stacker(devices=[0, 0])
    try:
        mo, mc = multi.ecc_match_clipped(frames, ECC, clip, return_counts=True)
    finally:
        multi.close()
    assert np.array_equal(mo.cpu().numpy(), base.cpu().numpy()) and np.array_equal(mc.cpu().numpy(), bcnt.cpu().numpy())
    # T = 16 against a smaller T on a converged stack: the kept sets of all but a few pixels, and the same bits run to run.
    # (Not the same bits as T = 8: the centre update c + (sum of (s - c)) / k can keep moving c by an ulp from pass to
    # pass, and a sample at the edge of [L, U] can flip — DESIGN.md section 4.5.)
    o16, c16 = st.ecc_match_clipped(frames, ECC, SigmaClipParameters(2.0, 2.0, 16), return_counts=True)
    o8, c8 = st.ecc_match_clipped(frames, ECC, SigmaClipParameters(2.0, 2.0, 8), return_counts=True)
    same = (c16 == c8).cpu().numpy()
    assert same.mean() >= 0.999
    assert np.abs(o16.cpu().numpy() - o8.cpu().numpy())[same].max() <= 1e-6
    o16b, c16b = st.ecc_match_clipped(frames, ECC, SigmaClipParameters(2.0, 2.0, 16), return_counts=True)
    assert np.array_equal(o16b.cpu().numpy(), o16.cpu().numpy()) and np.array_equal(c16b.cpu().numpy(), c16.cpu().numpy())


@pytest.mark.parametrize("clip", [SigmaClipParameters(0.0, 3.0, 2), SigmaClipParameters(3.0, -1.0, 2),
                                  SigmaClipParameters(float("nan"), 3.0, 2), SigmaClipParameters(3.0, float("inf"), 2),
                                  SigmaClipParameters(3.0, 3.0, 0), SigmaClipParameters(3.0, 3.0, 17)])
def test_invalid_clip_parameters_are_rejected(st, clip):
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    with pytest.raises(InvalidParams, match="sigma clipping"):
        st.ecc_match_clipped(frames, ECC, clip)
    with pytest.raises(InvalidParams, match="sigma clipping"):
        st.keypoint_match_clipped(frames, KP, clip)
    with pytest.raises(InvalidParams, match="sigma clipping"):
        st.clip_stack(frames, [np.eye(3)] * 3, clip)


def test_output_geometry_mismatch_is_rejected(st):
    import ctypes as C
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    frames, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(frames.numpy())
    out = np.empty((96, 127, 3), np.float32)
    img = _ffi.ImageF32(out.ctypes.data, 127, 96, 3, HOST, 0)
    cp, ep = SigmaClipParameters()._c(), ECC._c()
    assert st._lib.stk_ecc_match_clipped(st._h, C.byref(m.c_frames), C.byref(ep), 0.0, C.byref(cp), C.byref(img), None, None) == 2
    assert b"geometry" in st._lib.stk_last_error(st._h)


def test_fullsize_u8_ecc_clipped(st):
    frames, _ = synth.make_stack(64, 3840, 2160, device="cuda")
    clip = SigmaClipParameters(3.0, 3.0, 2)
    out, cnt, stats = st.ecc_match_clipped(frames, ECC, clip, return_stats=True, return_counts=True)
    ref, ref_k = _clip_of(st, frames, stats, clip)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(cnt.cpu().numpy(), ref_k.cpu().numpy())
    assert int(cnt.min()) < 64

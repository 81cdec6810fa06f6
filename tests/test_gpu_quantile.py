"""Median and quantile stacking on the GPU: stk_quantile_stack / stk_ecc_match_quantile / stk_keypoint_match_quantile against
the numpy restatement of the definition (test_cpu_quantile.quantile_restate), whose samples come from the engine's own
single-frame warp (Stacker.warp_accumulate with the same matrices)."""
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REFLECT, BORDER_REPLICATE, BORDER_WRAP, RANSAC, EccMatchParameters,
                               InvalidParams, KeyPointMatchParameters, MotionType, QuantileParameters, Stacker, synth)
from libstacker_rs_amd.api import NotImplementedYet
from test_cpu_quantile import quantile_restate

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


def noisy_frames(rng, n, h, w, cn, dtype):
    """n noisy copies of one random scene, ~3 % of each frame's pixels replaced by bright or dark outliers."""
    base = rng.random((h, w, cn))
    frames = []
    for _ in range(n):
        f = base + rng.normal(0, 0.05, base.shape)
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


def samples_of(st, frames, warps, include=None, **kw):
    idx = [i for i in range(len(frames)) if include is None or include[i]]
    return np.stack([np.asarray(st.warp_accumulate(frames[i], warps[i], acc=None, **kw)) for i in idx])


# (depth, channels, affine, border, border value, subpixel bits, N, q, (h, w), include subset)
CASES = [
    (np.uint8, 3, False, BORDER_CONSTANT, (0.25, 0.5, 0.75, 0), 0, 11, 0.5, (45, 131), True),     # u8 BGR fast kernel
    (np.uint8, 3, True, BORDER_CONSTANT, (0, 0, 0, 0), 0, 64, 0.73, (40, 200), False),            # fast kernel, affine
    (np.uint8, 3, False, BORDER_CONSTANT, (0, 0, 0, 0), 0, 3, 0.5, (1, 65), False),               # one-row frame: generic
    (np.uint8, 3, False, BORDER_REPLICATE, (0, 0, 0, 0), 0, 2, 0.5, (33, 97), False),
    (np.uint8, 1, True, BORDER_REFLECT, (0, 0, 0, 0), 5, 11, 0.1, (30, 61), False),
    (np.uint8, 4, True, BORDER_CONSTANT, (0.1, 0.2, 0.3, 0.4), 5, 11, 1.0, (31, 77), True),
    (np.uint16, 3, False, BORDER_CONSTANT, (0.5, 0.5, 0.5, 0), 0, 11, 0.5, (29, 67), False),
    (np.uint16, 1, False, BORDER_WRAP, (0, 0, 0, 0), 0, 3, 0.0, (28, 59), False),
    (np.uint16, 4, True, BORDER_REPLICATE, (0, 0, 0, 0), 5, 64, 0.5, (27, 63), False),
    (np.float32, 3, True, BORDER_CONSTANT, (0.3, 0.6, 0.9, 0), 0, 1, 0.73, (25, 71), False),
    (np.float32, 1, False, BORDER_REPLICATE, (0, 0, 0, 0), 5, 2, 0.1, (24, 33), False),
    (np.float32, 4, False, BORDER_REPLICATE, (0, 0, 0, 0), 5, 11, 0.0, (23, 69), True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-N{c[6]}-q{c[7]}-{c[8][0]}x{c[8][1]}{'-inc' if c[9] else ''}" for c in CASES])
def test_quantile_stack_matches_restatement(st, case):
    dtype, cn, affine, border, bv, sub, n, q, (h, w), subset = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    frames = noisy_frames(rng, n + (1 if subset else 0), h, w, cn, dtype)
    warps = small_warps(rng, len(frames), affine)
    include = None
    if subset:
        include = [1] * len(frames)
        include[len(frames) // 2] = 0
    kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=_ALPHA[dtype])
    st.set_option("warp_subpixel_bits", sub)
    try:
        ref = quantile_restate(samples_of(st, frames, warps, include, **kw), q)
        out = st.quantile_stack(frames, warps, q, include, **kw)
        import torch
        dout = st.quantile_stack(torch.from_numpy(np.stack(frames)).cuda(), warps, QuantileParameters(q), include, **kw)
    finally:
        st.set_option("warp_subpixel_bits", 0)
    np.testing.assert_array_equal(out, ref)
    np.testing.assert_array_equal(dout.cpu().numpy(), ref)


def test_large_n_selection(st):
    rng = np.random.default_rng(5)
    n, h, w = 1024, 6, 21
    frames = noisy_frames(rng, n, h, w, 1, np.uint16)
    warps = small_warps(rng, n, True)
    kw = dict(is_affine=True, border_mode=BORDER_REPLICATE, alpha=_ALPHA[np.uint16])
    samples = samples_of(st, frames, warps, **kw)
    for q in (0.5, 0.1, 1.0):
        np.testing.assert_array_equal(st.quantile_stack(frames, warps, q, **kw), quantile_restate(samples, q))


def test_band_rows_change_no_bit(st):
    rng = np.random.default_rng(9)
    n, h, w = 11, 37, 53                             # 37 rows: not a multiple of 3
    frames = noisy_frames(rng, n, h, w, 3, np.uint8)
    warps = small_warps(rng, n, False)
    ref = quantile_restate(samples_of(st, frames, warps), 0.73)
    outs = []
    for rows in (1, 3, 0):
        st.set_option("quantile_band_rows", rows)
        try:
            outs.append(st.quantile_stack(frames, warps, 0.73))
        finally:
            st.set_option("quantile_band_rows", 0)
    for o in outs:
        np.testing.assert_array_equal(o, ref)


def test_infinities_and_nans(st):
    rng = np.random.default_rng(13)
    n, h, w = 11, 20, 40
    frames = noisy_frames(rng, n, h, w, 3, np.float32)
    for i in (1, 4, 7):
        frames[i][rng.integers(0, h, 30), rng.integers(0, w, 30), rng.integers(0, 3, 30)] = np.inf
    frames[2][rng.integers(0, h, 20), rng.integers(0, w, 20), rng.integers(0, 3, 20)] = -np.inf
    frames[9][rng.integers(0, h, 10), rng.integers(0, w, 10), rng.integers(0, 3, 10)] = np.nan
    # identity warps in the classic 4-weight path (weights 1, 0, 0, 0): a planted inf stays an inf sample there (the exact
    # path's lerp, fma(0, inf - p, p), makes it NaN) and NaN at the pixels that have it as a zero-weight tap
    warps = [np.eye(3)] * n
    kw = dict(alpha=1.0)
    st.set_option("warp_subpixel_bits", 5)
    try:
        samples = samples_of(st, frames, warps, **kw)
        outs = {q: st.quantile_stack(frames, warps, q, **kw) for q in (0.0, 0.5, 0.73, 1.0)}
    finally:
        st.set_option("warp_subpixel_bits", 0)
    assert np.isnan(samples).any() and np.isposinf(samples).any() and np.isneginf(samples).any()
    for q, out in outs.items():
        np.testing.assert_array_equal(out, quantile_restate(samples, q))     # NaN positions included
        assert np.isnan(out[np.isnan(samples).any(axis=0)]).all()
    assert np.isposinf(outs[1.0]).any() and np.isneginf(outs[0.0]).any()


def _quantile_of(st, frames, stats, q, include=None, **kw):
    return st.quantile_stack(frames, [s["warp"] for s in stats], q, include, **kw)


def test_ecc_match_quantile_equals_quantile_stack_on_its_warps(st):
    frames, _ = synth.make_stack(6, 256, 192, device="cuda")
    out, stats = st.ecc_match_quantile(frames, ECC, 0.5, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    _, pstats = st.ecc_match(frames, ECC, return_stats=True)
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["rho"] == b["rho"]
        assert np.array_equal(a["warp"], b["warp"])
    ref = _quantile_of(st, frames, stats, 0.5)
    np.testing.assert_array_equal(out.cpu().numpy(), ref.cpu().numpy())
    # host-fed: the same bits, output on the host
    hout = st.ecc_match_quantile(frames.cpu().numpy(), ECC, QuantileParameters(0.5))
    np.testing.assert_array_equal(hout, out.cpu().numpy())
    q1 = st.ecc_match_quantile(frames.cpu().numpy(), ECC, 0.1)
    np.testing.assert_array_equal(q1, _quantile_of(st, frames, stats, 0.1).cpu().numpy())


def test_keypoint_match_quantile_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 640, 480)
    frames = frames.numpy()
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    dropped, out, stats = st.keypoint_match_quantile(stack, KP, 0.5, return_stats=True)
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["n_matches"] == b["n_matches"] and np.array_equal(a["warp"], b["warp"])
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    np.testing.assert_array_equal(out, _quantile_of(st, stack, stats, 0.5, include))
    samples = samples_of(st, stack, [s["warp"] for s in stats], include)
    assert samples.shape[0] == 4
    np.testing.assert_array_equal(out, quantile_restate(samples, 0.5))


def test_median_returns_the_clean_scene_under_trails_and_hot_pixels(st):
    n, h, w = 9, 120, 160
    rng = np.random.default_rng(21)
    clean = (rng.random((h, w, 3)) * 200).astype(np.uint8)
    frames = [clean.copy() for _ in range(n)]
    frames[2][50:53, 10:150] = 255                     # a trail in two frames
    frames[6][80:82, 20:140] = 255
    for i in (1, 4, 7):                                # hot pixels in three frames
        frames[i][rng.integers(0, h, 40), rng.integers(0, w, 40)] = 255
    warps = [np.eye(3)] * n
    med = st.quantile_stack(frames, warps, 0.5)
    truth = clean.astype(np.float32) * np.float32(1.0 / 255.0)
    np.testing.assert_array_equal(med, truth)
    mean = np.mean(np.stack([f.astype(np.float32) * np.float32(1.0 / 255.0) for f in frames]), axis=0)
    assert np.abs(mean - truth)[50:53, 10:150].min() > 0.02       # (255 - 199) / 9 / 255 at least


def test_options_do_not_change_a_quantile_bit(st):
    frames, _ = synth.make_stack(20, 640, 480, device="cuda")
    base = st.ecc_match_quantile(frames, ECC, 0.5).cpu().numpy()
    for name, val, back in (("ecc_slots", 4, 0), ("prep_overlap", 0, 1), ("quantile_band_rows", 7, 0)):
        st.set_option(name, val)
        try:
            o = st.ecc_match_quantile(frames, ECC, 0.5)
        finally:
            st.set_option(name, back)
        np.testing.assert_array_equal(o.cpu().numpy(), base, err_msg=name)
    kres = []
    for lanes in (1, 3):
        st.set_option("kp_lanes", lanes)
        try:
            kres.append(st.keypoint_match_quantile(frames, KP, 0.5))
        finally:
            st.set_option("kp_lanes", 3)
    assert kres[0][0] == kres[1][0]
    np.testing.assert_array_equal(kres[0][1].cpu().numpy(), kres[1][1].cpu().numpy())
    multi = Stacker(devices=[0, 0])                   # a multi-device context runs them on its first device
    try:
        mo = multi.ecc_match_quantile(frames, ECC, 0.5)
    finally:
        multi.close()
    np.testing.assert_array_equal(mo.cpu().numpy(), base)


@pytest.mark.parametrize("q", [QuantileParameters(-0.1), QuantileParameters(1.5), QuantileParameters(float("nan")),
                               QuantileParameters(float("inf"))])
def test_invalid_quantile_parameters_are_rejected(st, q):
    frames, _ = synth.make_stack(3, 128, 96)
    frames = frames.numpy()
    with pytest.raises(InvalidParams, match="quantile"):
        st.ecc_match_quantile(frames, ECC, q)
    with pytest.raises(InvalidParams, match="quantile"):
        st.keypoint_match_quantile(frames, KP, q)
    with pytest.raises(InvalidParams, match="quantile"):
        st.quantile_stack(frames, [np.eye(3)] * 3, q)


def test_parameter_and_geometry_errors(st):
    import ctypes as C
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    frames, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(frames.numpy())
    ep = ECC._c()
    out = np.empty((96, 128, 3), np.float32)
    img = _ffi.ImageF32(out.ctypes.data, 128, 96, 3, HOST, 0)
    # null parameters, reserved != 0
    assert st._lib.stk_ecc_match_quantile(st._h, C.byref(m.c_frames), C.byref(ep), 0.0, None, C.byref(img), None) == 2
    assert b"quantile" in st._lib.stk_last_error(st._h)
    bad = _ffi.QuantileParams(0.5, 1)
    assert st._lib.stk_ecc_match_quantile(st._h, C.byref(m.c_frames), C.byref(ep), 0.0, C.byref(bad), C.byref(img), None) == 2
    assert b"quantile" in st._lib.stk_last_error(st._h)
    # output geometry, packing
    qp = QuantileParameters()._c()
    small = np.empty((96, 127, 3), np.float32)
    simg = _ffi.ImageF32(small.ctypes.data, 127, 96, 3, HOST, 0)
    assert st._lib.stk_ecc_match_quantile(st._h, C.byref(m.c_frames), C.byref(ep), 0.0, C.byref(qp), C.byref(simg), None) == 2
    assert b"geometry" in st._lib.stk_last_error(st._h)
    wide = np.empty((96, 130, 3), np.float32)
    wimg = _ffi.ImageF32(wide.ctypes.data, 128, 96, 3, HOST, 130 * 3 * 4)
    assert st._lib.stk_ecc_match_quantile(st._h, C.byref(m.c_frames), C.byref(ep), 0.0, C.byref(qp), C.byref(wimg), None) == 2
    assert b"tightly packed" in st._lib.stk_last_error(st._h)
    # no frame included; BORDER_TRANSPARENT
    with pytest.raises(InvalidParams, match="quantile"):
        st.quantile_stack(frames.numpy(), [np.eye(3)] * 3, 0.5, [0, 0, 0])
    with pytest.raises(NotImplementedYet):
        st.quantile_stack(frames.numpy(), [np.eye(3)] * 3, 0.5, border_mode=5)


def test_fullsize_u8_ecc_median(st):
    frames, _ = synth.make_stack(64, 3840, 2160, device="cuda")
    out, stats = st.ecc_match_quantile(frames, ECC, 0.5, return_stats=True)
    warps = [s["warp"] for s in stats]
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got, st.quantile_stack(frames, warps, 0.5).cpu().numpy())
    # ~12 rows against the restatement: first, last, band edges (a 4 GiB band holds 1456 rows of 64 4K BGR frames), random
    rng = np.random.default_rng(3)
    rows = sorted({0, 1, 1455, 1456, 1457, 2159} | set(rng.integers(0, 2160, 6).tolist()))
    samples = np.stack([st.warp_accumulate(frames[i], warps[i], acc=None)[rows].cpu().numpy() for i in range(64)])
    np.testing.assert_array_equal(got[rows], quantile_restate(samples, 0.5))

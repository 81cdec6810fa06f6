"""Noise estimation on the GPU: stk_stack_noise's histograms against np.bincount and its statistics against the numpy
restatement (tests/noise_restate.py), exactly, over shapes, depths, channel counts, memory layouts and contents; the
whole-stack noise-weighted forms against their parts, bit for bit; the refusals."""
import ctypes as C

import numpy as np
import pytest

import noise_restate as nr
from libstacker_rs_amd import (RANSAC, EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType, NOISE_DTYPE, NoiseParameters,
                               NotImplementedYet, Stacker, WeightParameters, _ffi, noise_weights, synth)

pytestmark = pytest.mark.gpu

# (w, h): one residual; a row and a column of residuals; one tile plus a sliver in both directions (the depth-16 tile is 32
# rows: three tiles down); three tiles across
SHAPES = [(3, 3), (3, 5), (5, 3), (67, 65), (130, 70)]
CONTENTS = ("random", "constant", "checkerboard", "sky", "max")
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
NOISE_SIGMAS = (1.5, 2.5, 3.5, 4.5, 6.0)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def content(kind, rng, h, w, cn, dt):
    """one frame h x w x cn whose channel planes differ"""
    top = np.iinfo(dt).max
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for c in range(cn):
        if kind == "random":
            p = rng.integers(0, top + 1, (h, w))
        elif kind == "constant":
            p = np.full((h, w), (top // 7) * (c + 1))
        elif kind == "checkerboard":
            p = ((xx + yy + c) & 1) * top
        elif kind == "sky":                                                # three grey levels: nearly every lane of a wave adds to one of three bins
            p = (top // 12) * (c + 1) + rng.choice(3, size=(h, w), p=[0.3, 0.5, 0.2])
        else:
            p = np.full((h, w), top)
        planes.append(p)
    return np.stack(planes, -1).astype(dt)


_REF = {}


def reference(depth, cn, shape):
    """the frames of the five contents at this depth, channel count and shape, with their restated statistics and
    histograms: computed once and shared"""
    key = (depth, cn, shape)
    if key not in _REF:
        w, h = shape
        dt = np.uint8 if depth == 8 else np.uint16
        rng = np.random.default_rng(1000 * depth + 10 * cn + w)
        frames = [content(k, rng, h, w, cn, dt) for k in CONTENTS]
        stats, hist = nr.stack_stats(frames)
        for a in (stats, hist, *frames):
            a.setflags(write=False)
        _REF[key] = (frames, stats, hist)
    return _REF[key]


def lay_out(frames, layout, device):
    """the frames as a list in the layout asked: tight; rows padded to a stride that is / is not a multiple of 4 bytes; the
    base one element past an aligned address"""
    import torch
    out = []
    for f in frames:
        h, w, cn = f.shape
        es = f.dtype.itemsize
        if layout == "tight":
            a = np.array(f)
        elif layout in ("padded4", "padded_odd"):
            pad = 1
            while ((w + pad) * cn * es) % 4 != 0:
                pad += 1
            if layout == "padded_odd" and (cn * es) % 4 != 0:
                pad += 1                                                   # (four u8 channels or two u16 pairs: every stride is a multiple of 4)
            parent = np.full((h, w + pad, cn), 0xA5, f.dtype)
            parent[:, :w] = f
            a = parent
        else:
            flat = np.zeros(f.size + 1, f.dtype)
            flat[1:] = f.reshape(-1)
            a = flat
        if device:
            a = torch.from_numpy(a).cuda()
        if layout in ("padded4", "padded_odd"):
            a = a[:, :w]
        elif layout == "misaligned":
            a = a[1:].reshape(h, w, cn) if not device else a[1:].view(h, w, cn)
        out.append(a)
    return out


def check(got_stats, got_hist, stats, hist, what):
    assert got_hist.shape == hist.shape and got_hist.dtype == np.uint32
    assert np.array_equal(got_hist, hist), (what, np.argwhere(got_hist != hist)[:5])
    assert got_stats.tobytes() == np.ascontiguousarray(stats).tobytes(), (what, got_stats, stats)


@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("depth", [8, 16])
def test_stack_noise_equals_bincount_and_the_restatement(st, depth, cn):
    for shape in SHAPES:
        frames, stats, hist = reference(depth, cn, shape)
        bv, br = nr.bins(depth)
        assert hist.shape == (5, cn, bv + br) and int(hist[0, 0, :bv].sum()) == shape[0] * shape[1]
        assert int(hist[0, 0, bv:].sum()) == (shape[0] - 2) * (shape[1] - 2)
        for device in (False, True):
            for layout in ("tight", "padded4", "padded_odd", "misaligned"):
                got_stats, got_hist = st.stack_noise(lay_out(frames, layout, device), return_hist=True)
                check(got_stats, got_hist, stats, hist, (shape, device, layout))
                assert st.timing()["prep_ms"] > 0
        # n = 1, and without the histograms
        one = st.stack_noise([frames[0]])
        assert one.shape == (1, 4) and one.tobytes() == np.ascontiguousarray(stats[:1]).tobytes()
    # what the contents are there for
    _, stats, _ = reference(depth, cn, (67, 65))
    top = 255 if depth == 8 else 65535
    for c in range(cn):
        assert stats[1, c]["flags"] == 1 and stats[1, c]["sigma"] == 0.0 and stats[4, c]["median"] == top      # constant, all-max
        assert (stats[2, c]["res_median"], stats[2, c]["flags"]) == ((2040, 0) if depth == 8 else (65535, 3))  # checkerboard
        assert stats[3, c]["mad"] <= 1 and 0 < stats[3, c]["sigma"] < 1.5                                       # three-level sky
    assert np.all(stats[:, cn:]["kept"] == 0) and np.all(stats[:, cn:]["sigma"] == 0.0)                         # unused channel slots


def test_one_tensor_stack_and_host_batches(st):
    """a contiguous 4-D device tensor (the pointers an arithmetic progression), and host frames through a frame workspace
    that holds one frame at a time"""
    import torch
    frames, stats, hist = reference(8, 3, (130, 70))
    got_stats, got_hist = st.stack_noise(torch.from_numpy(np.stack(frames)).cuda(), return_hist=True)
    check(got_stats, got_hist, stats, hist, "4-D tensor")
    small = Stacker(0)
    try:
        small.set_option("upload_batch", 1)
        got_stats, got_hist = small.stack_noise(frames, return_hist=True)
    finally:
        small.close()
    check(got_stats, got_hist, stats, hist, "host batches of one frame")


@pytest.mark.parametrize("depth", [8, 16])
def test_same_bits_twice_and_after_another_entry_point(st, depth):
    import torch
    frames, stats, hist = reference(depth, 3, (130, 70))
    dev = lay_out(frames, "tight", True)
    a = st.stack_noise(dev, return_hist=True)
    b = st.stack_noise(dev, return_hist=True)
    # another entry point dirties the workspaces the pass uses (the scoring pass shares its workspace)
    u8 = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (3, 200, 300, 3), dtype=np.uint8)).cuda()
    st.stack_sharpness(u8)
    st.ecc_match(torch.from_numpy(synth.make_stack(3, 256, 192)[0].numpy()).cuda(), ECC)
    c = st.stack_noise(dev, return_hist=True)
    for got in (a, b, c):
        check(got[0], got[1], stats, hist, depth)


def noisy_stack():
    frames, _ = synth.make_stack(5, 256, 192, noise_sigma=0.0)
    rng = np.random.default_rng(77)
    f = frames.numpy().astype(np.float64)
    for i, s in enumerate(NOISE_SIGMAS):
        f[i] += rng.normal(0.0, s, f[i].shape)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _applied_bytes(applied):
    return [(a["gain"].tobytes(), a["offset"].tobytes(), np.float32(a["weight"]).tobytes(), a["flags"]) for a in applied]


def test_ecc_match_noise_weighted_equals_its_parts(st):
    import torch
    host = noisy_stack()
    dev = torch.from_numpy(host).cuda()
    wp = WeightParameters(2, True, 2)                                      # gain normalisation
    user = [1.0, 1.0, 2.0, 1.0, 0.5]
    npar = NoiseParameters(0.25)
    # the existing weighted form first: its bits are its parts' bits, as before this change
    wout, wapplied, wstats = st.ecc_match_weighted(dev, ECC, wp, user, return_stats=True, return_applied=True)
    warps = [s["warp"] for s in wstats]
    ref = st.weighted_stack(dev, warps, applied=wapplied, coverage=True)
    assert np.array_equal(wout.cpu().numpy(), ref.cpu().numpy())
    assert [a["weight"] for a in wapplied] == user
    # the noise-weighted form
    out, cov, applied, noise, stats = st.ecc_match_noise_weighted(dev, ECC, wp, user, npar, return_stats=True, return_coverage=True,
                                                                  return_applied=True, return_noise=True)
    assert st.timing()["finalize_ms"] > 0
    for a, b in zip(stats, wstats):                                        # 1. the plain call's stats
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and np.array_equal(a["warp"], b["warp"])
    for a, b in zip(applied, wapplied):                                    # 2. the weighted form's gains and offsets
        assert np.array_equal(a["gain"], b["gain"]) and np.array_equal(a["offset"], b["offset"]) and a["flags"] == b["flags"]
    ns = st.stack_noise(dev)                                               # 3. stk_stack_noise on the same frames
    assert noise.tobytes() == ns.tobytes() == nr.stack_stats(list(host))[0].tobytes()
    w = noise_weights(ns, 3, applied=wapplied, weights=user, sigma_floor=0.25)   # 4. stk_noise_weights with those records
    assert [np.float32(a["weight"]) for a in applied] == list(w)
    parts = [dict(a, weight=float(w[i])) for i, a in enumerate(wapplied)]
    ref, ref_cov = st.weighted_stack(dev, warps, applied=parts, coverage=True, return_coverage=True)          # 5. the weighted fold
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(cov.cpu().numpy(), ref_cov.cpu().numpy())
    # the weights do what they are for: the estimates follow the planted noise, and a noisier frame weighs less
    est = ns["sigma"][:, 0]
    print("planted", NOISE_SIGMAS, "estimated", est.tolist(), "weights", w.tolist())
    assert np.all(np.diff(est) > 0) and w[1] / user[1] > w[3] / user[3] > w[4] / user[4]
    # host-fed: the same bits, outputs on the host
    hout, happlied = st.ecc_match_noise_weighted(host, ECC, wp, user, npar, return_applied=True)
    assert np.array_equal(hout, out.cpu().numpy()) and _applied_bytes(happlied) == _applied_bytes(applied)
    # and the existing form again, after the noise-weighted one used the context: the bits it returned before
    again = st.ecc_match_weighted(dev, ECC, wp, user)
    assert np.array_equal(again.cpu().numpy(), wout.cpu().numpy())


def test_keypoint_match_noise_weighted_equals_its_parts_with_a_dropped_frame(st):
    host = noisy_stack()
    stack = [host[0], host[1], np.full_like(host[0], 128), host[2], host[3]]         # a featureless frame: dropped
    wp = WeightParameters(3, True, 2)
    dropped, out, cov, applied, noise, stats = st.keypoint_match_noise_weighted(stack, KP, wp, None, None, return_stats=True,
                                                                                 return_coverage=True, return_applied=True, return_noise=True)
    wd, wout, wapplied, wstats = st.keypoint_match_weighted(stack, KP, wp, None, return_stats=True, return_applied=True)
    assert dropped == wd == 1 and stats[2]["status"] == 1 and applied[2]["weight"] == 0.0
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    ns = st.stack_noise(stack)
    assert noise.tobytes() == ns.tobytes()
    w = noise_weights(ns, 3, applied=wapplied, include=include, sigma_floor=NoiseParameters().floor(8))
    assert w[2] == 0.0 and [np.float32(a["weight"]) for a in applied] == list(w)
    parts = [dict(a, weight=float(w[i])) for i, a in enumerate(wapplied)]
    ref, ref_cov = st.weighted_stack(stack, warps, applied=parts, include=include, coverage=True, return_coverage=True)
    assert np.array_equal(out, ref) and np.array_equal(cov, ref_cov)


def test_refusals(st):
    import torch
    rng = np.random.default_rng(2)
    ok = rng.integers(0, 256, (2, 8, 9, 3), dtype=np.uint8)
    for bad in (ok[:, :2], ok[:, :, :2]):                                  # height, width below 3
        with pytest.raises(InvalidParams):
            st.stack_noise(list(bad))
    with pytest.raises(NotImplementedYet):
        st.stack_noise(list(ok.astype(np.float32)))
    with pytest.raises(NotImplementedYet):
        st.stack_noise(torch.from_numpy(ok.astype(np.float32)).cuda())
    # above 2^27 pixels: refused before a byte is read, so the frame need not exist
    lib = _ffi.load()
    ptrs = (C.c_void_p * 1)(ok.ctypes.data)
    stats = np.zeros((1, 4), NOISE_DTYPE)
    big = _ffi.Frames(C.cast(ptrs, C.POINTER(C.c_void_p)), 1, 16384, 8193, 1, 8, 0, 0)
    assert lib.stk_stack_noise(st._h, C.byref(big), stats.ctypes.data_as(C.POINTER(_ffi.NoiseStat)), None) == 7
    fine = _ffi.Frames(C.cast(ptrs, C.POINTER(C.c_void_p)), 1, 9, 8, 3, 8, 0, 0)
    assert lib.stk_stack_noise(st._h, C.byref(fine), None, None) == 2      # null statistics
    assert lib.stk_stack_noise(st._h, C.byref(fine), stats.ctypes.data_as(C.POINTER(_ffi.NoiseStat)), None) == 0
    assert stats.tobytes() == nr.stack_stats([ok[0]])[0].tobytes()
    # the whole-stack forms: the floor, the depth, the frames' size
    frames = torch.from_numpy(synth.make_stack(3, 256, 192)[0].numpy()).cuda()
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(InvalidParams):
            st.ecc_match_noise_weighted(frames, ECC, noise=NoiseParameters(floor))
        with pytest.raises(InvalidParams):
            st.keypoint_match_noise_weighted(frames, KP, noise=NoiseParameters(floor))
    with pytest.raises(NotImplementedYet):
        st.ecc_match_noise_weighted(frames.float(), ECC)
    with pytest.raises(InvalidParams):
        st.ecc_match_noise_weighted(frames, ECC, weights=[1.0, -1.0, 1.0])
    with pytest.raises(InvalidParams):
        st.ecc_match_noise_weighted(frames, ECC, WeightParameters(5))

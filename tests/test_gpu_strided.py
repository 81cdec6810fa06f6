"""Padded and misaligned frame rows (stk_frames.row_stride_bytes) through every stack entry point.

One fixture idea: a CANVAS (N, Hc, Wc, C) holds unrelated content — another seeded random image for the integer types, NaN
for f32 — and the stack under test is a window of it, handed over where it lies (api._Marshalled passes row-strided views
in place). A tap taken from the wrong row, column or frame therefore changes the result. The reference of every case is the
same call on the contiguous copy of the window, and the relation is BIT EQUALITY of the image and of every stat the call
returns (an entry point's bits do not depend on how its input is laid out); the tight call itself is
anchored to the oracle by the rest of the suite, and `warp_accumulate` / `grey` / `grey_blur_f32` are anchored here once
more, directly, at the bars of test_gpu_stages.py.

Every case asserts its layout class from the real addresses (frame pointers and row stride): the alignment of the stride,
of the best and the worst aligned frame base, whether the frames are evenly spaced and whether that spacing differs from
stride * height. The classes are what the kernels dispatch on: WARPFRAME_SRC_ALIGNED4 per frame ((base | stride) & 3), the
dword / 8-byte / 16-byte gates of kernels_prep.hip, the streaming template kernel for evenly spaced frames, the byte-by-byte
route of the quality pass. Every GPU case keeps at least one canvas row below its window and one pixel to its right."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REFLECT_101, EccMatchParameters, InvalidParams, KeyPointMatchParameters,
                               MotionType, QuantileParameters, RANSAC, SigmaClipParameters, WeightParameters, api, synth)

pytestmark = pytest.mark.gpu

N, H = 5, 237                     # frames; window rows: no multiple of a 4-row warp tile, a 32-row blur segment or tile
SCENE_W, SCENE_H = 336, 248
ECC = EccMatchParameters(MotionType.Homography, 50, 1e-5, 5)
ECC_AFFINE = EccMatchParameters(MotionType.Affine, 50, 1e-5, 3)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
ALPHA = {"u8": 1.0 / 255.0, "u16": 1.0 / 65535.0, "f32": 1.0 / 255.0}
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}


# ---- content: the tightly packed stacks, made once and never written --------------------------------------------------
@functools.lru_cache(None)
def _scene():
    frames, _ = synth.make_stack(N, SCENE_W, SCENE_H)
    return frames.numpy()


@functools.lru_cache(None)
def _content(kind, w):
    """(N, H, w, C) of `kind` = u8c3 | u8c4 | u8c1 | u16c3 | f32c3 | f32c1: windows 320 / 323 / 324 wide of one scene."""
    depth, cn = kind.split("c")
    s = _scene()[:, 5:5 + H, 6:6 + w]
    rng = np.random.default_rng(17)
    if cn == "4":
        s = np.concatenate([s, rng.integers(0, 256, s.shape[:3] + (1,), dtype=np.uint8)], axis=3)
    elif cn == "1":
        s = s[..., 1:2]
    if depth == "u16":                                    # real 16-bit content, not just scaled 8-bit
        s = np.minimum(s.astype(np.uint32) * 257 + rng.integers(0, 200, s.shape), 65535).astype(np.uint16)
    s = np.ascontiguousarray(s.astype(DTYPE[depth]))
    s.setflags(write=False)
    return s


def _aligned(shape, dtype, align=512):
    """A host array whose base is aligned like a device allocation, so that a layout has one class on both sides."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.empty(nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + nbytes].view(dtype).reshape(shape)


# ---- layouts ----------------------------------------------------------------------------------------------------------
# (Hc, Wc, offsets): the canvas planes and where the window lies in them — one (y0, x0) for all planes (the frames are a
# 4-D view, evenly spaced Hc * Wc pixels apart) or one per plane (a list of views, unevenly spaced)
UNEVEN = ((4, 0), (3, 7), (5, 4), (2, 7), (6, 0))
LAYOUTS = {
    # Wc * 3 % 4 == 0
    "x0":       (248, 336, ((4, 0),)),
    "x2":       (248, 336, ((4, 2),)),
    "x4":       (248, 336, ((4, 4),)),
    "x7":       (248, 336, ((3, 7),)),
    "uneven":   (248, 336, UNEVEN),
    # Wc odd: the row stride of u8 x 3 is odd; Hc odd as well: the frame bases alternate in alignment
    "odd_alt":  (247, 335, ((3, 7),)),
    "odd_alt0": (247, 335, ((3, 0),)),
    "odd_x0":   (248, 335, ((4, 0),)),
    "odd_x4":   (248, 335, ((4, 4),)),
    # u16: strides that are a multiple of 8 / of 4 only
    "w332":     (248, 332, ((4, 0),)),
    "w334":     (248, 334, ((4, 0),)),
}


def _window(kind, w, layout, device):
    """(frames, canvas): the window views of a freshly filled canvas, host arrays or tensors on cuda:0."""
    import torch
    content = _content(kind, w)
    n, h, _, c = content.shape
    hc, wc, offs = LAYOUTS[layout]
    offs = offs * n if len(offs) == 1 else offs
    canvas = _aligned((n, hc, wc, c), content.dtype)
    rng = np.random.default_rng(hc * 1000 + wc)
    if content.dtype == np.float32:
        canvas[...] = np.nan
    else:
        canvas[...] = rng.integers(0, np.iinfo(content.dtype).max + 1, canvas.shape, dtype=content.dtype)
    for i, (y0, x0) in enumerate(offs):
        assert y0 + h < hc and x0 + w < wc               # a canvas row below the window and a pixel to its right
        canvas[i, y0:y0 + h, x0:x0 + w] = content[i]
    if device:
        canvas = torch.from_numpy(canvas).to("cuda:0")
    if len(set(offs)) == 1:
        y0, x0 = offs[0]
        frames = canvas[:, y0:y0 + h, x0:x0 + w]
    else:
        frames = [canvas[i, y0:y0 + h, x0:x0 + w] for i, (y0, x0) in enumerate(offs)]
    return frames, canvas


def _tight(kind, w, device):
    import torch
    t = _content(kind, w)
    return torch.from_numpy(t.copy()).to("cuda:0") if device else t


def _alignment(v, cap):
    a = 1
    while a < cap and v % (2 * a) == 0:
        a *= 2
    return a


def _layout_class(frames, cap):
    """From the real addresses: (stride alignment, worst base alignment, best base alignment) capped at `cap`, the row
    stride in bytes, whether the frames are evenly spaced and whether that step equals stride * height."""
    fr = list(frames)
    torch_like = hasattr(fr[0], "data_ptr")
    ptrs = [f.data_ptr() if torch_like else f.ctypes.data for f in fr]
    el = fr[0].element_size() if torch_like else fr[0].itemsize
    stride = fr[0].stride(0) * el if torch_like else fr[0].strides[0]
    assert all((f.stride(0) * el if torch_like else f.strides[0]) == stride for f in fr)
    h, w = fr[0].shape[:2]
    c = fr[0].shape[2] if len(fr[0].shape) == 3 else 1
    assert stride > w * c * el                                       # padded: never the tight row
    steps = {b - a for a, b in zip(ptrs, ptrs[1:])}
    al = [_alignment(p, cap) for p in ptrs]
    return dict(align=(_alignment(stride, cap), min(al), max(al)), stride=stride, even=len(steps) == 1,
                step_is_frame=steps == {stride * h})


def _check_class(frames, cap, align, even=True):
    cls = _layout_class(frames, cap)
    assert cls["align"] == align, cls
    assert cls["even"] == even and not cls["step_is_frame"], cls      # evenly spaced, but never stride * height apart
    # what the marshalling hands over is exactly this: the views' own pointers and their stride
    m = api._Marshalled(frames)
    fr = list(frames)
    assert m.c_frames.row_stride_bytes == cls["stride"]
    assert [m.c_frames.data[i] for i in range(m.n)] == [f.data_ptr() if hasattr(f, "data_ptr") else f.ctypes.data for f in fr]


# ---- bit equality of everything a call returns -------------------------------------------------------------------------
def _flat(x, out):
    if isinstance(x, dict):
        for k in sorted(x):
            _flat(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flat(v, out)
    elif hasattr(x, "data_ptr"):
        out.append(x.cpu().numpy())
    else:
        out.append(np.asarray(x))
    return out


def _assert_same_bits(got, ref, what):
    a, b = _flat(got, []), _flat(ref, [])
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            d = np.flatnonzero(np.ascontiguousarray(x).reshape(-1).view(np.uint8) != np.ascontiguousarray(y).reshape(-1).view(np.uint8))
            raise AssertionError(f"{what}: result {k} ({x.dtype}{x.shape}) differs from the tight call's in {d.size} bytes, first at byte {d[0]}")


_REF = {}


def _reference(st, key, call, kind, w, device):
    """The same call on the contiguous stack, made once per (call, content, location)."""
    key = (key, kind, w, device)
    if key not in _REF:
        _REF[key] = _flat(call(st, _tight(kind, w, device)), [])
    return _REF[key]


def _run(st, calls, kind, w, layout, device, cap, align, even=True):
    frames, canvas = _window(kind, w, layout, device)
    _check_class(frames, cap, align, even)
    before = canvas.clone() if device else canvas.copy()
    for name, call in calls.items():
        _assert_same_bits(call(st, frames), _reference(st, name, call, kind, w, device), f"{name} {kind} w={w} {layout} {'device' if device else 'host'}")
    _assert_same_bits(canvas, before, "the canvas itself")           # the engine writes nothing into a frame's surroundings


LOC = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])

# ---- whole-stack alignment + fold ---------------------------------------------------------------------------------------
WHOLE_U8 = {
    "ecc_match": lambda st, f: st.ecc_match(f, ECC, return_stats=True),
    "ecc_match affine": lambda st, f: st.ecc_match(f, ECC_AFFINE, return_stats=True),
    "ecc_match scaled": lambda st, f: st.ecc_match(f, ECC, scale_down_width=160, return_stats=True),
    "keypoint_match": lambda st, f: st.keypoint_match(f, KP, return_stats=True),
    "keypoint_match scaled": lambda st, f: st.keypoint_match(f, KP, scale_down_width=200, return_stats=True),
    "hybrid_match": lambda st, f: st.hybrid_match(f, KP, ECC, return_stats=True),
    "ecc_match_weighted": lambda st, f: st.ecc_match_weighted(f, ECC, WeightParameters(3, True, 3), [1, 2, 0.5, 1, 1.5], return_stats=True,
                                                            return_coverage=True, return_applied=True),
}

# u8 x 3: {stride % 4 == 0, != 0} x {every base % 4 == 0, some base % 4 != 0} x {w % 4 == 0, != 0}; `uneven`: the frames
# of ONE launch differ in WARPFRAME_SRC_ALIGNED4 (bases 0, 1, 0, 1, 0 mod 4 under an aligned stride)
U8C3 = [("x0", 320, (4, 4, 4), True), ("x4", 323, (4, 4, 4), True), ("x7", 320, (4, 1, 1), True), ("x7", 323, (4, 1, 1), True),
        ("uneven", 320, (4, 1, 4), False), ("uneven", 323, (4, 1, 4), False),
        ("odd_x0", 320, (1, 4, 4), True), ("odd_x4", 323, (1, 4, 4), True), ("odd_alt", 320, (1, 1, 4), True), ("odd_alt", 323, (1, 1, 4), True)]


@LOC
@pytest.mark.parametrize("layout,w,align,even", U8C3, ids=[f"{l}-{w}" for l, w, _, _ in U8C3])
def test_whole_stack_u8(stacker, layout, w, align, even, device):
    _run(stacker, WHOLE_U8, "u8c3", w, layout, device, 4, align, even)


WHOLE_F32 = {k: WHOLE_U8[k] for k in ("ecc_match", "ecc_match affine", "ecc_match scaled", "ecc_match_weighted")}


@LOC
@pytest.mark.parametrize("layout,w,even", [("x7", 323, True), ("uneven", 320, False), ("odd_alt", 320, True)])
def test_whole_stack_f32(stacker, layout, w, even, device):
    _run(stacker, WHOLE_F32, "f32c3", w, layout, device, 4, (4, 4, 4), even)   # f32: alignment cannot vary at element granularity


WHOLE_BGRA = {k: WHOLE_U8[k] for k in ("ecc_match", "ecc_match scaled", "keypoint_match", "keypoint_match scaled")}   # (hybrid_match takes 3 channels)


@LOC
@pytest.mark.parametrize("layout,w,even", [("x7", 323, True), ("uneven", 320, False), ("odd_alt", 320, True)])
def test_whole_stack_bgra(stacker, layout, w, even, device):
    _run(stacker, WHOLE_BGRA, "u8c4", w, layout, device, 4, (4, 4, 4), even)


# u16 x 3 (hybrid_match: bgr16_to_grey8 x8 / x4 / generic, the 16-bit template kernels, warp_accumulate_u16c3_kernel):
# stride % 16 == 0, % 8 only, % 4 only, % 4 == 2; the base likewise; w % 8 == 0, % 4 == 0 only, odd
U16C3 = [("x0", 320, (16, 16, 16), True), ("x4", 320, (16, 8, 8), True), ("x2", 320, (16, 4, 4), True), ("x7", 320, (16, 2, 2), True),
         ("w332", 320, (8, 16, 16), True), ("w334", 324, (4, 16, 16), True), ("x4", 324, (16, 8, 8), True), ("x0", 323, (16, 16, 16), True),
         ("odd_alt0", 323, (2, 2, 16), True), ("uneven", 320, (16, 2, 16), False)]
WHOLE_U16 = {"hybrid_match": WHOLE_U8["hybrid_match"]}


@LOC
@pytest.mark.parametrize("layout,w,align,even", U16C3, ids=[f"{l}-{w}" for l, w, _, _ in U16C3])
def test_whole_stack_u16(stacker, layout, w, align, even, device):
    _run(stacker, WHOLE_U16, "u16c3", w, layout, device, 16, align, even)


# ---- shard-level: the sum image itself padded ----------------------------------------------------------------------------
@LOC
@pytest.mark.parametrize("which", ["ecc", "keypoint"])
def test_shards_into_a_padded_sum(stacker, which, device):
    import torch
    w = 323
    frames, _ = _window("u8c3", w, "x7", device)
    _check_class(frames, 4, (4, 1, 1))
    sentinel = np.float32(-12345.5)

    def shard(f, sum_img, add_ref):
        if which == "ecc":
            return stacker.ecc_match_shard(f, ECC, add_ref, sum_img)
        return stacker.keypoint_match_shard(f, KP, add_ref, sum_img)
    for add_ref in (True, False):
        tight_sum = torch.full((H, w, 3), float(sentinel), dtype=torch.float32, device="cuda:0")
        ref = shard(_tight("u8c3", w, device), tight_sum, add_ref)
        big = torch.full((H + 2, w + 5, 3), float(sentinel), dtype=torch.float32, device="cuda:0")   # 15 floats of padding per row
        view = big[1:1 + H, 2:2 + w]
        assert not view.is_contiguous() and view.stride(0) * 4 % 4 == 0
        got = shard(frames, view, add_ref)
        _assert_same_bits((got, view), (ref, tight_sum), f"{which}_match_shard add_reference={add_ref}")
        outside = torch.ones_like(big, dtype=torch.bool)
        outside[1:1 + H, 2:2 + w] = False
        assert bool((big[outside] == float(sentinel)).all())             # the padding floats keep their sentinel
    # a shard of the reference frame alone that does not add it: the sum is zeroed, its padding is not
    big = torch.full((H + 2, w + 5, 3), float(sentinel), dtype=torch.float32, device="cuda:0")
    view = big[1:1 + H, 2:2 + w]
    added = shard(frames[:1], view, False)[0]
    assert added == 0 and bool((view == 0).all()) and int((big == float(sentinel)).sum()) == big.numel() - view.numel()


# ---- combines over fixed, given warps ------------------------------------------------------------------------------------
def _warps(w, affine):
    rng = np.random.default_rng(23)
    G = [np.eye(3)] + [synth.random_homography(rng, w, H, 2.0) for _ in range(N - 1)]
    if affine:
        G = [g[:2] / g[2, 2] for g in G]
    return G


def _combines(kind, w):
    depth = kind.split("c")[0]
    cn = int(kind.split("c")[1])
    gain = 1.0 + 0.01 * np.arange(N * cn, dtype=np.float32).reshape(N, cn)
    offset = 0.002 * np.arange(N * cn, dtype=np.float32).reshape(N, cn)[::-1]
    weights = [1, 2, 0.5, 1, 1.5]
    include = [1, 1, 0, 1, 1]
    calls = {}
    for tag, kw in (("projective constant", dict(is_affine=False, border_mode=BORDER_CONSTANT, border_value=(0.25, 0.5, 0.75, 1.0))),
                    ("affine reflect101", dict(is_affine=True, border_mode=BORDER_REFLECT_101))):
        kw = dict(kw, alpha=ALPHA[depth])
        Ms = _warps(w, kw["is_affine"])
        # the weighted family: coverage needs BORDER_CONSTANT with border value 0; the other border mode goes without coverage
        cov = kw["border_mode"] == BORDER_CONSTANT
        kww = dict(kw, border_value=(0, 0, 0, 0), coverage=cov)
        calls.update({
            f"clip_stack {tag}": lambda st, f, kw=kw, Ms=Ms: st.clip_stack(f, Ms, SigmaClipParameters(2.0, 2.5, 2), include, return_counts=True, **kw),
            f"quantile_stack {tag}": lambda st, f, kw=kw, Ms=Ms: st.quantile_stack(f, Ms, QuantileParameters(0.4), **kw),
            f"weighted_stack {tag}": lambda st, f, kw=kww, Ms=Ms: st.weighted_stack(f, Ms, gain, offset, weights, include, return_coverage=True, **kw),
            f"overlap_moments 1 {tag}": lambda st, f, kw=kw, Ms=Ms: st.overlap_moments(f, Ms, stat_step=1, **kw),
            f"overlap_moments 3 {tag}": lambda st, f, kw=kw, Ms=Ms: st.overlap_moments(f, Ms, include, stat_step=3, **kw),
            f"clip_stack_weighted {tag}": lambda st, f, kw=kww, Ms=Ms: st.clip_stack_weighted(f, Ms, SigmaClipParameters(2.0, 2.5, 2), gain, offset, weights,
                                                                                           return_counts=True, return_kept_weight=True, **kw),
            f"quantile_stack_weighted {tag}": lambda st, f, kw=kww, Ms=Ms: st.quantile_stack_weighted(f, Ms, 0.5, gain, offset, weights, include,
                                                                                                   return_counts=True, **kw),
        })
    return calls


COMBINE_CASES = [("u8c3", "x0", 320, 4, (4, 4, 4), True), ("u8c3", "x7", 323, 4, (4, 1, 1), True), ("u8c3", "uneven", 320, 4, (4, 1, 4), False),
                 ("u8c3", "odd_alt", 323, 4, (1, 1, 4), True),
                 ("u8c4", "x7", 323, 4, (4, 4, 4), True), ("u8c4", "odd_alt", 320, 4, (4, 4, 4), True),
                 ("u8c1", "odd_alt", 323, 4, (1, 1, 4), True),
                 ("u16c3", "x0", 320, 16, (16, 16, 16), True), ("u16c3", "x7", 320, 16, (16, 2, 2), True), ("u16c3", "uneven", 323, 16, (16, 2, 16), False),
                 ("u16c3", "odd_alt0", 323, 16, (2, 2, 16), True),
                 ("f32c3", "x7", 323, 4, (4, 4, 4), True), ("f32c3", "uneven", 320, 4, (4, 4, 4), False), ("f32c1", "odd_alt", 323, 4, (4, 4, 4), True)]


@LOC
@pytest.mark.parametrize("kind,layout,w,cap,align,even", COMBINE_CASES, ids=[f"{k}-{l}-{w}" for k, l, w, _, _, _ in COMBINE_CASES])
def test_combines_over_given_warps(stacker, kind, layout, w, cap, align, even, device):
    _run(stacker, _combines(kind, w), kind, w, layout, device, cap, align, even)


# ---- whole-stack sharpness -------------------------------------------------------------------------------------------------
SHARP_CASES = [("u8c1", "odd_alt", 323, (1, 1, 4), True), ("u8c1", "x7", 320, (4, 1, 1), True), ("u8c1", "x4", 320, (4, 4, 4), True),
               ("u8c3", "odd_alt", 320, (1, 1, 4), True), ("u8c3", "x0", 320, (4, 4, 4), True), ("u8c3", "uneven", 323, (4, 1, 4), False),
               ("u8c4", "odd_alt", 323, (4, 4, 4), True), ("u8c4", "uneven", 320, (4, 4, 4), False)]


@LOC
@pytest.mark.parametrize("kind,layout,w,align,even", SHARP_CASES, ids=[f"{k}-{l}-{w}" for k, l, w, _, _ in SHARP_CASES])
def test_stack_sharpness(stacker, kind, layout, w, align, even, device):
    calls = {f"stack_sharpness {k}": (lambda st, f, k=k: st.stack_sharpness(f, k)) for k in (3, 7)}
    _run(stacker, calls, kind, w, layout, device, 4, align, even)


# ---- stage level: against the tight call AND against the oracle ---------------------------------------------------------------
STAGE_LAYOUTS = [("x0", 320), ("x7", 320), ("x7", 323), ("odd_alt", 320), ("odd_alt", 323)]
H_PROJ = np.array([[1.01, 0.02, -3.3], [-0.015, 0.99, 4.1], [2e-5, -1e-5, 1.0]])
A_AFF = np.array([[0.99, 0.03, 1.7], [-0.03, 1.01, -2.2]])


def _one_frame(kind, w, layout, device, i=1):
    frames, canvas = _window(kind, w, layout, device)
    f = frames[i]
    assert not (f.is_contiguous() if device else f.flags.c_contiguous)
    return f, _tight(kind, w, device)[i], _content(kind, w)[i]


@LOC
@pytest.mark.parametrize("layout,w", STAGE_LAYOUTS)
@pytest.mark.parametrize("kind", ["u8c3", "u16c3", "f32c3", "u8c4"])
def test_grey(stacker, kind, layout, w, device):
    f, tight, host = _one_frame(kind, w, layout, device)
    got = stacker.grey(f)
    _assert_same_bits(got, stacker.grey(tight), "grey")
    assert np.array_equal(_flat(got, [])[0], oracle.grey(host[..., :3]))                 # the bar of test_grey_bit_exact


@LOC
@pytest.mark.parametrize("layout,w", STAGE_LAYOUTS)
@pytest.mark.parametrize("kind", ["u8c3", "u16c3"])
def test_grey_blur_f32(stacker, kind, layout, w, device):
    f, tight, host = _one_frame(kind, w, layout, device)
    for ksize in (3, 5, 7):
        got = stacker.grey_blur_f32(f, ksize)
        _assert_same_bits(got, stacker.grey_blur_f32(tight, ksize), f"grey_blur_f32 {ksize}")
        # the bars of test_fused_grey_blur_bit_exact / test_fused_grey_blur_u16_bit_exact: the oracle's bits
        g = oracle.grey(host)
        assert np.array_equal(_flat(got, [])[0], oracle.gaussian_blur_f32(g if kind == "u8c3" else g.astype(np.float32), ksize)), ksize


@LOC
@pytest.mark.parametrize("layout,w", STAGE_LAYOUTS)
@pytest.mark.parametrize("kind", ["u8c3", "u16c3", "f32c3", "u8c4", "f32c1"])
def test_warp_accumulate(stacker, kind, layout, w, device):
    f, tight, host = _one_frame(kind, w, layout, device)
    for M, kw in ((H_PROJ, {}), (A_AFF, dict(is_affine=True, border_mode=BORDER_REFLECT_101)), (np.eye(3), dict(border_value=(0.5, 0.25, 0.125, 1.0)))):
        got = stacker.warp_accumulate(f, M, **kw)
        _assert_same_bits(got, stacker.warp_accumulate(tight, M, **kw), "warp_accumulate")
        ref = oracle.warp_frame(host, M, **kw)
        # the bar of test_warp_perspective_matches_oracle: identical f32 operation sequence, <= 1e-6 abs (x 257 for 16-bit at alpha 1/255)
        assert np.max(np.abs(_flat(got, [])[0] - ref)) <= 1e-6 * (257.0 if kind == "u16c3" else 1.0)


@pytest.mark.parametrize("kind,layout,w", [("u8c3", "x7", 323), ("u8c3", "x0", 320), ("u16c3", "odd_alt0", 323), ("f32c3", "x7", 320)])
def test_warp_accumulate_into_a_padded_device_accumulator(stacker, kind, layout, w):
    import torch
    f, tight, host = _one_frame(kind, w, layout, True)
    c = host.shape[2]
    rng = np.random.default_rng(5)
    fill = torch.from_numpy(rng.random((H + 3, w + 4, c), dtype=np.float32)).to("cuda:0")
    for M, kw in ((H_PROJ, {}), (A_AFF, dict(is_affine=True, border_mode=BORDER_REFLECT_101))):
        big = fill.clone()
        view = big[2:2 + H, 3:3 + w]
        ref = stacker.warp_accumulate(tight, M, acc=view.contiguous(), **kw)
        got = stacker.warp_accumulate(f, M, acc=view, **kw)
        assert got is view
        _assert_same_bits(view, ref, "warp_accumulate into a padded accumulator")
        outside = torch.ones_like(big, dtype=torch.bool)
        outside[2:2 + H, 3:3 + w] = False
        assert torch.equal(big[outside], fill[outside])                       # the accumulator's padding is untouched


@LOC
def test_convert_f32_still_refuses_a_padded_frame(stacker, device):
    f, tight, host = _one_frame("u8c3", 320, "x7", device)
    with pytest.raises(InvalidParams, match="tightly packed"):
        stacker.convert_f32(f)
    assert np.array_equal(_flat(stacker.convert_f32(tight), [])[0], oracle.convert_f32(host))


# ---- validation: a stride below the row, a stride that is no whole number of elements --------------------------------------
def _families(st, kind, w):
    import torch
    Ms = _warps(w, False)[:3]                                       # (the test hands over three frames)

    def shard_sum():
        return torch.zeros((H, w, 3), dtype=torch.float32, device="cuda:0")
    fam = {
        "ecc_match": lambda f: st.ecc_match(f, ECC),
        "keypoint_match": lambda f: st.keypoint_match(f, KP),
        "hybrid_match": lambda f: st.hybrid_match(f, KP, ECC),
        "clip_stack": lambda f: st.clip_stack(f, Ms),
        "quantile_stack": lambda f: st.quantile_stack(f, Ms),
        "weighted_stack": lambda f: st.weighted_stack(f, Ms),
        "overlap_moments": lambda f: st.overlap_moments(f, Ms),
        "clip_stack_weighted": lambda f: st.clip_stack_weighted(f, Ms),
        "quantile_stack_weighted": lambda f: st.quantile_stack_weighted(f, Ms),
        "ecc_match_weighted": lambda f: st.ecc_match_weighted(f, ECC),
        "ecc_match_clipped": lambda f: st.ecc_match_clipped(f, ECC),
        "keypoint_match_quantile": lambda f: st.keypoint_match_quantile(f, KP),
        "grey": lambda f: st.grey(f[0]),
        "grey_blur_f32": lambda f: st.grey_blur_f32(f[0], 5),
        "warp_accumulate": lambda f: st.warp_accumulate(f[0], H_PROJ),
        "convert_f32": lambda f: st.convert_f32(f[0]),
        "ecc_match_shard": lambda f: st.ecc_match_shard(f, ECC, True, shard_sum()),
        "hybrid_match_shard": lambda f: st.hybrid_match_shard(f, KP, ECC, True, shard_sum()),
    }
    if kind == "u8c3":
        fam.update({
            "stack_sharpness": lambda f: st.stack_sharpness(f, 3),
            "ecc_match_ranked": lambda f: st.ecc_match_ranked(f, ECC),
            "keypoint_match_ranked": lambda f: st.keypoint_match_ranked(f, KP),
            "keypoint_match_shard": lambda f: st.keypoint_match_shard(f, KP, True, shard_sum()),
            "keypoint_match_clipped": lambda f: st.keypoint_match_clipped(f, KP),
            "keypoint_match_weighted": lambda f: st.keypoint_match_weighted(f, KP),
            "ecc_match_quantile": lambda f: st.ecc_match_quantile(f, ECC),
            "ecc_match_clipped_weighted": lambda f: st.ecc_match_clipped_weighted(f, ECC),
            "ecc_match_quantile_weighted": lambda f: st.ecc_match_quantile_weighted(f, ECC),
            "keypoint_match_clipped_weighted": lambda f: st.keypoint_match_clipped_weighted(f, KP),
            "keypoint_match_quantile_weighted": lambda f: st.keypoint_match_quantile_weighted(f, KP),
        })
    return fam


@LOC
@pytest.mark.parametrize("kind,bad", [("u8c3", -1), ("u16c3", -2), ("u16c3", +1), ("f32c3", +2), ("f32c3", -4)])
def test_invalid_strides_are_refused_and_the_context_stays_usable(stacker, monkeypatch, kind, bad, device):
    """bad < 0: the stride is that many bytes short of a tight row; bad > 0: that many bytes beyond a tight row of a buffer
    that HAS room for it, but no multiple of the element size."""
    w = 320
    el = DTYPE[kind[:-2]]().itemsize
    tight_row = w * 3 * el
    frames, _ = _window(kind, w, "x0", device)                       # (rows of 336 pixels: a stride a few bytes above the tight row stays inside)
    frames = list(frames)[:3]
    real = api._Marshalled

    class Bad(real):
        def __init__(self, fr):
            super().__init__(fr)
            self.c_frames.row_stride_bytes = tight_row + bad
    good = {}
    fam = _families(stacker, kind, w)
    # the entry points that take 16-bit / f32 frames at all (8-bit BGR: every one of the table)
    per_type = {"u16c3": ("hybrid_match", "hybrid_match_shard", "clip_stack", "quantile_stack", "weighted_stack", "overlap_moments", "clip_stack_weighted",
                          "quantile_stack_weighted", "grey", "grey_blur_f32", "warp_accumulate", "convert_f32"),
                "f32c3": ("ecc_match", "ecc_match_shard", "clip_stack", "quantile_stack", "weighted_stack", "overlap_moments", "clip_stack_weighted",
                          "quantile_stack_weighted", "ecc_match_weighted", "ecc_match_clipped", "grey", "grey_blur_f32", "warp_accumulate",
                          "convert_f32")}
    names = [k for k in fam if kind == "u8c3" or k in per_type[kind]]
    for name in names:
        monkeypatch.setattr(api, "_Marshalled", Bad)
        with pytest.raises(InvalidParams, match="row stride"):
            fam[name](frames)
        monkeypatch.setattr(api, "_Marshalled", real)
        if name != "convert_f32":                                    # (which refuses the padded frame for its own reason)
            good[name] = fam[name](frames)                           # the context took no harm: the same call with the true stride
    tight = list(_tight(kind, w, device))[:3]
    for name in ("ecc_match", "hybrid_match", "clip_stack", "warp_accumulate"):
        if name in good:
            _assert_same_bits(good[name], fam[name](tight), name)


def test_mixed_geometry_refuses_invalid_strides(stacker):
    """stk_keypoint_match_mixed: per-frame geometry; a stride below a frame's row in any entry, also when all entries are
    equal and the stack goes on to stk_keypoint_match."""
    from libstacker_rs_amd import _ffi
    fr = [np.ascontiguousarray(f) for f in _content("u8c3", 320)[:3]]
    small = np.ascontiguousarray(fr[1][:200, :300])
    n = 3
    out = np.empty((H, 320, 3), np.float32)
    img = _ffi.ImageF32(out.ctypes.data, 320, H, 3, 0, 0)
    p = KP._c()
    dropped = C.c_int32(0)

    def call(frames, geos):
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        geo = (_ffi.FrameGeometry * n)(*[_ffi.FrameGeometry(*g) for g in geos])
        frs = _ffi.Frames(C.cast(ptrs, C.POINTER(C.c_void_p)), n, 320, H, 3, 8, 0, 0)
        return stacker._lib.stk_keypoint_match_mixed(stacker._h, C.byref(frs), geo, C.byref(p), 0.0, C.byref(img), C.byref(dropped), None)
    assert call(fr, [(320, H, 959)] * 3) == 2                                           # uniform: through check_frames
    assert call([fr[0], small, fr[2]], [(320, H, 0), (300, 200, 899), (320, H, 0)]) == 2  # frame by frame
    assert call([fr[0], small, fr[2]], [(320, H, 0), (300, 200, 0), (320, H, 0)]) == 0
    base = out.copy()
    assert call([fr[0], small, fr[2]], [(320, H, 960), (300, 200, 900), (320, H, 960)]) == 0 and np.array_equal(out, base)

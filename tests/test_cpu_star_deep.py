"""CPU tests of star registration on 16-bit and f32 frames (include/stacker.h, stk_star_deep_params): the restatement of the
key and of detection on it (tests/star_deep_restate.py) against star_restate on 8-bit frames and against the header's
consequences, the faint-star field the 16-bit key exists for, the restated pipeline on the eight motions rendered at 16
bits, and the struct, the symbols and what the three new wrappers hand to the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import libstacker_rs_amd as ls
import star_deep_restate as sd
import star_restate as sr
from libstacker_rs_amd import StarDeepParameters, StarParameters, _ffi, synth
from test_cpu_api_calls import CTX, new_stacker
from test_cpu_star import H, MOTIONS, SEED, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_star_detect_deep", "stk_star_align_deep", "stk_star_match_deep")
# the generator's 8-bit defaults (sky 18 .. 28, noise sigma 2, faintest peak 24) and the detector's min_contrast 8, in
# 16-bit counts
DEEP16 = dict(sky=(18.0 * 257, 28.0 * 257), noise_sigma=2.0 * 257, min_peak=24.0 * 257, depth=16)
P16 = dict(min_contrast=8 * 257)
# The faint field: sky about 2000 ADU, noise sigma 40, peaks 200 (1 + Pareto(10)) ADU: 200 .. 260 over the sky on this seed.
# min_contrast: the default 8 is 4 sigma of the generator's default noise (sigma 2); in this field's key units 4 sigma = 160.
# (8 * 257 = 2056 ADU would exceed every star of the field: the factor between the units of two fields is their noise's.)
FAINT = dict(sky=(1980.0, 2020.0), noise_sigma=40.0, min_peak=200.0, pareto_shape=10.0, depth=16)
FAINT_P = dict(min_contrast=160)
FAINT_SEED = 2
# The faint STACK: the same sky and noise with 240 stars per frame area of 220 (1 + Pareto(20)) ADU and max_stars = 400 (a single star: 220 .. 300 ADU; where two overlap the sum is brighter). A
# centroid of such a star carries a few tenths of a pixel of noise and the corner error of a fit falls with the square root of
# the stars it rests on: with 60 stars of the field above the four seeds tried gave 0.28 .. 0.70 px, with these 240 seed 2
# gives 0.27 / 0.22 / 0.16 px (seeds 3 .. 6: 0.19 .. 1.2 px, and one wrong fit of 2.4 px).
FAINT_STACK = dict(FAINT, min_peak=220.0, pareto_shape=20.0)
FAINT_STACK_P = dict(min_contrast=160, max_stars=400)


def motion_stack16(k, seed=SEED):
    ang, tx, ty, sc, ns = MOTIONS[k]
    mots = [None, synth.star_motion(W, H, ang, tx, ty, sc, 1e-6, -1e-6)]
    return synth.make_star_stack(mots, W, H, ns, seed=seed + k, **DEEP16)


def faint_stack(n=4, channels=3):
    """frame 0 and n - 1 frames turned and shifted by up to a few degrees and pixels, and one of them by half a turn"""
    mots = [None] + [synth.star_motion(W, H, a, tx, ty) for a, tx, ty in ((3.0, 6.0, -4.0), (180.0, 2.0, 1.0), (-7.0, -9.0, 5.0))][:n - 1]
    return synth.make_star_stack(mots, W, H, 240, seed=FAINT_SEED, channels=channels, **FAINT_STACK)


def reduce8(f16):
    """the (K + 128) / 257 reduction of a 16-bit frame: what the 8-bit aligners are given"""
    return ((sd.key(f16).astype(np.int64) + 128) // 257).astype(np.uint8)


# ---- 1. on 8-bit frames the restatement is star_restate's -------------------------------------------------------------
def test_the_generator_at_depth_8_is_unchanged_and_at_16_is_seeded():
    a, Ga = synth.make_star_stack([None], 64, 48, 20, seed=3)
    b, _ = synth.make_star_stack([None], 64, 48, 20, seed=3, depth=8)
    assert a.dtype == np.uint8 and np.array_equal(a, b)
    c, _ = synth.make_star_stack([None], 64, 48, 20, seed=3, channels=4, **DEEP16)
    d, _ = synth.make_star_stack([None], 64, 48, 20, seed=3, channels=4, **DEEP16)
    assert c.dtype == np.uint16 and c.shape == (1, 48, 64, 4) and np.array_equal(c, d) and (c[..., 3] == 65535).all()
    assert c[..., 0].max() > 24 * 257 and np.array_equal(c[..., 0], c[..., 2])
    with pytest.raises(ValueError):
        synth.make_star_stack([None], 64, 48, 20, depth=32)


@pytest.mark.parametrize("cn", [1, 3, 4])
def test_restatement_on_u8_frames_equals_star_restate(cn):
    frames, _ = synth.make_star_stack([None, synth.star_motion(200, 150, 33.0, 5.0, -4.0)], 200, 150, 40, seed=5, channels=cn)
    rng = np.random.default_rng(cn)
    noise = rng.integers(0, 256, (70, 130) + ((cn,) if cn > 1 else ()), dtype=np.uint8)
    found = 0
    for f in list(frames) + [noise]:
        for p in (StarParameters(), StarParameters(radius=2, min_pixels=1, max_stars=1024), StarParameters(radius=7, kappa=1.0, min_contrast=3, max_stars=50)):
            want, n_want = sr.detect(f, p)
            got, n_got = sd.detect(f, p)
            assert n_got == n_want and got.tobytes() == want.tobytes()
            found += len(want)
    assert found > 100


def test_key_by_hand():
    # u16 BGR: (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14; the weights sum to 2^14, so equal channels give the value itself
    f = np.array([[[65535, 65535, 65535, 7], [1000, 2000, 3000, 9]]], np.uint16)
    assert sd.key(f).tolist() == [[65535, (1000 * 1868 + 2000 * 9617 + 3000 * 4899 + 8192) >> 14]]
    assert sd.key(f[..., :3]).tolist() == sd.key(f).tolist()               # the fourth channel is not read
    assert sd.key(np.array([[300, 65535]], np.uint16)).tolist() == [[300, 65535]]
    # f32, one channel: rint to even, the clamp, NaN -> 0, the infinities
    v = np.array([[0.5, 1.5, 2.5, -3.0, 65535.4, 65536.0, 1e9, np.nan, np.inf, -np.inf]], np.float32)
    assert sd.key(v).tolist() == [[0, 2, 2, 0, 65535, 65535, 65535, 0, 65535, 0]]
    assert sd.key(np.array([[0.25, 1.0, 2.0]], np.float32), StarDeepParameters(f32_scale=65535.0)).tolist() == [[16384, 65535, 65535]]
    # f32 BGR: (b * 0.114f + g * 0.587f) + r * 0.299f in f32; +inf and -inf in one pixel make a NaN
    px = np.array([[[100.0, 200.0, 300.0], [np.inf, -np.inf, 1.0]]], np.float32)
    gf = np.float32(np.float32(np.float32(100.0) * np.float32(0.114)) + np.float32(np.float32(200.0) * np.float32(0.587))) + np.float32(np.float32(300.0) * np.float32(0.299))
    assert sd.key(px).tolist() == [[int(np.rint(gf)), 0]]


def test_consequences_of_the_definition():
    rng = np.random.default_rng(11)
    g = rng.integers(0, 24, (70, 130)).astype(np.uint8)
    for y, x in zip(rng.integers(8, 62, 12), rng.integers(8, 122, 12)):
        g[y - 1:y + 2, x - 1:x + 2] = rng.integers(60, 256)
    p = StarParameters(min_pixels=2)
    want, n = sr.detect(g, p)
    assert len(want) >= 6
    got16, n16 = sd.detect(g.astype(np.uint16), p)                         # a one-channel u16 frame with values <= 255
    assert n16 == n and got16.tobytes() == want.tobytes()
    f16, _ = synth.make_star_stack([None], 200, 150, 40, seed=5, **DEEP16)
    p = StarParameters(**P16)
    a, na = sd.detect(f16[0], p)
    b, nb = sd.detect(f16[0].astype(np.float32), p, StarDeepParameters(1.0))   # an f32 frame holding the u16 values
    assert len(a) >= 20 and na == nb and a.tobytes() == b.tobytes()


def test_tile_statistics_by_hand():
    # 64 x 64 = 4096 keys, k = 2048. 2000 keys of 300 (high byte 1), 2096 of 40000 (high byte 156): the 2048th smallest is
    # 40000; |K - med| is 0 for 2096 keys: mad 0, d = min_contrast
    K = np.full(4096, 40000, np.int64)
    K[:2000] = 300
    med, mad, thr = sd.tile_stats(K.reshape(64, 64), StarParameters(min_contrast=1000))
    assert (med[0, 0], mad[0, 0], thr[0, 0]) == (40000, 0, 41000)
    # 0 .. 4095 times 16: k-th smallest = 2047 * 16 = 32752; |K - med| = 16 |i - 2047|: the values 0, 16, 16, 32, 32, ... so the
    # 2048th smallest is 16 * 1024 = 16384 (1 + 2 * 1023 = 2047 values lie below it)
    K = np.arange(4096, dtype=np.int64) * 16
    med, mad, thr = sd.tile_stats(K.reshape(64, 64), StarParameters(kappa=1.0, min_contrast=1))
    ks = np.float32(np.float64(np.float32(1.0)) * 1.4826)
    assert (med[0, 0], mad[0, 0]) == (32752, 16384) and thr[0, 0] == 32752 + int(np.ceil(ks * np.float32(16384)))
    # the clamp: ks * mad beyond 65536 gives d = 65536, and no key reaches the threshold
    med, mad, thr = sd.tile_stats(K.reshape(64, 64), StarParameters(kappa=100.0, min_contrast=1))
    assert thr[0, 0] == 32752 + 65536
    assert sd.detect(K.reshape(64, 64).astype(np.uint16), StarParameters(kappa=100.0, min_contrast=1))[1] == 0


# ---- 2. the faint field ---------------------------------------------------------------------------------------------
def test_faint_stars_are_found_on_the_key_and_lost_by_the_8_bit_reduction():
    """480 x 360, sky 1980 .. 2020 ADU, noise sigma 40, 60 stars per frame area with peaks 200 .. 260 ADU over the sky
    (noise-free render; seed 2). Measured here: the detection on the key finds 51 stars (51 peaks) under the default
    parameters with min_contrast = 160 ADU; star_restate.detect on the (K + 128) / 257 reduction — a frame of grey 7 and 8, the
    brightest star one level up — finds 0. min_stars is 6."""
    frames, _ = synth.make_star_stack([None], W, H, 60, seed=FAINT_SEED, channels=1, **FAINT)
    clean, _ = synth.make_star_stack([None], W, H, 60, seed=FAINT_SEED, channels=1, **dict(FAINT, noise_sigma=0.0))
    over = int(clean[0].max()) - 2020
    assert frames.dtype == np.uint16 and 200 <= over <= 300
    p = StarParameters(**FAINT_P)
    deep, n_deep = sd.detect(frames[0], p)
    flat, n_flat = sr.detect(reduce8(frames[0]), StarParameters())
    print("faint field: brightest star", over, "ADU over the sky; key:", len(deep), "stars,", n_deep, "peaks; 8-bit reduction:", len(flat), "stars")
    assert len(deep) >= 4 * p.min_stars                                     # with room: four times what a frame needs
    assert len(flat) < p.min_stars and len(flat) <= 1
    # they are stars, not noise: the same field without noise has a peak within 1.5 px of (nearly) every one
    truth, _ = sd.detect(clean[0], StarParameters(min_contrast=40))
    d = np.hypot(deep["x"][:, None] - truth["x"][None, :], deep["y"][:, None] - truth["y"][None, :]).min(1)
    assert (d <= 1.5).mean() >= 0.9


def test_faint_stack_registers_on_the_key_only():
    frames, G = faint_stack(4, channels=1)
    stats, lists = sd.align(list(frames), StarParameters(**FAINT_STACK_P))
    assert [s["status"] for s in stats] == [0, 0, 0, 0]
    errs = [synth.corner_error(stats[i]["warp"], G[i], W, H) for i in range(1, 4)]
    print("faint stack: corner errors", np.round(errs, 3), "stars", [len(l) for l in lists])
    assert max(errs) <= 0.5
    stats8, lists8 = sr.align([reduce8(f) for f in frames])
    assert [s["status"] for s in stats8] == [0, 1, 1, 1] and max(len(l) for l in lists8) < StarParameters().min_stars


# ---- 3. the eight motions at 16 bits --------------------------------------------------------------------------------
def test_restated_deep_pipeline_on_the_motions_at_16_bits():
    results = []
    for k in range(len(MOTIONS)):
        frames, G = motion_stack16(k)
        assert frames.dtype == np.uint16 and frames.shape == (2, H, W, 3)
        stats, lists = sd.align(list(frames), StarParameters(**P16))
        err = synth.corner_error(stats[1]["warp"], G[1], W, H)
        results.append((MOTIONS[k][0], len(lists[0]), len(lists[1]), stats[1]["status"], stats[1]["n_matches"], stats[1]["n_inliers"], round(err, 3)))
    print(results)
    for r in results:                                                      # the project's own bar (test_cpu_star.py)
        if min(r[1], r[2]) >= 12:
            assert r[3] == 0 and r[-1] <= 0.5, r
    assert sum(min(r[1], r[2]) >= 12 for r in results) >= 7


# ---- 4. struct, symbols, wrappers -----------------------------------------------------------------------------------
def test_struct_layout_symbols_and_table_against_the_header(tmp_path):
    fields = [f for f, _ in _ffi.StarDeepParams._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(stk_star_deep_params));\n' +
                   "".join('  printf(" %%zu", offsetof(stk_star_deep_params, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_ffi.StarDeepParams)] + [getattr(_ffi.StarDeepParams, f).offset for f in fields] == [8, 0, 4]
    lib = _ffi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stacker.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name) and re.search(r" T %s\b" % name, nm)
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        res, sig = _ffi.SIGNATURES[name]
        assert res is _ffi.c_status and len(args.split(",")) == len(sig), name
        assert sig[2] is C.POINTER(_ffi.StarParams) and sig[3] is C.POINTER(_ffi.StarDeepParams)
    assert _ffi.SIGNATURES["stk_star_match_deep"][1][4] is C.c_double
    rs = open(os.path.join(ROOT, "rust", "src", "amd_ffi.rs")).read()
    assert all("pub fn %s(" % name in rs for name in NEW) and "pub struct stk_star_deep_params" in rs
    assert ls.StarDeepParameters is StarDeepParameters and "StarDeepParameters" in ls.__all__
    d = StarDeepParameters()._c()
    assert (d.f32_scale, d.reserved) == (1.0, 0) and StarDeepParameters(65535.0)._c().f32_scale == 65535.0
    for method in ("star_detect_deep", "star_align_deep", "star_match_deep"):
        assert callable(getattr(ls.Stacker, method))


def _frames_of_arg(arg):
    f = arg._obj                                                           # byref(m.c_frames): the structure itself
    assert isinstance(f, _ffi.Frames)
    return dict(n=f.n, width=f.width, height=f.height, channels=f.channels, depth=f.depth, location=f.location, stride=f.row_stride_bytes,
                data=[bytes(C.string_at(f.data[k], f.width * f.height * f.channels * (f.depth // 8))) for k in range(f.n)])


def _spy_frames(st, name, seen):
    """the stand-in's function `name`, recording the stk_frames it is given AT CALL TIME into `seen`"""
    real = getattr(st._lib, name)

    def call(*a):
        seen["frames"] = _frames_of_arg(a[1])
        return real(*a)
    setattr(st._lib, name, call)


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32])
def test_what_the_wrappers_hand_to_the_c_abi(dt):
    rng = np.random.default_rng(8)
    n, h, w, cn = 3, 6, 7, 3
    frames = rng.integers(0, 200, (n, h, w, cn)).astype(dt)
    depth = 8 * np.dtype(dt).itemsize
    sp, dp = StarParameters(radius=3, max_stars=7, min_contrast=900, border_value=(1.0, 2.0)), StarDeepParameters(f32_scale=16.0)

    def check_frames(seen):
        f = seen["frames"]
        assert (f["n"], f["width"], f["height"], f["channels"], f["depth"], f["location"], f["stride"]) == (n, w, h, cn, depth, 0, 0)
        assert f["data"] == [frames[i].tobytes() for i in range(n)]

    st, seen = new_stacker(), {}
    _spy_frames(st, "stk_star_detect_deep", seen)
    lists, peaks = st.star_detect_deep(frames, sp, dp, return_peaks=True)
    name, snap = st._lib.last()
    check_frames(seen)
    assert name == "stk_star_detect_deep" and snap[0] == CTX and snap[2] == _bytes_of(sp._c()) and snap[3] == _bytes_of(dp._c())
    assert all(snap[4:7]) and snap[6] == peaks.ctypes.data and len(lists) == n and peaks.dtype == np.int32 and peaks.shape == (n,)
    assert isinstance(st.star_detect_deep(frames), list)
    assert st._lib.last()[1][2:4] == [_bytes_of(StarParameters()._c()), _bytes_of(StarDeepParameters()._c())]

    st, seen = new_stacker(), {}
    st._lib.pokes = {4: 2}
    _spy_frames(st, "stk_star_align_deep", seen)
    dropped, stats = st.star_align_deep(frames, sp, dp)
    name, snap = st._lib.last()
    check_frames(seen)
    assert name == "stk_star_align_deep" and snap[2:4] == [_bytes_of(sp._c()), _bytes_of(dp._c())] and snap[4] and snap[5]
    assert dropped == 2 and len(stats) == n and set(stats[0]) >= {"status", "warp", "n_keypoints", "n_matches", "n_inliers"}

    for return_stats in (False, True):
        for alpha, want in ((None, {8: 1.0 / 255.0, 16: 1.0 / 65535.0, 32: 1.0 / 16.0}[depth]), (0.125, 0.125)):
            st, seen = new_stacker(), {}
            st._lib.pokes = {6: 1}
            _spy_frames(st, "stk_star_match_deep", seen)
            res = st.star_match_deep(frames, sp, dp, alpha=alpha, return_stats=return_stats)
            name, snap = st._lib.last()
            check_frames(seen)
            assert name == "stk_star_match_deep" and snap[2:4] == [_bytes_of(sp._c()), _bytes_of(dp._c())]
            assert type(snap[4]) is float and snap[4] == want
            assert isinstance(res, tuple) and len(res) == 2 + return_stats and res[0] == 1
            out = res[1]
            assert out.shape == (h, w, cn) and out.dtype == np.float32 and snap[5]["data"] == out.ctypes.data
            assert (snap[5]["width"], snap[5]["height"], snap[5]["channels"]) == (w, h, cn) and snap[6] and snap[7]
    for method in ("star_detect_deep", "star_align_deep", "star_match_deep"):
        with pytest.raises(ls.NotEnoughFiles):
            getattr(new_stacker(), method)([])


def test_the_8_bit_wrappers_hand_over_what_they_did():
    """star_detect, star_align and star_match are built from the same helpers now: the C function and the argument count"""
    frames = np.zeros((2, 6, 7, 3), np.uint8)
    for method, cname, nargs in (("star_detect", "stk_star_detect", 6), ("star_align", "stk_star_align", 5), ("star_match", "stk_star_match", 6)):
        st = new_stacker()
        getattr(st, method)(frames, StarParameters(radius=3))
        name, snap = st._lib.last()
        assert name == cname and len(snap) == nargs and snap[2] == _bytes_of(StarParameters(radius=3)._c())

"""Blot-and-compare rejection maps (include/stacker.h, stk_reject_params) without a GPU: the numpy restatement
(reject_restate.py) against answers worked out by hand, the experiment the feature exists for (a planted trail and hot
pixels in a dithered stack, drizzled with and without the maps), and the ctypes mirror against the header."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import drizzle_restate as dr
import reject_restate as rr
from libstacker_rs_amd import RejectParameters, _ffi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = pytest.mark.parametrize("dtype", [np.float64, F], ids=["f64", "f32"])


def shift(sx, sy):
    M = np.eye(3)
    M[0, 2], M[1, 2] = sx, sy
    return M


def params(**kw):
    base = dict(snr1=4.0, snr2=3.0, scale1=1.2, scale2=0.7, read_noise=0.01, poisson_gain=0.0, min_count=0)
    base.update(kw)
    return RejectParameters(**base)


@MODES
def test_constant_clean_image_first_flag_and_grow(dtype):
    """C = 0.5 everywhere, identity, rn = 0.01, pg = 0: D = 0 and the tests are |u - 0.5| > 0.04 and > 0.03.
    (4, 4) at +0.05 fails the first. (5, 4) at +0.035 passes the first (0.035 < 0.04), fails the second (0.035 > 0.03) and
    has a flagged neighbour: rejected through the grow step only. (6, 4) at +0.035 is next to (5, 4), which carries no
    FIRST flag: kept, the grow step does not chain. (2, 4) at +0.035 is two away from (4, 4): kept. (8, 7) at +0.035 has
    no flagged neighbour: kept."""
    h, w = 10, 12
    clean = np.full((h, w, 1), 0.5, F)
    frame = clean.copy()
    frame[4, 4], frame[4, 5], frame[4, 6], frame[4, 2], frame[7, 8] = 0.55, 0.535, 0.535, 0.535, 0.535
    out, rej, jud, d = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(), dtype=dtype)
    assert np.array_equal(d["D"], np.zeros((h, w, 1), dtype))
    want = np.ones((h, w), F)
    want[4, 4] = want[4, 5] = 0
    assert np.array_equal(out, want) and rej == 2
    assert d["f1"].sum() == 1 and d["f1"][4, 4] and d["f2"][4, 5] and not d["f1"][4, 5]
    # identity: ix = x, so the last column and the last row (ix + 1 > sw - 1) are not judged
    assert jud == (h - 1) * (w - 1) and not d["judged"][:, -1].any() and not d["judged"][-1].any()
    # an identity matrix with C equal to the frame rejects nothing
    out, rej, _, _ = rr.reject_frame(clean, np.eye(3), False, 1.0, clean, params(read_noise=0.0), dtype=dtype)
    assert rej == 0 and np.array_equal(out, np.ones((h, w), F))


@MODES
def test_ramp_gradient_term(dtype):
    """C = x / 16 (slope s = 2^-4 along x): D = s at every judged pixel (at x = 0 from the right neighbour alone). rn = 0:
    the test is e > scale * s. A sample off by 1.125 s (dyadic: the same number in both modes) is kept under scale1 = 1.2
    and rejected under scale1 = 1.0."""
    h, w, s = 8, 14, 2.0 ** -4
    clean = np.tile((np.arange(w) * s).astype(F)[None, :, None], (h, 1, 1))
    frame = clean.copy()
    frame[3, 6] += F(1.125 * s)
    out, rej, jud, d = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(read_noise=0.0, scale2=1.2), dtype=dtype)
    assert np.array_equal(d["D"][d["judged"]], np.full((jud, 1), s, dtype))
    assert rej == 0 and np.array_equal(out, np.ones((h, w), F))
    out, rej, _, d = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(read_noise=0.0, scale1=1.0, scale2=1.2), dtype=dtype)
    assert rej == 1 and out[3, 6] == 0 and d["f1"][3, 6]
    # the default second scale does not reject it on its own either: no first flag, nothing to grow from
    out, rej, _, _ = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(read_noise=0.0), dtype=dtype)
    assert rej == 0


@MODES
def test_integer_translation_blots_exactly(dtype):
    """Forward warp (+2, -1): frame pixel (x, y) lies at frame-0 coordinate (x + 2, y - 1), ax = ay = 0 and
    B(x, y) = C[y - 1][x + 2]. Valid: 0 <= x + 2, x + 3 <= sw - 1, 0 <= y - 1, y <= sh - 1: row 0 (its taps leave frame 0),
    columns sw - 2, sw - 1 (they leave it too) and column sw - 3 (the last in-frame ring) are not judged and keep 1,
    whatever the frame holds there."""
    rng = np.random.default_rng(3)
    h, w = 9, 11
    clean = rng.uniform(0, 1, (h, w, 1)).astype(F)
    B, valid = rr.blot(clean, shift(2, -1), False, dtype=dtype, halo=0)
    want_valid = np.zeros((h, w), bool)
    want_valid[1:, :w - 3] = True
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(B[1:, :w - 3], clean[:h - 1, 2:w - 1].astype(dtype))
    frame = np.zeros((h, w, 1), F)
    frame[1:, :w - 3] = clean[:h - 1, 2:w - 1]
    frame[0, :], frame[:, w - 3:] = 9.0, 9.0                     # wildly off where nothing can be compared
    frame[5, 4] += F(0.5)
    out, rej, jud, _ = rr.reject_frame(frame, shift(2, -1), False, 1.0, clean, params(scale1=0.0, scale2=0.0), dtype=dtype)
    want = np.ones((h, w), F)
    want[5, 4] = 0
    assert np.array_equal(out, want) and rej == 1 and jud == (h - 1) * (w - 3)
    # the same through an affine table entry
    out_a, rej_a, jud_a, _ = rr.reject_frame(frame, shift(2, -1), True, 1.0, clean, params(scale1=0.0, scale2=0.0), dtype=dtype)
    assert np.array_equal(out_a, out) and (rej_a, jud_a) == (rej, jud)


@MODES
def test_a_thin_clean_pixel_judges_nothing(dtype):
    """cnt < min_count at clean pixel (5, 3) (x, y): under the identity exactly the frame pixels (4 .. 5, 2 .. 3), whose four
    taps include it, become unjudged."""
    h, w = 8, 10
    clean = np.full((h, w, 1), 0.5, F)
    frame = np.full((h, w, 1), 0.9, F)                            # everything judged is rejected
    cnt = np.full((h, w), 5, np.int32)
    cnt[3, 5] = 2
    base, _, jud0, d0 = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(min_count=3), dtype=dtype)
    out, rej, jud, d = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(min_count=3), counts=cnt, dtype=dtype)
    gone = d0["judged"] & ~d["judged"]
    want = np.zeros((h, w), bool)
    want[2:4, 4:6] = True
    assert np.array_equal(gone, want) and jud == jud0 - 4 and rej == jud
    assert np.array_equal(out == 1, ~d["judged"])
    # min_count = 2 accepts it
    _, _, jud2, _ = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(min_count=2), counts=cnt, dtype=dtype)
    assert jud2 == jud0


@MODES
def test_input_maps(dtype):
    h, w = 8, 10
    clean = np.full((h, w, 1), 0.5, F)
    frame = clean.copy()
    frame[2, 2], frame[4, 6] = 0.9, 0.9
    mi = np.full((h, w), 0.25, F)
    mi[2, 2] = 0.0                                              # a zero input pixel is not judged and stays 0
    out, rej, jud, d = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(), map_in=mi, dtype=dtype)
    want = mi.copy()
    want[4, 6] = 0.0
    assert np.array_equal(out, want) and rej == 1 and not d["judged"][2, 2] and jud == (h - 1) * (w - 1) - 1
    # a masked pixel is no seed of the grow step either
    frame[2, 3] = 0.535
    out, rej, _, _ = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(), map_in=mi, dtype=dtype)
    assert out[2, 3] == F(0.25) and rej == 1
    # in place: the definition reads a pixel's own input value only
    buf = mi.copy()
    buf[...] = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(), map_in=buf, dtype=dtype)[0]
    assert np.array_equal(buf, out)


@MODES
def test_nan_keeps(dtype):
    """A NaN in C makes B NaN at the pixels whose taps include it: e is NaN, every comparison false, the pixels are kept
    whatever they hold. A neighbour's gradient skips the NaN difference (fmax). A NaN sample is kept."""
    h, w = 8, 10
    clean = np.full((h, w, 1), 0.5, F)
    clean[3, 5] = np.nan
    frame = np.full((h, w, 1), 0.5, F)
    frame[2:4, 4:6] = 0.9                                        # the four pixels the NaN reaches
    frame[6, 2] = np.nan
    frame[6, 7] = 0.9
    out, rej, _, d = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, params(), dtype=dtype)
    want = np.ones((h, w), F)
    want[6, 7] = 0
    assert np.array_equal(out, want) and rej == 1
    assert np.isnan(d["B"][2:4, 4:6]).all() and not np.isnan(d["D"]).any()


@MODES
def test_records_bring_a_frame_onto_the_clean_level(dtype):
    """A frame at half the level with g = 2 (and one at level - 0.25 with o = 0.25) judges like the original: dyadic
    values, the products are exact."""
    rng = np.random.default_rng(5)
    h, w = 9, 12
    clean = (rng.integers(64, 192, (h, w, 1)) / 256.0).astype(F)
    frame = clean.copy()
    frame[4, 4] += F(0.25)
    frame[6, 8] -= F(0.125)
    p = params(read_noise=2.0 ** -6, scale1=0.0, scale2=0.0)          # (C is white noise: the gradient term is switched off)
    ref = rr.reject_frame(frame, np.eye(3), False, 1.0, clean, p, dtype=dtype)
    assert ref[1] >= 2
    half = rr.reject_frame(frame * F(0.5), np.eye(3), False, 1.0, clean, p, gain=[2.0], dtype=dtype)
    off = rr.reject_frame(frame - F(0.25), np.eye(3), False, 1.0, clean, p, offset=[0.25], dtype=dtype)
    for got in (half, off):
        assert np.array_equal(got[0], ref[0]) and got[1:3] == ref[1:3]


def test_degenerate_sizes():
    p = params()
    out, rej, jud = rr.reject_maps([np.full((1, 1, 1), 9.0, F)], [np.eye(3)], False, 1.0, np.zeros((1, 1, 1), F), p)
    assert np.array_equal(out, np.ones((1, 1, 1), F)) and rej[0] == 0 and jud[0] == 0
    clean = np.full((3, 5, 1), 0.5, F)
    frame = clean.copy()
    frame[1, 1] = 0.9
    out, rej, jud = rr.reject_maps([frame], [np.eye(3)], False, 1.0, clean, p)
    assert rej[0] == 1 and jud[0] == 2 * 4 and out[0, 1, 1] == 0


def test_struct_layout_matches_the_header(tmp_path):
    names = ["snr1", "snr2", "scale1", "scale2", "read_noise", "poisson_gain", "min_count", "reserved"]
    src = tmp_path / "reject_sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n'
                   '    printf("%d' + " %d" * len(names) + '\\n", (int)sizeof(stk_reject_params)'
                   + "".join(f", (int)offsetof(stk_reject_params, {n})" for n in names) + ");\n    return 0;\n}\n")
    exe = tmp_path / "reject_sizes"
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _ffi.RejectParams
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert [n for n, _ in S._fields_] == names
    p = RejectParameters(snr1=5.0, snr2=2.5, scale1=1.5, scale2=0.5, read_noise=0.25, poisson_gain=0.125, min_count=4)._c()
    assert (p.snr1, p.snr2, p.scale1, p.scale2, p.read_noise, p.poisson_gain, p.min_count, p.reserved) == (5.0, 2.5, 1.5, 0.5, 0.25, 0.125, 4, 0)
    d = RejectParameters()
    assert (d.snr1, d.snr2, d.scale1, d.scale2, d.min_count) == (4.0, 3.0, 1.2, 0.7, 3)


def _header_functions():
    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    _, _, funcs, _ = gen.parse(open(os.path.join(ROOT, "include", "stacker.h")).read())
    return {name: plist for name, _, plist in funcs}


STRUCTS = {"stk_frames": _ffi.Frames, "stk_ecc_params": _ffi.EccParams, "stk_keypoint_params": _ffi.KeypointParams,
           "stk_drizzle_params": _ffi.DrizzleParams, "stk_weight_params": _ffi.WeightParams, "stk_frame_weight": _ffi.FrameWeight,
           "stk_image_f32": _ffi.ImageF32, "stk_frame_stats": _ffi.FrameStats}


@pytest.mark.parametrize("name", ["stk_reject_maps", "stk_ecc_match_drizzle_rejected", "stk_keypoint_match_drizzle_rejected"])
def test_symbols_and_argument_lists_match_the_header(name):
    """Every argument of the ctypes signature against the header's declaration: scalars by type, pointers as pointers, and a
    typed pointer as the mirror of the struct the header names. stk_reject_params must be typed."""
    lib = _ffi.load()
    assert name in _ffi.SIGNATURES and hasattr(lib, name)
    res, args = _ffi.SIGNATURES[name]
    decl = _header_functions()[name]
    assert res is _ffi.c_status and len(args) == len(decl)
    scalars = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}
    for (pname, ctype), a in zip(decl, args):
        if "*" not in ctype:
            assert a is scalars[ctype.strip()], (pname, ctype, a)
            continue
        base = ctype.replace("const", "").replace("*", "").strip()
        if a is C.c_void_p:
            assert base != "stk_reject_params", pname
            continue
        assert ctype.count("*") == 1 and issubclass(a, C._Pointer), (pname, ctype, a)
        want = _ffi.RejectParams if base == "stk_reject_params" else C.c_int32 if base == "int32_t" else STRUCTS[base]
        assert a._type_ is want, (pname, ctype, a)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rejection_maps_keep_a_trail_out_of_the_drizzle(seed):
    """8 one-channel frames of 48 x 40 on quarter-pixel dithers (reject_restate.reject_stack), a trail in frame 5 and six hot
    pixels in each of frames 2 and 7, noise of 2 grey levels. Clean image: the restated coverage-aware median. Maps at
    rn = 2 / 255, pg = 0, snr (4, 3), scale (1.2, 0.7), min_count = 3; drizzle at scale 2, pixfrac 0.7; errors 8 output pixels
    in, against the drizzle of the defect-free stack. The f64 restatements measured, seeds 1, 2, 3:
      planted core pixels rejected    0.940, 0.918, 0.925   (asserted >= 0.85)
      clean pixels rejected           0, 0, 0               (asserted <= 0.005)
      RMS with maps / without         0.152, 0.160, 0.161   (asserted <= 0.3; 0.273 / 1.797, 0.285 / 1.778, 0.294 / 1.827 grey levels)."""
    bad, good, warps, planted = rr.reject_stack(seed)
    alpha = 1.0 / 255.0
    clean, cnt = rr.median_clean(bad, warps, alpha)
    p = rr.quality_params()
    n = len(bad)
    maps = np.ones((n, rr.RH, rr.RW), F)
    judged = np.zeros((n, rr.RH, rr.RW), bool)
    for i in range(n):
        maps[i], _, _, d = rr.reject_frame(bad[i], warps[i], False, alpha, clean, p, counts=cnt, dtype=np.float64)
        judged[i] = d["judged"]
    As = [dr.grid_matrix(M, False, 2.0) for M in warps]
    oh, ow = 2 * rr.RH, 2 * rr.RW
    with_maps, _ = dr.drizzle(bad, As, False, alpha, 2.0, 0.7, 0.0, oh, ow, maps=list(maps))
    without, _ = dr.drizzle(bad, As, False, alpha, 2.0, 0.7, 0.0, oh, ow)
    reference, _ = dr.drizzle(good, As, False, alpha, 2.0, 0.7, 0.0, oh, ow)
    hit, false_alarm, ratio, e_with, e_without = rr.quality_measures(maps, judged, planted, with_maps * 255.0, without * 255.0,
                                                                     reference * 255.0)
    print(f"seed {seed}: core rejected {hit:.4f}, clean rejected {false_alarm:.6f}, rms {e_with:.4f} / {e_without:.4f} = {ratio:.4f}")
    assert hit >= 0.85
    assert false_alarm <= 0.005
    assert ratio <= 0.3

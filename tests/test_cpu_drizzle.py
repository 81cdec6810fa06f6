"""Drizzle integration (include/stacker.h, stk_drizzle_params) without a GPU: the numpy restatement (drizzle_restate.py)
against answers worked out by hand, against the bilinear mean it must reduce to, the quality gain the feature exists for,
and the ctypes mirror against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import drizzle_restate as dr
from interp_restate import invert
from libstacker_rs_amd import DrizzleParameters, _ffi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shift(sx, sy):
    M = np.eye(3)
    M[0, 2], M[1, 2] = sx, sy
    return M


@pytest.mark.parametrize("dtype", [np.float64, F], ids=["f64", "f32"])
def test_hand_computed_3x3_at_scale_2_pixfrac_half(dtype):
    """One 3 x 3 frame, s = 2, p = 0.5, 6 x 6 output. u = X / 2 - 0.25, hx = 0.25, the drop of source pixel j is
    [j - 0.25, j + 0.25].
    Identity: X = 0: u = -0.25, jn = 0, d = -0.25, footprint [-0.5, 0] meets drop 0 in [-0.25, 0]: ox = 0.25. X = 1:
      u = 0.25, footprint [0, 0.5] meets drop 0 in [0, 0.25]: ox = 0.25. Every output pixel overlaps exactly one drop, by
      0.25 per axis: wgt = den = 1/16 everywhere, out[Y][X] = src[Y // 2][X // 2], no holes.
    The frame moved by +0.25 px in x (forward warp): u = X / 2 - 0.5. X even: u = j - 0.5, jn = j (ax = 0.5 rounds up),
      d = -0.5, footprint [-0.75, -0.25] touches the drops [-1.25, -0.75] and [-0.25, 0.25] in a point only: ox = 0, a
      hole. X odd: u = j exactly, footprint [-0.25, 0.25] = the drop: ox = 0.5. So den = 0.5 * 0.25 = 1/8 in the odd columns
      and 0 in the even ones, where out = fill.
    Both frames together, the second holding 10 x the values: den = 1/16 and 3/16; in the odd columns
      out = (a / 16 + 10 a / 8) / (3 / 16) = 7 a."""
    src = np.arange(1, 10, dtype=np.uint8).reshape(3, 3, 1)
    big = np.repeat(np.repeat(src[..., 0].astype(np.float64), 2, 0), 2, 1)
    A0, A1 = dr.grid_matrix(np.eye(3), False, 2.0), dr.grid_matrix(shift(0.25, 0), False, 2.0)
    assert np.array_equal(A0, [0.5, 0, -0.25, 0, 0.5, -0.25, 0, 0, 1]) and np.array_equal(A1, [0.5, 0, -0.5, 0, 0.5, -0.25, 0, 0, 1])
    out, den = dr.drizzle([src], [A0], False, 1.0, 2.0, 0.5, -7.0, 6, 6, dtype=dtype)
    assert out.dtype == dtype and np.array_equal(den, np.full((6, 6), 1 / 16)) and np.array_equal(out[..., 0], big)
    out, den = dr.drizzle([src], [A1], False, 1.0, 2.0, 0.5, -7.0, 6, 6, dtype=dtype)
    assert np.array_equal(den[:, 0::2], np.zeros((6, 3))) and np.array_equal(den[:, 1::2], np.full((6, 3), 1 / 8))
    assert np.array_equal(out[:, 0::2, 0], np.full((6, 3), -7.0)) and np.array_equal(out[:, 1::2, 0], big[:, 1::2])
    out, den = dr.drizzle([src, (src * 10).astype(np.uint8)], [A0, A1], False, 1.0, 2.0, 0.5, -7.0, 6, 6, dtype=dtype)
    assert np.array_equal(den[:, 0::2], np.full((6, 3), 1 / 16)) and np.array_equal(den[:, 1::2], np.full((6, 3), 3 / 16))
    assert np.array_equal(out[:, 0::2, 0], big[:, 0::2]) and np.array_equal(out[:, 1::2, 0], 7 * big[:, 1::2])
    # the same under an affine table entry (the footprint comes from the table, not from the pixel)
    oa, da = dr.drizzle([src, (src * 10).astype(np.uint8)], [A0, A1], True, 1.0, 2.0, 0.5, -7.0, 6, 6, dtype=dtype)
    assert np.array_equal(oa, out) and np.array_equal(da, den)


def test_hand_computed_weight_record_mask_and_canvas():
    """s = 1, p = 1, one 2 x 2 frame [[10, 20], [30, 40]] on a 4 x 3 canvas with origin (-1, 0): output column X shows
    frame column X - 1, so column 0 and column 3 are holes. Gain 2, offset 1, weight 3: out = 2 v + 1 and den = 3. A map
    that is 0 at pixel (0, 1) removes that pixel: a hole again."""
    src = np.array([[10, 20], [30, 40]], np.uint8)[..., None]
    A = dr.grid_matrix(np.eye(3), False, 1.0, -1.0, 0.0)
    kw = dict(gain=[[2.0]], offset=[[1.0]], weights=[3.0])
    out, den = dr.drizzle([src], [A], False, 1.0, 1.0, 1.0, 5.0, 3, 4, **kw)
    assert np.array_equal(den, [[0, 3, 3, 0], [0, 3, 3, 0], [0, 0, 0, 0]])
    assert np.array_equal(out[..., 0], [[5, 21, 41, 5], [5, 61, 81, 5], [5, 5, 5, 5]])
    mask = np.array([[1, 0], [1, 0.5]], F)
    out, den = dr.drizzle([src], [A], False, 1.0, 1.0, 1.0, 5.0, 3, 4, maps=[mask], **kw)
    assert np.array_equal(den, [[0, 3, 0, 0], [0, 3, 1.5, 0], [0, 0, 0, 0]])
    assert np.array_equal(out[..., 0], [[5, 21, 5, 5], [5, 61, 81, 5], [5, 5, 5, 5]])
    # a frame with weight 0 is skipped, whatever it holds
    bad = np.full((2, 2, 1), np.nan, F)
    o2, d2 = dr.drizzle([src.astype(F), bad], [A, A], False, 1.0, 1.0, 1.0, 5.0, 3, 4, gain=[[2.0], [1.0]], offset=[[1.0], [0.0]],
                        weights=[3.0, 0.0])
    assert np.array_equal(o2[..., 0], [[5, 21, 41, 5], [5, 61, 81, 5], [5, 5, 5, 5]])


def test_the_matrix_is_the_folds_inverse_composed_with_the_grid():
    H = np.array([[1.01, 0.02, -3.3], [-0.015, 0.99, 4.1], [2e-5, -1e-5, 1.0]])
    for M, aff in ((H, False), (np.array([[0.9, -0.3, 2.5], [0.3, 0.9, -1.25], [0, 0, 1.0]]), True)):
        assert np.array_equal(np.asarray(dr.inverse64(M, aff)).astype(F), invert(M, aff).astype(F))
        assert np.array_equal(dr.grid_matrix(M, aff, 1.0), invert(M, aff))          # s = 1, origin 0: the fold's own matrix
        s, ox, oy = 1.5, -2.25, 3.5
        A = dr.grid_matrix(M, aff, s, ox, oy)
        G = np.array([[1 / s, 0, 0.5 / s - 0.5 + ox], [0, 1 / s, 0.5 / s - 0.5 + oy], [0, 0, 1]])
        assert np.allclose(A.reshape(3, 3), np.linalg.inv(M) @ G, rtol=3e-7, atol=3e-7)


def test_scale_1_pixfrac_1_translations_are_the_bilinear_mean():
    """s = 1, p = 1, origin 0, pure translations (multiples of 1/64 px: exact in f32): the f64 restatement is the f64
    bilinear, coverage-weighted mean to 1e-12, den is its summed coverage."""
    rng = np.random.default_rng(7)
    n = 5
    frames = [rng.uniform(0, 1, (dr.QH, dr.QW, 1)).astype(F) for _ in range(n)]
    warps = [shift(*(rng.integers(-200, 200, 2) / 64.0)) for _ in range(n)]
    As = [dr.grid_matrix(M, False, 1.0) for M in warps]
    out, den = dr.drizzle(frames, As, False, 1.0, 1.0, 1.0, 0.0, dr.QH, dr.QW)
    ref, cov = dr.bilinear_mean64(frames, warps, 1)
    assert cov.min() < 1.0 < cov.max()                 # the rim is partly covered: the coverage weighting is exercised
    assert np.abs(den - cov).max() <= 1e-12 and np.abs(out[..., 0] - ref).max() <= 1e-12


def test_struct_layout_matches_the_header(tmp_path):
    names = ["scale", "pixfrac", "origin_x", "origin_y", "fill", "reserved"]
    src = tmp_path / "drizzle_sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n'
                   '    printf("%d' + " %d" * len(names) + '\\n", (int)sizeof(stk_drizzle_params)'
                   + "".join(f", (int)offsetof(stk_drizzle_params, {n})" for n in names) + ");\n    return 0;\n}\n")
    exe = tmp_path / "drizzle_sizes"
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = _ffi.DrizzleParams
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] == [24, 0, 4, 8, 12, 16, 20]
    assert [n for n, _ in S._fields_] == names
    p = DrizzleParameters(scale=3.0, pixfrac=0.4, origin_x=-1.5, origin_y=2.0, fill=9.0)._c()
    assert (p.scale, p.pixfrac, p.origin_x, p.origin_y, p.fill, p.reserved) == (3.0, F(0.4), -1.5, 2.0, 9.0, 0)
    assert DrizzleParameters(scale=1.5).out_shape(31, 45) == (47, 68)
    lib = _ffi.load()
    for name in ("stk_drizzle_stack", "stk_ecc_match_drizzle", "stk_keypoint_match_drizzle"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_drizzle_recovers_detail_the_bilinear_mean_cannot(seed):
    """A 24 x 32 scene of 12 cosines with radial frequencies up to 0.6 cycles per pixel, seen pixel-integrated by 16 frames
    on the 4 x 4 grid of quarter-pixel offsets, rounded to u8. On the fine grid (s = 2), three coarse pixels in from the
    edge, the f64 drizzle at p = 0.5 must come within 0.65 x the RMS error of the f64 bilinear mean of the same frames
    against the point-sampled scene (measured here: 0.607, 0.592, 0.583 for seeds 1, 2, 3; den >= 1.0, no holes). The same
    stack at s = 1, p = 1 is the bilinear mean: a ratio of 1."""
    frames, warps, scene = dr.quality_stack(seed)
    truth, inner = dr.quality_truth(scene, 2)
    As = [dr.grid_matrix(M, False, 2.0) for M in warps]
    out, den = dr.drizzle(frames, As, False, 1.0, 2.0, 0.5, 0.0, 2 * dr.QH, 2 * dr.QW)
    yard, _ = dr.bilinear_mean64(frames, warps, 2)
    e_d, e_b = dr.rms(out[..., 0], truth, inner), dr.rms(yard, truth, inner)
    print(f"seed {seed}: drizzle {e_d:.4f}, bilinear {e_b:.4f}, ratio {e_d / e_b:.4f}, den min {den[inner].min()}")
    assert den[inner].min() >= 1.0
    assert e_d <= 0.65 * e_b
    truth1, inner1 = dr.quality_truth(scene, 1)
    As1 = [dr.grid_matrix(M, False, 1.0) for M in warps]
    out1, _ = dr.drizzle(frames, As1, False, 1.0, 1.0, 1.0, 0.0, dr.QH, dr.QW)
    yard1, _ = dr.bilinear_mean64(frames, warps, 1)
    assert abs(dr.rms(out1[..., 0], truth1, inner1) / dr.rms(yard1, truth1, inner1) - 1.0) <= 1e-9

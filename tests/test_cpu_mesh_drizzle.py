"""Mesh-displaced drizzle (include/stacker.h, the block after stk_drizzle_params) without a GPU: the numpy restatement
(mesh_drizzle_restate.py) against answers worked out by hand, against the plain drizzle and the mesh fold it must reduce
to, the quality the combination exists for, and the symbols against the header."""
import os
import re

import numpy as np
import pytest

import drizzle_restate as dr
import mesh_drizzle_restate as mr
from libstacker_rs_amd import _ffi
from test_cpu_mesh import QM, _cosines, grid_restate, mesh_field_restate, quality_mesh_restated, quality_mesh_stack

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("dtype", [np.float64, F], ids=["f64", "f32"])


def shift(sx, sy):
    M = np.eye(3)
    M[0, 2], M[1, 2] = sx, sy
    return M


def rot(deg, cx, cy, tx=0.0, ty=0.0):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1.0]])


def const_field(w, h, step, dx, dy):
    gw, gh = grid_restate(w, h, step)
    D = np.zeros((gh, gw, 2), F)
    D[..., 0], D[..., 1] = dx, dy
    return D


# ---- hand-computed cases ------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("scale,pixfrac", [(1.0, 1.0), (2.0, 0.5)])
def test_constant_field_is_plain_drizzle_of_the_shifted_frame(dtype, scale, pixfrac):
    """A constant field d = (2, -1) moves every output coordinate by s d, so the identity entry reads source coordinate
    x0 + 2, y0 - 1: what plain drizzle reads under the forward translation (-2, +1). All values dyadic: the same bits. The
    slopes are 0, so the footprint is the table's."""
    rng = np.random.default_rng(1)
    h, w = 21, 27
    f = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    oh, ow = int(h * scale), int(w * scale)
    A = dr.grid_matrix(np.eye(3), True, scale)
    D = const_field(w, h, 8, 2.0, -1.0)
    for aff in (True, False):
        got = mr.mesh_drizzle([f], [A], aff, 1.0, scale, pixfrac, -1.0, oh, ow, [D], 8, dtype=dtype)
        ref = dr.drizzle([f], [dr.grid_matrix(shift(-2.0, 1.0), aff, scale)], aff, 1.0, scale, pixfrac, -1.0, oh, ow, dtype=dtype)
        assert got[0].dtype == dtype and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert (ref[1] > 0).mean() > 0.8 and (ref[1] == 0).any()


@BOTH
def test_a_known_gradient_scales_the_footprint(dtype):
    """w = 33, step 8: nodes on x = 0, 8, .. 32. The field d_0 = x / 4 (node k holds 2 k), d_1 = 0 has the Jacobian
    E = [[1.25, 0], [0, 1]]: under the identity at s = 1 the output pixel X reads source coordinate 1.25 X and covers
    1.25 source pixels, hx = 0.5 x 1.25 = 0.625 where plain drizzle has 0.5. With p = 1 the drops tile the line, so the
    overlaps along x sum to 2 hx = 1.25 and along y to 1: den = 1.25 exactly wherever the footprint is inside the frame
    (0.625 <= 1.25 X <= 31.875), against 1 for plain drizzle; at X = 0 the part left of the frame is missing: 1.125."""
    h, w = 17, 33
    f = np.full((h, w, 1), 100, np.uint8)
    gw, gh = grid_restate(w, h, 8)
    D = np.zeros((gh, gw, 2), F)
    D[..., 0] = 2.0 * np.arange(gw)[None, :]
    d0, d1, e00, e01, e10, e11 = mr.field_sample(D, h, w, w, h, 8, 1.0, dtype=dtype)
    assert np.array_equal(d0, np.tile(np.arange(w) / 4.0, (h, 1))) and (d1 == 0).all()
    # (x = 32 is the last node itself: k1 = k there, the differences along x vanish and the slope is 0)
    assert (e00[:, :32] == 1.25).all() and (e00[:, 32] == 1).all() and (e01 == 0).all() and (e10 == 0).all() and (e11 == 1).all()
    A = dr.grid_matrix(np.eye(3), True, 1.0)
    for aff in (True, False):
        out, den = mr.mesh_drizzle([f], [A], aff, 1.0, 1.0, 1.0, 0.0, h, w, [D], 8, dtype=dtype)
        plain = mr.mesh_drizzle([f], [A], aff, 1.0, 1.0, 1.0, 0.0, h, w, [None], 8, dtype=dtype)
        assert np.array_equal(den[:, 1:26], np.full((h, 25), 1.25)) and np.array_equal(plain[1], np.ones((h, w)))
        assert np.array_equal(den[:, 0], np.full(h, 1.125)) and np.array_equal(out[:, :26, 0], np.full((h, 26), 100.0))
        assert (den[:, 27:] == 0).all()                         # 1.25 X - 0.625 > 32.5: past the frame


@BOTH
def test_a_canvas_pixel_outside_frame_0_takes_the_edge_value_and_slope_0(dtype):
    """s = 1, origin (-3, -2): output column X is frame-0 column X - 3. Left of the frame (X < 3) the field is that of
    column 0 and the slope along x is 0, the slope along y is still the field's; above the frame likewise along y."""
    h, w = 17, 33
    gw, gh = grid_restate(w, h, 8)
    D = np.zeros((gh, gw, 2), F)
    D[..., 0] = 1.0 + 2.0 * np.arange(gw)[None, :] + 0.5 * np.arange(gh)[:, None]       # d_0 = 1 + x / 4 + y / 16
    oh, ow = h + 4, w + 6
    d0, d1, e00, e01, e10, e11 = mr.field_sample(D, oh, ow, w, h, 8, 1.0, -3.0, -2.0, dtype=dtype)
    Y, X = np.mgrid[0:oh, 0:ow]
    x0, y0 = np.clip(X - 3, 0, w - 1), np.clip(Y - 2, 0, h - 1)
    assert np.array_equal(d0, 1.0 + x0 / 4.0 + y0 / 16.0) and (d1 == 0).all()
    # (the last column, x = 32, and the last row, y = 16, are last nodes themselves: k1 = k, slope 0, as outside)
    inx, iny = (X >= 3) & (X - 3 < w - 1), (Y >= 2) & (Y - 2 < h - 1)
    assert np.array_equal(e00, np.where(inx, 1.25, 1.0)) and np.array_equal(e01, np.where(iny, 1.0 / 16, 0.0))
    assert (e10 == 0).all() and (e11 == 1).all()
    assert (~inx).any() and (~iny).any()


@BOTH
def test_a_nan_node_empties_its_pixels(dtype):
    """Node (1, 2) at (x, y) = (16, 8) is NaN: the lerp of the four cells around it is NaN (0 x NaN is NaN), so the pixels
    with 8 <= x < 24 and 0 <= y < 16 get a non-finite coordinate from this entry, no overlap, and with one entry den = 0
    and out = fill. Every other pixel is untouched."""
    rng = np.random.default_rng(2)
    h, w = 17, 33
    f = rng.integers(1, 256, (h, w, 1), dtype=np.uint8)
    D = const_field(w, h, 8, 0.0, 0.0)
    D[1, 2, 0] = np.nan
    A = dr.grid_matrix(np.eye(3), True, 1.0)
    out, den = mr.mesh_drizzle([f], [A], True, 1.0, 1.0, 1.0, -5.0, h, w, [D], 8, dtype=dtype)
    hit = np.zeros((h, w), bool)
    hit[0:16, 8:24] = True                                     # cells k = 1, 2 and j = 0, 1; x = 24 and y = 16 open the next cells
    assert (den[hit] == 0).all() and (out[hit] == -5.0).all()
    assert np.array_equal(den[~hit], np.ones((~hit).sum())) and np.array_equal(out[~hit][:, 0], f[~hit][:, 0].astype(dtype))


# ---- the three properties of the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["affine", "perspective"])
@pytest.mark.parametrize("scale,pixfrac,origin", [(1.0, 1.0, (0.0, 0.0)), (2.0, 0.7, (0.0, 0.0)), (3.0, 0.4, (-4.5, -2.25))])
def test_null_and_zero_fields_are_plain_drizzle_to_the_bit(kind, scale, pixfrac, origin):
    rng = np.random.default_rng(3)
    h, w, n = 37, 45, 3
    aff = kind == "affine"
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    warps = [rot(rng.uniform(-30, 30), w / 2, h / 2, *rng.uniform(-3, 3, 2)) for _ in range(n)]
    if not aff:
        for M in warps:
            M[2, :2] = rng.normal(0, 4e-4, 2)
    maps = [rng.uniform(0.5, 2.0, (h, w)).astype(F), None, (rng.random((h, w)) > 0.2).astype(F)]
    gain, offset, weights = rng.uniform(0.5, 1.5, (n, 3)), rng.uniform(0, 0.1, (n, 3)), rng.uniform(0.5, 2, n)
    As = [dr.grid_matrix(M, aff, scale, *origin) for M in warps]
    oh, ow = int(h * scale) + 5, int(w * scale) + 7
    zero = const_field(w, h, 8, 0.0, 0.0)
    for dtype in (F, np.float64):
        ref = dr.drizzle(frames, As, aff, 1 / 255, scale, pixfrac, 0.5, oh, ow, gain, offset, weights, maps, dtype=dtype)
        for fields in ([None] * n, [zero] * n, [None, zero, None]):
            got = mr.mesh_drizzle(frames, As, aff, 1 / 255, scale, pixfrac, 0.5, oh, ow, fields, 8, *origin, gain, offset, weights, maps,
                                  dtype=dtype)
            assert got[0].dtype == dtype and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("w,h,step", [(65, 53, 8), (45, 37, 16), (157, 120, 16)])
def test_scale_1_coordinates_are_the_mesh_folds(w, h, step):
    gw, gh = grid_restate(w, h, step)
    D = np.random.default_rng(4).uniform(-3, 3, (gh, gw, 2)).astype(F)
    fx, fy = mesh_field_restate(D, w, h, step)
    X, Y = mr.displaced_coords(D, h, w, w, h, step, 1.0, dtype=F)
    assert X.dtype == F and np.array_equal(X, fx) and np.array_equal(Y, fy)
    X0, Y0 = mr.displaced_coords(None, h, w, w, h, step, 1.0, dtype=F)
    fx0, fy0 = mesh_field_restate(None, w, h, step)
    assert np.array_equal(X0, fx0) and np.array_equal(Y0, fy0)
    assert mr.grid_map(1.0) == (1.0, 0.0, 0.0, 1.0)


# ---- the interface ---------------------------------------------------------------------------------------------------------
NAMES = ("stk_mesh_drizzle_stack", "stk_ecc_match_local_aligned_drizzle", "stk_keypoint_match_local_aligned_drizzle")


def test_symbols_and_arguments_against_the_header():
    header = open(os.path.join(ROOT, "include", "stacker.h")).read()
    lib = _ffi.load()
    for name in NAMES:
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        m = re.search(r"stk_status\s+" + name + r"\s*\(([^;]*)\);", header)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(_ffi.SIGNATURES[name][1]), name
    args = [a.strip() for a in re.search(r"stk_status\s+stk_mesh_drizzle_stack\s*\(([^;]*)\);", header).group(1).split(",")]
    plain = [a.strip() for a in re.search(r"stk_status\s+stk_drizzle_stack\s*\(([^;]*)\);", header).group(1).split(",")]
    assert args[:9] == plain[:9] and args[11:] == plain[9:]              # stk_drizzle_stack's arguments around fields, step
    assert args[9] == "const float* const* fields" and args[10] == "int32_t step"
    # the kernel's argument block grows at its end only: the plain kernels read what they read before
    dh = open(os.path.join(ROOT, "libstacker_rs_amd", "csrc", "drizzle.h")).read()
    body = dh[dh.index("struct DrizzleArgs"):]
    assert body.index("int ow, oh;") < body.index("const float* const* fields;") < body.index("float mesh_s;")
    from libstacker_rs_amd import Stacker
    for method in ("mesh_drizzle_stack", "ecc_match_local_aligned_drizzle", "keypoint_match_local_aligned_drizzle"):
        assert callable(getattr(Stacker, method))


# ---- the quality the combination exists for ---------------------------------------------------------------------------------
def quality_scene():
    """test_cpu_mesh.quality_mesh_stack's scene as a function: its generator's first draws are the texture's."""
    tex = _cosines(np.random.default_rng(QM["seed"]), QM["n_cos"], QM["fmax"])
    return lambda x, y: 128.0 + 90.0 * tex(x, y)


def quality_truth(scale):
    """The point-sampled scene on the output grid of `scale` over frame 0 and the interior, 12 coarse pixels in."""
    oh, ow = int(round(QM["h"] * scale)), int(round(QM["w"] * scale))
    Y, X = np.mgrid[0:oh, 0:ow].astype(np.float64)
    truth = quality_scene()((X + 0.5) / scale - 0.5, (Y + 0.5) / scale - 0.5)
    m = int(round(QM["margin"] * scale))
    inner = np.zeros((oh, ow), bool)
    inner[m:oh - m, m:ow - m] = True
    return truth, inner


@pytest.fixture(scope="module")
def quality():
    scene, frames, _ = quality_mesh_stack()
    fields = quality_mesh_restated(frames)[2]
    return scene, frames, fields


@pytest.mark.parametrize("scale,pixfrac", [(1.0, 1.0), (2.0, 0.7)])
def test_quality_through_the_fields_beats_plain_drizzle(quality, scale, pixfrac):
    """The stack of test_cpu_mesh (8 frames of 157 x 120, smooth 1 - 2.5 px fields, noise sigma 2, identity warps) drizzled
    through the restated fields against the same stack drizzled plainly: RMS error against the point-sampled scene at most
    half, the bar of test_cpu_mesh's own quality test (the f64 prototype measured 0.136 and 0.183), and den > 0 on the
    whole interior (the prototype's minima: 8.06 and 0.54)."""
    scene, frames, fields = quality
    truth, inner = quality_truth(scale)
    if scale == 1.0:
        assert np.array_equal(truth, scene)
    oh, ow = truth.shape
    n = len(frames)
    As = [dr.grid_matrix(np.eye(3), True, scale)] * n
    fr = [f[..., None] for f in frames]
    out, den = mr.mesh_drizzle(fr, As, True, 1.0, scale, pixfrac, 0.0, oh, ow, fields, QM["mesh"].step)
    plain, _ = mr.mesh_drizzle(fr, As, True, 1.0, scale, pixfrac, 0.0, oh, ow, [None] * n, QM["mesh"].step)
    e_mesh, e_plain = dr.rms(out[..., 0], truth, inner), dr.rms(plain[..., 0], truth, inner)
    print(f"scale {scale}, pixfrac {pixfrac}: through the fields {e_mesh:.3f}, plain {e_plain:.3f}, ratio {e_mesh / e_plain:.3f}, "
          f"smallest interior den {den[inner].min():.3f}")
    assert e_mesh <= 0.5 * e_plain
    assert den[inner].min() > 0

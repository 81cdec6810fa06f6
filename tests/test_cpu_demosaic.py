"""Colour-filter mosaics, CPU side: the numpy restatement (demosaic_restate.py) against a scalar, pixel-by-pixel loop written
from include/stacker.h; the properties the definition promises (own colour, constants, ramps, cropping, the reflection of
HA's green, saturation, rounding); the quality of the methods on a scene with correlated colours; the ctypes mirror against
a C compiler's sizeof; the new calls under a NULL context; what the wrappers hand to the C ABI; the host half under
ASan + UBSan as a stand-alone program."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import demosaic_restate as dr
import libstacker_rs_amd as lib
from libstacker_rs_amd import _ffi, synth
from libstacker_rs_amd.api import DEVICE, HOST, DrizzleParameters, InvalidParams, NotEnoughFiles
from test_cpu_api_calls import CTX, new_stacker

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(3, 3), (4, 3), (5, 4), (7, 6), (9, 8)]                    # w x h
DEPTHS = [(np.uint8, 8), (np.uint8, 32), (np.uint16, 16), (np.uint16, 32), (F, 32)]
INTERP = (dr.BILINEAR, dr.MHC, dr.HA)


def _mosaic(dtype, w, h, seed):
    rng = np.random.default_rng(seed)
    if dtype == F:
        return rng.normal(100, 60, (h, w)).astype(F)
    return rng.integers(0, np.iinfo(dtype).max + 1, (h, w)).astype(dtype)


# ---- the scalar loop: the header read literally, one pixel at a time; Python integers (no overflow) or float32 scalars ------
def _out(S, k, integer, od):
    if not integer:
        return S if k == 0 else F(S * F(1.0 / (1 << k)))
    if od == 32:
        return F(F(S) * F(1.0 / (1 << k)))
    return min(max((S + (1 << k) // 2) // (1 << k), 0), 255 if od == 8 else 65535)


def demosaic_scalar(mosaic, pattern, method, od):
    h, w = mosaic.shape
    integer = mosaic.dtype != F
    conv = int if integer else F
    K = (lambda v: v) if integer else F
    cell = dr.CELLS[pattern]
    col = lambda x, y: cell[(y & 1) * 2 + (x & 1)]
    M = lambda x, y: conv(mosaic[dr.reflect(y, h), dr.reflect(x, w)])
    if method == dr.SUPERPIXEL:
        out = np.zeros((h // 2, w // 2, 3), dr.DTYPES[od])
        for Y, X in itertools.product(range(h // 2), range(w // 2)):
            s = [M(2 * X + (k & 1), 2 * Y + (k >> 1)) for k in range(4)]
            g = [s[k] for k in range(4) if cell[k] == 1]
            out[Y, X] = (_out(s[cell.index(0)], 0, integer, od), _out(g[0] + g[1], 1, integer, od), _out(s[cell.index(2)], 0, integer, od))
        return out

    def g8(x, y):
        if col(x, y) == 1:
            return K(8) * M(x, y)
        c2 = K(2) * M(x, y)
        tH, tV = (c2 - M(x - 2, y)) - M(x + 2, y), (c2 - M(x, y - 2)) - M(x, y + 2)
        dH, dV = abs(M(x - 1, y) - M(x + 1, y)) + abs(tH), abs(M(x, y - 1) - M(x, y + 1)) + abs(tV)
        gH, gV = K(2) * (M(x - 1, y) + M(x + 1, y)) + tH, K(2) * (M(x, y - 1) + M(x, y + 1)) + tV
        return K(2) * gH if dH < dV else (K(2) * gV if dV < dH else gH + gV)

    d8 = lambda x, y: K(8) * M(x, y) - g8(x, y)
    out = np.zeros((h, w, 3), dr.DTYPES[od])
    with np.errstate(invalid="ignore", over="ignore"):
        for y, x in itertools.product(range(h), range(w)):
            c = M(x, y)
            h1, v1 = M(x - 1, y) + M(x + 1, y), M(x, y - 1) + M(x, y + 1)
            h2, v2 = M(x - 2, y) + M(x + 2, y), M(x, y - 2) + M(x, y + 2)
            x1, x2 = v1 + h1, v2 + h2
            d = (M(x - 1, y - 1) + M(x + 1, y - 1)) + (M(x - 1, y + 1) + M(x + 1, y + 1))
            px = [None, None, None]
            kind = col(x, y)
            px[kind] = _out(c, 0, integer, od)
            if kind == 1:
                rowc, colc = col(x + 1, y), col(x, y + 1)
                if method == dr.BILINEAR:
                    px[rowc], px[colc] = _out(h1, 1, integer, od), _out(v1, 1, integer, od)
                elif method == dr.MHC:
                    px[rowc] = _out(K(10) * c + K(8) * h1 - K(2) * d - K(2) * h2 + v2, 4, integer, od)
                    px[colc] = _out(K(10) * c + K(8) * v1 - K(2) * d - K(2) * v2 + h2, 4, integer, od)
                else:
                    G8 = K(8) * c
                    px[rowc] = _out((K(2) * G8 + d8(x - 1, y)) + d8(x + 1, y), 4, integer, od)
                    px[colc] = _out((K(2) * G8 + d8(x, y - 1)) + d8(x, y + 1), 4, integer, od)
            else:
                opp = 2 - kind
                if method == dr.BILINEAR:
                    px[1], px[opp] = _out(x1, 2, integer, od), _out(d, 2, integer, od)
                elif method == dr.MHC:
                    px[1] = _out(K(8) * c + K(4) * x1 - K(2) * x2, 4, integer, od)
                    px[opp] = _out(K(12) * c + K(4) * d - K(3) * x2, 4, integer, od)
                else:
                    G8 = g8(x, y)
                    px[1] = _out(G8, 3, integer, od)
                    px[opp] = _out((K(4) * G8 + (d8(x - 1, y - 1) + d8(x + 1, y - 1))) + (d8(x - 1, y + 1) + d8(x + 1, y + 1)), 5, integer, od)
            out[y, x] = px
    return out


@pytest.mark.parametrize("dtype,od", DEPTHS, ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
@pytest.mark.parametrize("pattern", dr.PATTERNS)
@pytest.mark.parametrize("method", dr.METHODS)
def test_restatement_is_the_scalar_loop(method, pattern, dtype, od):
    sizes = SIZES + ([(2, 2), (3, 2)] if method == dr.SUPERPIXEL else [])
    for k, (w, h) in enumerate(sizes):
        m = _mosaic(dtype, w, h, 10 * method + pattern + k)
        assert dr.same_bits(dr.demosaic_one(m, pattern, method, od), demosaic_scalar(m, pattern, method, od)), (w, h)


@pytest.mark.parametrize("method", dr.METHODS)
def test_restatement_is_the_scalar_loop_on_non_finite_f32(method):
    m = _mosaic(F, 9, 8, 3)
    m[2, 3], m[5, 5], m[0, 8], m[7, 0] = np.nan, np.inf, -np.inf, 3e38
    got = dr.demosaic_one(m, dr.GBRG, method, 32)
    assert dr.same_bits(got, demosaic_scalar(m, dr.GBRG, method, 32))
    assert np.isnan(got).any()


def test_site_colours_masks_and_the_mosaic_of_an_image():
    assert [dr.colour(p, 0, 0) for p in dr.PATTERNS] == [2, 1, 1, 0]
    for p in dr.PATTERNS:
        ys, xs = np.nonzero(dr.colours(p, 6, 8) == 2)
        assert set(xs & 1) == {p & 1} and set(ys & 1) == {p >> 1}                   # red sites: (pattern & 1, pattern >> 1)
        total = sum(dr.cfa_mask(8, 6, p, c) for c in range(3))
        assert np.array_equal(total, np.ones((6, 8), F))
        assert [int(dr.cfa_mask(8, 6, p, c).sum()) for c in range(3)] == [12, 24, 12]
        assert np.array_equal(dr.colours(p, 6, 8)[:, 1:], dr.colours(p ^ 1, 6, 7)) and np.array_equal(dr.colours(p, 6, 8)[1:], dr.colours(p ^ 2, 5, 8))
    assert [dr.reflect(i, 3) for i in range(-3, 6)] == [1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert [dr.reflect(i, 5) for i in (-3, -1, 5, 7)] == [3, 1, 3, 1]


@pytest.mark.parametrize("dtype,od", DEPTHS, ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
def test_own_colour_samples_come_back_unchanged(dtype, od):
    for method, pattern in itertools.product(INTERP, dr.PATTERNS):
        m = _mosaic(dtype, 11, 9, 40 + pattern)
        got = dr.demosaic_one(m, pattern, method, od)
        own = np.take_along_axis(got, dr.colours(pattern, 9, 11)[..., None], 2)[..., 0]
        assert np.array_equal(own, m.astype(got.dtype))
        assert np.array_equal(dr.mosaic_of(got, pattern), m.astype(got.dtype))


def test_a_constant_mosaic_gives_the_constant_image():
    for (dtype, od), method, pattern, v in itertools.product(DEPTHS, dr.METHODS, dr.PATTERNS, (0, 1, 77, 255)):
        got = dr.demosaic_one(np.full((6, 7), v, dtype), pattern, method, od)
        assert (got == v).all() and got.shape == ((3, 3, 3) if method == dr.SUPERPIXEL else (6, 7, 3))
    assert (dr.demosaic_one(np.full((5, 5), 65535, np.uint16), dr.RGGB, dr.HA, 16) == 65535).all()


def test_a_grey_ramp_is_reproduced_exactly_inside():
    yy, xx = np.mgrid[0:14, 0:17]
    for (a, b), (dtype, od), method, pattern in itertools.product([(3, 5), (7, 0), (0, 2), (4, 4)], DEPTHS[:4], INTERP, dr.PATTERNS):
        ramp = (a * xx + b * yy + 9).astype(dtype)
        got = dr.demosaic_one(ramp, pattern, method, od)
        want = np.repeat(ramp[..., None], 3, 2).astype(got.dtype)
        assert np.array_equal(got[3:-3, 3:-3], want[3:-3, 3:-3]), (a, b, method, pattern)


def test_cropping_switches_the_pattern():
    for (dtype, od), method, pattern in itertools.product(DEPTHS, INTERP, dr.PATTERNS):
        m = _mosaic(dtype, 17, 15, 7)
        full = dr.demosaic_one(m, pattern, method, od)
        col = dr.demosaic_one(np.ascontiguousarray(m[:, 1:]), pattern ^ 1, method, od)
        row = dr.demosaic_one(np.ascontiguousarray(m[1:]), pattern ^ 2, method, od)
        assert dr.same_bits(col[4:-4, 3:-4], full[4:-4, 4:-4]) and dr.same_bits(row[3:-4, 4:-4], full[4:-4, 4:-4])


def test_ha_green_under_reflection_is_the_formula_on_the_reflected_mosaic():
    """G8 outside the frame, evaluated on the reflected mosaic, is G8 at the reflected position: exactly for integers (the
    formulas are symmetric in W / E and N / S); in f32 up to the order of the two subtractions of tH."""
    for (w, h), dtype in itertools.product(SIZES + [(12, 10)], (np.uint8, np.uint16)):
        m = _mosaic(dtype, w, h, w + h)
        full = dr.g8_plane(np.pad(m.astype(np.int64), 3, mode="reflect"))             # positions -1 .. h, -1 .. w
        assert full.shape == (h + 2, w + 2)
        assert np.array_equal(full, np.pad(full[1:-1, 1:-1], 1, mode="reflect"))
    m = _mosaic(F, 12, 10, 5)
    full = dr.g8_plane(np.pad(m, 3, mode="reflect"))
    np.testing.assert_allclose(full, np.pad(full[1:-1, 1:-1], 1, mode="reflect"), rtol=1e-5, atol=1e-3)


def test_sums_stay_inside_int32_and_saturate():
    # |S| <= (sum of |coefficients|) * 65535: MHC 40; HA: |G8| <= 16, |D8| <= 24, row 2 * 8 + 48, opposite 4 * 16 + 4 * 24
    assert max(8 + 16 + 8, 10 + 16 + 8 + 4 + 2, 12 + 16 + 12) * 65535 < 2 ** 24
    assert max(16, 24, 2 * 8 + 2 * 24, 4 * 16 + 4 * 24) * 65535 < 2 ** 24
    for dtype, od in DEPTHS[:4]:
        top = np.iinfo(dtype).max
        yy, xx = np.mgrid[0:9, 0:10]
        boards = [((xx + yy) & 1) * top, ((xx + yy + 1) & 1) * top, (xx & 1) * top, (yy & 1) * top, ((xx >> 1) + (yy >> 1) & 1) * top]
        spike = np.zeros((9, 10), np.int64)
        spike[4, 5] = spike[0, 0] = spike[8, 9] = top
        for board, method, pattern in itertools.product(boards + [spike, top - spike], dr.METHODS, dr.PATTERNS):
            m = board.astype(dtype)
            got = dr.demosaic_one(m, pattern, method, od)
            assert dr.same_bits(got, demosaic_scalar(m, pattern, method, od))
            assert od == 32 or (got.min() >= 0 and got.max() <= top)        # (f32 output is not clamped)
    # a spike's MHC neighbours go negative before the clamp, and above the top next to a hole
    m = np.zeros((7, 7), np.uint8)
    m[3, 3] = 255
    assert dr.demosaic_one(m, dr.RGGB, dr.MHC, 32).min() < 0 and dr.demosaic_one(m, dr.RGGB, dr.MHC, 8).min() == 0
    assert dr.demosaic_one(255 - m, dr.RGGB, dr.MHC, 32).max() > 255 and dr.demosaic_one(255 - m, dr.RGGB, dr.MHC, 8).max() == 255


def test_rounding_ties_at_every_divisor():
    for k in range(1, 6):
        D = 1 << k
        S = np.array([D // 2, D + D // 2, -D // 2, -D - D // 2, D // 2 - 1, -D // 2 - 1], np.int64)       # .5, 1.5, -.5, -1.5, just below
        assert list(dr.finish(S, k, True, 16)) == [1, 2, 0, 0, 0, 0]                                          # half up; negatives clamp
        assert list(dr.finish(S + 8 * D, k, True, 16)) == [9, 10, 8, 7, 8, 7]                                 # floor((S + D / 2) / D)
        assert list(dr.finish(S, k, True, 32)) == [0.5, 1.5, -0.5, -1.5, 0.5 - 1 / D, -0.5 - 1 / D]
    m = np.zeros((5, 5), np.uint8)
    m[2, 1] = 1
    got = dr.demosaic_one(m, dr.GBRG, dr.BILINEAR, 8)             # GBRG: (1, 2) is B; (2, 2) is G with B in its row: h1 / 2 = 0.5 -> 1
    assert dr.colour(dr.GBRG, 1, 2) == 0 and got[2, 2, 0] == 1 and dr.demosaic_one(m, dr.GBRG, dr.BILINEAR, 32)[2, 2, 0] == 0.5
    assert got[1, 1, 0] == 1 and got[1, 2, 0] == 0                # v1 / 2 = 0.5 -> 1 above the B; d / 4 = 0.25 -> 0 at the R beside that


# ---- quality, on the restatement alone --------------------------------------------------------------------------------------
def _scene(w, h, correlated):
    s = synth.render_scene(w, h)
    s = s[(s.shape[0] - h) // 2:(s.shape[0] - h) // 2 + h, (s.shape[1] - w) // 2:(s.shape[1] - w) // 2 + w]
    if correlated:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        grey = s.astype(np.float64).mean(2)
        tint = [1.0 + 0.25 * np.sin(xx / 37.0 + c) * np.cos(yy / 29.0 - c) for c in range(3)]
        s = np.stack([grey * t for t in tint], -1)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def quality_ratios(w, h, correlated):
    truth = _scene(w, h, correlated)
    rms = {}
    for method in INTERP:
        err = dr.demosaic_one(dr.mosaic_of(truth, dr.RGGB), dr.RGGB, method, 32)[4:-4, 4:-4].astype(np.float64) - truth[4:-4, 4:-4]
        rms[method] = float(np.sqrt((err ** 2).mean()))
    return rms[dr.MHC] / rms[dr.BILINEAR], rms[dr.HA] / rms[dr.BILINEAR]


@pytest.mark.parametrize("w,h", [(256, 192), (131, 97)])
def test_mhc_and_ha_beat_bilinear_where_the_colours_are_correlated(w, h):
    """Measured: MHC / bilinear and HA / bilinear RMS error, 4 px inside; the figures are in DESIGN §4.25."""
    mhc, ha = quality_ratios(w, h, True)
    print("correlated", w, h, "MHC / bilinear", round(mhc, 3), "HA / bilinear", round(ha, 3))
    assert mhc < 1.0 and ha < 1.0
    mhc_i, ha_i = quality_ratios(w, h, False)
    print("independent colours", w, h, "MHC / bilinear", round(mhc_i, 3), "HA / bilinear", round(ha_i, 3))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_struct_size_is_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "stacker.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %d\\n", (int)sizeof(stk_mosaic), (int)offsetof(stk_mosaic, n), (int)offsetof(stk_mosaic, depth),\n'
                   "           (int)offsetof(stk_mosaic, pattern), (int)offsetof(stk_mosaic, row_stride_bytes));\n    return 0;\n}\n")
    exe = tmp_path / "sizes"
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K = _ffi.Mosaic
    assert got == [C.sizeof(K), K.n.offset, K.depth.offset, K.pattern.offset, K.row_stride_bytes.offset] == [40, 8, 20, 28, 32]


def test_parameter_mirrors():
    hdr = open(os.path.join(ROOT, "include", "stacker.h")).read()
    for name, value in [("CFA_RGGB", 0), ("CFA_GRBG", 1), ("CFA_GBRG", 2), ("CFA_BGGR", 3), ("DEMOSAIC_BILINEAR", 0), ("DEMOSAIC_MHC", 1),
                        ("DEMOSAIC_HA", 2), ("DEMOSAIC_SUPERPIXEL", 3)]:
        assert getattr(lib, name) == value and "STK_%s = %d" % (name, value) in hdr and name in lib.__all__
    assert (dr.RGGB, dr.GRBG, dr.GBRG, dr.BGGR) == (lib.CFA_RGGB, lib.CFA_GRBG, lib.CFA_GBRG, lib.CFA_BGGR)
    assert (dr.BILINEAR, dr.MHC, dr.HA, dr.SUPERPIXEL) == (lib.DEMOSAIC_BILINEAR, lib.DEMOSAIC_MHC, lib.DEMOSAIC_HA, lib.DEMOSAIC_SUPERPIXEL)
    assert [f for f, _ in _ffi.Mosaic._fields_] == ["data", "n", "width", "height", "depth", "location", "pattern", "row_stride_bytes"]


def test_every_new_call_refuses_a_null_context():
    so = _ffi.load()
    plane = np.zeros((4, 4), np.uint8)
    ptr = (C.c_void_p * 1)(plane.ctypes.data)
    mo = _ffi.Mosaic(C.cast(ptr, C.POINTER(C.c_void_p)), 1, 4, 4, 8, 0, 0, 0)
    out = np.zeros((4, 4, 3), np.uint8)
    optr = (C.c_void_p * 1)(out.ctypes.data)
    mask = np.full((4, 4), 7.0, F)
    INVALID = 2
    assert so.stk_demosaic(None, C.byref(mo), 1, 8, C.cast(optr, C.c_void_p), 0) == INVALID
    assert so.stk_cfa_mask(None, 4, 4, 0, 1, C.c_void_p(mask.ctypes.data), 0) == INVALID
    assert not out.any() and (mask == 7.0).all()


# ---- what the wrappers hand to the C ABI ------------------------------------------------------------------------------------
def _mosaic_of_call(snap):
    return _ffi.Mosaic.from_buffer_copy(snap[1])


def test_demosaic_hands_over_the_planes_and_its_own_outputs():
    st = new_stacker()
    frames = np.random.default_rng(0).integers(0, 65536, (3, 6, 10), dtype=np.uint16)
    st._lib.reads = {4: ("tbl", 3, 8)}
    for files in (frames, list(frames), [f[..., None] for f in frames]):
        res = st.demosaic(files, lib.CFA_GBRG)
        name, snap = st._lib.last()
        mo = _mosaic_of_call(snap)
        assert name == "stk_demosaic" and snap[0] == CTX and snap[2] == lib.DEMOSAIC_MHC and snap[3] == 16 and snap[5] == 0
        assert (mo.n, mo.width, mo.height, mo.depth, mo.location, mo.pattern, mo.row_stride_bytes) == (3, 10, 6, 16, HOST, lib.CFA_GBRG, 0)
        assert res.shape == (3, 6, 10, 3) and res.dtype == np.uint16
        assert snap[4][1] == [res.ctypes.data + i * 6 * 10 * 3 * 2 for i in range(3)]
    res = st.demosaic(frames, lib.CFA_RGGB, lib.DEMOSAIC_HA, out_depth=32)
    name, snap = st._lib.last()
    assert res.shape == (3, 6, 10, 3) and res.dtype == F and snap[2] == lib.DEMOSAIC_HA and snap[3] == 32
    assert snap[4][1] == [res.ctypes.data + i * 6 * 10 * 3 * 4 for i in range(3)]
    res = st.demosaic(frames[:, :5, :7], lib.CFA_BGGR, lib.DEMOSAIC_SUPERPIXEL)                       # a window: padded rows, half-size output
    name, snap = st._lib.last()
    mo = _mosaic_of_call(snap)
    assert res.shape == (3, 2, 3, 3) and (mo.width, mo.height, mo.row_stride_bytes, mo.pattern) == (7, 5, 20, lib.CFA_BGGR)
    assert [mo.data[i] for i in range(3)] == [frames[i].ctypes.data for i in range(3)]


def test_demosaic_out_follows_calibrates_rules():
    st = new_stacker()
    frames = np.zeros((2, 6, 10), np.uint8)
    st._lib.reads = {4: ("tbl", 2, 8)}
    wide = np.zeros((2, 6, 14, 3), np.uint8)
    outs = [wide[0, :, 2:12], wide[1, :, 2:12]]
    assert st.demosaic(frames, 0, out=outs) is outs
    name, snap = st._lib.last()
    assert snap[5] == 14 * 3 and snap[4][1] == [o.ctypes.data for o in outs]
    tight = [np.zeros((6, 10, 3), F) for _ in range(2)]
    st.demosaic(frames, 0, out_depth=32, out=tight)
    assert st._lib.last()[1][5] == 10 * 3 * 4
    n_calls = len(st._lib.calls)
    for bad, kw in [(tight[:1], dict(out_depth=32)), (tight, {}), ([np.zeros((6, 10), np.uint8)] * 2, {}), ([np.zeros((3, 5, 3), np.uint8)] * 2, {}),
                    ([wide[0, :, 2:12], np.zeros((6, 10, 3), np.uint8)], {}), ([wide[0, :, 2:12, ::-1]] * 2, {}),
                    ([np.zeros((6, 10, 3), np.uint8)] * 2, dict(out_depth=12))]:
        with pytest.raises(InvalidParams):
            st.demosaic(frames, 0, out=bad, **kw)
    with pytest.raises(InvalidParams):
        st.demosaic(np.zeros((2, 6, 10, 3), np.uint8), 0)                    # multi-channel input: the wrapper's own refusal
    with pytest.raises(NotEnoughFiles):
        st.demosaic([], 0)
    assert len(st._lib.calls) == n_calls
    half = [np.zeros((3, 5, 3), np.uint8)] * 2
    st.demosaic(frames, 0, lib.DEMOSAIC_SUPERPIXEL, out=half)
    assert len(st._lib.calls) == n_calls + 1


def test_cfa_mask_hands_over_its_plane():
    st = new_stacker()
    plane = st.cfa_mask(10, 6, lib.CFA_GRBG, 2)
    name, snap = st._lib.last()
    assert name == "stk_cfa_mask" and snap == [CTX, 10, 6, lib.CFA_GRBG, 2, plane.ctypes.data, HOST]
    assert plane.shape == (6, 10) and plane.dtype == F
    assert DEVICE == 1


def test_cfa_drizzle_stack_is_three_drizzle_calls_with_the_mask_repeated():
    st = new_stacker()
    frames = np.random.default_rng(1).integers(0, 256, (3, 6, 10), dtype=np.uint8)
    warps = np.tile(np.eye(3), (3, 1, 1))
    st._lib.reads = {8: ("tbl", 3, 6 * 10 * 4)}
    image, den = st.cfa_drizzle_stack(frames, warps, lib.CFA_GBRG, DrizzleParameters(scale=2.0), alpha=1.0)
    assert image.shape == den.shape == (12, 20, 3) and image.dtype == den.dtype == F
    names = [n for n, _ in st._lib.calls]
    assert names == ["stk_cfa_mask", "stk_drizzle_stack"] * 3
    for c in range(3):
        mask_call, drizzle = st._lib.calls[2 * c][1], st._lib.calls[2 * c + 1][1]
        assert mask_call[1:5] == [10, 6, lib.CFA_GBRG, c] and mask_call[6] == HOST
        assert drizzle[8][1] == [mask_call[5]] * 3                           # the one plane, n times
        assert drizzle[1]["channels"] == 1 and drizzle[1]["n"] == 3 and drizzle[5] == 1.0
        assert drizzle[9]["width"] == 20 and drizzle[9]["height"] == 12 and drizzle[9]["channels"] == 1 and drizzle[10] is not None
    for kw in (dict(maps=[None] * 3), dict(return_den=True)):
        with pytest.raises(InvalidParams):
            st.cfa_drizzle_stack(frames, warps, 0, **kw)
    with pytest.raises(InvalidParams):
        st.cfa_drizzle_stack(np.zeros((3, 6, 10, 3), np.uint8), warps, 0)


# ---- the host half as a stand-alone program under ASan + UBSan ---------------------------------------------------------------
@pytest.mark.timeout(600)
def test_host_half_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "demosaic_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "demosaic_harness.cpp"), "-o", exe, "-ldl", "-lpthread"]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=500)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

"""CPU tests of the display stretch (include/stacker.h, "display stretch"): the struct layouts, the symbols, _ffi.SIGNATURES,
the Rust table and __all__ against the header; stk_stretch_auto against the restatement (tests/stretch_restate.py) bit for
bit; stk_stretch_table against it within 1 f32 ulp (the host libm and numpy may differ in the last f64 bit; the sRGB table is
built from pow, so it has the same bound); every refusal that needs no GPU; what the wrappers hand to the C ABI; identities of
the restatement; the quality of the definition on the restatement, before any GPU run; the kernel map's rows; the sanitizer
harness.

Quality, measured on this f32 restatement, seeds 0, 1, 2. The scene of stretch_restate.scene: 128 x 96 x 3,
channel backgrounds 0.020 / 0.031 / 0.012 with a small gradient, noise sigma 0.002 / 0.0025 / 0.0015, 15 Gaussian stars; the
unlinked rule with the defaults (shadows_clip -2.8, target 0.25), curve MTF, f32 output:
                                                     seed 0    seed 1    seed 2    worst    bar = 1.5 x worst
  worst |channel median - 0.25|                       2.98e-8   2.98e-8   0         2.98e-8  4.47e-8
  largest - smallest channel median                   2.98e-8   2.98e-8   0         2.98e-8  4.47e-8
    (one ulp of 0.25 is 2.98e-8: the median sample lands on the target or beside it. The slope of the curve at the sky is about
     30, and black and midtone are rounded to f32 once, after the rule's f64)
  samples clipped to 0                                0.190 %   0.117 %   0.165 %            bar 1 % (the issue's)
The table's error against the exact asinh at K = 4096, over 200 000 random x, 100 001 even ones and the middle of every
interval:            beta 10: 1.16e-7    beta 100: 5.41e-6    beta 1000: 3.70e-4     bars: 1.5 x each
  (the error is the chord's: asinh''/8 K^2 near 0, where the curve bends most: it grows with beta^2 / asinh(beta))."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import libstacker_rs_amd as ls
import stretch_restate as sr
from libstacker_rs_amd import (CURVE_ASINH, CURVE_GAMMA, CURVE_SRGB, DEPTH_F32, DEPTH_U8, DEPTH_U16, STAT_DTYPE, STRETCH_LINEAR, STRETCH_MTF,
                               STRETCH_TABLE, AutoStretchParameters, InvalidParams, StretchParameters, _ffi, stretch_auto, stretch_table)
from test_cpu_api_calls import CTX, new_stacker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_image_stats", "stk_stretch", "stk_stretch_auto", "stk_stretch_table", "stk_auto_stretch")
SEEDS = (0, 1, 2)
BAR_MEDIAN = 1.5 * 2.98e-8
BAR_ASINH = {10.0: 1.5 * 1.16e-7, 100.0: 1.5 * 5.41e-6, 1000.0: 1.5 * 3.70e-4}
F = np.float32


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


def _ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- layouts, symbols, the Rust table -------------------------------------------------------------------------------
LAYOUTS = {"stk_image_stat": (_ffi.ImageStat, [40, 0, 8, 12, 16, 20, 24]),
           "stk_stretch_params": (_ffi.StretchParams, [68, 0, 4, 8, 12, 16, 32, 48, 64]),
           "stk_stretch_auto_params": (_ffi.StretchAutoParams, [40, 0, 8, 16, 24, 32, 36]),
           "stk_image_out": (_ffi.ImageOut, [40, 0, 8, 12, 16, 20, 24, 32])}


def test_struct_layouts_symbols_and_table_against_the_header(tmp_path):
    lines = []
    for name, (cls, _) in LAYOUTS.items():
        lines += ['  printf("%%zu", sizeof(%s));\n' % name] + ['  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_] + ['  printf("\\n");\n']
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n' + "".join(lines) + '  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [[int(v) for v in ln.split()] for ln in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    for row, (name, (cls, want)) in zip(got, LAYOUTS.items()):
        assert row == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_] == want, name
    assert STAT_DTYPE.itemsize == 40 and [STAT_DTYPE.fields[f][1] for f in STAT_DTYPE.names] == [0, 8, 12, 16, 20, 24]
    assert sr.STAT == STAT_DTYPE
    lib = _ffi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stacker.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    rs = open(os.path.join(ROOT, "rust", "src", "amd_ffi.rs")).read()
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name) and re.search(r" T %s\b" % name, nm)
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        res, sig = _ffi.SIGNATURES[name]
        assert res is _ffi.c_status and len(args.split(",")) == len(sig), name
        assert "pub fn %s(" % name in rs
    for name in LAYOUTS:
        assert "pub struct %s" % name in rs
    assert "pub const STK_STRETCH_TABLE: c_int = 2;" in rs and "pub const STK_CURVE_SRGB: c_int = 2;" in rs and "pub midtone: [f32; 4]," in rs
    assert re.search(r"STK_STRETCH_LINEAR\s*=\s*0,\s*STK_STRETCH_MTF\s*=\s*1,\s*STK_STRETCH_TABLE\s*=\s*2", hdr)
    assert re.search(r"STK_CURVE_ASINH\s*=\s*0,\s*STK_CURVE_GAMMA\s*=\s*1,\s*STK_CURVE_SRGB\s*=\s*2", hdr)
    assert (STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE, CURVE_ASINH, CURVE_GAMMA, CURVE_SRGB, DEPTH_U8, DEPTH_U16, DEPTH_F32) == (0, 1, 2, 0, 1, 2, 8, 16, 32)
    assert (sr.LINEAR, sr.MTF, sr.TABLE, sr.ASINH, sr.GAMMA, sr.SRGB) == (0, 1, 2, 0, 1, 2)
    for name in ("StretchParameters", "AutoStretchParameters", "stretch_auto", "stretch_table", "STAT_DTYPE", "STRETCH_LINEAR", "STRETCH_MTF", "STRETCH_TABLE",
                 "CURVE_ASINH", "CURVE_GAMMA", "CURVE_SRGB", "DEPTH_U8", "DEPTH_U16", "DEPTH_F32"):
        assert name in ls.__all__ and hasattr(ls, name)
    for method in ("image_stats", "stretch_image", "auto_stretch_image"):
        assert callable(getattr(ls.Stacker, method))
    c = StretchParameters()._c()
    assert (c.curve, c.colour, c.out_depth, c.reserved, c.out_scale) == (1, 0, 32, 0, 1.0)
    assert list(c.black) == [0.0] * 4 and list(c.white) == [1.0] * 4 and list(c.midtone) == [0.5] * 4
    a = AutoStretchParameters()._c()
    assert (a.shadows_clip, a.target_background, a.white, a.white_quantile, a.linked, a.white_mode) == (-2.8, 0.25, 1.0, 0.999, 0, 0)


# ---- 1. the auto rule -----------------------------------------------------------------------------------------------
def _records(rows):
    """rows: (count, min, max, median, mad, q0) per channel"""
    st = np.zeros(len(rows), STAT_DTYPE)
    for k, (n, mn, mx, med, mad, q0) in enumerate(rows):
        st[k]["count"], st[k]["min"], st[k]["max"], st[k]["median"], st[k]["mad"] = n, mn, mx, med, mad
        st[k]["q"][0] = q0
    return st


def _same_rule(st, **kw):
    got = stretch_auto(st, AutoStretchParameters(**kw))
    b, w, m = sr.auto(st, **kw)
    assert (got.curve, got.colour, got.out_depth, got.out_scale) == (STRETCH_MTF, 0, DEPTH_F32, 1.0)
    assert got.black.tobytes() == b.tobytes() and got.white.tobytes() == w.tobytes() and got.midtone.tobytes() == m.tobytes(), (kw, got, b, w, m)
    return got


def test_the_auto_rule_equals_the_restatement():
    rng = np.random.default_rng(2)
    cases = [_records([(1000, 0.01, 0.9, 0.02, 0.002, 0.5), (1000, 0.02, 0.95, 0.031, 0.0025, 0.6), (1000, 0.005, 0.8, 0.012, 0.0015, 0.4)]),
             _records([(10, 0.1, 0.7, 0.2, 0.0, 0.3)]),                                                   # MAD = 0
             _records([(50, 0.25, 0.25, 0.25, 0.0, 0.25)] * 3),                                           # a constant image
             _records([(7, 0.3, 0.9, 0.3, 0.1, 0.8)]),                                                    # median = min: x0 = 0
             _records([(0, 0, 0, 0, 0, 0)] * 3),                                                          # nothing counted
             _records([(9, -5.0, -1.0, -3.0, 0.5, -2.0), (9, -50.0, 100.0, 3.0, 20.0, 90.0), (9, 1e-20, 1e20, 1.0, 0.5, 1e10), (0, 0, 0, 0, 0, 0)])]
    for _ in range(40):
        rows = []
        for c in range(3):
            v = np.sort(rng.random(5).astype(F) * F(10 ** rng.uniform(-3, 3)))
            rows.append((100, v[0], v[4], v[1 + rng.integers(2)], F(rng.random() * float(v[2] - v[0])), v[3]))
        cases.append(_records(rows))
    for st in cases:
        for linked in (0, 1):
            for white_mode in (0, 1, 2):
                for clip, target, white in ((-2.8, 0.25, 1.0), (0.0, 0.1, 0.5), (-10.0, 0.9, 3.0)):
                    _same_rule(st, shadows_clip=clip, target_background=target, linked=linked, white_mode=white_mode, white=white)
    got = _same_rule(cases[2], white_mode=1)                                    # the constant image: max <= c0, so w = c0 + 1; x0 = 0
    assert got.black[:3].tolist() == [0.25] * 3 and got.white[:3].tolist() == [1.25] * 3 and got.midtone[:3].tolist() == [0.5] * 3
    got = _same_rule(cases[3])
    assert got.black[0] == F(0.3) and got.midtone[0] == 0.5
    got = _same_rule(cases[0], linked=1)
    assert len(set(got.black[:3].tolist())) == 1 and len(set(got.midtone[:3].tolist())) == 1
    assert got.black[3] == 0 and got.white[3] == 1 and got.midtone[3] == 0.5
    # the midtone sends the median to the target: mtf(mtf(t, x0), x0) = t
    st = cases[0]
    p = stretch_auto(st)
    for c in range(3):
        x0 = (float(st[c]["median"]) - float(p.black[c])) / (float(p.white[c]) - float(p.black[c]))
        assert abs(sr.mtf64(float(p.midtone[c]), x0) - 0.25) < 1e-5


# ---- 2. the tables --------------------------------------------------------------------------------------------------
def test_the_tables_against_the_restatement():
    for kind, params in ((CURVE_ASINH, (0.5, 10.0, 100.0, 1000.0, 1e6)), (CURVE_GAMMA, (0.3, 1.0, 2.2, 5.0)), (CURVE_SRGB, (0.0,))):
        for param in params:
            for knots in (2, 3, 255, 4096, 65536):
                t = stretch_table(kind, param, knots)
                assert t.shape == (knots + 1,) and t.dtype == np.float32
                assert _ulps(t, sr.table(kind, param, knots)).max() <= 1, (kind, param, knots)
                assert t[0] == 0.0 and t[knots] == 1.0 and (np.diff(t) >= 0).all() and np.isfinite(t).all()
    assert stretch_table(CURVE_GAMMA, 1.0, 8).tolist() == [k / 8 for k in range(9)]
    srgb = stretch_table(CURVE_SRGB, 0.0, 1000)
    assert abs(float(srgb[2]) - 12.92 * 0.002) < 1e-7 and abs(float(srgb[500]) - (1.055 * 0.5 ** (1 / 2.4) - 0.055)) < 1e-7


def test_the_asinh_table_against_the_exact_curve():
    rng = np.random.default_rng(0)
    K = 4096
    x = np.concatenate([rng.random(200000), np.linspace(0.0, 1.0, 100001), (np.arange(K) + 0.5) / K]).astype(F)
    for beta, bar in BAR_ASINH.items():
        got = sr.curve_f32(x, sr.TABLE, tab=stretch_table(CURVE_ASINH, beta, K)).astype(np.float64)
        err = float(np.abs(got - np.arcsinh(beta * x.astype(np.float64)) / math.asinh(beta)).max())
        print("asinh table, beta %g, K %d: worst error %.3e (bar %.3e)" % (beta, K, err, bar))
        assert err <= bar


# ---- 3. refusals that need no GPU -----------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    lib = _ffi.load()
    nan, inf = float("nan"), float("inf")
    t = (C.c_float * 9)()
    for kind, param, knots in ((3, 1.0, 8), (-1, 1.0, 8), (0, 0.0, 8), (0, -1.0, 8), (0, nan, 8), (0, inf, 8), (1, 0.0, 8), (1, nan, 8), (0, 1.0, 1), (0, 1.0, 0),
                               (0, 1.0, -5), (0, 1.0, 65537), (0, 1.0, 1 << 30)):
        assert lib.stk_stretch_table(kind, param, knots, t) == 2, (kind, param, knots)
        with pytest.raises(InvalidParams):
            stretch_table(kind, param, knots)
    assert lib.stk_stretch_table(0, 1.0, 8, None) == 2 and lib.stk_stretch_table(2, nan, 8, t) == 0       # sRGB does not read its parameter
    import tracemalloc
    tracemalloc.start()                                                         # the wrapper refuses before it allocates the table
    with pytest.raises(InvalidParams):
        stretch_table(0, 1.0, 1 << 30)
    assert tracemalloc.get_traced_memory()[1] < 1 << 20
    tracemalloc.stop()
    good = _records([(100, 0.01, 0.9, 0.02, 0.002, 0.5)] * 3)
    for bad in (dict(shadows_clip=0.1), dict(shadows_clip=nan), dict(shadows_clip=-inf), dict(target_background=0.0), dict(target_background=1.0),
                dict(target_background=nan), dict(white=inf), dict(white=nan), dict(linked=2), dict(linked=-1), dict(white_mode=3), dict(white_mode=-1),
                dict(white_quantile=1.5), dict(white_quantile=nan)):
        with pytest.raises(InvalidParams):
            stretch_auto(good, AutoStretchParameters(**bad))
    for field in ("min", "max", "median", "mad"):
        for v in (nan, inf):
            st = good.copy()
            st[1][field] = v
            with pytest.raises(InvalidParams):
                stretch_auto(st)
    st = good.copy()
    st[0]["count"] = -1
    with pytest.raises(InvalidParams):
        stretch_auto(st)
    for bad in (good[:2], np.zeros(3, np.float32), np.zeros(5, STAT_DTYPE), np.zeros((1, 3), STAT_DTYPE)):
        with pytest.raises(InvalidParams):
            stretch_auto(bad)
    out, rec4 = _ffi.StretchParams(), np.zeros(4, STAT_DTYPE)
    recs = rec4.ctypes.data_as(C.POINTER(_ffi.ImageStat))
    assert lib.stk_stretch_auto(None, 3, None, C.byref(out)) == 2 and lib.stk_stretch_auto(recs, 3, None, None) == 2
    assert lib.stk_stretch_auto(recs, 2, None, C.byref(out)) == 2 and lib.stk_stretch_auto(recs, 0, None, C.byref(out)) == 2
    assert lib.stk_stretch_auto(recs, 3, None, C.byref(out)) == 0 and out.curve == 1     # null parameters: the defaults
    # the entry points without a context
    img, o, p = _ffi.ImageF32(), _ffi.ImageOut(), StretchParameters()._c()
    assert lib.stk_image_stats(None, C.byref(img), None, 0, 0, None, 0, recs) == 2
    assert lib.stk_stretch(None, C.byref(img), C.byref(p), None, 0, C.byref(o)) == 2
    assert lib.stk_auto_stretch(None, C.byref(img), None, 0, 0, None, 1, 0, 1.0, None, 0, C.byref(o), None, None) == 2
    # the wrappers' own refusals, before any C call
    st = new_stacker()
    image = np.zeros((40, 50, 3), np.float32)
    for bad in (lambda: st.image_stats(image.astype(np.float64)), lambda: st.image_stats(image, mask=np.zeros((40, 51), np.float32)),
                lambda: st.image_stats(image, mask=np.zeros((40, 50, 3), np.float32)), lambda: st.image_stats(image, quantiles=[0.1] * 5),
                lambda: st.stretch_image(image.astype(np.uint8)), lambda: st.stretch_image(image, out=np.zeros((40, 50, 3), np.uint8)),
                lambda: st.stretch_image(image, StretchParameters(out_depth=DEPTH_U8), out=np.zeros((40, 50, 3), np.float32)),
                lambda: st.stretch_image(image, StretchParameters(out_depth=DEPTH_U16), out=np.zeros((40, 100, 3), np.uint16)[:, ::2]),
                lambda: st.stretch_image(image, StretchParameters(out_depth=12)), lambda: st.stretch_image(image, StretchParameters(black=[0.0] * 5)),
                lambda: st.stretch_image(image, StretchParameters(curve=STRETCH_TABLE)), lambda: st.stretch_image(image, StretchParameters(curve=STRETCH_TABLE, table=[0.0, 1.0])),
                lambda: st.stretch_image(image, StretchParameters(curve=STRETCH_TABLE, table=np.zeros(65538))),
                lambda: st.auto_stretch_image(image, curve=STRETCH_TABLE), lambda: st.auto_stretch_image(image, out_depth=7),
                lambda: st.auto_stretch_image(image, mask=np.zeros((41, 50), np.float32))):
        with pytest.raises(InvalidParams):
            bad()
    assert not st._lib.calls


# ---- 4. what the wrappers hand to the C ABI -------------------------------------------------------------------------
def test_what_the_wrappers_hand_to_the_c_abi():
    rng = np.random.default_rng(3)
    h, w = 20, 30
    for cn in (1, 3, 4):
        image = rng.random((h, w, cn)).astype(np.float32)
        desc = dict(data=image.ctypes.data, width=w, height=h, channels=cn, location=0, row_stride_bytes=0)
        st = new_stacker()
        rec = st.image_stats(image)
        name, snap = st._lib.last()
        assert name == "stk_image_stats" and snap[0] == CTX and snap[1] == desc and snap[2] is None and snap[3:7] == [0, 0, None, 0] and snap[7] is not None
        assert rec.shape == (min(cn, 3),) and rec.dtype == STAT_DTYPE
        st.image_stats(image, quantiles=[0.25, 1.0])
        snap = st._lib.last()[1]
        assert snap[6] == 2 and snap[5] == np.float64(0.25).tobytes()
        for depth, dtype in ((DEPTH_U8, np.uint8), (DEPTH_U16, np.uint16), (DEPTH_F32, np.float32)):
            p = StretchParameters(out_depth=depth)
            out = st.stretch_image(image, p)
            name, snap = st._lib.last()
            assert name == "stk_stretch" and snap[0] == CTX and snap[1] == desc and snap[2] == _bytes_of(p._c()) and snap[3] is None and snap[4] == 0
            assert out.shape == (h, w, cn) and out.dtype == dtype
            o = _ffi.ImageOut.from_buffer_copy(snap[5])
            assert (o.data, o.width, o.height, o.channels, o.depth, o.location, o.row_stride_bytes) == (out.ctypes.data, w, h, cn, depth, 0, 0)
        out = st.auto_stretch_image(image)
        name, snap = st._lib.last()
        assert name == "stk_auto_stretch" and snap[1] == desc and snap[2] is None and snap[3:5] == [0, 0] and snap[5] == _bytes_of(AutoStretchParameters()._c())
        assert snap[6:11] == [1, 0, 1.0, None, 0] and snap[12] is None and snap[13] is None and out.dtype == np.float32
        res, rec, used = st.auto_stretch_image(image, return_stats=True, return_params=True)
        snap = st._lib.last()[1]
        assert snap[12] is not None and snap[13] is not None and rec.shape == (min(cn, 3),) and isinstance(used, StretchParameters)
    # parameters, a table, a mask with padded rows, a padded image, the caller's output, in place
    tab = stretch_table(CURVE_ASINH, 50.0, 16)
    p = StretchParameters(curve=STRETCH_TABLE, colour=1, out_depth=DEPTH_U16, black=[0.1, 0.2, 0.3], white=2.0, midtone=[0.25, 0.5], out_scale=3.0, table=tab)
    wide = rng.random((h, w + 5, 3)).astype(np.float32)
    image = wide[:, :w]
    mine = np.zeros((h, w + 2, 3), np.uint16)[:, :w]
    st = new_stacker()
    assert st.stretch_image(image, p, out=mine) is mine
    snap = st._lib.last()[1]
    c = _ffi.StretchParams.from_buffer_copy(snap[2])
    assert (c.curve, c.colour, c.out_depth, c.reserved, c.out_scale) == (2, 1, 16, 0, 3.0)
    assert list(c.black) == [F(0.1), F(0.2), F(0.3), 0.0] and list(c.white) == [2.0] * 4 and list(c.midtone) == [0.25, 0.5, 0.5, 0.5]
    assert snap[1]["data"] == wide.ctypes.data and snap[1]["row_stride_bytes"] == (w + 5) * 12 and snap[4] == 16
    assert bytes(C.string_at(snap[3], 17 * 4)) == tab.tobytes()
    o = _ffi.ImageOut.from_buffer_copy(snap[5])
    assert (o.data, o.width, o.height, o.channels, o.depth, o.location, o.row_stride_bytes) == (mine.ctypes.data, w, h, 3, 16, 0, (w + 2) * 6)
    assert st.stretch_image(image, StretchParameters(), out=image) is image
    snap = st._lib.last()[1]
    o = _ffi.ImageOut.from_buffer_copy(snap[5])
    assert (o.data, o.row_stride_bytes, o.depth) == (snap[1]["data"], snap[1]["row_stride_bytes"], 32)
    mwide = rng.random((h, w + 3)).astype(np.float32)
    auto = AutoStretchParameters(shadows_clip=-1.5, target_background=0.2, linked=1, white_mode=2, white=0.8, white_quantile=0.99)
    out8 = np.zeros((h, w, 3), np.uint8)
    assert st.auto_stretch_image(image, auto, curve=STRETCH_TABLE, colour=1, out_depth=DEPTH_U8, out_scale=2.0, table=tab, mask=mwide[:, :w], out=out8) is out8
    name, snap = st._lib.last()
    assert snap[2] == mwide.ctypes.data and snap[3] == (w + 3) * 4 and snap[4] == 0 and snap[6:9] == [2, 1, 2.0] and snap[10] == 16
    a = _ffi.StretchAutoParams.from_buffer_copy(snap[5])
    assert (a.shadows_clip, a.target_background, a.white, a.white_quantile, a.linked, a.white_mode) == (-1.5, 0.2, 0.8, 0.99, 1, 2)
    st.image_stats(image, mask=mwide[:, :w])
    snap = st._lib.last()[1]
    assert snap[2] == mwide.ctypes.data and snap[3] == (w + 3) * 4 and snap[4] == 0
    grey = rng.random((h, w)).astype(np.float32)
    assert st.stretch_image(grey).shape == (h, w, 1) and st._lib.last()[1][1]["channels"] == 1


# ---- 5. identities of the restatement -------------------------------------------------------------------------------
def test_identities_of_the_restatement():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(20000), [0.0, 1.0, 0.5, 2.0 ** -24, 1 - 2.0 ** -24]]).astype(F)
    assert sr.curve_f32(x, sr.MTF, 0.5).tobytes() == x.tobytes()                # m = 0.5: (-0.5 x) / fma(0, x, -0.5) = x
    for m in (0.01, 0.1, 0.3, 0.7, 0.99):
        y = sr.curve_f32(x, sr.MTF, m)
        assert y[-5] == 0 and 1 - y[-4] <= 2.0 ** -23 and (y >= 0).all() and (y <= 1).all()      # (k - m is m - 1 to within an ulp only)
        assert abs(float(y[-3]) - (1 - m)) < 1e-6                               # mtf(m, 0.5) = 1 - m ... and mtf(m, m) = 0.5
        assert abs(float(sr.curve_f32(F(m), sr.MTF, m)) - 0.5) < 1e-6
    for t in (0.1, 0.25, 0.8):                                                  # mtf(mtf(t, x), x) = t: the rule's f64, within 2 f32 ulp
        xs = rng.uniform(0.001, 0.999, 1000)
        assert _ulps(sr.mtf64(sr.mtf64(t, xs), xs).astype(F), np.full(1000, t, F)).max() <= 2
    d = ((rng.random((9, 11, 3)) - 0.25) * 2).astype(F)
    d[0, 0, 0], d[0, 1, 1], d[0, 2, 2], d[1, 0, 0] = np.nan, np.inf, -np.inf, -0.0
    lin = sr.stretch(d, sr.LINEAR)
    with np.errstate(invalid="ignore"):
        want = np.fmin(np.fmax(d, F(0)), F(1))
    assert np.array_equal(lin, want) and lin[0, 0, 0] == 0 and lin[0, 1, 1] == 1 and lin[0, 2, 2] == 0
    # a table that is the identity; two knots; x = 1 reads the last interval
    ident = (np.arange(17) / 16).astype(F)
    got = sr.stretch(d, sr.TABLE, tab=ident)
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24
    assert sr.curve_f32(F(1.0), sr.TABLE, tab=np.array([0.0, 0.25, 1.0], F)) == 1.0
    # colour mode under the linear curve is the per-channel result; grey pixels are treated alike in both modes
    assert np.abs(sr.stretch(d, sr.LINEAR, colour=1).astype(np.float64) - want).max() <= 2.0 ** -23
    grey = np.repeat(rng.random((5, 7, 1)).astype(F), 3, 2)
    a, b = sr.stretch(grey, sr.MTF, 0, midtone=0.1), sr.stretch(grey, sr.MTF, 1, midtone=0.1)
    # (L, the curve's three operations twice, g / L and x s: some eight roundings of values of at most 1)
    assert np.abs(a.astype(np.float64) - b).max() <= 8 * 2.0 ** -24
    # half to even: y * 255 on .5
    half = np.array([[0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255]], F)
    assert (half * F(255)).astype(F).tolist() == [[0.5, 1.5, 2.5, 254.5]]
    assert sr.stretch(half, sr.LINEAR, out_depth=8)[..., 0].tolist() == [[0, 2, 2, 254]]
    assert sr.stretch(np.array([[0.0, 1.0, 5.0, -5.0, np.nan]], F), sr.LINEAR, out_depth=16)[..., 0].tolist() == [[0, 65535, 65535, 0, 0]]
    # the statistics: -0 is +0, the lower median, the quantile ranks
    v = np.array([[3.0, -0.0, 0.0, np.nan, np.inf, -2.0, 7.0, -np.inf]], F)
    s = sr.stats(v, quantiles=(0.0, 1.0, 0.2, 0.21))[0]
    assert (s["count"], s["min"], s["max"], s["median"]) == (5, -2.0, 7.0, 0.0) and s["mad"] == 2.0
    assert s["q"].tolist() == [-2.0, 7.0, -2.0, 0.0] and not np.signbit(s["median"])
    assert sr.stats(np.array([[1.0, 2.0]], F))[0]["median"] == 1.0              # N even: the smaller of the two
    assert sr.stats(np.full((2, 2), np.nan, F))[0].tobytes() == bytes(40)


# ---- 6. quality, on the restatement ---------------------------------------------------------------------------------
def _median(a):
    s = np.sort(np.asarray(a).reshape(-1))
    return float(s[(s.size + 1) // 2 - 1])


def test_auto_stretch_quality_of_the_definition():
    for seed in SEEDS:
        d = sr.scene(seed)
        out, st, (b, w, m) = sr.auto_stretch(d)
        med = [_median(out[..., c]) for c in range(3)]
        off = max(abs(v - 0.25) for v in med)
        clipped = float((out == 0).mean())
        print("seed %d: medians %s, worst offset %.3e, spread %.3e, clipped %.4f %%" % (seed, med, off, max(med) - min(med), 100 * clipped))
        assert off <= BAR_MEDIAN and max(med) - min(med) <= BAR_MEDIAN
        assert clipped < 0.01 and all(float((out[..., c] == 0).mean()) < 0.01 for c in range(3))
        assert (st["median"] < 0.05).all() and min(med) > 5 * float(st["median"].max())    # the picture was black and is not any more
        # linked: one black, white and midtone for all, so under the linear curve the offsets of the channel medians from
        # black keep their ratio (channel 2's sky is below the common black point and clips: channels 0 and 1 are held)
        lb, lw, lm = sr.auto(st, linked=1)
        assert len(set(lb[:3].tolist())) == len(set(lw[:3].tolist())) == len(set(lm[:3].tolist())) == 1
        lin = sr.stretch(d, sr.LINEAR, black=lb, white=lw)
        r_in = (float(st[1]["median"]) - float(lb[1])) / (float(st[0]["median"]) - float(lb[0]))
        r_out = _median(lin[..., 1]) / _median(lin[..., 0])
        assert abs(r_out / r_in - 1.0) < 4 * 2.0 ** -23, (r_in, r_out)
        mtf_out = sr.stretch(d, sr.MTF, black=lb, white=lw, midtone=lm)
        assert _median(mtf_out[..., 1]) > _median(mtf_out[..., 0]) > _median(mtf_out[..., 2])      # the colour of the sky is kept


# ---- 7. the kernel map of the new unit ------------------------------------------------------------------------------
def test_the_extra_unit_has_its_kernel_map_and_every_kernel_a_gpu_test(tmp_path):
    """tests/kernel_extra_stretch.tsv (tools/kernel_coverage.py, EXTRA: the last table, where every later unit goes). Only this
    unit's rows are checked, and neither the table's contents nor any total row count is pinned: the kernels of the unit,
    recomputed with the Makefile's own command, are the rows of the file; every row names a GPU test file that exists,
    qualifies and is marked gpu; no kernel is listed twice anywhere; write_map on copies returns every map byte for byte. The
    rows were written from the symbol names and the test file that launches each kernel, not from a trace. Only kernel symbol
    names are read."""
    import shutil
    from test_cpu_kernel_map import kc
    unit = "post/kernels_stretch"
    assert unit in kc.EXTRA
    path = kc.extra_file(unit)
    assert os.path.basename(path) == "kernel_extra_" + kc.EXTRA[unit] + ".tsv"
    assert path not in kc.parts() + kc.supplements() + [kc.own_file(u) for u in kc.OWN] + [kc.post_file(u) for u in kc.POST]
    assert os.path.isfile(os.path.join(kc.CSRC, unit + ".hip"))
    rows = kc.read_rows(path)
    assert rows and all(r[0] == unit for r in rows) and all(r in kc.read_extra() for r in rows)
    for _, mangled, demangled, files in rows:
        assert mangled.startswith("_ZN3stk") and "stk::" in demangled and files
        for f in files:
            assert kc.qualifies(f) and re.search(r"pytest\.mark\.gpu\b", open(os.path.join(ROOT, "tests", f)).read())
    assert not kc.uncovered(rows)
    listed = [r[1] for r in kc.read_map() + kc.read_own() + kc.read_post() + kc.read_extra()]
    assert len(set(listed)) == len(listed)
    assert not any(r[0] in kc.EXTRA for r in kc.read_map() + kc.read_own() + kc.read_post())
    # the default unit set leaves the table's units out; asked for, they are there
    assert unit not in kc.unit_commands() and unit in kc.unit_commands(extra=True)
    assert set(kc.unit_commands(extra=True)) - set(kc.unit_commands()) == set(kc.EXTRA) & set(kc.unit_commands(extra=True))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is not None:                                         # (as tests/test_cpu_kernel_map.py: no compiler, no recomputation)
        built = kc.build_kernels(workdir=str(tmp_path), extra=True)
        assert unit in built and {(unit, n) for n in built[unit]} == {(r[0], r[1]) for r in rows}
    # write_map on copies: every committed map returns byte for byte
    files = [kc.MAP] + kc.parts() + kc.supplements() + [kc.own_file(u) for u in sorted(kc.OWN)] + [kc.post_file(u) for u in sorted(kc.POST)]
    files += [kc.extra_file(u) for u in sorted(kc.EXTRA)]
    files = [f for f in files if os.path.isfile(f)]
    copies = [str(tmp_path / os.path.basename(f)) for f in files]
    for src, dst in zip(files, copies):
        open(dst, "w").write(open(src).read())
    kernels, seen = {}, {}
    for u, mangled, _, tests in kc.read_map(copies[0]) + kc.read_own(copies[0]) + kc.read_post(copies[0]) + kc.read_extra(copies[0]):
        kernels.setdefault(u, []).append(mangled)
        seen[mangled] = set(tests)
    kc.write_map({u: sorted(v) for u, v in kernels.items()}, seen, copies[0])
    assert all(open(src).read() == open(dst).read() for src, dst in zip(files, copies))


# ---- 8. the sanitizer harness ---------------------------------------------------------------------------------------
def test_stretch_host_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "stretch_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "stretch_harness.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=500)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

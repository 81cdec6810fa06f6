"""Frame calibration, CPU side: the numpy restatement (calibrate_restate.py) against a scalar, pixel-by-pixel loop and
against a planted stack whose arithmetic is exact in f32; the comparator network of kernels_calibrate.hip by the 0 / 1
principle; the ctypes mirrors against a C compiler's sizeof; the four entry points under a NULL context."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import calibrate_restate as cr
from libstacker_rs_amd import CalibrationParameters, DefectParameters, _ffi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the scalar loop: the definition read literally, one pixel and channel at a time --------------------------------------
def _rank(v):
    """Sort key of the definition's order without the integer trick: numbers by value, -0 below +0, NaN above all."""
    v = float(v)
    return (1, 0.0, 0) if math.isnan(v) else (0, v, 0 if math.copysign(1.0, v) < 0 else 1)


def _median_scalar(vals):
    a = sorted(vals, key=_rank)
    m = len(a)
    a = [F(np.nan) if math.isnan(float(x)) else F(x) for x in a]
    if m % 2:
        return a[(m - 1) // 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return F(F(a[m // 2 - 1] + a[m // 2]) * F(0.5))


def _value_scalar(raw, B, D, Fl, s, fm, fmin, ped):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = F(raw)
        if B is not None:
            v = F(v - F(B))
        if D is not None:
            v = F(v - F(F(s) * F(D)))
        if Fl is not None:
            t = F(v * F(fm))
            f = F(fmin) if math.isnan(float(Fl)) else max(F(Fl), F(fmin))
            v = F(t / f)
        return F(v + F(ped))


def _store_scalar(v, out_depth):
    if out_depth == 32:
        return F(v)
    if math.isnan(float(v)):
        return 0
    hi = 255 if out_depth == 8 else 65535
    r = float(np.rint(F(v)))
    return int(min(max(r, 0.0), float(hi)))


def calibrate_scalar(frames, bias, dark, flat, dark_scale, flat_mean, flat_min, pedestal, defects, step, out_depth):
    n, h, w, cn = frames.shape
    cc = min(cn, 3)
    out = np.zeros(frames.shape, {8: np.uint8, 16: np.uint16, 32: F}[out_depth])
    at = lambda m, y, x, c: None if m is None else m[y, x, c]
    for i, y, x, c in itertools.product(range(n), range(h), range(w), range(cn)):
        if c >= cc:
            out[i, y, x, c] = _store_scalar(F(frames[i, y, x, c]), out_depth)
            continue
        s = 1.0 if dark_scale is None else dark_scale[i]
        val = lambda yy, xx: _value_scalar(frames[i, yy, xx, c], at(bias, yy, xx, c), at(dark, yy, xx, c), at(flat, yy, xx, c), s,
                                           None if flat is None else flat_mean[c], flat_min, pedestal)
        v = val(y, x)
        if defects is not None and (defects[y, x] >> c) & 1:
            good = [val(y + dy * step, x + dx * step) for dx, dy in cr.OFFSETS
                    if 0 <= y + dy * step < h and 0 <= x + dx * step < w and not (defects[y + dy * step, x + dx * step] >> c) & 1]
            if good:
                v = _median_scalar(good)
        out[i, y, x, c] = _store_scalar(v, out_depth)
    return out


def _small_case(dtype, cn, seed, nan_master=False):
    rng = np.random.default_rng(seed)
    n, h, w = 2, 7, 9
    if dtype == F:
        frames = rng.normal(100, 40, (n, h, w, cn)).astype(F)
    else:
        frames = rng.integers(0, np.iinfo(dtype).max + 1, (n, h, w, cn)).astype(dtype)
    top = 255.0 if dtype != np.uint16 else 65535.0
    bias = rng.uniform(0, top / 8, (h, w, cn)).astype(F)
    dark = rng.uniform(0, top / 8, (h, w, cn)).astype(F)
    flat = rng.uniform(0.2, 2.0, (h, w, cn)).astype(F)
    flat[1, 1, 0] = 0.0                                    # below flat_min: clamped
    if nan_master:
        bias[2, 3, 0] = np.nan
        dark[4, 4, cn - 1] = np.inf
        flat[5, 2, 0] = np.nan
    defects = (rng.random((h, w)) < 0.25).astype(np.uint8) * rng.integers(1, 8, (h, w)).astype(np.uint8)
    defects[0, 0] = 7
    defects[2:5, 5:8] = 7                                  # a whole 3 x 3 block: its centre has no good neighbour at step 1
    return frames, bias, dark, flat, defects


@pytest.mark.parametrize("subset", list(itertools.product([0, 1], repeat=4)), ids=lambda s: "bdfm=" + "".join(map(str, s)))
def test_restatement_is_the_scalar_loop_for_every_master_subset(subset):
    frames, bias, dark, flat, defects = _small_case(np.uint8, 3, 1)
    b, d, f, m = subset
    kw = dict(bias=bias if b else None, dark=dark if d else None, flat=flat if f else None, dark_scale=[1.0, 2.5] if d else None,
              flat_mean=[1.0, 0.9, 1.1, 1.0], flat_min=0.05, pedestal=3.25, defects=defects if m else None, step=1)
    for od in (8, 32):
        got = cr.calibrate_restate(frames, out_depth=od, **kw)
        want = calibrate_scalar(frames, kw["bias"], kw["dark"], kw["flat"], kw["dark_scale"], kw["flat_mean"], 0.05, 3.25, kw["defects"], 1, od)
        assert cr.same_bits(got, want)


@pytest.mark.parametrize("dtype,cn,od", [(np.uint8, 1, 8), (np.uint16, 4, 16), (np.uint16, 3, 32), (F, 3, 32), (F, 4, 32)])
@pytest.mark.parametrize("step", [1, 2])
def test_restatement_is_the_scalar_loop_for_depths_steps_and_nan_masters(dtype, cn, od, step):
    frames, bias, dark, flat, defects = _small_case(dtype, cn, 2 + cn, nan_master=True)
    kw = dict(bias=bias, dark=dark, flat=flat, dark_scale=[0.5, 2.0], flat_mean=[1.0, 2.0, 0.5, 1.0], flat_min=0.25, pedestal=-2.0,
              defects=defects, step=step)
    got = cr.calibrate_restate(frames, out_depth=od, **kw)
    want = calibrate_scalar(frames, bias, dark, flat, kw["dark_scale"], kw["flat_mean"], 0.25, -2.0, defects, step, od)
    assert cr.same_bits(got, want)
    if od == 32:
        assert np.isnan(got).any()                         # the NaN of the masters reached the output somewhere
    if cn == 4:
        assert np.array_equal(got[..., 3].astype(np.float64), frames[..., 3].astype(np.float64))      # alpha untouched


def test_rounding_saturation_and_the_order():
    v = np.array([0.5, 1.5, 2.5, -0.5, 254.5, 255.5, 300.0, -7.0, np.nan, np.inf, -np.inf], F)
    assert list(cr.to_depth(v, 8)) == [0, 2, 2, 0, 254, 255, 255, 0, 0, 255, 0]              # half to even, clamp, NaN -> 0
    assert list(cr.to_depth(np.array([65534.5, 65535.5, 7e4], F), 16)) == [65534, 65535, 65535]
    vals = np.array([np.nan, 3.0, -np.inf, 0.0, -0.0, np.inf, -2.0, 1.0], F)
    order = np.argsort(cr.order_key(vals), kind="stable")
    assert list(order) == [2, 6, 4, 3, 7, 1, 5, 0]
    assert cr.same_bits(cr.from_key(cr.order_key(vals)), vals)
    pres = np.ones(8, bool)
    med, m = cr.median_rule(vals[:, None], pres[:, None])
    assert m[0] == 8 and med[0] == F(0.5)                  # (a_3 + a_4) / 2 = (0 + 1) / 2
    pres[0] = pres[5] = False                              # six left: -inf -2 -0 0 1 3 -> (-0 + 0) / 2
    med, m = cr.median_rule(vals[:, None], pres[:, None])
    assert m[0] == 6 and med[0] == 0.0
    pres[:] = False
    pres[[0, 1, 7]] = True                                 # 1 3 NaN -> 3
    assert cr.median_rule(vals[:, None], pres[:, None])[0][0] == F(3.0)
    pres[7] = False                                        # 3 NaN -> NaN
    assert np.isnan(cr.median_rule(vals[:, None], pres[:, None])[0][0])


def test_defect_map_restatement_by_hand():
    m = np.full((5, 6, 1), 10.0, F)
    m[2, 2, 0] = 31.0                                      # hot by 21
    m[0, 0, 0] = 4.0                                       # a corner: three neighbours, dead at ratio 0.5
    m[4, 5, 0] = np.inf
    got, counts = cr.defect_map_restate(m, high=True, low=False, high_abs=20.0)
    want = np.zeros((5, 6), np.uint8)
    want[2, 2] = want[4, 5] = 1
    assert np.array_equal(got, want) and list(counts) == [2, 0, 0, 0]
    got2, counts2 = cr.defect_map_restate(m, high=False, low=True, low_ratio=0.5, previous=got)
    want[0, 0] = 1
    assert np.array_equal(got2, want) and counts2[0] == 3
    one, c1 = cr.defect_map_restate(np.full((1, 1, 3), 5.0, F), high=True, low=True)                # no neighbour: no test applies
    assert one[0, 0] == 0 and c1.sum() == 0
    two, _ = cr.defect_map_restate(np.array([[[1.0], [100.0]], [[1.0], [1.0]]], F), high=True, high_abs=10.0, step=2)
    assert not two.any()                                   # 2 x 2 at step 2: nobody has a neighbour


# ---- the planted stack ----------------------------------------------------------------------------------------------------
def test_planted_defects_are_found_exactly():
    p = cr.planted()
    dmap, counts = cr.defect_map_restate(p["dark"], high=True, low=False, high_abs=20.0)
    dmap, counts = cr.defect_map_restate(p["flat"], high=False, low=True, low_ratio=0.5, previous=dmap)
    assert np.array_equal(dmap, p["defects"]) and p["hot"].sum() == 5 and p["dead"].sum() == 5
    assert list(counts[:3]) == [int((p["hot"] | p["dead"])[..., c].sum()) for c in range(3)]


def test_planted_calibration_returns_the_scene_exactly():
    p = cr.planted()
    kw = dict(bias=p["bias"], dark=p["dark"], flat=p["flat"], dark_scale=p["scale"], flat_mean=[cr.FLAT_LEVEL] * 4, flat_min=1.0)
    for od in (8, 32):
        got = cr.calibrate_restate(p["lights"], defects=p["defects"], out_depth=od, **kw)
        assert all(np.array_equal(g.astype(F), p["scene"]) for g in got)
    bare = cr.calibrate_restate(p["lights"], out_depth=32)
    assert not any(np.array_equal(g, p["scene"]) for g in bare)
    unrepaired = cr.calibrate_restate(p["lights"], out_depth=32, **kw)
    wrong = unrepaired[0] != p["scene"]
    assert wrong.any() and not (wrong & ~(p["hot"] | p["dead"])).any()        # only the planted pixels are off without the map


def test_planted_masters_come_back_from_their_frames():
    p = cr.planted()
    bias_f, dark_f, flat_f = cr.planted_calibration_frames(p)
    mb, kb = cr.master_stack_restate(bias_f)
    assert np.array_equal(mb, p["bias"]) and kb.min() == 4 and (kb == 4).sum() == 3          # the hit, in three channels
    md, _ = cr.master_stack_restate(cr.calibrate_restate(dark_f, bias=mb, out_depth=32))
    assert np.array_equal(md, p["dark"])
    mf, _ = cr.master_stack_restate(cr.calibrate_restate(flat_f, bias=mb, out_depth=32), normalize=2, stat_step=4)
    assert np.array_equal(mf, p["flat"])
    assert list(cr.image_mean_restate(p["bias"])) == [float(p["bias"][..., c].astype(np.float64).mean()) for c in range(3)]


# ---- the kernel's comparator network, by the 0 / 1 principle ----------------------------------------------------------------
def test_the_comparator_network_sorts():
    src = open(os.path.join(ROOT, "libstacker_rs_amd", "csrc", "kernels_calibrate.hip")).read()
    body = src[src.index("cal_median8("):src.index("const int jl")]
    pairs = [(int(a), int(b)) for a, b in re.findall(r"CAL_CX\((\d), (\d)\)", body)]
    assert len(pairs) == 19 and all(0 <= a < b < 8 for a, b in pairs)
    for bits in itertools.product([0, 1], repeat=8):
        k = list(bits)
        for a, b in pairs:
            k[a], k[b] = min(k[a], k[b]), max(k[a], k[b])
        assert k == sorted(bits)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_struct_sizes_are_the_c_compilers(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "stacker.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d %d\\n", (int)sizeof(stk_calibration), (int)sizeof(stk_defect_params),\n'
                   "           (int)offsetof(stk_calibration, flat_mean), (int)offsetof(stk_calibration, defects_or_null),\n"
                   "           (int)offsetof(stk_calibration, out_depth));\n    return 0;\n}\n")
    exe = tmp_path / "sizes"
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    K = _ffi.Calibration
    assert got == [C.sizeof(K), C.sizeof(_ffi.DefectParams), K.flat_mean.offset, K.defects_or_null.offset, K.out_depth.offset]
    assert C.sizeof(_ffi.DefectParams) == 24


def test_parameter_mirrors():
    d = DefectParameters(high=True, low=True, high_abs=12.5, low_ratio=0.25, step=2, accumulate=True)._c()
    assert (d.tests, d.high_abs, d.low_ratio, d.step, d.accumulate, d.reserved) == (3, 12.5, 0.25, 2, 1, 0)
    assert DefectParameters()._c().tests == 1
    c = CalibrationParameters()
    assert c.bias is None and c.defects is None and c.defect_step == 1 and c.pedestal == 0.0 and c.out_depth is None


def test_every_new_call_refuses_a_null_context():
    lib = _ffi.load()
    for name in ("stk_calibrate", "stk_defect_map", "stk_image_mean", "stk_master_stack"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    img = np.zeros((2, 2, 3), F)
    im = _ffi.ImageF32(img.ctypes.data, 2, 2, 3, 0, 0)
    frame = np.zeros((2, 2, 3), np.uint8)
    ptr = (C.c_void_p * 1)(frame.ctypes.data)
    fr = _ffi.Frames(C.cast(ptr, C.POINTER(C.c_void_p)), 1, 2, 2, 3, 8, 0, 0)
    out = np.zeros((2, 2, 3), np.uint8)
    optr = (C.c_void_p * 1)(out.ctypes.data)
    cal = _ffi.Calibration()
    cal.defect_step, cal.out_depth = 1, 8
    dp = DefectParameters()._c()
    clip = _ffi.RobustClipParams(3.0, 3.0, 0.5, 2)
    mp = np.zeros((2, 2), np.uint8)
    mean = np.zeros(4)
    INVALID = 2
    assert lib.stk_calibrate(None, C.byref(fr), C.byref(cal), C.cast(optr, C.c_void_p), 0) == INVALID
    assert lib.stk_defect_map(None, C.byref(im), C.byref(dp), C.c_void_p(mp.ctypes.data), 0, None) == INVALID
    assert lib.stk_image_mean(None, C.byref(im), C.c_void_p(mean.ctypes.data)) == INVALID
    assert lib.stk_master_stack(None, C.byref(fr), 0, 4, C.byref(clip), C.byref(im), None) == INVALID

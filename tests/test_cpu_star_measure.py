"""CPU tests of star measurement (include/stacker.h, stk_star_measure_params): the struct layouts, the symbols and the Rust
table against the header; the restatement (tests/star_measure_restate.py) by hand on a 5-star toy frame; the host functions
stk_star_shape_derive, stk_star_frame_quality, stk_star_quality_scores and stk_star_quality_weights against the restatement
bit for bit; stk_rank_frames on the scores; what the wrappers hand to the C ABI; every refusal of the host functions; the
sanitizer harness; and the accuracy of the definition itself on Gaussian star fields, before any GPU run."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import libstacker_rs_amd as ls
import star_deep_restate as sd
import star_measure_restate as sm
from libstacker_rs_amd import (QUALITY_DTYPE, SHAPE_DTYPE, InvalidParams, SelectParameters, StarDeepParameters, StarMeasureParameters, StarParameters,
                               StarQualityParameters, _ffi)
from test_cpu_api_calls import CTX, new_stacker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_star_measure", "stk_star_shape_derive", "stk_star_frame_quality", "stk_star_quality_scores", "stk_star_quality_weights",
       "stk_star_match_quality_weighted")
STRUCTS = (("stk_star_measure_params", _ffi.StarMeasureParams, 32), ("stk_star_shape", _ffi.StarShape, 152),
           ("stk_star_quality", _ffi.StarQuality, 48), ("stk_star_quality_params", _ffi.StarQualityParams, 40))
W, H = 480, 360


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


# ---- 1. layouts, symbols, the Rust table ----------------------------------------------------------------------------
def test_struct_layouts_symbols_and_table_against_the_header(tmp_path):
    lines = []
    for cname, cls, _ in STRUCTS:
        lines.append('  printf("%%zu", sizeof(%s));\n' % cname)
        lines += ['  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_]
        lines.append('  printf("\\n");\n')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    rows = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (cname, cls, size), row in zip(STRUCTS, rows):
        got = [int(v) for v in row.split()]
        assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], cname
        assert got[0] == size, cname
    assert SHAPE_DTYPE.itemsize == C.sizeof(_ffi.StarShape) and QUALITY_DTYPE.itemsize == C.sizeof(_ffi.StarQuality)
    for dt, cls in ((SHAPE_DTYPE, _ffi.StarShape), (QUALITY_DTYPE, _ffi.StarQuality)):
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(f, getattr(cls, f).offset) for f, _ in cls._fields_]
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
    for cname, _, _ in STRUCTS:
        assert "pub struct %s" % cname in rs
    assert re.search(r"STK_STAR_SCORE_FWHM\s*=\s*0,\s*STK_STAR_SCORE_ROUND\s*=\s*1,\s*STK_STAR_SCORE_SNR\s*=\s*2,\s*STK_STAR_SCORE_COUNT\s*=\s*3", hdr)
    assert (ls.STAR_SCORE_FWHM, ls.STAR_SCORE_ROUND, ls.STAR_SCORE_SNR, ls.STAR_SCORE_COUNT) == (0, 1, 2, 3)
    for name in ("StarMeasureParameters", "StarQualityParameters", "star_shape_derive", "star_frame_quality", "star_quality_scores",
                 "star_quality_weights", "SHAPE_DTYPE", "QUALITY_DTYPE"):
        assert name in ls.__all__ and hasattr(ls, name)
    m, q = StarMeasureParameters()._c(), StarQualityParameters()._c()
    assert (m.radius, m.ring_inner, m.ring_outer, m.kappa, m.min_contrast, m.min_pixels, m.saturation, m.reserved) == (7, 10, 14, 3.0, 1, 5, 0, 0)
    assert (q.fwhm_max, q.ecc_max, q.min_measured, q.fwhm_power, q.ecc_power, q.snr_power, q.reserved) == (0.0, 0.0, 5, 2, 0, 0, 0)
    for method in ("star_measure", "star_match_quality_weighted"):
        assert callable(getattr(ls.Stacker, method))


def test_the_nine_kernels_have_their_rows_in_a_supplement_of_the_kernel_map(tmp_path):
    """tests/kernel_map_star_measure.tsv: one row per instantiation, each naming the GPU test file; tools/kernel_coverage.py
    reads it with tests/kernel_map.tsv (tests/test_cpu_kernel_map.py holds the union against the tree) and `map` keeps a
    kernel in the file that lists it."""
    from test_cpu_kernel_map import kc
    extra = os.path.join(ROOT, "tests", "kernel_map_star_measure.tsv")
    assert extra in kc.supplements()
    rows = kc.read_file(extra)
    assert len(rows) == 9 and all(r[0] == "kernels_star_measure" and "star_measure_kernel<" in r[2] and r[3] == ["test_gpu_star_measure.py"] for r in rows)
    assert {re.search(r"<(.*?)>", r[2]).group(1) for r in rows} == {"%s, %d" % (t, c) for t in ("unsigned char", "unsigned short", "float") for c in (1, 3, 4)}
    main = kc.read_file(kc.MAP)
    assert not {r[1] for r in rows} & {r[1] for r in main} and len(kc.read_map()) == len(main) + 9
    # write_map on a copy: every row returns to its file, byte for byte
    a, b = str(tmp_path / "kernel_map.tsv"), str(tmp_path / "kernel_map_star_measure.tsv")
    for src, dst in ((kc.MAP, a), (extra, b)):
        open(dst, "w").write(open(src).read())
    kernels, seen = {}, {}
    for unit, mangled, _, files in kc.read_map(a):
        kernels.setdefault(unit, []).append(mangled)
        seen[mangled] = set(files)
    kc.write_map({u: sorted(v) for u, v in kernels.items()}, seen, a)
    assert open(a).read() == open(kc.MAP).read() and open(b).read() == open(extra).read()


# ---- 2. the restatement by hand -------------------------------------------------------------------------------------
def test_restatement_by_hand_on_a_toy_frame():
    """40 x 40, sky 100, R = 2, ring 3 .. 3: the ring is the four pixels at distance exactly 3, the aperture the 13 pixels
    with dx^2 + dy^2 <= 4."""
    g = np.full((40, 40), 100, np.uint16)
    g[19:22, 19:22] = 200                                                   # A: a 3 x 3 block around (20, 20)
    g[10, 10], g[10, 11] = 300, 200                                         # B: two pixels in a row
    g[20, 2] = 500                                                          # D: at px = R, the ring cut by the frame
    g[20, 5], g[17, 2], g[23, 2] = 110, 90, 100                             #    its three ring pixels inside the frame
    g[29:32, 29:32] = 65535                                                 # E: saturated
    stars = [(20, 20), (10, 10), (1, 20), (2, 20), (30, 30)]                # C = (1, 20): px < R
    mp = StarMeasureParameters(radius=2, ring_inner=3, ring_outer=3, min_pixels=1, saturation=60000)
    a, b, c, d, e = sm.measure(g, np.array(stars), mp)
    ints = lambda s: tuple(int(s[f]) for f in ("S", "Sx", "Sy", "Sxx", "Syy", "Sxy", "bg", "mad", "thr", "npix", "peak", "n_ring", "flags"))
    assert ints(a) == (900, 0, 0, 600, 600, 0, 100, 0, 1, 9, 200, 4, 0)
    assert (a["x"], a["y"], a["cxx"], a["cyy"], a["cxy"], a["ecc"]) == (20.0, 20.0, 600.0 / 900.0, 600.0 / 900.0, 0.0, 0.0)
    assert a["fwhm"] == 2.3548200450309493 * np.sqrt((600.0 / 900.0 + 600.0 / 900.0) / 2.0) and a["snr"] == 900.0 / (0.5 * 3.0)
    # B: v = 200 at dx = 0 and 100 at dx = 1: no extent in y, so no positive minor axis (bit 3); x, y and the moments stay
    assert ints(b) == (300, 100, 0, 100, 0, 0, 100, 0, 1, 2, 300, 4, 8)
    third = 100.0 / 300.0
    assert (b["x"], b["y"], b["cxx"], b["cyy"], b["fwhm"], b["ecc"], b["snr"]) == (10.0 + third, 10.0, third - third * third, 0.0, 0.0, 0.0, 0.0)
    # C: bit 0 and zeros
    assert ints(c) == (0,) * 12 + (1,) and (c["px"], c["py"]) == (1, 20) and all(c[f] == 0.0 for f in sm.DOUBLES)
    # D: three ring pixels 90, 100, 110: k = 2, bg = 100; |K - bg| = 10, 0, 10: mad = 10; thr = ceil(f32(3 * 1.4826) * 10) = 45
    assert ints(d) == (400, 0, 0, 0, 0, 0, 100, 10, 45, 1, 500, 3, 8)
    # E: saturated (bit 1): measured, not derived
    assert e["flags"] == 2 and e["peak"] == 65535 and e["npix"] == 9 and e["S"] == 9 * 65435 and e["fwhm"] == 0.0


def test_restatement_by_hand_uses_its_parameters():
    g = np.full((40, 40), 100, np.uint16)
    g[19:22, 19:22] = 200
    mp = StarMeasureParameters(radius=2, ring_inner=3, ring_outer=3, min_pixels=10)
    s = sm.measure(g, np.array([(20, 20)]), mp)[0]
    assert s["npix"] == 9 and s["flags"] == 4 and s["fwhm"] == 0.0          # npix < min_pixels
    s = sm.measure(g, np.array([(20, 20)]), StarMeasureParameters(radius=2, ring_inner=3, ring_outer=3, min_contrast=101))[0]
    assert s["npix"] == 0 and s["S"] == 0 and s["flags"] == 4 and s["thr"] == 101
    # the same frame at three depths and channel counts gives the same integers
    want = sm.measure(g, np.array([(20, 20)]), StarMeasureParameters(radius=2, ring_inner=3, ring_outer=3))[0]
    for f, deep in ((np.stack([g] * 3, -1), None), (g.astype(np.float32), StarDeepParameters(1.0)), ((g.astype(np.float32) / 4)[..., None].repeat(4, -1), StarDeepParameters(4.0))):
        assert sm.measure(f, np.array([(20, 20)]), StarMeasureParameters(radius=2, ring_inner=3, ring_outer=3), deep)[0].tobytes() == want.tobytes()


# ---- 3. the host functions against the restatement, bit for bit -----------------------------------------------------
def _random_shapes(rng, count):
    s = np.zeros(count, SHAPE_DTYPE)
    big = 65535 * 144 * 441
    s["S"] = rng.integers(0, 65535 * 441, count)
    s["S"][rng.random(count) < 0.1] = 0
    s["Sx"], s["Sy"], s["Sxy"] = (rng.integers(-12, 13, count) * s["S"] // 7 for _ in range(3))
    s["Sxx"], s["Syy"] = rng.integers(0, 144, count) * s["S"], rng.integers(0, 144, count) * s["S"]
    wild = rng.random(count) < 0.1
    s["Sxx"][wild] = rng.integers(0, big, int(wild.sum()))
    s["px"], s["py"] = rng.integers(0, 4096, count), rng.integers(0, 4096, count)
    s["bg"], s["mad"], s["npix"] = rng.integers(0, 65536, count), rng.integers(0, 300, count), rng.integers(1, 442, count)
    s["mad"][rng.random(count) < 0.2] = 0
    s["flags"] = np.where(rng.random(count) < 0.2, rng.integers(1, 8, count), 0)
    s["x"] = s["fwhm"] = np.nan                                             # stale values are overwritten
    return s


def test_shape_derive_equals_the_restatement():
    rng = np.random.default_rng(1)
    s = _random_shapes(rng, 3000)
    got, want = ls.star_shape_derive(s), sm.derive(s)
    assert got.tobytes() == want.tobytes()
    assert ((want["flags"] & 8) != 0).sum() > 20 and (want["fwhm"] > 0).sum() > 500 and (want["flags"] == 4).sum() > 20
    assert ls.star_shape_derive(got).tobytes() == got.tobytes()             # idempotent
    assert ls.star_shape_derive(np.zeros(0, SHAPE_DTYPE)).shape == (0,)
    # measured fields
    f, _ = sm.make_field(200, 150, 30, (2.0, 1.5, 0.3), seed=4)
    stars, _ = sd.detect(f, StarParameters())
    sh = sm.measure(f, stars)
    assert len(sh) > 15 and ls.star_shape_derive(sh).tobytes() == sh.tobytes()


def _quality_lists(rng):
    """frames with many stars, one star, no star, no measured star, and ties"""
    lists = [sm.derive(_random_shapes(rng, k)) for k in (40, 1, 0, 7, 12, 33)]
    lists[3]["flags"] |= 4                                                  # stars, none measured
    lists[3] = sm.derive(lists[3])
    t = lists[4]
    t[:] = t[0]                                                             # 12 equal shapes ...
    t["flags"] = 0
    t["S"], t["Sx"], t["Sy"], t["Sxx"], t["Syy"], t["Sxy"], t["npix"] = 1000, 10, -10, 4000, 2000, 300, 30
    t["mad"][:6] = 9                                                        # ... but for two values of mad, six each: the lower median
    t["mad"][6:] = 11
    lists[4] = sm.derive(t)
    return lists


def test_frame_quality_and_scores_equal_the_restatement():
    rng = np.random.default_rng(2)
    lists = _quality_lists(rng)
    got, want = ls.star_frame_quality(lists), sm.frame_quality(lists)
    assert got.tobytes() == want.tobytes()
    assert want["n_measured"].tolist()[1:4] == [int(lists[1]["flags"][0] == 0), 0, 0] and want["n_stars"].tolist() == [40, 1, 0, 7, 12, 33]
    assert all(want[2][f] == 0 for f in ("fwhm", "ecc", "snr", "bg", "noise")) and all(want[3][f] == 0 for f in ("fwhm", "ecc", "snr"))
    assert want[4]["noise"] == 1.4826 * 9 and want[4]["n_measured"] == 12   # the lower of the two middle values
    sc, sw = ls.star_quality_scores(got), sm.quality_scores(want)
    assert sc.tobytes() == sw.tobytes() and sc.shape == (6, 4)
    assert sc[2].tolist() == [0.0, 0.0, 0.0, 0.0] and sc[0, 0] == 1.0 / want[0]["fwhm"] and sc[0, 3] == want[0]["n_measured"]
    # the medians are taken each on its own: the frame's fwhm and ecc need not come from one star
    good = lists[0][lists[0]["flags"] == 0]
    assert want[0]["fwhm"] == np.sort(good["fwhm"])[(len(good) + 1) // 2 - 1] and want[0]["ecc"] == np.sort(good["ecc"])[(len(good) + 1) // 2 - 1]


def _quality(rows):
    q = np.zeros(len(rows), QUALITY_DTYPE)
    for i, (fw, ec, sn, m) in enumerate(rows):
        q[i]["fwhm"], q[i]["ecc"], q[i]["snr"], q[i]["n_measured"], q[i]["n_stars"] = fw, ec, sn, m, m
    return q


Q6 = [(3.1, 0.30, 40.0, 50), (2.7, 0.25, 55.0, 60), (5.9, 0.70, 21.0, 30), (2.7, 0.41, 33.0, 4), (4.0, 0.10, 60.0, 9), (0.0, 0.0, 0.0, 0)]


@pytest.mark.parametrize("powers", list(itertools.product(range(5), repeat=3))[3::7] + [(k, k, k) for k in range(5)] + [(2, 0, 0)])
def test_quality_weights_equal_the_restatement_at_every_power(powers):
    q = _quality(Q6)
    u = np.array([1.0, 0.5, 2.0, 1.0, 0.0, 3.0], np.float32)
    for kw in (dict(), dict(fwhm_max=4.0), dict(ecc_max=0.3, min_measured=1), dict(fwhm_max=3.0, ecc_max=0.26)):
        p = StarQualityParameters(fwhm_power=powers[0], ecc_power=powers[1], snr_power=powers[2], **kw)
        for reference, include, weights in ((-1, None, None), (0, None, u), (2, [1, 1, 1, 1, 0, 0], u), (-1, [0, 1, 1, 1, 1, 1], None)):
            want = sm.quality_weights(q, p, reference, include, weights)
            assert want is not None
            w, inc, rej = ls.star_quality_weights(q, p, reference, include, weights)
            assert w.tobytes() == want[0].tobytes() and inc.tolist() == want[1].tolist() and rej == want[2]
            assert (w[inc == 0] == 0).all() and inc[5] == 0


def test_quality_weights_by_hand():
    q = _quality(Q6)
    w, inc, rej = ls.star_quality_weights(q)                                # defaults: fwhm_power 2, min_measured 5
    assert inc.tolist() == [1, 1, 1, 0, 1, 0] and rej == 2                   # frames 3 and 5 have fewer than 5 measured stars
    F = 2.7
    assert w.tolist() == [np.float32((F / 3.1) * (F / 3.1)), 1.0, np.float32((F / 5.9) * (F / 5.9)), 0.0, np.float32((F / 4.0) * (F / 4.0)), 0.0]
    # a failing reference passes all the same; an excluded frame that would fail is not counted as rejected
    w, inc, rej = ls.star_quality_weights(q, StarQualityParameters(fwhm_max=3.0), reference=2, include=[1, 1, 1, 0, 1, 1])
    assert inc.tolist() == [0, 1, 1, 0, 0, 0] and rej == 3 and w[2] == np.float32((2.7 / 5.9) * (2.7 / 5.9))
    # ties and zero denominators: a factor whose denominator is 0 is 1
    z = _quality([(0.0, 1.0, 0.0, 9), (0.0, 1.0, 0.0, 9)])
    w, inc, rej = ls.star_quality_weights(z, StarQualityParameters(fwhm_power=4, ecc_power=4, snr_power=4), weights=[0.25, 3.0])
    assert w.tolist() == [0.25, 3.0] and inc.tolist() == [1, 1] and rej == 0


def test_host_function_refusals():
    q = _quality(Q6)
    P = StarQualityParameters
    for p, kw in ((P(fwhm_power=5), {}), (P(ecc_power=-1), {}), (P(snr_power=5), {}), (P(min_measured=0), {}), (P(fwhm_max=float("nan")), {}),
                  (P(fwhm_max=-1.0), {}), (P(ecc_max=float("inf")), {}), (P(min_measured=100), {}),              # no passing frame
                  (P(), dict(reference=5)), (P(), dict(reference=3, include=[1, 1, 1, 0, 1, 1])), (P(), dict(reference=6)), (P(), dict(reference=-2)),
                  (P(), dict(weights=[1, 1, 1, 1, 1, -1])), (P(), dict(weights=[1, 1, float("nan"), 1, 1, 1])), (P(), dict(include=[0] * 6))):
        assert sm.quality_weights(q, p, kw.get("reference", -1), kw.get("include"), kw.get("weights")) is None
        with pytest.raises(InvalidParams):
            ls.star_quality_weights(q, p, **kw)
    for f in ("fwhm", "ecc", "snr"):
        for v in (float("nan"), float("inf"), -1.0):
            b = q.copy()
            b[1][f] = v
            assert sm.quality_weights(b) is None
            with pytest.raises(InvalidParams):
                ls.star_quality_weights(b)
    with pytest.raises(InvalidParams):
        ls.star_quality_weights(q, include=[1, 1])

    class Reserved(StarQualityParameters):
        def _c(self):
            c = super()._c()
            c.reserved = 1
            return c
    with pytest.raises(InvalidParams):
        ls.star_quality_weights(q, Reserved())
    lib = _ffi.load()
    shape1, n1, q1 = np.zeros(1, SHAPE_DTYPE), np.zeros(1, np.int32), np.zeros(1, QUALITY_DTYPE)
    sp, qp = shape1.ctypes.data_as(C.POINTER(_ffi.StarShape)), q1.ctypes.data_as(C.POINTER(_ffi.StarQuality))
    assert lib.stk_star_shape_derive(None, 1) == 2 and lib.stk_star_shape_derive(sp, -1) == 2 and lib.stk_star_shape_derive(None, 0) == 0
    assert lib.stk_star_frame_quality(sp, C.c_void_p(n1.ctypes.data), 1, 1, qp) == 0
    for args in ((None, C.c_void_p(n1.ctypes.data), 1, 1, qp), (sp, None, 1, 1, qp), (sp, C.c_void_p(n1.ctypes.data), 0, 1, qp),
                 (sp, C.c_void_p(n1.ctypes.data), 1, 0, qp), (sp, C.c_void_p(n1.ctypes.data), 1, 1, None)):
        assert lib.stk_star_frame_quality(*args) == 2
    n1[0] = 2                                                               # more stars than max_stars
    assert lib.stk_star_frame_quality(sp, C.c_void_p(n1.ctypes.data), 1, 1, qp) == 2
    sc = np.zeros(4)
    assert lib.stk_star_quality_scores(qp, 1, C.c_void_p(sc.ctypes.data)) == 0
    assert lib.stk_star_quality_scores(None, 1, C.c_void_p(sc.ctypes.data)) == 2 and lib.stk_star_quality_scores(qp, 1, None) == 2
    assert lib.stk_star_quality_scores(qp, 0, C.c_void_p(sc.ctypes.data)) == 2
    with pytest.raises(InvalidParams):
        ls.star_frame_quality([])


# ---- 4. accuracy of the definition, and ranking ---------------------------------------------------------------------
def _frame_quality(f, mp=None):
    stars, _ = sd.detect(f, StarParameters())
    return sm.frame_quality([sm.measure(f, stars, mp)])[0]


@pytest.fixture(scope="module")
def planted():
    """frames of 480 x 360, sky 2000, noise sigma 40, 120 stars with peaks 400 .. 20 000 ADU; circular sigma by frame"""
    sig = (1.2, 2.5, 1.6, 2.0)
    return sig, [_frame_quality(sm.make_field(W, H, 120, s, seed=3)[0]) for s in sig]


def test_fwhm_of_circular_gaussians_is_within_the_band(planted):
    sig, qs = planted
    ratios = [float(q["fwhm"]) / (2.3548 * s) for s, q in zip(sig, qs)]
    print("sigma", sig, "measured stars", [int(q["n_measured"]) for q in qs], "fwhm / true", np.round(ratios, 3), "ecc", [round(float(q["ecc"]), 3) for q in qs])
    assert all(q["n_measured"] >= 90 for q in qs)
    assert all(0.88 <= r <= 1.02 for r in ratios), ratios


def test_eccentricity_of_an_elliptical_psf():
    q = _frame_quality(sm.make_field(W, H, 120, (2.4, 1.6, 0.6), seed=3)[0])
    print("sigma (2.4, 1.6) at 0.6 rad: median ecc %.3f (true %.3f), fwhm %.3f" % (q["ecc"], sm.true_ecc(2.4, 1.6), q["fwhm"]))
    assert abs(sm.true_ecc(2.4, 1.6) - 0.745) < 1e-3 and abs(float(q["ecc"]) - 0.745) <= 0.05


def test_rank_frames_orders_by_planted_fwhm(planted):
    sig, qs = planted
    scores = ls.star_quality_scores(np.array(qs, QUALITY_DTYPE))
    order, kept, w = ls.rank_frames(scores, SelectParameters(metric=ls.STAR_SCORE_FWHM, drop_worst=1, weight_mode=1))
    assert order.tolist() == [0, 2, 3, 1] and kept == 3                     # sharpest first: sigma 1.2, 1.6, 2.0, 2.5
    assert w[0] == 1.0 and w[1] == np.float32(scores[2, 0] / scores[0, 0])
    order, kept, _ = ls.rank_frames(scores, SelectParameters(metric=ls.STAR_SCORE_COUNT))
    assert sorted(order.tolist()) == [0, 1, 2, 3] and kept == 4


def quality_stack(n_sharp=2, n_soft=6, w=240, h=180):
    """8 unmoved u16 frames of one field with fresh noise: two at sigma 1.3 and six at sigma 2.6"""
    sig = [1.3] * n_sharp + [2.6] * n_soft
    return sig, [sm.make_field(w, h, 40, s, seed=21, noise_seed=100 + i)[0] for i, s in enumerate(sig)]


def test_quality_weights_sharpen_the_restated_mean():
    """the weighted mean (fwhm_power 2) of the stack against the equal mean: the median FWHM of the stars measured on the
    result. Measured here: 5.22 px against 5.60 px, ratio 0.93 (the bar is 0.95)."""
    sig, frames = quality_stack()
    lists = [sm.measure(f, sd.detect(f, StarParameters())[0]) for f in frames]
    q = sm.frame_quality(lists)
    assert q["fwhm"][:2].max() < q["fwhm"][2:].min()
    wq, inc, rej = sm.quality_weights(q, StarQualityParameters(fwhm_power=2), reference=0)
    assert inc.all() and rej == 0 and wq[:2].min() > 2.5 * wq[2:].max()
    stack = np.stack(frames).astype(np.float64)
    res = []
    for wts in (wq.astype(np.float64), np.ones(len(frames))):
        mean = np.rint((stack * wts[:, None, None]).sum(0) / wts.sum()).astype(np.uint16)
        res.append(float(_frame_quality(mean)["fwhm"]))
    print("median FWHM on the weighted mean %.3f px, on the equal mean %.3f px, ratio %.3f" % (res[0], res[1], res[0] / res[1]))
    assert res[0] < 0.95 * res[1]


# ---- 5. what the wrappers hand to the C ABI -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32])
def test_what_the_wrappers_hand_to_the_c_abi(dt):
    rng = np.random.default_rng(8)
    n, h, w, cn = 3, 6, 7, 3
    frames = rng.integers(0, 200, (n, h, w, cn)).astype(dt)
    depth = 8 * np.dtype(dt).itemsize
    dp, mp = StarDeepParameters(f32_scale=16.0), StarMeasureParameters(radius=3, ring_inner=5, ring_outer=6, kappa=2.5, saturation=60000)
    stars = [np.zeros(k, ls.STAR_DTYPE) for k in (2, 0, 5)]
    for i, s in enumerate(stars):
        s["px"], s["py"] = np.arange(len(s)) + i, np.arange(len(s)) + 2 * i
    seen = {}
    st = new_stacker()
    real = st._lib.stk_star_measure

    def spy(*a):
        f = C.cast(a[1], C.POINTER(_ffi.Frames)).contents if not hasattr(a[1], "_obj") else a[1]._obj
        seen["frames"] = (f.n, f.width, f.height, f.channels, f.depth, f.location, f.row_stride_bytes)
        seen["data"] = [bytes(C.string_at(f.data[k], w * h * cn * (depth // 8))) for k in range(f.n)]
        seen["stars"] = bytes(C.string_at(a[4].value if hasattr(a[4], "value") else a[4], n * 5 * ls.STAR_DTYPE.itemsize))
        seen["counts"] = bytes(C.string_at(a[5].value if hasattr(a[5], "value") else a[5], 4 * n))
        return real(*a)
    st._lib.stk_star_measure = spy
    shapes = st.star_measure(frames, stars, mp, dp)
    name, snap = st._lib.last()
    assert name == "stk_star_measure" and snap[0] == CTX and snap[2] == _bytes_of(dp._c()) and snap[3] == _bytes_of(mp._c()) and snap[6] == 5
    assert seen["frames"] == (n, w, h, cn, depth, 0, 0) and seen["data"] == [frames[i].tobytes() for i in range(n)]
    tab = np.zeros((n, 5), ls.STAR_DTYPE)
    for i, s in enumerate(stars):
        tab[i, :len(s)] = s
    assert seen["stars"] == tab.tobytes() and seen["counts"] == np.array([2, 0, 5], np.int32).tobytes() and snap[7] is not None
    assert [len(s) for s in shapes] == [2, 0, 5] and all(s.dtype == SHAPE_DTYPE for s in shapes)
    st.star_measure(frames, stars)
    assert st._lib.last()[1][2:4] == [_bytes_of(StarDeepParameters()._c()), _bytes_of(StarMeasureParameters()._c())]
    with pytest.raises(InvalidParams):
        st.star_measure(frames, stars[:2])
    with pytest.raises(ls.NotEnoughFiles):
        new_stacker().star_measure([], [])

    sp, qp = StarParameters(radius=3, max_stars=7, min_contrast=900, border_value=(1.0, 2.0)), StarQualityParameters(fwhm_max=4.5, ecc_power=1)
    u = np.array([1.0, 0.5, 2.0], np.float32)
    for alpha, want in ((None, {8: 1.0 / 255.0, 16: 1.0 / 65535.0, 32: 1.0 / 16.0}[depth]), (0.125, 0.125)):
        for flags in itertools.product((False, True), repeat=4):
            st = new_stacker()
            st._lib.pokes = {11: 2, 12: 1}
            res = st.star_match_quality_weighted(frames, sp, dp, mp, qp, alpha=alpha, coverage=flags[0], weights=u, return_coverage=flags[0],
                                                 return_applied=flags[1], return_quality=flags[2], return_stats=flags[3])
            name, snap = st._lib.last()
            assert name == "stk_star_match_quality_weighted" and snap[0] == CTX
            assert snap[2:6] == [_bytes_of(sp._c()), _bytes_of(dp._c()), _bytes_of(mp._c()), _bytes_of(qp._c())]
            assert type(snap[6]) is float and snap[6] == want and snap[7] == int(flags[0]) and snap[8] is not None
            assert isinstance(res, tuple) and len(res) == 3 + sum(flags) and res[:2] == (2, 1)
            out = res[2]
            assert out.shape == (h, w, cn) and out.dtype == np.float32 and snap[9]["data"] == out.ctypes.data
            assert (snap[10] is not None) == flags[0] and all(snap[k] is not None for k in (11, 12, 13, 14, 15))
            rest = list(res[3:])
            if flags[0]:
                assert rest.pop(0).shape == (h, w)
            if flags[1]:
                assert len(rest.pop(0)) == n
            if flags[2]:
                assert rest.pop(0).dtype == QUALITY_DTYPE
            if flags[3]:
                assert len(rest.pop(0)) == n
            assert rest == []
    st = new_stacker()
    st.star_match_quality_weighted(frames)
    snap = st._lib.last()[1]
    assert snap[2:6] == [_bytes_of(StarParameters()._c()), _bytes_of(StarDeepParameters()._c()), _bytes_of(StarMeasureParameters()._c()),
                         _bytes_of(StarQualityParameters()._c())] and snap[7] == 1 and snap[8] is None
    with pytest.raises(InvalidParams):
        new_stacker().star_match_quality_weighted(frames, weights=[1.0, 2.0])
    with pytest.raises(ls.NotEnoughFiles):
        new_stacker().star_match_quality_weighted([])


# ---- 6. the sanitizer harness ---------------------------------------------------------------------------------------
def test_host_functions_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "star_quality_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "star_quality_harness.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=500)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

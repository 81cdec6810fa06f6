"""CPU tests of deconvolution (include/stacker.h, "deconvolution"): the struct layout, the symbols, _ffi.SIGNATURES and the Rust
table against the header; stk_psf_model and stk_psf_from_shapes against the restatement (tests/deconvolve_restate.py) bit for
bit and by hand; every refusal that needs no GPU; what the wrappers hand to the C ABI; identities of the restatement; the
quality of the definition on the restatement, before any GPU run; the kernel map's rows; the sanitizer harness.

Quality: the scene of deconvolve_restate.scene (96 x 72, 12 stars of sigma 0.8 on a slowly varying sky, blurred
by an elliptical Gaussian of sigma 2.0 x 1.4 rotated 0.5 rad, R = 6, shot noise), deconvolved with the PSF that blurred it,
floor 1e-6, seeds 0, 1, 2. Measured on this restatement:
                                                     seed 0    seed 1    seed 2    worst    bar = 1.5 x worst
  RMS error / the input's, 10 iterations, lambda 0    0.6475    0.6347    0.6428    0.6475   0.9713
  RMS error / the input's, 30 iterations, lambda 0    0.4633    0.4449    0.4570    0.4633   0.6950
  the same, 10 iterations, lambda 0.002, tv_eps 1     0.6601    0.6466    0.6552    0.6601   0.9902
  median FWHM after 30 / before                       0.6052    0.6150    0.6092    0.6150   0.9225
    (before 4.316 4.262 4.315 px, after 10: 2.965 3.003 3.004, after 30: 2.612 2.621 2.629)
  |total flux after 30 / before - 1|                  2.0e-5    4.1e-5    1.6e-5    4.1e-5   6.2e-5"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deconvolve_restate as dr
import libstacker_rs_amd as ls
import star_measure_restate as sm
from libstacker_rs_amd import (PSF_GAUSSIAN, PSF_MOFFAT, SHAPE_DTYPE, DeconvolveParameters, InvalidParams, StarMeasureParameters, _ffi, psf_from_shapes,
                               psf_model)
from test_cpu_api_calls import CTX, new_stacker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_deconvolve", "stk_psf_model", "stk_psf_from_shapes")
SEEDS = (0, 1, 2)
BAR_RMS10, BAR_RMS30, BAR_RMS_TV10 = 1.5 * 0.6475, 1.5 * 0.4633, 1.5 * 0.6601
BAR_FWHM30, BAR_FLUX30 = 1.5 * 0.6150, 1.5 * 4.1e-5
TV = dict(lam=0.002, tv_eps=1.0)


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


def median_fwhm(image, stars):
    """the lower median of the FWHM of the measured stars at the known positions (the restated stk_star_measure)"""
    sh = sm.measure(image, stars, StarMeasureParameters())
    good = sh[sh["flags"] == 0]
    assert len(good) >= 10
    return float(sm.lower_median(good["fwhm"]))


# ---- layouts, symbols, the Rust table -------------------------------------------------------------------------------
def test_struct_layout_symbols_and_table_against_the_header(tmp_path):
    cls = _ffi.DeconvParams
    lines = ['  printf("%zu", sizeof(stk_deconv_params));\n'] + ['  printf(" %%zu", offsetof(stk_deconv_params, %s));\n' % f for f, _ in cls._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n' + "".join(lines) + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_] and got[0] == 32
    assert [f for f, _ in cls._fields_] == ["iterations", "radius", "floor", "pedestal", "lambda", "tv_eps", "amount", "reserved"]
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
    assert "pub struct stk_deconv_params" in rs and "pub const STK_PSF_MOFFAT: c_int = 1;" in rs
    assert re.search(r"STK_PSF_GAUSSIAN\s*=\s*0,\s*STK_PSF_MOFFAT\s*=\s*1", hdr) and (PSF_GAUSSIAN, PSF_MOFFAT) == (0, 1)
    for name in ("DeconvolveParameters", "psf_model", "psf_from_shapes", "PSF_GAUSSIAN", "PSF_MOFFAT"):
        assert name in ls.__all__ and hasattr(ls, name)
    for method in ("deconvolve_image", "psf_from_image"):
        assert callable(getattr(ls.Stacker, method))
    c = DeconvolveParameters()._c()
    assert (c.iterations, c.radius, c.floor, c.pedestal, getattr(c, "lambda"), c.tv_eps, c.amount, c.reserved) == (
        30, 8, np.float32(1e-6), 0.0, 0.0, np.float32(1e-3), 1.0, 0)


# ---- 1. the PSF functions -------------------------------------------------------------------------------------------
COVS = [(2.0, 2.0, 0.0), (4.0, 1.96, 0.8), dr.SCENE_COV, (0.3, 7.5, -1.2), (1e-3, 1e-3, 0.0), (1.0, 1.0, 1.0 - 1e-12), (30.0, 50.0, 10.0)]


@pytest.mark.parametrize("kind,beta", [(PSF_GAUSSIAN, 2.5), (PSF_MOFFAT, 2.5), (PSF_MOFFAT, 1.0 + 1e-9), (PSF_MOFFAT, 4.765), (PSF_MOFFAT, 100.0)])
def test_psf_model_equals_the_restatement(kind, beta):
    for radius in (1, 2, 3, 8, 16):
        for cov in COVS:
            got, want = psf_model(radius, *cov, kind=kind, beta=beta), dr.psf_model(kind, beta, radius, *cov)
            assert got.shape == (2 * radius + 1,) * 2 and got.dtype == np.float32 and got.tobytes() == want.tobytes(), (radius, cov)
            assert got.tobytes() == got[::-1, ::-1].tobytes()                  # point symmetry
            assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-6


def test_psf_model_by_hand():
    """3 x 3, S = 2 I: q = (i^2 + j^2) / 2, taps 1, e^-1/4 (edges), e^-1/2 (corners) over their sum."""
    import math
    e, c = math.exp(-0.25), math.exp(-0.5)
    total = 1.0 + 4.0 * e + 4.0 * c
    want = np.array([[c, e, c], [e, 1.0, e], [c, e, c]]) / total
    got = psf_model(1, 2.0, 2.0).astype(np.float64)
    assert np.abs(got - want).max() < 1e-7 and got[1, 1] == np.float32(1.0 / total)
    # the f64 values sum to 1 to rounding: the f32 taps sum to 1 within (2R+1)^2 roundings of the largest tap
    for radius, cov in ((8, (4.0, 4.0, 0.0)), (16, dr.SCENE_COV)):
        p = psf_model(radius, *cov).astype(np.float64)
        assert abs(p.sum() - 1.0) <= p.size * 2.0 ** -24 * p.max()
    # the second moments of the model return the covariance within the sampling and truncation error at R >= 4 sigma
    for radius, cov in ((8, (4.0, 1.96, 0.8)), (8, dr.SCENE_COV), (16, (9.0, 16.0, -5.0)), (6, (2.0, 2.0, 0.0))):
        for kind in (PSF_GAUSSIAN,):
            p = psf_model(radius, *cov, kind=kind).astype(np.float64)
            j, i = np.mgrid[-radius:radius + 1, -radius:radius + 1]
            assert abs((p * i).sum()) < 1e-7 and abs((p * j).sum()) < 1e-7
            got = ((p * i * i).sum(), (p * j * j).sum(), (p * i * j).sum())
            assert np.allclose(got, cov, rtol=5e-3, atol=5e-3), (got, cov)
    # Moffat and Gaussian share the half-maximum contour: q = 2 ln 2 there. S = s^2 I, the point (h, 0), h = s sqrt(2 ln 2)
    s2 = 18.0 / (2.0 * math.log(2.0))                                          # h^2 = 18: no pixel centre; use the ratio of taps
    for beta in (1.5, 2.5, 4.765):
        g, m = psf_model(8, s2, s2).astype(np.float64), psf_model(8, s2, s2, kind=PSF_MOFFAT, beta=beta).astype(np.float64)
        # (3, 3) has i^2 + j^2 = 18 = h^2: half the maximum in both
        assert abs(g[8 + 3, 8 + 3] / g[8, 8] - 0.5) < 1e-6 and abs(m[8 + 3, 8 + 3] / m[8, 8] - 0.5) < 1e-6
        assert m[8, 16] / m[8, 8] > g[8, 16] / g[8, 8]                          # and Moffat's wings are the heavier


def _shapes(rng, n, flagged=0.2):
    s = np.zeros(n, SHAPE_DTYPE)
    s["cxx"], s["cyy"], s["cxy"] = rng.uniform(2, 5, n), rng.uniform(2, 5, n), rng.uniform(-1, 1, n)
    s["snr"] = rng.uniform(1, 100, n)
    s["flags"] = np.where(rng.random(n) < flagged, rng.integers(1, 16, n), 0)
    return s


def test_psf_from_shapes_equals_the_restatement_and_refuses():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 10, 11, 200):
        for min_snr, scale in ((0.0, 1.0), (30.0, 1.0), (0.0, 1.0 / 0.95), (60.0, 1.1)):
            s = _shapes(rng, n)
            want = dr.psf_from_shapes(s, min_snr, scale)
            if want is None:
                with pytest.raises(InvalidParams):
                    psf_from_shapes(s, min_snr, scale)
            else:
                got = psf_from_shapes(s, min_snr, scale, return_used=True)
                assert np.array(got[:3]).tobytes() == np.array(want[:3]).tobytes() and got[3] == want[3]
                assert psf_from_shapes(s, min_snr, scale) == got[:3]
    # by hand: lower medians, each on its own
    s = np.zeros(4, SHAPE_DTYPE)
    s["cxx"], s["cyy"], s["cxy"], s["snr"] = [4, 1, 3, 2], [5, 8, 6, 7], [0.4, 0.1, 0.3, 0.2], [10, 20, 30, 40]
    assert psf_from_shapes(s) == (2.0, 6.0, 0.2) and psf_from_shapes(s, scale=2.0) == (8.0, 24.0, 0.8)
    assert psf_from_shapes(s, min_snr=20.0, return_used=True) == (2.0, 7.0, 0.2, 3)
    s["flags"][1] = 4
    assert psf_from_shapes(s, return_used=True) == (3.0, 6.0, 0.3, 3)
    for bad in (dict(min_snr=41.0), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(min_snr=float("nan"))):
        with pytest.raises(InvalidParams):
            psf_from_shapes(s, **bad)
    s["flags"] = 1
    with pytest.raises(InvalidParams):
        psf_from_shapes(s)                                                      # every shape flagged
    with pytest.raises(InvalidParams):
        psf_from_shapes(np.zeros(0, SHAPE_DTYPE))                               # no shape
    s["flags"] = 0
    s["cxy"] = 10.0
    with pytest.raises(InvalidParams):
        psf_from_shapes(s)                                                      # not positive definite


def test_refusals_without_a_gpu():
    for bad in (dict(radius=0), dict(radius=17), dict(cxx=0.0), dict(cyy=-1.0), dict(cxy=2.0), dict(cxy=-2.0), dict(cxx=float("nan")),
                dict(cyy=float("inf")), dict(kind=2), dict(kind=-1), dict(kind=PSF_MOFFAT, beta=1.0), dict(kind=PSF_MOFFAT, beta=0.5),
                dict(kind=PSF_MOFFAT, beta=float("nan")), dict(kind=PSF_MOFFAT, beta=float("inf"))):
        with pytest.raises(InvalidParams):
            psf_model(**dict(dict(radius=2, cxx=2.0, cyy=2.0, cxy=0.0), **bad))
    assert psf_model(2, 2.0, 2.0, kind=PSF_GAUSSIAN, beta=float("nan")).shape == (5, 5)      # beta is Moffat's
    lib = _ffi.load()
    assert lib.stk_psf_model(0, 2.5, 1, 2.0, 2.0, 0.0, None) == 2
    d = C.c_double(0)
    assert lib.stk_psf_from_shapes(None, 1, 0.0, 1.0, C.byref(d), C.byref(d), C.byref(d), None) == 2
    assert lib.stk_psf_from_shapes(None, -1, 0.0, 1.0, C.byref(d), C.byref(d), C.byref(d), None) == 2
    one = np.zeros(1, SHAPE_DTYPE)
    one["cxx"], one["cyy"] = 2.0, 2.0
    sp = one.ctypes.data_as(C.POINTER(_ffi.StarShape))
    assert lib.stk_psf_from_shapes(sp, 1, 0.0, 1.0, C.byref(d), C.byref(d), C.byref(d), None) == 0 and d.value == 0.0
    assert lib.stk_psf_from_shapes(sp, 1, 0.0, 1.0, None, C.byref(d), C.byref(d), None) == 2
    # stk_deconvolve without a context
    img = _ffi.ImageF32()
    p = DeconvolveParameters()._c()
    assert lib.stk_deconvolve(None, C.byref(img), None, C.byref(p), None, 0, 0, C.byref(img)) == 2


# ---- 2. what the wrappers hand to the C ABI -------------------------------------------------------------------------
def test_what_the_wrappers_hand_to_the_c_abi():
    rng = np.random.default_rng(3)
    h, w = 20, 30
    psf = psf_model(2, 1.5, 1.2, 0.3)
    for cn in (1, 3, 4):
        image = rng.random((h, w, cn)).astype(np.float32)
        st = new_stacker()
        st._lib.reads = {2: 25 * 4}
        out = st.deconvolve_image(image, psf)
        name, snap = st._lib.last()
        assert name == "stk_deconvolve" and snap[0] == CTX and snap[2][1] == psf.tobytes()
        assert snap[1] == dict(data=image.ctypes.data, width=w, height=h, channels=cn, location=0, row_stride_bytes=0)
        assert snap[3] == _bytes_of(DeconvolveParameters(radius=2)._c()) and snap[4] is None and snap[5] == 0 and snap[6] == 0
        assert out.shape == (h, w, cn) and out.dtype == np.float32
        assert snap[7] == dict(data=out.ctypes.data, width=w, height=h, channels=cn, location=0, row_stride_bytes=0)
    # parameters, a mask with padded rows, a padded image, the caller's output, in place
    p = DeconvolveParameters(iterations=7, radius=2, floor=1e-4, pedestal=3.0, lambda_=0.01, tv_eps=0.5, amount=0.75)
    wide = rng.random((h, w + 5, 3)).astype(np.float32)
    image = wide[:, :w]
    mwide = rng.random((h, w + 3)).astype(np.float32)
    mine = np.zeros((h, w + 2, 3), np.float32)[:, :w]
    st = new_stacker()
    st._lib.reads = {2: 25 * 4}
    assert st.deconvolve_image(image, psf, p, mask=mwide[:, :w], out=mine) is mine
    snap = st._lib.last()[1]
    c = _ffi.DeconvParams.from_buffer_copy(snap[3])
    assert (c.iterations, c.radius, c.floor, c.pedestal, getattr(c, "lambda"), c.tv_eps, c.amount, c.reserved) == (
        7, 2, np.float32(1e-4), 3.0, np.float32(0.01), 0.5, 0.75, 0)
    assert snap[1]["data"] == wide.ctypes.data and snap[1]["row_stride_bytes"] == (w + 5) * 12
    assert snap[4] == mwide.ctypes.data and snap[5] == (w + 3) * 4 and snap[6] == 0
    assert snap[7] == dict(data=mine.ctypes.data, width=w, height=h, channels=3, location=0, row_stride_bytes=(w + 2) * 12)
    assert st.deconvolve_image(image, psf, p, out=image) is image
    snap = st._lib.last()[1]
    assert snap[7] == snap[1]
    grey = rng.random((h, w)).astype(np.float32)
    assert st.deconvolve_image(grey, psf).shape == (h, w, 1) and st._lib.last()[1][1]["channels"] == 1
    # the wrapper's own refusals
    for bad in (lambda: st.deconvolve_image(image, psf[:4]), lambda: st.deconvolve_image(image, psf, DeconvolveParameters(radius=3)),
                lambda: st.deconvolve_image(image.astype(np.float64), psf), lambda: st.deconvolve_image(image, psf, mask=mwide),
                lambda: st.deconvolve_image(image, psf, mask=rng.random((h, w, 3)).astype(np.float32)),
                lambda: st.deconvolve_image(image, psf, out=np.zeros((h, w, 3), np.float64)),
                lambda: st.deconvolve_image(image, psf, out=np.zeros((h, 2 * w, 3), np.float32)[:, ::2]),
                lambda: st.psf_from_image(image.astype(np.float64), 4)):
        with pytest.raises(InvalidParams):
            bad()


# ---- 3. identities of the restatement -------------------------------------------------------------------------------
def _messy(rng, h, w, cn):
    d = (rng.random((h, w, cn)) * 100 - 10).astype(np.float32)
    d[1, 2, 0], d[3, 4, 0], d[5, 6, 0], d[7, 1, 0], d[2, 7, 0] = np.nan, np.inf, -np.inf, 0.0, -0.0
    return d


def test_identities_of_the_restatement():
    rng = np.random.default_rng(5)
    h, w = 14, 17
    d = _messy(rng, h, w, 4)
    delta = np.zeros((5, 5), np.float32)
    delta[2, 2] = 1.0
    for pedestal in (0.0, 12.5):
        with np.errstate(invalid="ignore"):
            D = (d[..., :3] + np.float32(pedestal)).astype(np.float32)
        want = d.copy()
        want[..., :3] = np.where(np.isfinite(D) & (D >= 0), D, np.float32(0)) - np.float32(pedestal)
        for it in (1, 2, 5):
            got = dr.deconvolve(d, delta, iterations=it, pedestal=pedestal)       # a delta PSF: A = u, r = 1 or 0, v = u
            assert got.tobytes() == want.tobytes(), (pedestal, it)
        psf = dr.psf_model(dr.GAUSSIAN, 0, 2, 1.5, 1.2, 0.3)
        assert dr.deconvolve(d, psf, iterations=3, pedestal=pedestal, amount=0.0).tobytes() == want.tobytes()
        assert dr.deconvolve(d, psf, iterations=3, pedestal=pedestal, amount=0.0, **TV).tobytes() == want.tobytes()
        # lambda = 0 skips the regulariser; the same bits come out of its arithmetic at lambda = 0 (v / fmaxf(fmaf(-0, div, 1), 0.5))
        clean = np.abs(rng.random((h, w, 3)) * 100).astype(np.float32)
        a = dr.deconvolve(clean, psf, iterations=3, pedestal=pedestal)
        assert a.tobytes() == dr.deconvolve(clean, psf, iterations=3, pedestal=pedestal, lam=0.0, force_tv=True).tobytes()
        assert a.tobytes() != dr.deconvolve(clean, psf, iterations=3, pedestal=pedestal, **TV).tobytes()
        assert a.tobytes() != clean.tobytes()
    # alpha passes through, the channels do not mix, a 2-D image is its own one channel
    a = dr.deconvolve(d, psf, iterations=2)
    assert a[..., 3].tobytes() == d[..., 3].tobytes()
    for c in range(3):
        assert dr.deconvolve(d[..., c], psf, iterations=2).tobytes() == a[..., c].tobytes()
    # keep: the outputs at earlier counts are those of shorter runs
    full, kept = dr.deconvolve(d, psf, iterations=4, keep=(2,))
    assert kept[2].tobytes() == a.tobytes() and full.tobytes() == dr.deconvolve(d, psf, iterations=4).tobytes()
    # an asymmetric PSF: convolution and correlation differ, and a point spreads along the taps, not against them
    P = np.zeros((3, 3), np.float32)
    P[0, 2], P[1, 1] = 0.25, 0.75                                               # j = -1, i = +1
    u = np.zeros((7, 7), np.float32)
    u[3, 3] = 1.0
    A = dr.tap_sum(P, u, 1, True)
    assert A[3, 3] == 0.75 and A[2, 4] == 0.25 and A.sum() == 1.0                # A(x, y) = P[j][i] u(x - i, y - j): (4, 2) - (1, -1)
    Cc = dr.tap_sum(P, u, 1, False)
    assert Cc[3, 3] == 0.75 and Cc[4, 2] == 0.25 and Cc.sum() == 1.0             # C(x, y) = P[j][i] u(x + i, y + j)


# ---- 4. quality, on the restatement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quality():
    """per seed: the scene, and the outputs after 10 and 30 iterations at lambda 0 and after 10 with the regulariser. The seeds
    ride as the channels of one image: the channels are independent."""
    scenes = [dr.scene(s) for s in SEEDS]
    blurred = np.stack([s[1] for s in scenes], 2)
    o30, kept = dr.deconvolve(blurred, scenes[0][2], iterations=30, keep=(10,))
    otv = dr.deconvolve(blurred, scenes[0][2], iterations=10, **TV)
    return [dict(truth=s[0], blurred=s[1], stars=s[3], o10=kept[10][..., k], o30=o30[..., k], otv=otv[..., k]) for k, s in enumerate(scenes)]


def test_quality_of_the_definition(quality):
    for seed, q in zip(SEEDS, quality):
        r10, r30, rtv = (dr.rms_ratio(q[k], q["blurred"], q["truth"]) for k in ("o10", "o30", "otv"))
        f0, f10, f30 = (median_fwhm(q[k], q["stars"]) for k in ("blurred", "o10", "o30"))
        flux = abs(dr.flux_ratio(q["o30"], q["blurred"]) - 1.0)
        print("seed %d: rms 10 %.4f, 30 %.4f, tv 10 %.4f; fwhm %.3f -> %.3f -> %.3f (%.4f); flux %.1e" % (seed, r10, r30, rtv, f0, f10, f30, f30 / f0, flux))
        assert r30 < r10 < 1.0 and rtv < 1.0                                    # structural, on every seed
        assert f30 < f10 < f0
        assert r10 <= BAR_RMS10 and r30 <= BAR_RMS30 and rtv <= BAR_RMS_TV10    # 1.5 x the worst seed of the header's table
        assert f30 / f0 <= BAR_FWHM30 and flux <= BAR_FLUX30
    assert BAR_RMS30 < BAR_RMS10 < 1.0 and BAR_FWHM30 < 1.0


# ---- 5. the kernel map of the new unit -------------------------------------------------------------------------------
def test_the_new_unit_has_its_own_kernel_map_and_every_kernel_a_gpu_test(tmp_path):
    """tests/kernel_own_deconvolve.tsv (tools/kernel_coverage.py, OWN): the existing tests pin kc.read_map() to the committed map
    files, so the rows of kernels_deconvolve.hip live in a map that read_map does not return, and this test holds it to what
    tests/test_cpu_kernel_map.py asks of the others: the kernels of the unit, recomputed with the Makefile's own command, are
    the rows of the file; every row names a GPU test file that exists, qualifies and is marked gpu; no kernel is listed twice
    anywhere; write_map returns every row to its file byte for byte. Only kernel symbol names are read."""
    import shutil
    from test_cpu_kernel_map import kc
    assert kc.OWN == {"kernels_deconvolve": "deconvolve"}                       # (a unit joins this table only with a test like this one)
    own = kc.own_file("kernels_deconvolve")
    assert os.path.basename(own) == "kernel_own_deconvolve.tsv" and own not in kc.parts() + kc.supplements()
    rows = kc.read_rows(own)
    assert rows == kc.read_own() and len(rows) == 9 and all(r[0] == "kernels_deconvolve" for r in rows)
    for unit, mangled, demangled, files in rows:
        assert mangled.startswith("_ZN3stk") and "stk::" in demangled and files == ["test_gpu_deconvolve.py"]
        text = open(os.path.join(ROOT, "tests", files[0])).read()
        assert kc.qualifies(files[0]) and re.search(r"pytest\.mark\.gpu\b", text)
    names = sorted(re.search(r"(deconv_\w+(<[^>]*>)?)\(", r[2]).group(1) for r in rows)
    assert names == ["deconv_init_kernel<1>", "deconv_init_kernel<3>", "deconv_init_kernel<4>", "deconv_ratio_kernel<16>", "deconv_ratio_kernel<8>",
                     "deconv_update_kernel<false, 16>", "deconv_update_kernel<false, 8>", "deconv_update_kernel<true, 16>", "deconv_update_kernel<true, 8>"]
    listed = [r[1] for r in kc.read_map()] + [r[1] for r in rows]
    assert len(set(listed)) == len(listed) and not any(r[0] in kc.OWN for r in kc.read_map())
    assert not kc.uncovered(rows)
    # every .hip unit is in exactly one of the two kernel sets, and the tree's kernels of this unit are the file's rows
    units = {os.path.splitext(f)[0] for f in os.listdir(kc.CSRC) if f.endswith(".hip")}
    assert set(kc.OWN) <= units and {r[0] for r in kc.read_map()} == units - set(kc.OWN)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is not None:                                         # (as tests/test_cpu_kernel_map.py: no compiler, no recomputation)
        built = kc.build_kernels(workdir=str(tmp_path), own=True)
        assert set(built) == set(kc.OWN) and {(u, n) for u, names in built.items() for n in names} == {(r[0], r[1]) for r in rows}
    # write_map on copies: the committed maps and this one return byte for byte
    files = [kc.MAP] + kc.parts() + kc.supplements() + [own]
    copies = [str(tmp_path / os.path.basename(f)) for f in files]
    for src, dst in zip(files, copies):
        open(dst, "w").write(open(src).read())
    kernels, seen = {}, {}
    for unit, mangled, _, tests in kc.read_map(copies[0]) + kc.read_own(copies[0]):
        kernels.setdefault(unit, []).append(mangled)
        seen[mangled] = set(tests)
    kc.write_map({u: sorted(v) for u, v in kernels.items()}, seen, copies[0])
    assert all(open(src).read() == open(dst).read() for src, dst in zip(files, copies))


# ---- 6. the sanitizer harness ---------------------------------------------------------------------------------------
def test_psf_host_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "psf_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "psf_harness.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=500)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

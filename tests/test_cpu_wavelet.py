"""CPU tests of the wavelet layers (include/stacker.h, "wavelet layers"): the struct layout, the symbols, _ffi.SIGNATURES, the
Rust table and __all__ against the header; stk_wavelet_noise_table against the independent restatement
(tests/wavelet_restate.py) and the header's values; every refusal that needs no GPU; what the wrappers hand to the C ABI;
identities of the restatement; the quality of the definition on the restatement, before any GPU run; the kernel map's rows;
the sanitizer harness.

Quality, measured on this f32 restatement, seeds 0, 1, 2.
Denoise: the scene of wavelet_restate.scene (128 x 96, a sinusoidal sky, 15 Gaussian stars of sigma 1 .. 1.8 and peak
100 .. 3000, white noise of sigma 8), 4 levels, HARD, thresholds 3 on every level, sigma estimated:
                                                     seed 0    seed 1    seed 2    worst    bar = 1.5 x worst
  RMS error / the input's                             0.5010    0.5165    0.4721    0.5165   0.7748
  |estimated sigma / 8 - 1|                           0.1032    0.1255    0.0772    0.1255   0.1882
    (sigma 8.826 9.004 8.617: the stars and the sky's curvature are in the first layer too and bias the MAD upward; on pure
     noise the estimate is within 1 %, see test_sigma_of_pure_noise)
Sharpen: the scene of deconvolve_restate.scene, 4 levels, gains 2, 1.5 on layers 0, 1, the median FWHM of the restated
stk_star_measure at the known positions:
  median FWHM after / before                          0.8578    0.8643    0.8583    0.8643   1.2964
    (before 4.316 4.262 4.315 px, after 3.702 3.684 3.703; the bar is above 1, so the test also asks after < before on
     every seed)
Reconstruction with the defaults, the worst |o - d| / max|d| over the three denoise scenes: J = 1: 0; J = 4: 9.1e-8;
J = 6: 9.1e-8 (per pixel, |o - d| / |d| <= 1.6e-7); the bound asserted is (2 J + 1) 2^-23: J subtractions, J sums and one fma,
each within half an ulp of a partial sum that is at most 2 max|d| in magnitude."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import deconvolve_restate as dr
import libstacker_rs_amd as ls
import star_measure_restate as sm
import wavelet_restate as wr
from libstacker_rs_amd import WAVELET_HARD, WAVELET_SOFT, InvalidParams, StarMeasureParameters, WaveletParameters, _ffi, wavelet_noise_table
from test_cpu_api_calls import CTX, new_stacker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_wavelet_process", "stk_wavelet_layers", "stk_wavelet_sigma", "stk_wavelet_noise_table")
SEEDS = (0, 1, 2)
E_HEADER = (0.8907963103, 0.2006638510, 0.0855075048, 0.0412174444, 0.0204249666, 0.0101897592, 0.0050920467, 0.0025456695)
BAR_RMS, BAR_SIGMA, BAR_FWHM = 1.5 * 0.5165, 1.5 * 0.1255, 1.5 * 0.8643
SHARPEN = [2.0, 1.5, 1.0, 1.0]


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


# ---- layouts, symbols, the Rust table -------------------------------------------------------------------------------
def test_struct_layout_symbols_and_table_against_the_header(tmp_path):
    cls = _ffi.WaveletParams
    lines = ['  printf("%zu", sizeof(stk_wavelet_params));\n'] + ['  printf(" %%zu", offsetof(stk_wavelet_params, %s));\n' % f for f, _ in cls._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n' + "".join(lines) + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == [136, 0, 4, 8, 12, 16, 48, 80, 112, 116, 120]
    assert [f for f, _ in cls._fields_] == ["levels", "mode", "sigma_given", "reserved", "gain", "threshold", "layer_amount", "residual_gain", "amount", "sigma"]
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
    assert "pub struct stk_wavelet_params" in rs and "pub const STK_WAVELET_SOFT: c_int = 1;" in rs and "pub gain: [f32; 8]," in rs
    assert re.search(r"STK_WAVELET_HARD\s*=\s*0,\s*STK_WAVELET_SOFT\s*=\s*1", hdr) and (WAVELET_HARD, WAVELET_SOFT) == (0, 1)
    for name in ("WaveletParameters", "wavelet_noise_table", "WAVELET_HARD", "WAVELET_SOFT"):
        assert name in ls.__all__ and hasattr(ls, name)
    for method in ("wavelet_image", "wavelet_layers", "wavelet_sigma"):
        assert callable(getattr(ls.Stacker, method))
    c = WaveletParameters()._c()
    assert (c.levels, c.mode, c.sigma_given, c.reserved, c.residual_gain, c.amount) == (4, 0, 0, 0, 1.0, 1.0)
    assert list(c.gain) == [1.0] * 8 and list(c.threshold) == [0.0] * 8 and list(c.layer_amount) == [1.0] * 8 and list(c.sigma) == [0.0] * 4


# ---- 1. the noise table ---------------------------------------------------------------------------------------------
def test_noise_table_against_the_restatement_and_the_header():
    want = wr.noise_table(8)                                                    # the 2-D impulse responses, not the closed form
    for levels in range(1, 9):
        got = wavelet_noise_table(levels)
        assert got.shape == (levels,) and got.dtype == np.float64
        assert np.abs(got - want[:levels]).max() <= 1e-12
        assert np.abs(got - np.array(E_HEADER[:levels])).max() <= 1e-9
    # by hand, level 0: psi = delta - b x b, |psi|^2 = 1 - 2 b0^2 + (sum b^2)^2, b0 = 0.375, sum b^2 = 35 / 128
    assert abs(wavelet_noise_table(1)[0] - (1.0 - 2.0 * 0.375 ** 2 + (35.0 / 128.0) ** 2) ** 0.5) < 1e-15
    # and by experiment: the layers of white noise have these deviations (128 x 128 samples: 1 / sqrt(2 N) = 0.6 %; the coarse
    # layers have few independent samples, so only the first three are held, to 5 %)
    rng = np.random.default_rng(1)
    lay = wr.layers(rng.normal(0.0, 1.0, (128, 128)).astype(np.float32), 3)
    for j in range(3):
        assert abs(float(lay[j].astype(np.float64).std()) / want[j] - 1.0) < 0.05, j


def test_refusals_without_a_gpu():
    lib = _ffi.load()
    e = (C.c_double * 8)()
    for levels in (0, -1, 9, 1 << 30):
        assert lib.stk_wavelet_noise_table(levels, e) == 2
        with pytest.raises(InvalidParams):
            wavelet_noise_table(levels)
    import tracemalloc
    tracemalloc.start()                                                         # the wrapper refuses before it allocates the table
    with pytest.raises(InvalidParams):
        wavelet_noise_table(1 << 30)
    assert tracemalloc.get_traced_memory()[1] < 1 << 20
    tracemalloc.stop()
    assert lib.stk_wavelet_noise_table(4, None) == 2
    assert lib.stk_wavelet_noise_table(8, e) == 0 and abs(e[7] - E_HEADER[7]) < 1e-9
    # the entry points without a context
    img = _ffi.ImageF32()
    p = WaveletParameters()._c()
    f = (C.c_float * 4)()
    assert lib.stk_wavelet_process(None, C.byref(img), C.byref(p), None, 0, 0, C.byref(img), None) == 2
    assert lib.stk_wavelet_layers(None, C.byref(img), 4, C.byref(img)) == 2
    assert lib.stk_wavelet_sigma(None, C.byref(img), C.cast(f, C.c_void_p), None) == 2
    # the wrappers' own refusals, before any C call
    st = new_stacker()
    image = np.zeros((40, 50, 3), np.float32)
    for bad in (lambda: st.wavelet_image(image.astype(np.float64)), lambda: st.wavelet_image(image, mask=np.zeros((40, 51), np.float32)),
                lambda: st.wavelet_image(image, mask=np.zeros((40, 50, 3), np.float32)), lambda: st.wavelet_image(image, out=np.zeros((40, 50, 3), np.float64)),
                lambda: st.wavelet_image(image, out=np.zeros((40, 100, 3), np.float32)[:, ::2]),
                lambda: st.wavelet_image(image, WaveletParameters(gains=[1.0] * 9)), lambda: st.wavelet_image(image, WaveletParameters(sigma=[1.0] * 5)),
                lambda: st.wavelet_layers(image, 0), lambda: st.wavelet_layers(image, 9), lambda: st.wavelet_layers(image.astype(np.float64), 2),
                lambda: st.wavelet_sigma(image.astype(np.uint8))):
        with pytest.raises(InvalidParams):
            bad()
    assert not st._lib.calls


# ---- 2. what the wrappers hand to the C ABI -------------------------------------------------------------------------
def test_what_the_wrappers_hand_to_the_c_abi():
    rng = np.random.default_rng(3)
    h, w = 20, 30
    for cn in (1, 3, 4):
        image = rng.random((h, w, cn)).astype(np.float32)
        st = new_stacker()
        out = st.wavelet_image(image)
        name, snap = st._lib.last()
        assert name == "stk_wavelet_process" and snap[0] == CTX
        assert snap[1] == dict(data=image.ctypes.data, width=w, height=h, channels=cn, location=0, row_stride_bytes=0)
        assert snap[2] == _bytes_of(WaveletParameters()._c()) and snap[3] is None and snap[4] == 0 and snap[5] == 0 and snap[7] is None
        assert out.shape == (h, w, cn) and out.dtype == np.float32
        assert snap[6] == dict(data=out.ctypes.data, width=w, height=h, channels=cn, location=0, row_stride_bytes=0)
        res, sigma = st.wavelet_image(image, return_sigma=True)
        assert st._lib.last()[1][7] is not None and sigma.shape == (min(cn, 3),) and sigma.dtype == np.float32
        lay = st.wavelet_layers(image, 3)
        name, snap = st._lib.last()
        assert name == "stk_wavelet_layers" and snap[0] == CTX and snap[2] == 3 and len(lay) == 4
        assert snap[3] == dict(data=lay[0].ctypes.data, width=w, height=h, channels=cn, location=0, row_stride_bytes=0)
        assert all(a.shape == (h, w, cn) and a.dtype == np.float32 for a in lay) and len({a.ctypes.data for a in lay}) == 4
        sg, med = st.wavelet_sigma(image, return_median=True)
        name, snap = st._lib.last()
        assert name == "stk_wavelet_sigma" and snap[1]["data"] == image.ctypes.data and snap[2] is not None and snap[3] is not None
        assert sg.shape == med.shape == (min(cn, 3),)
        st.wavelet_sigma(image)
        assert st._lib.last()[1][3] is None
    # parameters, a mask with padded rows, a padded image, the caller's output, in place
    p = WaveletParameters(levels=3, mode=WAVELET_SOFT, gains=[2.0, 1.5, 0.5], thresholds=[3.0, 2.0], layer_amounts=0.75, residual_gain=0.9, amount=0.6,
                          sigma=[4.0, 5.0, 6.0])
    wide = rng.random((h, w + 5, 3)).astype(np.float32)
    image = wide[:, :w]
    mwide = rng.random((h, w + 3)).astype(np.float32)
    mine = np.zeros((h, w + 2, 3), np.float32)[:, :w]
    st = new_stacker()
    assert st.wavelet_image(image, p, mask=mwide[:, :w], out=mine) is mine
    snap = st._lib.last()[1]
    c = _ffi.WaveletParams.from_buffer_copy(snap[2])
    assert (c.levels, c.mode, c.sigma_given, c.reserved, c.residual_gain, c.amount) == (3, 1, 1, 0, np.float32(0.9), np.float32(0.6))
    assert list(c.gain) == [2.0, 1.5, 0.5] + [1.0] * 5 and list(c.threshold) == [3.0, 2.0] + [0.0] * 6 and list(c.layer_amount) == [0.75] * 8
    assert list(c.sigma) == [4.0, 5.0, 6.0, 0.0]
    assert snap[1]["data"] == wide.ctypes.data and snap[1]["row_stride_bytes"] == (w + 5) * 12
    assert snap[3] == mwide.ctypes.data and snap[4] == (w + 3) * 4 and snap[5] == 0
    assert snap[6] == dict(data=mine.ctypes.data, width=w, height=h, channels=3, location=0, row_stride_bytes=(w + 2) * 12)
    assert st.wavelet_image(image, p, out=image) is image
    snap = st._lib.last()[1]
    assert snap[6] == snap[1]
    grey = rng.random((h, w)).astype(np.float32)
    assert st.wavelet_image(grey).shape == (h, w, 1) and st._lib.last()[1][1]["channels"] == 1
    c = WaveletParameters(sigma=2.5)._c()
    assert c.sigma_given == 1 and list(c.sigma) == [2.5] * 4


# ---- 3. identities of the restatement -------------------------------------------------------------------------------
def _messy(rng, h, w, cn):
    d = (rng.random((h, w, cn)) * 100 - 10).astype(np.float32)
    d[1, 2, 0], d[3, 4, 0], d[5, 6, 0], d[7, 1, 0], d[2, 7, 0], d[8, 8, 0], d[9, 3, 0] = np.nan, np.inf, -np.inf, 0.0, -0.0, 1e31, -9e29
    return d


def test_identities_of_the_restatement():
    rng = np.random.default_rng(5)
    # the defaults reconstruct the input to within the f32 rounding of the sums (the header's table)
    worst = {}
    for seed in SEEDS:
        d = wr.scene(seed)[1]
        for J in (1, 4, 6):
            o = wr.process(d, J)
            dev = float(np.abs(o.astype(np.float64) - d).max() / np.abs(d).max())
            worst[J] = max(worst.get(J, 0.0), dev)
            assert dev <= (2 * J + 1) * 2.0 ** -23, (seed, J, dev)
    print("reconstruction, worst |o - d| / max|d|:", {J: "%.2e" % v for J, v in worst.items()})
    # special values become 0 and every layer is finite; alpha passes through; the channels do not mix
    d = _messy(rng, 40, 37, 4)
    lay = wr.layers(d, 4)
    assert len(lay) == 5 and all(np.isfinite(a[..., :3]).all() for a in lay)
    assert all(a[..., 3].tobytes() == d[..., 3].tobytes() for a in lay)
    D = wr.sanitise(d[..., :3])
    assert D[1, 2, 0] == 0 and D[3, 4, 0] == 0 and D[5, 6, 0] == 0 and D[8, 8, 0] == 0 and D[9, 3, 0] == np.float32(-9e29)
    total = np.sum([a[..., :3].astype(np.float64) for a in lay], 0)
    assert np.abs(total - D).max() <= 9 * 2.0 ** -23 * np.abs(D).max()
    p = dict(levels=3, mode=wr.SOFT, gains=[1.5, 0.5, 2.0], thresholds_=[2.0, 1.0, 0.0], layer_amounts=[1.0, 0.5, 0.0], sigma_=3.0)
    a = wr.process(d, **p)
    assert a[..., 3].tobytes() == d[..., 3].tobytes()
    for c in range(3):
        assert wr.process(d[..., c], **p).tobytes() == a[..., c].tobytes()
    # a constant image: every layer is zero, the residual is the constant (the taps sum to 1 exactly in f32 for a power of two)
    const = np.full((20, 23), 64.0, np.float32)
    lay = wr.layers(const, 3)
    assert all(not a.any() for a in lay[:3]) and (lay[3] == 64.0).all()
    sg, med = wr.sigma(const)
    assert sg[0] == 0 and med[0] == 0
    assert wr.process(const, 3, thresholds_=5.0).tobytes() == const.tobytes()     # sigma 0: t = 0 and nothing is below it
    # linearity in the gain: with gains g on every layer and residual_gain 0 the output is g times the sum of the layers
    # (powers of two scale exactly); amount 0 returns the sanitised input; a zero mask too
    d = (rng.random((33, 35)) * 100).astype(np.float32)
    one = wr.process(d, 4, residual_gain=0.0)
    for g in (2.0, 0.5, -4.0):
        assert wr.process(d, 4, gains=g, residual_gain=0.0).tobytes() == (np.float32(g) * one).astype(np.float32).tobytes()
    assert wr.process(d, 4, gains=0.0).tobytes() == wr.layers(d, 4)[4].tobytes()  # the residual alone
    m4 = _messy(rng, 33, 35, 4)
    want = m4.copy()
    want[..., :3] = wr.sanitise(m4[..., :3])
    for got in (wr.process(m4, 4, gains=3.0, amount=0.0), wr.process(m4, 4, gains=3.0, mask=np.zeros((33, 35), np.float32))):
        # (equal as values, not as bits: fmaf(0, res - D, D) of a D = -0 is +0 where res - D > 0)
        assert np.array_equal(got[..., :3], want[..., :3]) and got[..., 3].tobytes() == want[..., 3].tobytes()
    # HARD with a threshold above every coefficient and layer_amount 1 removes the layers; layer_amount 0 keeps them
    assert wr.process(d, 3, thresholds_=1e6, sigma_=1.0).tobytes() == wr.layers(d, 3)[3].tobytes()
    assert wr.process(d, 3, thresholds_=1e6, sigma_=1.0, layer_amounts=0.0).tobytes() == wr.process(d, 3).tobytes()
    assert wr.process(d, 3, mode=wr.SOFT, thresholds_=1e6, sigma_=1.0, layer_amounts=0.0).tobytes() == wr.process(d, 3).tobytes()
    # the thresholds: f64 products cast once
    t = wr.thresholds(np.array([3.0, 2.5], np.float32), np.array([8.25, 0.0], np.float32), wr.noise_table(2), 2)
    assert t[0, 0] == np.float32(3.0 * 8.25 * wr.noise_table(1)[0]) and t[1].tolist() == [0.0, 0.0]


def test_sigma_of_pure_noise():
    """the estimator on what it is made for: white noise of sigma 5 on a flat sky, 256 x 256: within 1 % (the MAD of 65536
    samples has a relative deviation of 0.3 %)"""
    rng = np.random.default_rng(11)
    for n, (h, w) in enumerate(((256, 256), (255, 257))):                       # N even and N odd
        d = (1000.0 + rng.normal(0.0, 5.0, (h, w))).astype(np.float32)
        sg, med = wr.sigma(d)
        assert abs(float(sg[0]) / 5.0 - 1.0) < 0.01, sg
        w0 = np.abs(wr.layers(d, 1)[0]).reshape(-1)
        assert med[0] == np.sort(w0)[(w0.size + 1) // 2 - 1]


# ---- 4. quality, on the restatement ---------------------------------------------------------------------------------
def test_denoising_quality_of_the_definition():
    for seed in SEEDS:
        truth, noisy = wr.scene(seed)
        out, sg = wr.process(noisy, 4, wr.HARD, thresholds_=3.0, return_sigma=True)
        r = wr.rms_ratio(out, noisy, truth)
        serr = abs(float(sg[0]) / wr.SCENE_SIGMA - 1.0)
        print("seed %d: rms ratio %.4f, sigma %.3f (relative error %.4f)" % (seed, r, sg[0], serr))
        assert r < 1.0 and r <= BAR_RMS and serr <= BAR_SIGMA                   # 1.5 x the worst seed of the header's table
        assert sg[0] > wr.SCENE_SIGMA                                            # the stars bias the MAD upward
    assert BAR_RMS < 1.0


def median_fwhm(image, stars):
    """the lower median of the FWHM of the measured stars at the known positions (the restated stk_star_measure)"""
    sh = sm.measure(image, stars, StarMeasureParameters())
    good = sh[sh["flags"] == 0]
    assert len(good) >= 10
    return float(sm.lower_median(good["fwhm"]))


def test_sharpening_quality_of_the_definition():
    for seed in SEEDS:
        _, blurred, _, stars = dr.scene(seed)
        out = wr.process(blurred, 4, gains=SHARPEN)
        f0, f1 = median_fwhm(blurred, stars), median_fwhm(out, stars)
        print("seed %d: fwhm %.3f -> %.3f (%.4f)" % (seed, f0, f1, f1 / f0))
        assert f1 < f0 and f1 / f0 <= BAR_FWHM


# ---- 5. the kernel map of the new unit -------------------------------------------------------------------------------
def test_the_post_unit_has_its_kernel_map_and_every_kernel_a_gpu_test(tmp_path):
    """tests/kernel_post_wavelet.tsv (tools/kernel_coverage.py, POST): the existing tests pin kc.read_map() and kc.OWN, and ask
    that every .hip file directly in csrc/ is in one of them, so the unit lives in csrc/post/ with a map that neither returns,
    and this test holds it to what tests/test_cpu_deconvolve.py asks of its unit: the kernels of the unit, recomputed with the
    Makefile's own command, are the rows of the file; every row names a GPU test file that exists, qualifies and is marked
    gpu; no kernel is listed twice anywhere; write_map returns every row to its file byte for byte. The rows were written
    from the symbol names and the test file that launches each kernel, not from a trace. Only kernel symbol names are read."""
    import shutil
    from test_cpu_kernel_map import kc
    assert kc.POST == {"post/kernels_wavelet": "wavelet"}                       # (a unit joins this table only with a test like this one)
    post = kc.post_file("post/kernels_wavelet")
    assert os.path.basename(post) == "kernel_post_wavelet.tsv" and post not in kc.parts() + kc.supplements() + [kc.own_file(u) for u in kc.OWN]
    assert os.path.isfile(os.path.join(kc.CSRC, "post", "kernels_wavelet.hip"))
    rows = kc.read_rows(post)
    assert rows == kc.read_post() and len(rows) == 10 and all(r[0] == "post/kernels_wavelet" for r in rows)
    for unit, mangled, demangled, files in rows:
        assert mangled.startswith("_ZN3stk") and "stk::" in demangled and files == ["test_gpu_wavelet.py"]
        text = open(os.path.join(ROOT, "tests", files[0])).read()
        assert kc.qualifies(files[0]) and re.search(r"pytest\.mark\.gpu\b", text)
    names = sorted(re.search(r"(wavelet_\w+(<[^>]*>)?)\(", r[2]).group(1) for r in rows)
    assert names == ["wavelet_init_kernel<1>", "wavelet_init_kernel<3>", "wavelet_init_kernel<4>", "wavelet_level_kernel<false>", "wavelet_level_kernel<true>",
                     "wavelet_level_staged_kernel<false>", "wavelet_level_staged_kernel<true>",
                     "wavelet_select_hist_kernel", "wavelet_select_pick_kernel", "wavelet_select_reset_kernel"]
    listed = [r[1] for r in kc.read_map()] + [r[1] for r in kc.read_own()] + [r[1] for r in rows]
    assert len(set(listed)) == len(listed) and not any(r[0] in kc.POST for r in kc.read_map() + kc.read_own())
    assert not kc.uncovered(rows)
    # the three unit sets are disjoint and cover the Makefile's units; what the older tables return is what they returned
    cmds = set(kc.unit_commands())
    assert set(kc.POST) <= cmds and set(kc.OWN) <= cmds and not set(kc.POST) & set(kc.OWN)
    assert {r[0] for r in kc.read_map()} == cmds - set(kc.OWN) - set(kc.POST) and kc.OWN == {"kernels_deconvolve": "deconvolve"}
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is not None:                                         # (as tests/test_cpu_kernel_map.py: no compiler, no recomputation)
        built = kc.build_kernels(workdir=str(tmp_path), post=True)
        assert set(built) == set(kc.POST) and {(u, n) for u, names in built.items() for n in names} == {(r[0], r[1]) for r in rows}
    # write_map on copies: the committed maps and this one return byte for byte
    files = [kc.MAP] + kc.parts() + kc.supplements() + [kc.own_file(u) for u in sorted(kc.OWN)] + [post]
    copies = [str(tmp_path / os.path.basename(f)) for f in files]
    for src, dst in zip(files, copies):
        open(dst, "w").write(open(src).read())
    kernels, seen = {}, {}
    for unit, mangled, _, tests in kc.read_map(copies[0]) + kc.read_own(copies[0]) + kc.read_post(copies[0]):
        kernels.setdefault(unit, []).append(mangled)
        seen[mangled] = set(tests)
    kc.write_map({u: sorted(v) for u, v in kernels.items()}, seen, copies[0])
    assert all(open(src).read() == open(dst).read() for src, dst in zip(files, copies))


# ---- 6. the sanitizer harness ---------------------------------------------------------------------------------------
def test_wavelet_host_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "wavelet_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "wavelet_harness.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=500)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

"""CPU tests of noise estimation and inverse-variance frame weights (include/stacker.h, stk_noise_stat): the host
reduction stk_noise_from_hist and the weights stk_noise_weights, through the built library, against the numpy restatement
(tests/noise_restate.py) bit for bit; the struct layout, the symbols and the ctypes table against the header; every
refusal of the two host calls; what the Python wrappers hand to the C ABI; the estimator's quality on a synthetic star
field, on the restatement alone; and the host half under ASan + UBSan as a stand-alone program."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import libstacker_rs_amd as ls
import noise_restate as nr
from libstacker_rs_amd import NOISE_DTYPE, NoiseParameters, _ffi, noise_from_hist, noise_weights
from libstacker_rs_amd.api import EccMatchParameters, KeyPointMatchParameters, MotionType, WeightParameters
from test_cpu_api_calls import CTX, new_stacker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in _ffi.NoiseStat._fields_]
NEW = ("stk_noise_from_hist", "stk_stack_noise", "stk_noise_weights", "stk_ecc_match_noise_weighted", "stk_keypoint_match_noise_weighted")
SIGMAS = (1.5, 1.5, 2.0, 2.0, 3.0, 4.0, 6.0, 8.0)          # the issue's planted noise levels, in grey levels


def same(a, b):
    """two NOISE_DTYPE records (or arrays of them) agree in every bit"""
    return np.asarray(a, NOISE_DTYPE).tobytes() == np.asarray(b, NOISE_DTYPE).tobytes()


def frames_of(depth, h=41, w=53, seed=3):
    """the contents of the issue's list, one plane each: {name: plane}"""
    rng = np.random.default_rng(seed + depth)
    dt, top = (np.uint8, 255) if depth == 8 else (np.uint16, 65535)
    yy, xx = np.mgrid[0:h, 0:w]
    sky = rng.choice(np.array([20, 21, 22] if depth == 8 else [2000, 2001, 2002]), size=(h, w), p=[0.3, 0.5, 0.2])
    noisy = np.clip(np.rint((30 if depth == 8 else 3000) + rng.normal(0, 3 if depth == 8 else 300, (h, w))), 0, top)
    return {"random": rng.integers(0, top + 1, (h, w)).astype(dt), "constant": np.full((h, w), 77 if depth == 8 else 7777, dt),
            "zero": np.zeros((h, w), dt), "max": np.full((h, w), top, dt), "checkerboard": (((xx + yy) & 1) * top).astype(dt),
            "sky": sky.astype(dt), "noisy": noisy.astype(dt)}


# ---- stk_noise_from_hist == the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 16])
def test_from_hist_equals_the_restatement(depth):
    planes = frames_of(depth)
    got = {}
    for name, p in planes.items():
        hv, hr = nr.histograms(p)
        got[name] = noise_from_hist(hv, hr, depth == 16)
        want = nr.from_hist(hv, hr, depth == 16)
        assert same(got[name], want), (name, got[name], want)
        assert same(noise_from_hist(hv, hr, False), nr.from_hist(hv, hr, False)), name
    top = 255 if depth == 8 else 65535
    for name in ("constant", "zero", "max"):                                # no residual energy: flag bit 0, sigma 0
        g = got[name]
        assert g["flags"] == 1 and g["sigma"] == 0.0 and g["mad"] == 0 and g["res_median"] == 0 and g["kept"] == 39 * 51
    assert got["max"]["median"] == top and got["zero"]["median"] == 0
    cb = got["checkerboard"]                                                # every |r| is 8 x max
    if depth == 8:
        assert cb["res_median"] == 2040 and cb["flags"] == 0 and cb["kept"] == 39 * 51 and cb["sigma"] == 2040 * 1.0136 / 6.0
    else:
        assert cb["res_median"] == 65535 and cb["flags"] == 3 and cb["sigma"] == 0.0 and cb["kept"] == 0
    sky = got["sky"]
    assert sky["median"] == (21 if depth == 8 else 2001) and sky["mad"] in (0, 1) and sky["flags"] == 0 and 0.3 < sky["sigma"] < 1.2
    planted = 3.0 if depth == 8 else 300.0
    assert abs(got["noisy"]["sigma"] / planted - 1.0) < 0.1 and got["noisy"]["flags"] == 0


def test_from_hist_on_random_histograms_equals_the_restatement():
    rng = np.random.default_rng(11)
    for k in range(40):
        bv, br = (256, 2041) if k % 2 == 0 else (int(rng.integers(1, 400)), int(rng.integers(2, 3000)))
        hv = (rng.integers(0, 50, bv) * (rng.random(bv) < rng.uniform(0.02, 1.0))).astype(np.uint32)
        scale = rng.uniform(0.5, br)
        hr = np.bincount(np.minimum(np.abs(rng.normal(0, scale, 5000)).astype(np.int64), br - 1), minlength=br).astype(np.uint32)
        if k % 5 == 0:
            hr[br - 1] += 4000                                             # a heavy last bin: the cut runs into `top`
        for ov in (False, True):
            assert same(noise_from_hist(hv, hr, ov), nr.from_hist(hv, hr, ov)), (k, ov)
    z = np.zeros(256, np.uint32)                                           # empty histograms
    assert same(noise_from_hist(z, np.zeros(2041, np.uint32)), nr.from_hist(z, np.zeros(2041, np.uint32), False))
    big = np.zeros(65536, np.uint32)                                       # the largest sums: 2^27 pixels in the last regular bin
    big[65534] = 1 << 27
    assert same(noise_from_hist(big, big, True), nr.from_hist(big, big, True))


def test_from_hist_refusals():
    hv, hr = np.zeros(256, np.uint32), np.zeros(2041, np.uint32)
    lib = _ffi.load()
    out = _ffi.NoiseStat()
    a = lambda x: C.c_void_p(x.ctypes.data)
    assert lib.stk_noise_from_hist(a(hv), 256, a(hr), 2041, 0, C.byref(out)) == 0
    for args in ((None, 256, a(hr), 2041, 0, C.byref(out)), (a(hv), 256, None, 2041, 0, C.byref(out)), (a(hv), 256, a(hr), 2041, 0, None),
                 (a(hv), 0, a(hr), 2041, 0, C.byref(out)), (a(hv), 65537, a(hr), 2041, 0, C.byref(out)),
                 (a(hv), 256, a(hr), 1, 0, C.byref(out)), (a(hv), 256, a(hr), 65537, 0, C.byref(out)),
                 (a(hv), 256, a(hr), 2041, 2, C.byref(out)), (a(hv), 256, a(hr), 2041, -1, C.byref(out))):
        assert lib.stk_noise_from_hist(*args) == 2                         # STK_INVALID_PARAMS
    with pytest.raises(ls.InvalidParams):
        noise_from_hist(hv, np.zeros(1, np.uint32))


# ---- stk_noise_weights == the restatement ----------------------------------------------------------------------------
def _random_stats(rng, n):
    st = np.zeros((n, 4), NOISE_DTYPE)
    st["sigma"] = rng.uniform(0.0, 9.0, (n, 4)) * (rng.random((n, 4)) < 0.9)
    return st


def test_weights_equal_the_restatement():
    rng = np.random.default_rng(21)
    for k in range(60):
        n, cn = int(rng.integers(1, 9)), int(rng.choice([1, 3, 4]))
        st = _random_stats(rng, n)
        gain = rng.uniform(0.5, 2.0, (n, cn)).astype(np.float32) if k % 3 else None
        include = (rng.random(n) < 0.7).astype(np.int32) if k % 2 else None
        if include is not None and not include.any():
            include[int(rng.integers(0, n))] = 1
        user = rng.uniform(0.0, 3.0, n).astype(np.float32) if k % 4 < 2 else None
        floor = float(rng.choice([0.25, 1.0, 64.0, 1e-3]))
        got = noise_weights(st, cn, gain, include, user, floor)
        want = nr.weights(st, cn, gain, include, user, floor)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (k, got, want)
    # by hand: sigma 1, 2, 4 in every channel -> 1, 1/4, 1/16; a floor of 2 lifts the first frame to the second's level
    st = np.zeros((3, 4), NOISE_DTYPE)
    st["sigma"][:, :3] = [[1.0] * 3, [2.0] * 3, [4.0] * 3]
    assert noise_weights(st, 3).tolist() == [1.0, 0.25, 0.0625]
    assert noise_weights(st, 3, sigma_floor=2.0).tolist() == [1.0, 1.0, 0.25]
    assert noise_weights(st, 3, include=[0, 1, 1]).tolist() == [0.0, 1.0, 0.25]           # the first INCLUDED frame is the reference
    assert noise_weights(st, 3, gain=[[2.0] * 3, [1.0] * 3, [1.0] * 3]).tolist() == [1.0, 1.0, 0.25]   # a gain scales the noise it maps
    assert noise_weights(st, 3, weights=[2.0, 1.0, 0.0]).tolist() == [2.0, 0.25, 0.0]
    st["sigma"][:, 3] = 1e6                                                # the fourth channel does not enter: C = min(channels, 3)
    assert noise_weights(st, 4).tolist() == [1.0, 0.25, 0.0625]
    applied = [dict(gain=np.array([2.0, 2.0, 2.0], np.float32)), dict(gain=np.ones(3, np.float32)), dict(gain=np.ones(3, np.float32))]
    assert noise_weights(st, 3, applied=applied).tolist() == [1.0, 1.0, 0.25]


def test_weights_refusals():
    st = np.zeros((3, 4), NOISE_DTYPE)
    st["sigma"] = 1.0
    for floor in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ls.InvalidParams):
            noise_weights(st, 3, sigma_floor=floor)
    for u in ([1.0, -0.5, 1.0], [1.0, float("inf"), 1.0], [float("nan"), 1.0, 1.0]):
        with pytest.raises(ls.InvalidParams):
            noise_weights(st, 3, weights=u)
    with pytest.raises(ls.InvalidParams):
        noise_weights(st, 3, include=[0, 0, 0])                            # no frame included
    with pytest.raises(ls.InvalidParams):
        noise_weights(st, 2)                                               # channels
    with pytest.raises(ls.InvalidParams):
        noise_weights(st[:0], 3)                                           # n = 0
    with pytest.raises(ls.InvalidParams):
        noise_weights(st, 3, gain=[[0.0] * 3, [1.0] * 3, [1.0] * 3])       # a frame without variance
    bad = st.copy()
    bad["sigma"][1, 0] = np.nan
    with pytest.raises(ls.InvalidParams):
        noise_weights(bad, 3)
    assert noise_weights(bad, 3, include=[1, 0, 1]).tolist() == [1.0, 0.0, 1.0]           # an excluded frame's statistics are not read
    with pytest.raises(ls.InvalidParams):
        noise_weights(st[:, :3], 3)                                        # n x 4 expected
    with pytest.raises(ls.InvalidParams):
        noise_weights(st, 3, include=[1, 1])


# ---- layout, symbols, ctypes table -----------------------------------------------------------------------------------
def test_struct_layout_symbols_and_table_against_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(stk_noise_stat));\n' +
                   "".join('  printf(" %%zu", offsetof(stk_noise_stat, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_ffi.NoiseStat)] + [getattr(_ffi.NoiseStat, f).offset for f in FIELDS]
    assert C.sizeof(_ffi.NoiseStat) == 32 == NOISE_DTYPE.itemsize == nr.NOISE_DTYPE.itemsize
    assert [NOISE_DTYPE.fields[f][1] for f in FIELDS] == [getattr(_ffi.NoiseStat, f).offset for f in FIELDS]
    lib = _ffi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stacker.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        assert len(args.split(",")) == len(_ffi.SIGNATURES[name][1]), name
    sig = _ffi.SIGNATURES
    assert sig["stk_ecc_match_noise_weighted"][1][6] is C.c_double and sig["stk_keypoint_match_noise_weighted"][1][6] is C.c_double
    assert sig["stk_noise_weights"][1][6] is C.c_double
    assert NoiseParameters().floor(8) == 0.25 and NoiseParameters().floor(16) == 64.0 and NoiseParameters(2.0).floor(16) == 2.0


# ---- what the wrappers hand to the C ABI -----------------------------------------------------------------------------
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


def test_stack_noise_call():
    rng = np.random.default_rng(5)
    for dt, bins_ in ((np.uint8, 2297), (np.uint16, 131072)):
        for cn in (1, 3, 4):
            frames = rng.integers(0, 200, (2, 6, 7, cn)).astype(dt)
            st = new_stacker()
            seen = {}
            _spy_frames(st, "stk_stack_noise", seen)
            stats, hist = st.stack_noise(frames, return_hist=True)
            name, snap = st._lib.last()
            assert name == "stk_stack_noise" and snap[0] == CTX
            f = seen["frames"]
            assert (f["n"], f["width"], f["height"], f["channels"], f["depth"], f["location"], f["stride"]) == (2, 7, 6, cn, 8 * np.dtype(dt).itemsize, 0, 0)
            assert f["data"] == [frames[i].tobytes() for i in range(2)]
            assert stats.shape == (2, 4) and stats.dtype == NOISE_DTYPE and hist.shape == (2, cn, bins_) and hist.dtype == np.uint32
            assert snap[3] == hist.ctypes.data                             # the histograms land in the array returned
            st2 = new_stacker()
            assert st2.stack_noise(frames).shape == (2, 4) and st2._lib.last()[1][3] is None
    with pytest.raises(ls.NotEnoughFiles):
        new_stacker().stack_noise([])


@pytest.mark.parametrize("kind", ["ecc", "keypoint"])
def test_noise_weighted_match_call(kind):
    rng = np.random.default_rng(6)
    frames = rng.integers(0, 200, (3, 8, 12, 3)).astype(np.uint8)
    params = EccMatchParameters(MotionType.Affine, 50, 1e-3, 3) if kind == "ecc" else KeyPointMatchParameters()
    fn = "%s_match_noise_weighted" % kind
    nkp = 1 if kind == "keypoint" else 0
    for flags in ((False,) * 4, (True,) * 4, (True, False, True, False)):
        rs, rc, ra, rn = flags
        st = new_stacker()
        seen = {}
        _spy_frames(st, "stk_" + fn, seen)
        res = getattr(st, fn)(frames, params, WeightParameters(normalize=3, coverage=False, stat_step=2), [1.0, 2.0, 3.0], NoiseParameters(0.5), 6.5, return_stats=rs,
                              return_coverage=rc, return_applied=ra, return_noise=rn)
        name, snap = st._lib.last()
        assert name == "stk_" + fn and snap[0] == CTX and snap[3] == 6.5 and snap[6] == 0.5
        assert np.frombuffer(snap[4], np.int32).tolist() == [3, 0, 2, 0]   # the weight parameters
        f = seen["frames"]
        assert (f["n"], f["width"], f["height"], f["channels"], f["depth"]) == (3, 12, 8, 3, 8) and f["data"] == [x.tobytes() for x in frames]
        res = res if isinstance(res, tuple) else (res,)
        assert len(res) == 1 + nkp + sum(flags)
        img = res[nkp]
        assert img.shape == (8, 12, 3) and img.dtype == np.float32 and snap[7]["data"] == img.ctypes.data
        k = 1 + nkp
        if rc:
            assert res[k].shape == (8, 12) and res[k].dtype == np.float32
            k += 1
        if ra:
            assert len(res[k]) == 3 and set(res[k][0]) == {"gain", "offset", "weight", "flags"}
            k += 1
        if rn:
            assert res[k].shape == (3, 4) and res[k].dtype == NOISE_DTYPE
            k += 1
        if rs:
            assert len(res[k]) == 3 and "warp" in res[k][0]
        assert (snap[-1] is not None) == rn                                # the statistics: NULL unless wanted
    # the default floor follows the frames' depth
    st = new_stacker()
    getattr(st, fn)(frames, params)
    assert st._lib.last()[1][6] == 0.25
    if kind == "ecc":
        st = new_stacker()
        st.ecc_match_noise_weighted(frames.astype(np.uint16), params)
        assert st._lib.last()[1][6] == 64.0
    with pytest.raises(ls.InvalidParams):
        getattr(new_stacker(), fn)(frames, params, weights=[1.0, 2.0])


# ---- the estimator's quality, on the restatement alone -------------------------------------------------------------
def star_field(h=360, w=480, n_stars=100, seed=41):
    """a sky gradient with about 100 Gaussian stars, in grey levels, float64, below saturation"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 40.0 + 20.0 * xx / w + 10.0 * yy / h
    for _ in range(n_stars):
        x, y, a, s = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(20, 150), rng.uniform(1.2, 2.2)
        img += a * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
    return np.minimum(img, 235.0), rng


def test_estimator_quality_on_a_synthetic_star_field():
    scene, rng = star_field()
    frames = [np.clip(np.rint(scene + rng.normal(0.0, s, scene.shape)), 0, 255).astype(np.uint8) for s in SIGMAS]
    stats, _ = nr.stack_stats(frames)
    est = stats["sigma"][:, 0]
    rel = est / np.array(SIGMAS) - 1.0
    print("planted", SIGMAS, "estimated", np.round(est, 4).tolist(), "relative error", np.round(rel, 4).tolist())
    assert np.all(np.abs(rel) <= 0.10) and np.all(stats["flags"][:, 0] == 0)
    w = nr.weights(stats, 1, sigma_floor=0.25).astype(np.float64)
    stack = np.stack([f.astype(np.float64) for f in frames])
    rms = lambda m: math.sqrt(float(np.mean((m - scene) ** 2)))
    weighted, equal = rms(np.tensordot(w, stack, 1) / w.sum()), rms(stack.mean(0))
    s = np.array(SIGMAS)
    theory = (1.0 / np.sum(s ** -2.0)) ** 0.5 / (np.sum(s ** 2.0) ** 0.5 / len(s))
    print("rms weighted", weighted, "equal", equal, "ratio", weighted / equal, "theory", theory)
    assert abs(theory - 0.538) < 1e-3
    assert weighted / equal <= 1.1 * theory
    # the library's reduction of the same histograms gives the same weights
    lib_stats = np.zeros((len(frames), 4), NOISE_DTYPE)
    for i, f in enumerate(frames):
        lib_stats[i, 0] = noise_from_hist(*nr.histograms(f))
    assert same(lib_stats, stats) and noise_weights(lib_stats, 1).tobytes() == nr.weights(stats, 1).tobytes()


# ---- the host half as a stand-alone program under ASan + UBSan ------------------------------------------------------
@pytest.mark.timeout(600)
def test_host_half_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "noise_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "noise_harness.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=500)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

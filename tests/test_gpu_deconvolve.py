"""Deconvolution on the GPU (include/stacker.h, "deconvolution"): every output bit of stk_deconvolve against the numpy
restatement (tests/deconvolve_restate.py) over channel counts, sizes around the kernels' tile, radii, iteration counts, the
regulariser, masks, amounts, pedestals, special inputs, host and device images, padded and misaligned rows, in-place output;
history independence; every refusal that needs a context; the delta-PSF identity; and the pipeline check: a PSF from the
image's own stars, the deconvolution with it, and the star shapes before and after.

The kernels' tile is 64 pixels wide and 16 rows per row of outputs of a thread (DCV_TW, DCV_TH = 16 DCV_NY, common.h): the
sizes below lie around 64 and 128 wide and around 16 and 32 high, so they hold for one and for two rows per thread."""
import itertools

import numpy as np
import pytest

import deconvolve_restate as dr
from libstacker_rs_amd import (DeconvolveParameters, InvalidParams, Stacker, StarDeepParameters, StarMeasureParameters, StarParameters,
                               star_frame_quality)
from test_cpu_deconvolve import BAR_RMS30
from test_gpu_star_deep import _place

pytestmark = pytest.mark.gpu
T_W = 64
SIZES = [(T_W - 1, 15), (T_W, 16), (T_W + 1, 17), (2 * T_W + 1, 31), (T_W - 1, 32), (T_W + 1, 33), (70, 50), (3, 3)]      # (w, h); R = 2
TV = dict(lambda_=0.01, tv_eps=0.5)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _psf(rng, R):
    """no symmetry at all: random positive taps, normalised"""
    P = rng.random((2 * R + 1, 2 * R + 1)) + 0.05
    P[R, R] += 0.3 * P.sum()
    return (P / P.sum()).astype(np.float32)


def _image(rng, h, w, cn, special=True):
    """positive values of mixed size; special: NaN, +-inf, negatives, zeros, and a block of zeros wider than any PSF here, so
    that the blurred estimate falls below `floor`"""
    d = (rng.random((h, w, cn)) * np.exp(rng.uniform(0, 6, (h, w, cn)))).astype(np.float32)
    if special and h >= 8 and w >= 8:
        d[1, 2], d[2, 5, 0], d[3, 1, -1], d[5, 5], d[6, 2] = np.nan, np.inf, -np.inf, -3.5, 0.0
        d[h // 2:h // 2 + 8, w // 2:w // 2 + 8] = 0.0
    return d if cn > 1 else d[..., 0]


def _restate(d, P, p, mask=None):
    return dr.deconvolve(d, P, iterations=p.iterations, floor=p.floor, pedestal=p.pedestal, lam=p.lambda_, tv_eps=p.tv_eps, amount=p.amount, mask=mask)


def _check(st, d, P, p, mask=None, padded=False, device=False, mask_padded=False, mask_device=False, what=None):
    want = _restate(d, P, p, mask)
    assert np.isfinite(want).all() or not np.isfinite(d).all()
    m = None if mask is None else _place(mask, mask_padded, mask_device)
    if m is not None and len(m.shape) == 3:
        m = m[..., 0]
    got = _np(st.deconvolve_image(_place(d, padded, device), P, p, mask=m))
    want3 = want if want.ndim == 3 else want[..., None]
    assert got.shape == want3.shape and got.dtype == np.float32
    assert got.tobytes() == want3.tobytes(), (what, np.argwhere(got.view(np.uint32) != want3.view(np.uint32))[:4].tolist())
    return got


# ---- 1. channels x sizes around the tile ----------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_sizes_and_channels_equal_the_restatement(st, cn):
    rng = np.random.default_rng(10 + cn)
    P = _psf(rng, 2)
    for k, (w, h) in enumerate(SIZES):
        d = _image(rng, h, w, cn)
        p = DeconvolveParameters(iterations=2, radius=2, floor=1e-3, **(TV if k % 2 else {}))
        got = _check(st, d, P, p, padded=bool(k & 1), device=bool(k & 2), what=(w, h, cn))
        if cn == 4:
            assert got[..., 3].tobytes() == d[..., 3].tobytes()                  # alpha: the input's bits, NaN and inf included
        if h >= 16:
            D = np.where(np.isfinite(d) & (d >= 0), d, 0).astype(np.float32).reshape(h, w, -1)[..., 0]
            assert dr.tap_sum(P, D, 2, True).min() < np.float32(1e-3)           # `floor` is reached


# ---- 2. radii ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,w,h,it", [(1, 70, 50, 2), (2, 70, 50, 2), (3, 70, 50, 2), (8, 70, 50, 1), (8, 130, 34, 1), (16, 40, 36, 2), (9, 40, 36, 1), (12, 70, 20, 1),
                                      (1, 2, 2, 3), (3, 4, 4, 2), (8, 9, 9, 2), (16, 17, 17, 1), (5, 65, 6, 2), (7, 8, 40, 2)])
def test_radii_equal_the_restatement(st, R, w, h, it):
    rng = np.random.default_rng(100 + R + w)
    P = _psf(rng, R)
    for cn, tv, device in ((1, False, True), (3, True, False)):
        if R >= 8 and cn == 3 and w * h > 2000:
            continue                                                            # (the restatement's time)
        d = _image(rng, h, w, cn, special=R <= 3)
        _check(st, d, P, DeconvolveParameters(iterations=it, radius=R, floor=1e-3, **(TV if tv else {})), device=device, padded=tv, what=(R, w, h, cn))


# ---- 3. iterations, the regulariser, masks, amounts, pedestals --------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_parameters_equal_the_restatement(st, masked):
    rng = np.random.default_rng(7 + masked)
    h, w = 37, 70
    P = _psf(rng, 2)
    d = _image(rng, h, w, 3)
    mask = None
    if masked:
        mask = rng.random((h, w)).astype(np.float32)
        mask[:10, :20], mask[20:, 30:50] = 1.0, 0.0
    for k, (it, tv, amount, pedestal) in enumerate(itertools.product((1, 2, 5), (False, True), (1.0, 0.5, 0.0), (0.0, 7.25))):
        if it == 5 and amount == 0.5 and pedestal == 0.0:
            continue
        p = DeconvolveParameters(iterations=it, radius=2, floor=1e-3, pedestal=pedestal, amount=amount, **(TV if tv else {}))
        got = _check(st, d, P, p, mask, padded=bool(k & 1), device=bool(k & 2), mask_padded=bool(k & 4), mask_device=bool(k & 2) != bool(k & 8),
                     what=(it, tv, amount, pedestal))
        if amount == 0.0:
            with np.errstate(invalid="ignore"):
                D = (d + np.float32(pedestal)).astype(np.float32)
            assert got.tobytes() == (np.where(np.isfinite(D) & (D >= 0), D, np.float32(0)) - np.float32(pedestal)).astype(np.float32).tobytes()


def test_a_negative_pedestal_and_a_large_floor(st):
    rng = np.random.default_rng(3)
    d = _image(rng, 33, 65, 3)
    P = _psf(rng, 3)
    _check(st, d, P, DeconvolveParameters(iterations=3, radius=3, floor=50.0, pedestal=-2.0), device=True)
    _check(st, d, P, DeconvolveParameters(iterations=2, radius=3, floor=1e-30, pedestal=0.5, **TV))


def test_more_rows_than_one_launch_of_the_initialisation_covers(st):
    """the initialisation strides its rows by the grid: 4 x 65535 = 262140 rows per sweep; the passes' own limit is 65535 tiles"""
    rng = np.random.default_rng(4)
    h, w = 262140 + 9, 2
    d = (rng.random((h, w)) * 50).astype(np.float32)
    d[5, 1], d[h - 2, 0] = np.nan, -1.0
    _check(st, d, _psf(rng, 1), DeconvolveParameters(iterations=1, radius=1, floor=1e-3), device=True)
    d4 = (rng.random((h, w, 4)) * 50).astype(np.float32)
    _check(st, d4, _psf(rng, 1), DeconvolveParameters(iterations=1, radius=1, floor=1e-3, **TV))


# ---- 4. outputs the caller holds: padded, misaligned, in place --------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_outputs_the_caller_holds(st, device):
    rng = np.random.default_rng(21 + device)
    h, w, cn = 33, 65, 3
    P = _psf(rng, 2)
    d = _image(rng, h, w, cn)
    p = DeconvolveParameters(iterations=2, radius=2, floor=1e-3, pedestal=1.0, **TV)
    want = _restate(d, P, p)
    for pad_in, pad_out in itertools.product((False, True), repeat=2):
        src = _place(d.copy(), pad_in, device)
        out = _place(np.full((h, w, cn), -777.0, np.float32), pad_out, device)
        assert st.deconvolve_image(src, P, p, out=out) is out
        assert _np(out).tobytes() == want.tobytes(), (pad_in, pad_out)
        assert _np(src).tobytes() == d.tobytes()                                # the input is left as it was
        src = _place(d.copy(), pad_in, device)                                  # in place: same pointer, same stride
        assert st.deconvolve_image(src, P, p, out=src) is src
        assert _np(src).tobytes() == want.tobytes(), (pad_in, "in place")
    if not device:                                                              # only pixel bytes are written
        big = np.full((h, w + 3, cn), -777.0, np.float32)
        st.deconvolve_image(d, P, p, out=big[:, :w])
        assert big[:, :w].tobytes() == want.tobytes() and (big[:, w:] == -777.0).all()
        m4 = _image(rng, h, w, 4)
        big = np.full((h, w + 3, 4), -777.0, np.float32)
        big[:, :w] = m4
        st.deconvolve_image(big[:, :w], P, p, out=big[:, :w])
        assert big[:, :w].tobytes() == _restate(m4, P, p).tobytes() and (big[:, w:] == -777.0).all()


# ---- 5. history independence ------------------------------------------------------------------------------------------
def test_the_same_bits_whatever_the_context_held(st):
    rng = np.random.default_rng(5)
    d = _image(rng, 50, 70, 3)
    P, P8 = _psf(rng, 2), _psf(rng, 8)
    p = DeconvolveParameters(iterations=3, radius=2, floor=1e-3, **TV)
    a = st.deconvolve_image(d, P, p).tobytes()
    assert st.deconvolve_image(d, P, p).tobytes() == a
    st.deconvolve_image(_image(rng, 90, 150, 4), P8, DeconvolveParameters(iterations=1, radius=8))      # other planes, other taps
    assert st.deconvolve_image(d, P, p).tobytes() == a
    st.stack_sharpness([rng.integers(0, 255, (80, 90, 3), dtype=np.uint8) for _ in range(2)])
    assert st.deconvolve_image(d, P, p).tobytes() == a
    fresh = Stacker(0)
    assert fresh.deconvolve_image(d, P, p).tobytes() == a
    fresh.close()
    assert st.timing()["finalize_ms"] > 0.0


# ---- 6. refusals that need a context --------------------------------------------------------------------------------
def test_refusals(st):
    rng = np.random.default_rng(9)
    h, w = 20, 30
    d = _image(rng, h, w, 3, special=False)
    P = _psf(rng, 2)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(iterations=0), dict(iterations=1001), dict(floor=0.0), dict(floor=-1.0), dict(floor=nan), dict(floor=inf), dict(pedestal=nan),
                dict(pedestal=inf), dict(lambda_=-0.1), dict(lambda_=nan), dict(lambda_=inf), dict(tv_eps=0.0), dict(tv_eps=nan), dict(tv_eps=inf),
                dict(amount=-0.1), dict(amount=1.1), dict(amount=nan)):
        with pytest.raises(InvalidParams):
            st.deconvolve_image(d, P, DeconvolveParameters(**dict(dict(radius=2), **bad)))
    for R in (0, 17):
        with pytest.raises(InvalidParams):
            st.deconvolve_image(np.ones((40, 40), np.float32), np.full((2 * R + 1,) * 2, 1.0 / (2 * R + 1) ** 2, np.float32), DeconvolveParameters(radius=R))

    class Reserved(DeconvolveParameters):
        def _c(self):
            c = super()._c()
            c.reserved = 1
            return c
    with pytest.raises(InvalidParams):
        st.deconvolve_image(d, P, Reserved(radius=2))
    for shape in ((2, 30), (20, 2)):                                            # narrower or lower than radius + 1
        with pytest.raises(InvalidParams):
            st.deconvolve_image(np.ones(shape + (3,), np.float32), P)
    with pytest.raises(InvalidParams):
        st.deconvolve_image(np.ones((h, w, 2), np.float32), P)                  # two channels
    for k, v in ((0, -1e-3), (3, nan), (7, inf), (12, 0.1 * 1.0)):              # a negative, a NaN, an infinite tap; a sum off by 0.1
        Q = P.copy()
        Q.reshape(-1)[k] = Q.reshape(-1)[k] + v if k == 12 else v
        with pytest.raises(InvalidParams):
            st.deconvolve_image(d, Q)
    Q = (P.astype(np.float64) * (1.0 + 2e-3)).astype(np.float32)
    with pytest.raises(InvalidParams):
        st.deconvolve_image(d, Q)
    st.deconvolve_image(d, (P.astype(np.float64) * (1.0 + 5e-4)).astype(np.float32), DeconvolveParameters(iterations=1, radius=2))      # within 1e-3
    # overlaps: the output may be the image itself and nothing else
    buf = np.zeros((h + 1, w, 3), np.float32)
    buf[:h] = d
    with pytest.raises(InvalidParams):
        st.deconvolve_image(buf[:h], P, out=buf[1:])                            # shifted by a row
    wide = np.zeros((h, 2 * w, 3), np.float32)
    with pytest.raises(InvalidParams):
        st.deconvolve_image(wide[:, :w], P, out=wide.reshape(2 * h, w, 3)[:h])  # the same pointer, another stride
    mbuf = np.ones((h, w * 3), np.float32)
    with pytest.raises(InvalidParams):
        st.deconvolve_image(d, P, mask=mbuf[:, :w], out=mbuf.reshape(h, w, 3))  # the output over the mask
    with pytest.raises(InvalidParams):
        st.deconvolve_image(d, P, out=np.zeros((h, w + 1, 3), np.float32))      # another geometry
    with pytest.raises(InvalidParams):
        st.deconvolve_image(d, P, out=np.zeros((h, w), np.float32))
    import torch
    with pytest.raises(InvalidParams):
        st.deconvolve_image(d, P, out=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"))       # another location
    dev = torch.from_numpy(d).cuda()
    both = torch.zeros((h + 1, w, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(InvalidParams):
        st.deconvolve_image(both[:h], P, out=both[1:])
    # the context is still good
    p = DeconvolveParameters(iterations=1, radius=2)
    assert _np(st.deconvolve_image(dev, P, p)).tobytes() == _restate(d, P, p).tobytes()


# ---- 7. the delta PSF -----------------------------------------------------------------------------------------------
def test_a_delta_psf_returns_the_sanitised_input(st):
    rng = np.random.default_rng(2)
    d = _image(rng, 40, 70, 4)
    d[d > 0] += 1.0                                                             # (no value between 0 and floor)
    for R, it, pedestal in ((1, 1, 0.0), (3, 4, 0.0), (8, 2, 12.5), (16, 1, 0.0)):
        P = np.zeros((2 * R + 1,) * 2, np.float32)
        P[R, R] = 1.0
        got = st.deconvolve_image(d, P, DeconvolveParameters(iterations=it, radius=R, pedestal=pedestal))
        with np.errstate(invalid="ignore"):
            D = (d[..., :3] + np.float32(pedestal)).astype(np.float32)
        want = d.copy()
        want[..., :3] = np.where(np.isfinite(D) & (D >= 0), D, np.float32(0)) - np.float32(pedestal)
        assert got.tobytes() == want.tobytes(), (R, it)


# ---- 8. the pipeline --------------------------------------------------------------------------------------------------
def test_psf_from_the_image_sharpens_its_stars(st):
    """The CPU test's scene at seed 0: psf_from_image on the blurred image, deconvolve_image with that PSF, star_measure on the
    result: the frame-median FWHM falls and the RMS error against the unblurred scene meets the CPU test's bar."""
    truth, blurred, _, _ = dr.scene(0)
    sp, deep, mp = StarParameters(radius=5, kappa=6.0, min_contrast=50, min_pixels=5, max_stars=50), StarDeepParameters(1.0), StarMeasureParameters()
    psf, (cxx, cyy, cxy, used) = st.psf_from_image(blurred, dr.SCENE_R, deep, mp, sp, return_covariance=True)
    assert used >= 10 and psf.shape == (13, 13)
    tx, ty, txy = dr.SCENE_COV                                                  # the blur's covariance plus the stars' own 0.64
    assert abs(cxx - (tx + 0.64)) < 0.15 * tx and abs(cyy - (ty + 0.64)) < 0.15 * ty and abs(cxy - txy) < 0.15 * tx
    p = DeconvolveParameters(iterations=30, radius=dr.SCENE_R)
    out = st.deconvolve_image(blurred, psf, p)[..., 0]
    assert out.tobytes() == _restate(blurred, psf, p).tobytes()

    def quality(img):
        stars = st.star_detect_deep([img], sp, deep)
        return star_frame_quality(st.star_measure([img], stars, mp, deep))[0]
    before, after = quality(blurred), quality(out)
    ratio = dr.rms_ratio(out, blurred, truth)
    print("fwhm %.3f -> %.3f, rms ratio %.4f (bar %.4f), stars %d -> %d" % (before["fwhm"], after["fwhm"], ratio, BAR_RMS30, before["n_measured"], after["n_measured"]))
    assert before["n_measured"] >= 10 and after["n_measured"] >= 10
    assert after["fwhm"] < before["fwhm"]
    assert ratio <= BAR_RMS30
    # a device tensor takes the same road
    import torch
    assert st.psf_from_image(torch.from_numpy(blurred).cuda(), dr.SCENE_R, deep, mp, sp).tobytes() == psf.tobytes()

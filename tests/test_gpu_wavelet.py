"""The wavelet layers on the GPU (include/stacker.h, "wavelet layers"): every output bit of stk_wavelet_layers and
stk_wavelet_process against the numpy restatement (tests/wavelet_restate.py) over channel counts, the smallest image of every
level count, sizes around the kernels' tile, both modes, random gains, thresholds and layer amounts, given and estimated
sigma, masks, amounts, special inputs, host and device images, padded and misaligned rows, in-place output; the process
call's layers against stk_wavelet_layers' planes; the exact selection through stk_wavelet_sigma's median over scales, ties,
odd and even counts and medians on the digit boundaries of the radix rounds; every refusal that needs a context; history
independence; both forms of the level kernel; images of more rows than one sweep of the grid covers; the layers form's own
refusals.

The kernels' tile is 64 pixels wide and 16 rows high (WV_TW, WV_TH, common.h), a thread 4 rows 4 apart; the selection runs 4
rounds of 8 bits from the top of the 32-bit key (WV_ROUNDS, WV_DIGIT_BITS). The restatement takes the engine's noise table
(which tests/test_cpu_wavelet.py holds to an independent restatement within 1e-12), so that the f32 thresholds are the same
numbers."""
import functools
import itertools

import numpy as np
import pytest

import wavelet_restate as wr
from libstacker_rs_amd import (WAVELET_HARD, WAVELET_SOFT, DeconvolveParameters, InvalidParams, Stacker, WaveletParameters, psf_model,
                               wavelet_noise_table)
from test_gpu_star_deep import _place

pytestmark = pytest.mark.gpu
T_W, T_H = 64, 16
E = wavelet_noise_table(8)
SIZES = [(T_W - 1, T_H - 1), (T_W, T_H), (T_W + 1, T_H + 1), (2 * T_W + 1, 2 * T_H + 1), (70, 50), (67, 21), (5, 5)]      # (w, h); levels 2


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _image(rng, h, w, cn, special=True):
    """values of both signs and mixed size; special: NaN, +-inf, magnitudes above 1e30, zeros of both signs"""
    d = ((rng.random((h, w, cn)) - 0.3) * np.exp(rng.uniform(0, 6, (h, w, cn)))).astype(np.float32)
    if special and h >= 5 and w >= 5:
        d[1, 2], d[2, 4, 0], d[3, 1, -1], d[4, 4], d[0, 0], d[4, 0, 0], d[0, 3, 0] = np.nan, np.inf, -np.inf, 1e31, -1e31, 0.0, -0.0
        d[h - 1, w - 1, 0], d[h - 2, w - 1, -1] = 1e30, -1e30                    # the largest magnitudes that are kept
    return d if cn > 1 else d[..., 0]


def _random_params(rng, levels, mode, sigma=None, amount=1.0, residual_gain=None):
    """(WaveletParameters, the restatement's keywords): random tables that include the values 0 and 1"""
    gains = rng.uniform(-1.0, 3.0, levels)
    thr = rng.uniform(0.0, 4.0, levels)
    la = rng.uniform(0.0, 1.0, levels)
    gains[rng.integers(levels)] = 1.0
    thr[rng.integers(levels)] = 0.0
    la[rng.integers(levels)] = 1.0
    if levels > 1:
        gains[0], la[levels - 1] = 0.0 if levels > 2 else gains[0], 0.0
    rg = float(rng.uniform(0.5, 1.5)) if residual_gain is None else residual_gain
    p = WaveletParameters(levels=levels, mode=mode, gains=list(gains), thresholds=list(thr), layer_amounts=list(la), residual_gain=rg, amount=amount, sigma=sigma)
    kw = dict(levels=levels, mode=mode, gains=gains, thresholds_=thr, layer_amounts=la, residual_gain=rg, amount=amount, sigma_=sigma, e=E)
    return p, kw


def _same(got, want, what=None):
    got = _np(got)
    want3 = want if want.ndim == 3 else want[..., None]
    assert got.shape == want3.shape and got.dtype == np.float32
    assert got.tobytes() == want3.tobytes(), (what, np.argwhere(got.view(np.uint32) != want3.view(np.uint32))[:4].tolist())
    return got


def _check(st, d, p, kw, mask=None, padded=False, device=False, mask_padded=False, mask_device=False, what=None):
    want, wsig = wr.process(d, mask=mask, return_sigma=True, want_sigma=True, **kw)
    m = None if mask is None else _place(mask, mask_padded, mask_device)
    if m is not None and len(m.shape) == 3:
        m = m[..., 0]
    got, sig = st.wavelet_image(_place(d, padded, device), p, mask=m, return_sigma=True)
    assert sig.tobytes() == wsig.tobytes(), (what, sig, wsig)
    return _same(got, want, what)


def _check_layers(st, d, levels, padded=False, device=False, what=None):
    want = wr.layers(d, levels)
    got = st.wavelet_layers(_place(d, padded, device), levels)
    assert len(got) == levels + 1
    for k in range(levels + 1):
        _same(got[k], want[k], (what, "layer", k))
    return [_np(g) for g in got]


# ---- 1. the smallest image of every level count ---------------------------------------------------------------------
@pytest.mark.parametrize("levels", range(1, 9))
def test_the_smallest_image_of_every_level_count(st, levels):
    rng = np.random.default_rng(40 + levels)
    n = 2 ** levels + 1
    cn = (1, 3, 4)[levels % 3]
    d = _image(rng, n, n, cn)
    _check_layers(st, d, levels, padded=bool(levels & 1), device=bool(levels & 2), what=levels)
    p, kw = _random_params(rng, levels, levels & 1)
    _check(st, d, p, kw, padded=bool(levels & 2), device=bool(levels & 1), what=levels)
    wide = _image(rng, n, n + 6, 1, special=False)                               # the minimum in one dimension only
    _check(st, wide, *_random_params(rng, levels, WAVELET_SOFT, sigma=2.0), what=(levels, "wide"))
    _check_layers(st, np.ascontiguousarray(wide.T), levels, what=(levels, "tall"))
    for shape in ((n - 1, n), (n, n - 1)):                                       # one below the minimum
        with pytest.raises(InvalidParams):
            st.wavelet_image(np.ones(shape, np.float32), WaveletParameters(levels=levels))
        with pytest.raises(InvalidParams):
            st.wavelet_layers(np.ones(shape, np.float32), levels)


# ---- 2. channels x sizes around the tile ----------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_sizes_and_channels_equal_the_restatement(st, cn):
    rng = np.random.default_rng(10 + cn)
    for k, (w, h) in enumerate(SIZES):
        d = _image(rng, h, w, cn)
        got = _check_layers(st, d, 2, padded=bool(k & 2), device=bool(k & 1), what=(w, h, cn))
        p, kw = _random_params(rng, 2, k & 1, sigma=None if k % 3 else [5.0, 0.0, 7.5])
        out = _check(st, d, p, kw, padded=bool(k & 1), device=bool(k & 2), what=(w, h, cn))
        if cn == 4:
            assert out[..., 3].tobytes() == d[..., 3].tobytes()                  # alpha: the input's bits, NaN and inf included
            assert all(g[..., 3].tobytes() == d[..., 3].tobytes() for g in got)


# ---- 3. modes, tables, sigma, masks, amounts ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [WAVELET_HARD, WAVELET_SOFT])
def test_parameters_equal_the_restatement(st, mode):
    rng = np.random.default_rng(7 + mode)
    h, w = 37, 70
    d = _image(rng, h, w, 3)
    mask = rng.random((h, w)).astype(np.float32)
    mask[:10, :20], mask[20:, 30:50] = 1.0, 0.0
    for k, (levels, sigma, amount, masked) in enumerate(itertools.product((1, 3, 5), (None, 3.5, [2.0, 0.0, 9.0]), (1.0, 0.5, 0.0), (False, True))):
        if levels == 5 and amount == 0.5 and not masked:
            continue
        p, kw = _random_params(rng, levels, mode, sigma=sigma, amount=amount)
        got = _check(st, d, p, kw, mask if masked else None, padded=bool(k & 1), device=bool(k & 2), mask_padded=bool(k & 4),
                     mask_device=bool(k & 2) != bool(k & 8), what=(levels, sigma, amount, masked))
        if amount == 0.0:
            assert np.array_equal(got, wr.sanitise(d))                          # (as values: a D = -0 may come out as +0)
    # the defaults are the reconstruction; gains on the fine layers change the image; a threshold with the estimated sigma
    out = _check(st, d, WaveletParameters(), dict(levels=4, e=E))
    D = wr.sanitise(d)
    assert np.abs(out.astype(np.float64) - D).max() <= 9 * 2.0 ** -23 * np.abs(D).max()
    clean = _image(rng, h, w, 3, special=False)
    p, kw = WaveletParameters(levels=4, mode=mode, thresholds=3.0), dict(levels=4, mode=mode, thresholds_=3.0, e=E)
    got, sig = st.wavelet_image(clean, p, return_sigma=True)
    assert (sig > 0).all() and sig.tobytes() == wr.sigma(clean, E[0])[0].tobytes()
    _same(got, wr.process(clean, **kw))
    assert got.tobytes() != clean.tobytes()


# ---- 4. outputs the caller holds: padded, misaligned, in place --------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_outputs_the_caller_holds(st, device):
    rng = np.random.default_rng(21 + device)
    h, w, cn = 33, 65, 3
    d = _image(rng, h, w, cn)
    p, kw = _random_params(rng, 3, WAVELET_SOFT, amount=0.75)
    want = wr.process(d, **kw)
    for pad_in, pad_out in itertools.product((False, True), repeat=2):
        src = _place(d.copy(), pad_in, device)
        out = _place(np.full((h, w, cn), -777.0, np.float32), pad_out, device)
        assert st.wavelet_image(src, p, out=out) is out
        assert _np(out).tobytes() == want.tobytes(), (pad_in, pad_out)
        assert _np(src).tobytes() == d.tobytes()                                # the input is left as it was
        src = _place(d.copy(), pad_in, device)                                  # in place: same pointer, same stride
        assert st.wavelet_image(src, p, out=src) is src
        assert _np(src).tobytes() == want.tobytes(), (pad_in, "in place")
    if not device:                                                              # only pixel bytes are written
        big = np.full((h, w + 3, cn), -777.0, np.float32)
        st.wavelet_image(d, p, out=big[:, :w])
        assert big[:, :w].tobytes() == want.tobytes() and (big[:, w:] == -777.0).all()
        m4 = _image(rng, h, w, 4)
        big = np.full((h, w + 3, 4), -777.0, np.float32)
        big[:, :w] = m4
        st.wavelet_image(big[:, :w], p, out=big[:, :w])
        assert big[:, :w].tobytes() == wr.process(m4, **kw).tobytes() and (big[:, w:] == -777.0).all()


# ---- 5. the process call's layers are stk_wavelet_layers' planes ----------------------------------------------------
def test_the_process_call_works_on_the_layers_call_planes(st):
    rng = np.random.default_rng(31)
    h, w, levels = 45, 83, 4
    d = _image(rng, h, w, 3)
    mask = rng.random((h, w)).astype(np.float32)
    lay = [np.moveaxis(_np(g), 2, 0) for g in st.wavelet_layers(d, levels)]
    for mode in (WAVELET_HARD, WAVELET_SOFT):
        p, kw = _random_params(rng, levels, mode, amount=0.8)
        got, sig = st.wavelet_image(d, p, mask=mask, return_sigma=True)
        gain, thr, la = (wr._table(kw[k], 8, f) for k, f in (("gains", 1.0), ("thresholds_", 0.0), ("layer_amounts", 1.0)))
        o = wr.combine(lay[:levels], lay[levels], wr.sanitise(np.moveaxis(d, 2, 0)), wr.thresholds(thr, sig, E, levels), la, gain, mode, kw["residual_gain"], 0.8, mask)
        assert got.tobytes() == np.moveaxis(o, 0, 2).tobytes()


# ---- 6. the selection -------------------------------------------------------------------------------------------------
def _check_sigma(st, d, device=False, padded=False, what=None):
    wsig, wmed = wr.sigma(d, E[0])
    sig, med = st.wavelet_sigma(_place(d, padded, device), return_median=True)
    assert med.tobytes() == wmed.tobytes() and sig.tobytes() == wsig.tobytes(), (what, med, wmed)
    assert st.wavelet_sigma(_place(d, padded, device)).tobytes() == wsig.tobytes()
    return med


def test_the_median_of_random_images_at_three_scales(st):
    rng = np.random.default_rng(50)
    for k, (scale, (h, w), cn) in enumerate(itertools.product((1e-30, 1.0, 1e30), ((33, 64), (35, 67), (3, 3)), (1, 3))):      # N even, N odd
        d = (np.clip(rng.normal(0.0, 0.3, (h, w, cn)), -0.99, 0.99) * scale).astype(np.float32)
        assert (np.abs(d) <= 1e30).all()
        med = _check_sigma(st, d if cn > 1 else d[..., 0], device=bool(k & 1), padded=bool(k & 2), what=(scale, h, w, cn))
        assert (med > 0).all()
    d = _image(rng, 40, 70, 4)                                                  # special values, and alpha is not measured
    assert _check_sigma(st, d).shape == (3,)
    deep = (rng.normal(0.0, 1.0, (16, 40)) * 1e-38).astype(np.float32)          # subnormal magnitudes: keys below 2^23
    _check_sigma(st, deep)


def test_the_median_under_heavy_ties(st):
    rng = np.random.default_rng(51)
    const = np.full((40, 70, 3), 12.5, np.float32)
    med = _check_sigma(st, const)
    assert not med.any() and not st.wavelet_sigma(const).any()
    p, kw = WaveletParameters(levels=3, thresholds=5.0), dict(levels=3, thresholds_=5.0, e=E)
    out, sig = st.wavelet_image(const, p, return_sigma=True)                     # sigma 0: t = 0, nothing is below it
    assert not sig.any() and _np(out).tobytes() == const.tobytes() == wr.process(const, **kw).tobytes()
    two = np.where(np.arange(70)[None, :] < 31, np.float32(3.0), np.float32(100.0)) * np.ones((41, 1), np.float32)
    assert _check_sigma(st, two.astype(np.float32), device=True)[0] == 0.0       # two levels: most of the first layer is 0
    for step in (8, 4, 3):                                                      # an impulse grid: few distinct magnitudes
        grid = np.zeros((45, 71), np.float32)
        grid[::step, ::step] = 64.0
        med = _check_sigma(st, grid, what=step)
        assert (med[0] == 0.0) == (step == 8)
    few = rng.integers(0, 3, (37, 66, 3)).astype(np.float32)                     # three levels at random
    _check_sigma(st, few, padded=True)


def _bands(keys, w=131, h=37):
    """A checkerboard (-1)^(x+y) A(x) with three bands of columns, 40 % / 30 % / 30 %, of amplitudes with the bit patterns
    `keys` (ascending, at most 22 significant bits each, so that 3 A is exact): away from the band borders the smoothed
    plane is exactly 0 and |w_0| = A, so the median is the middle band's amplitude."""
    amp = np.array(keys, np.uint32).view(np.float32)
    x = np.arange(w)
    A = np.where(x < 52, amp[0], np.where(x < 92, amp[1], amp[2])).astype(np.float32)
    sign = np.where((x[None, :] + np.arange(h)[:, None]) % 2 == 0, np.float32(1), np.float32(-1))
    return (sign * A[None, :]).astype(np.float32)


@pytest.mark.parametrize("keys", [(0x3FFFFFFC, 0x40000000, 0x40000004),      # the first value of the digits of rounds 1, 2 and 3
                                  (0x3FFFFFF8, 0x3FFFFFFC, 0x40000000),      # the last value of the digits of rounds 1 and 2
                                  (0x3F80FFFC, 0x3F810000, 0x3F810004),      # first of rounds 2 and 3, the prefix changes below the median
                                  (0x3F7FFFFC, 0x3F800000, 0x3F800004),      # 1.0: round 1's digit changes below the median, 7F -> 80
                                  (0x3EFFFFFC, 0x3F000000, 0x3F000004),      # the first value of a digit of round 0 (0x3F)
                                  (0x3EFFFFF8, 0x3EFFFFFC, 0x3F000000)])     # the last value of a digit of round 0 (0x3E FF FF ..)
def test_the_median_on_the_digit_boundaries_of_the_radix_rounds(st, keys):
    d = _bands(keys)
    med = _check_sigma(st, d, device=True, what=[hex(k) for k in keys])
    assert int(med.view(np.uint32)[0]) == keys[1]                                # the case is what it says
    _check_sigma(st, np.stack([d, d[::-1], -d], 2), what="three channels")


LOW_BYTE_SEEDS = ((448, 0xFF), (221, 0x00))                                  # median keys 0x3F226DFF and 0x3F065400


def test_the_median_on_the_last_value_of_the_last_digit(st):
    """The bands above have amplitudes of 22 bits, so their keys end in 00, 04, .. FC. Random images whose median key ends in
    0xFF and in 0x00 were found by a seed search on the restatement (5 x 7 pixels, seeds from 0 up)."""
    for seed, low in LOW_BYTE_SEEDS:
        d = np.random.default_rng(seed).normal(0.0, 1.0, (5, 7)).astype(np.float32)
        med = _check_sigma(st, d, what=seed)
        assert int(med.view(np.uint32)[0]) & 0xFF == low, (seed, hex(int(med.view(np.uint32)[0])))




# ---- 7. refusals that need a context --------------------------------------------------------------------------------
def test_refusals(st):
    rng = np.random.default_rng(9)
    h, w = 20, 30
    d = _image(rng, h, w, 3, special=False)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(levels=0), dict(levels=9), dict(levels=5), dict(mode=2), dict(mode=-1), dict(gains=nan), dict(gains=[1.0, inf]), dict(thresholds=-0.1),
                dict(thresholds=nan), dict(thresholds=[0.0, 0.0, 0.0, 0.0, inf]), dict(layer_amounts=1.1), dict(layer_amounts=-0.1), dict(layer_amounts=nan),
                dict(residual_gain=nan), dict(residual_gain=inf), dict(amount=-0.1), dict(amount=1.1), dict(amount=nan), dict(sigma=-1.0), dict(sigma=nan),
                dict(sigma=[1.0, 1.0, 1.0, inf])):
        with pytest.raises(InvalidParams):
            st.wavelet_image(d, WaveletParameters(**dict(dict(levels=2), **bad)))

    class Reserved(WaveletParameters):
        def _c(self):
            c = super()._c()
            c.reserved = 1
            return c
    with pytest.raises(InvalidParams):
        st.wavelet_image(d, Reserved(levels=2))
    with pytest.raises(InvalidParams):
        st.wavelet_image(np.ones((h, w, 2), np.float32))                        # two channels
    with pytest.raises(InvalidParams):
        st.wavelet_sigma(np.ones((2, 30), np.float32))                          # lower than 3 rows
    p = WaveletParameters(levels=2)
    # overlaps: the output may be the image itself and nothing else
    buf = np.zeros((h + 1, w, 3), np.float32)
    buf[:h] = d
    with pytest.raises(InvalidParams):
        st.wavelet_image(buf[:h], p, out=buf[1:])                               # shifted by a row
    wide = np.zeros((h, 2 * w, 3), np.float32)
    with pytest.raises(InvalidParams):
        st.wavelet_image(wide[:, :w], p, out=wide.reshape(2 * h, w, 3)[:h])     # the same pointer, another stride
    mbuf = np.ones((h, w * 3), np.float32)
    with pytest.raises(InvalidParams):
        st.wavelet_image(d, p, mask=mbuf[:, :w], out=mbuf.reshape(h, w, 3))     # the output over the mask
    with pytest.raises(InvalidParams):
        st.wavelet_image(d, p, out=np.zeros((h, w + 1, 3), np.float32))         # another geometry
    with pytest.raises(InvalidParams):
        st.wavelet_image(d, p, out=np.zeros((h, w), np.float32))
    import torch
    with pytest.raises(InvalidParams):
        st.wavelet_image(d, p, out=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"))          # another location
    dev = torch.from_numpy(d).cuda()
    both = torch.zeros((h + 1, w, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(InvalidParams):
        st.wavelet_image(both[:h], p, out=both[1:])
    # the context is still good
    assert _np(st.wavelet_image(dev, p)).tobytes() == wr.process(d, 2, e=E).tobytes()


# ---- 8. history independence ------------------------------------------------------------------------------------------
def test_the_same_bits_whatever_the_context_held(st):
    rng = np.random.default_rng(5)
    d = _image(rng, 50, 70, 3)
    p, kw = _random_params(rng, 4, WAVELET_SOFT)

    def run(s):
        out, sig = s.wavelet_image(d, p, return_sigma=True)
        return out.tobytes() + sig.tobytes() + b"".join(g.tobytes() for g in s.wavelet_layers(d, 3)) + s.wavelet_sigma(d).tobytes()
    a = run(st)
    assert run(st) == a
    for byte in (0x00, 0xFF, 0x7F):
        st.set_option("debug_poison", byte)
        assert st.timing()["debug_poison_bytes"] > 0
        assert run(st) == a, "after debug_poison 0x%02X" % byte
    st.wavelet_image(_image(rng, 90, 150, 4), WaveletParameters(levels=6, thresholds=2.0))          # other planes, other counts
    assert run(st) == a
    st.deconvolve_image(np.abs(_image(rng, 60, 80, 3, special=False)), psf_model(2, 1.5, 1.2, 0.3), DeconvolveParameters(iterations=2, radius=2))
    assert run(st) == a
    fresh = Stacker(0)
    assert run(fresh) == a
    fresh.close()
    st.wavelet_image(d, p)
    assert st.timing()["finalize_ms"] > 0.0


# ---- 9. both forms of the level kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["direct", "staged"])
def test_both_forms_of_the_level_kernel_equal_the_restatement(st, form, monkeypatch):
    """STK_WAVELET_FORM (wavelet.cpp) forces the direct or the LDS-staged level kernel at the spacings where both exist
    (s <= 32; beyond, the direct one runs under either): whichever is the default, both give the restatement's bits. The staged
    tile is 64 columns x 16 rows of one residue class, so at level j a block of 16 * 2^j image rows: heights around those."""
    monkeypatch.setenv("STK_WAVELET_FORM", form)
    rng = np.random.default_rng(70)
    for k, (w, h, levels, cn) in enumerate(((63, 15, 2, 3), (64, 16, 2, 1), (65, 17, 3, 4), (129, 33, 4, 3), (70, 65, 5, 1), (131, 135, 7, 1), (67, 513, 6, 1),
                                            (5, 5, 2, 3), (33, 257, 5, 3))):
        d = _image(rng, h, w, cn)
        _check_layers(st, d, levels, padded=bool(k & 1), device=bool(k & 2), what=(form, w, h, levels))
        p, kw = _random_params(rng, levels, k & 1, amount=0.7)
        _check(st, d, p, kw, mask=rng.random((h, w)).astype(np.float32), padded=bool(k & 2), device=bool(k & 1), what=(form, w, h, levels))


@functools.lru_cache(maxsize=None)
def _tall():
    """(image, restated output, restated sigma): computed once for both forms"""
    rng = np.random.default_rng(71)
    h, w = 1048600, 3
    d = rng.normal(0.0, 50.0, (h, w)).astype(np.float32)
    d[5, 1], d[h - 2, 0] = np.nan, 1e31
    return (d,) + wr.process(d, 1, wr.SOFT, gains=1.5, thresholds_=2.0, e=E, return_sigma=True)


@pytest.mark.parametrize("form", ["direct", "staged"])
def test_more_rows_than_one_sweep_of_the_grid_covers(st, form, monkeypatch):
    """every kernel strides its rows by the grid: 65535 workgroup rows cover 4 x 65535 rows of the initialisation, 16 x 65535 =
    1 048 560 rows of a level at spacing 1 and of the histogram; 1 048 600 rows need a second sweep of each"""
    monkeypatch.setenv("STK_WAVELET_FORM", form)
    d, want, wsig = _tall()
    got, sig = st.wavelet_image(d, WaveletParameters(levels=1, mode=WAVELET_SOFT, gains=1.5, thresholds=2.0), return_sigma=True)
    assert sig.tobytes() == wsig.tobytes()
    _same(got, want, form)


# ---- 10. the layers form's own refusals -----------------------------------------------------------------------------
def test_refusals_of_the_layers_form(st):
    import ctypes as C
    from libstacker_rs_amd import _ffi
    h, w, levels = 20, 30, 2
    d = np.ones((h, w, 3), np.float32)
    img = _ffi.ImageF32(d.ctypes.data, w, h, 3, 0, 0)

    def call(bufs, shapes=None, location=0):
        arr = (_ffi.ImageF32 * (levels + 1))()
        for k, b in enumerate(bufs):
            hh, ww, cc = (shapes or {}).get(k, (h, w, 3))
            arr[k] = _ffi.ImageF32(b.ctypes.data, ww, hh, cc, location, 0)
        return st._lib.stk_wavelet_layers(st._h, C.byref(img), levels, C.cast(arr, C.POINTER(_ffi.ImageF32)))
    fresh = [np.zeros((h, w, 3), np.float32) for _ in range(3)]
    assert call(fresh) == 0
    assert call([fresh[0], fresh[1], fresh[0]]) == 2                            # two outputs are the same image
    big = np.zeros((h + 1, w, 3), np.float32)
    assert call([big[:h], big[1:], fresh[2]]) == 2                              # two outputs overlap by all but a row
    assert call([fresh[0], d, fresh[2]]) == 2                                   # an output is the input: only the process form may
    both = np.ones((h + 1, w, 3), np.float32)
    img2 = _ffi.ImageF32(both.ctypes.data, w, h, 3, 0, 0)
    arr = (_ffi.ImageF32 * 3)(*[_ffi.ImageF32(b.ctypes.data, w, h, 3, 0, 0) for b in (fresh[0], both[1:], fresh[2])])
    assert st._lib.stk_wavelet_layers(st._h, C.byref(img2), levels, C.cast(arr, C.POINTER(_ffi.ImageF32))) == 2       # an output over part of the input
    assert call(fresh, {1: (h, w + 1, 3)}) == 2 and call(fresh, {2: (h, w, 1)}) == 2 and call(fresh, {0: (h - 1, w, 3)}) == 2   # geometry of one output
    assert call(fresh, location=1) == 2                                         # another location
    assert st._lib.stk_wavelet_layers(st._h, C.byref(img), levels, None) == 2
    assert st._lib.stk_wavelet_layers(st._h, C.byref(img), 0, C.cast((_ffi.ImageF32 * 3)(), C.POINTER(_ffi.ImageF32))) == 2
    lay = st.wavelet_layers(d, levels)                                          # the context is still good
    assert _np(lay[2]).tobytes() == wr.layers(d, levels)[2].tobytes()

"""The display stretch on the GPU (include/stacker.h, "display stretch"): every field of stk_image_stats and every output
bit of stk_stretch and stk_auto_stretch against the numpy restatement (tests/stretch_restate.py): the smallest images, sizes
around the kernels' tile, 1 / 3 / 4 channels, masks, NaN and infinities, negative values and zeros of both signs, heavy
ties, keys on the digit boundaries of every radix round (for the median and for the MAD), the median in the first and in
the last bin, quantiles at the ends and beside k / N, padded and misaligned rows, host and device images, images of more
rows than one sweep of a grid covers; every depth, curve and colour mode, samples at and beyond black and white, L = 0,
half-to-even cases, tables of 2 and 65536 knots, alpha, outputs the caller holds, in place; the whole form against its
parts; every refusal that needs a context; history independence.

The statistics' workgroup is 64 columns x 4 rows and its grid at most about 1024 workgroups (ST_TARGET_BLOCKS, common.h), rows
beyond them strided; the selection runs 4 rounds of 8 bits from the top of the 32-bit key (ST_ROUNDS, ST_DIGIT_BITS). The
stretch's thread owns 4 consecutive pixels of a row, a workgroup 256 columns x 4 rows, at most 65535 workgroup rows."""
import functools
import itertools

import numpy as np
import pytest

import stretch_restate as sr
from libstacker_rs_amd import (CURVE_ASINH, CURVE_GAMMA, DEPTH_F32, DEPTH_U8, DEPTH_U16, STAT_DTYPE, STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE,
                               AutoStretchParameters, InvalidParams, Stacker, StretchParameters, WaveletParameters, stretch_auto, stretch_table)
from test_gpu_star_deep import _place as _place_rows

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = [(1, 1), (2, 1), (1, 2)]                                              # (w, h)
SIZES = [(w, h) for w in (63, 64, 65, 129) for h in (1, 5, 33)]
DEPTHS = {DEPTH_U8: np.uint8, DEPTH_U16: np.uint16, DEPTH_F32: np.float32}


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _place(frame, padded, device):
    """as test_gpu_star_deep._place: host or device, tightly packed from an aligned base or (padded) rows 5 elements longer from
    a base one element past an aligned address. An image of one row has no row step to pad: it is placed misaligned alone."""
    f3 = frame if frame.ndim == 3 else frame[..., None]
    if not padded or f3.shape[0] > 1:
        return _place_rows(frame, padded, device)
    h, w, cn = f3.shape
    if device:
        import torch
        big = torch.zeros(w * cn + 4, dtype=torch.from_numpy(f3[:1, :1]).dtype, device="cuda")
        big[1:1 + w * cn] = torch.from_numpy(np.ascontiguousarray(f3).reshape(-1)).cuda()
        return big[1:1 + w * cn].view(1, w, cn)
    big = np.zeros(w * cn + 16, frame.dtype)
    off = (-big.ctypes.data % 16) // big.itemsize + 1
    big[off:off + w * cn] = f3.reshape(-1)
    return big[off:off + w * cn].reshape(1, w, cn)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _image(rng, h, w, cn, special=True):
    """a linear image: sky, a few bright samples, values below 0 and above 1; special: NaN, +-inf, zeros of both signs"""
    d = (0.02 + 0.01 * rng.standard_normal((h, w, cn)) + (rng.random((h, w, cn)) < 0.05) * rng.random((h, w, cn)) * 1.5).astype(F)
    d[np.abs(d) < 1e-30] = 0.0
    if special and h * w >= 25:
        flat = d.reshape(-1, cn)
        flat[1], flat[3, 0], flat[5, -1], flat[7, 0], flat[9, 0], flat[11, -1] = np.nan, np.inf, -np.inf, 0.0, -0.0, -0.0
    return d if cn > 1 else d[..., 0]


def _same_stats(st, d, mask=None, quantiles=(), padded=False, device=False, mask_padded=False, mask_device=False, what=None):
    want = sr.stats(d, mask, quantiles)
    m = None if mask is None else _place(mask, mask_padded, mask_device)
    if m is not None and len(m.shape) == 3:
        m = m[..., 0]
    got = st.image_stats(_place(d, padded, device), mask=m, quantiles=quantiles)
    assert got.dtype == STAT_DTYPE and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (what, got, want)
    return got


def _same_image(got, want, what=None):
    got = _np(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got.view(bits) != want.view(bits))[:4].tolist())
    return got


def _random_stretch(rng, curve, colour, depth, tab=None):
    """(StretchParameters, the restatement's keywords)"""
    black = rng.uniform(-0.01, 0.02, 4)
    white = black + rng.uniform(0.1, 1.2, 4)
    mid = rng.uniform(0.01, 0.6, 4)
    scale = float(rng.choice([1.0, 255.0, 0.37]))
    p = StretchParameters(curve=curve, colour=colour, out_depth=depth, black=list(black), white=list(white), midtone=list(mid), out_scale=scale, table=tab)
    return p, dict(curve=curve, colour=colour, out_depth=depth, black=black.astype(F), white=white.astype(F), midtone=mid.astype(F), out_scale=scale, tab=tab)


def _check_stretch(st, d, p, kw, padded=False, device=False, what=None):
    return _same_image(st.stretch_image(_place(d, padded, device), p), sr.stretch(d, **kw), what)


TABLES = {k: stretch_table(CURVE_ASINH, 200.0, k) for k in (2, 37, 65536)}


# ---- 1. statistics: sizes and channels ------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_statistics_of_sizes_and_channels(st, cn):
    rng = np.random.default_rng(10 + cn)
    for k, (w, h) in enumerate(SMALL + SIZES):
        d = _image(rng, h, w, cn)
        n = w * h
        qs = (0.0, 1.0, 1.0 / n, min(1.0, (n // 3 + 1e-9 * n) / n))             # the ends, 1 / N, just above k / N
        got = _same_stats(st, d, quantiles=qs, padded=bool(k & 1), device=bool(k & 2), what=(w, h, cn))
        assert got.shape == (min(cn, 3),)
        mask = (rng.random((h, w)) - 0.4).astype(F)                              # about 40 % of it is not > 0
        if h * w >= 25:
            mask[0, 0], mask[0, 2] = np.nan, -0.0
        _same_stats(st, d, mask, qs[:2], padded=bool(k & 2), device=bool(k & 1), mask_padded=bool(k & 4), mask_device=bool(k & 1) != bool(k & 8), what=(w, h, cn, "mask"))
    two = np.array([[5.0, -3.0]], F)                                            # N even: the lower median is the smaller value
    assert _same_stats(st, two)[0]["median"] == -3.0 and _same_stats(st, np.ascontiguousarray(two.T))[0]["median"] == -3.0


def test_statistics_of_empty_and_nearly_empty_channels(st):
    rng = np.random.default_rng(20)
    d = _image(rng, 33, 65, 3)
    d[..., 1] = np.nan
    d[::2, :, 2], d[1::2, :, 2] = np.inf, -np.inf
    got = _same_stats(st, d, quantiles=(0.5,))
    assert got[1].tobytes() == bytes(40) and got[2].tobytes() == bytes(40) and got[0]["count"] > 0
    nothing = np.zeros((33, 65), F)
    nothing[3, 4] = -1.0
    got = _same_stats(st, _image(rng, 33, 65, 4), nothing, (0.1, 0.9), device=True)
    assert got.tobytes() == bytes(120)
    one = nothing.copy()
    one[17, 40] = 1e-30
    got = _same_stats(st, _image(rng, 33, 65, 3, special=False), one, (0.0, 1.0), mask_device=True)
    assert (got["count"] == 1).all() and (got["mad"] == 0).all() and (got["min"] == got["max"]).all()
    allnan = np.full((5, 7, 3), np.nan, F)
    assert _same_stats(st, allnan).tobytes() == bytes(120)


def test_statistics_of_negative_values_and_both_zeros(st):
    rng = np.random.default_rng(21)
    d = (-np.abs(_image(rng, 33, 64, 3, special=False)) - F(1e-3)).astype(F)
    got = _same_stats(st, d, quantiles=(0.25, 0.75))
    assert (got["max"] < 0).all()
    zeros = np.where(rng.random((33, 65)) < 0.5, F(0.0), F(-0.0)).astype(F)     # -0 counts as +0: min, max and median are +0
    got = _same_stats(st, zeros, quantiles=(0.0, 1.0))
    assert not np.signbit(got["min"]).any() and not np.signbit(got["max"]).any() and not np.signbit(got["median"]).any() and not np.signbit(got["q"]).any()
    mixed = np.concatenate([np.full(20, -0.0, F), np.full(21, 0.0, F), -np.abs(rng.standard_normal(40)).astype(F) - F(0.5), np.abs(rng.standard_normal(40)).astype(F) + F(0.5)])
    got = _same_stats(st, rng.permutation(mixed).reshape(11, 11), quantiles=(0.33, 0.5, 0.66))
    assert got[0]["median"] == 0 and not np.signbit(got[0]["median"])
    scales = np.stack([rng.standard_normal((35, 67)) * s for s in (1e-30, 1.0, 1e30)], 2).astype(F)
    scales[np.abs(scales) < 1.2e-38] = 0
    _same_stats(st, scales, quantiles=(0.01, 0.99), padded=True, device=True)


def test_statistics_under_heavy_ties(st):
    rng = np.random.default_rng(22)
    h, w = 33, 65
    n = h * w
    const = np.full((h, w, 3), 12.5, F)
    got = _same_stats(st, const, quantiles=(0.0, 0.3, 1.0))
    assert (got["mad"] == 0).all() and (got["median"] == 12.5).all()
    more = rng.standard_normal(n).astype(F)
    more[:n // 2 + 5] = 0.75                                                    # more than half equal: MAD 0
    assert _same_stats(st, rng.permutation(more).reshape(h, w), device=True)[0]["mad"] == 0
    for low in (True, False):                                                   # exactly half equal, below and above the rest
        even = np.abs(rng.standard_normal(n - 1)).astype(F) + F(1.0)
        even[:(n - 1) // 2] = 0.5 if low else 9.0
        got = _same_stats(st, rng.permutation(even).reshape(32, 67), quantiles=(0.5,), what=low)
        assert got[0]["count"] == n - 1 and (got[0]["median"] == 0.5) == low
    few = rng.integers(0, 3, (37, 66, 3)).astype(F)
    _same_stats(st, few, quantiles=(0.1, 0.5, 0.9), padded=True)


def _bands(bits, n=4811, negate=False, rng=None):
    """values with the bit patterns `bits` (ascending, positive floats) in the proportions 40 % / 30 % / 30 %, shuffled: the
    lower median is the middle one"""
    v = np.array(bits, np.uint32).view(F)
    a = np.concatenate([np.full(n * 4 // 10, v[0], F), np.full(n * 3 // 10, v[1], F), np.full(n - n * 4 // 10 - n * 3 // 10, v[2], F)])
    return (rng or np.random.default_rng(1)).permutation(-a if negate else a)


BOUNDARIES = [(0x3FFFFFFC, 0x40000000, 0x40000004),      # the first value of the digits of rounds 1, 2 and 3
              (0x3FFFFFF8, 0x3FFFFFFC, 0x40000000),      # the last value of the digits of rounds 1 and 2
              (0x3F80FFFF, 0x3F810000, 0x3F810001),      # ..FFFF / ..0000: the prefix changes below the median
              (0x3F7FFFFE, 0x3F7FFFFF, 0x3F800000),      # the last value of the last digit: ..FF, beside 1.0
              (0x3F7FFFFF, 0x3F800000, 0x3F800001),      # 1.0: the digits of rounds 1 .. 3 change below the median
              (0x3EFFFFFF, 0x3F000000, 0x3F000001),      # the first value of a digit of round 0
              (0x3EFFFFFE, 0x3EFFFFFF, 0x3F000000),      # the last value of a digit of round 0
              (0x3F012300, 0x3F012301, 0x3F012302)]      # keys that differ only in the last digit


@pytest.mark.parametrize("bits", BOUNDARIES)
def test_statistics_on_the_digit_boundaries_of_the_radix_rounds(st, bits):
    rng = np.random.default_rng(30)
    for negate in (False, True):                                                # (negated, the order and the keys' bits are reversed)
        a = _bands(bits, negate=negate, rng=rng)
        d = a.reshape(17, 283)
        got = _same_stats(st, d, quantiles=(0.4, 0.4 + 1e-4, 0.7, 0.7 + 1e-3), device=negate, what=[hex(b) for b in bits])
        assert int(np.abs(got[0]["median"]).view(np.uint32)) == bits[1]          # the case is what it says
    # the MAD on the same keys: one zero, the bands with both signs: the median is 0 and the deviations are the bands
    amp = np.sort(_bands(bits, n=2405, rng=rng))
    sym = rng.permutation(np.concatenate([[F(0)], amp, -amp]).astype(F))
    got = _same_stats(st, sym.reshape(17, 283), quantiles=(0.5,))
    assert got[0]["median"] == 0 and int(got[0]["mad"].view(np.uint32)) == bits[1]
    both = np.stack([_bands(bits, rng=rng).reshape(17, 283), sym.reshape(17, 283), _bands(bits, negate=True, rng=rng).reshape(17, 283)], 2)
    _same_stats(st, both, quantiles=(0.3, 0.71), padded=True, what="three channels")


def test_the_median_in_the_first_and_in_the_last_bin(st):
    """keys begin with 0x00 for finite values below -1.7e38 and with 0xFF for those above 1.7e38"""
    rng = np.random.default_rng(31)
    big = rng.uniform(1.8e38, 3.3e38, (33, 65)).astype(F)
    for d in (big, -big, np.stack([big, -big, big[::-1]], 2)):
        got = _same_stats(st, d, quantiles=(0.0, 1.0, 0.5))
        assert (np.abs(got["median"]) > 1.7e38).all()
    lo = np.where(rng.random((33, 65)) < 0.6, -big, F(1.0)).astype(F)            # the median in the first bin, the rest elsewhere
    assert _same_stats(st, lo, quantiles=(0.9,), device=True)[0]["median"] < -1.7e38
    hi = np.where(rng.random((33, 65)) < 0.6, big, F(-1.0)).astype(F)
    assert _same_stats(st, hi, quantiles=(0.1,))[0]["median"] > 1.7e38


@functools.lru_cache(maxsize=None)
def _tall():
    rng = np.random.default_rng(32)
    d = (0.02 + 0.01 * rng.standard_normal((16500, 3, 3))).astype(F)
    d[5, 1], d[16499, 2, 0] = np.nan, np.inf
    return d, sr.stats(d, None, (0.25, 0.999))


def test_statistics_of_more_rows_than_one_sweep_of_the_grid_covers(st):
    """a narrow image's grid is 1 x 1024 workgroups of 4 rows: 16 500 rows need four more sweeps"""
    d, want = _tall()
    assert st.image_stats(d, quantiles=(0.25, 0.999)).tobytes() == want.tobytes()
    assert st.image_stats(_place(d, True, True), quantiles=(0.25, 0.999)).tobytes() == want.tobytes()


@pytest.mark.parametrize("form", ["direct", "merged"])
def test_both_forms_of_the_histogram_kernel_equal_the_restatement(st, form, monkeypatch):
    """STK_STRETCH_HIST_FORM (stretch.cpp) forces one LDS atomic per key or one per run of equal digits of a thread (where a
    channel has one histogram: round 0, the MAD's rounds, and every round of a call without quantiles): whichever is the
    default, both give the restatement's bits. A thread's samples are rows 4 x the grid's height apart in one column."""
    monkeypatch.setenv("STK_STRETCH_HIST_FORM", form)
    rng = np.random.default_rng(33)
    for k, (w, h, cn) in enumerate(((1, 1, 1), (2, 1, 3), (1, 2, 4), (63, 5, 4), (64, 33, 3), (65, 33, 1), (129, 33, 3), (5, 1201, 3))):
        d = _image(rng, h, w, cn)
        _same_stats(st, d, padded=bool(k & 1), device=bool(k & 2), what=(form, w, h, cn))
        _same_stats(st, d, (rng.random((h, w)) - 0.4).astype(F), padded=bool(k & 2), device=bool(k & 1), what=(form, w, h, cn, "mask"))
        _same_stats(st, d, quantiles=(0.1, 0.9), what=(form, w, h, cn, "quantiles"))
    runs = np.repeat(rng.integers(0, 4, (40, 3, 1)), 50, 0).reshape(2000, 3).astype(F) * F(0.25)      # long runs of equal values down every column
    runs[::397] = np.nan
    _same_stats(st, np.stack([runs, runs[::-1], -runs], 2), what=(form, "runs"))
    _same_stats(st, runs, (np.arange(2000)[:, None] % 7 > 0).astype(F) * np.ones((1, 3), F), what=(form, "runs", "mask"))
    test_statistics_under_heavy_ties(st)
    test_statistics_of_empty_and_nearly_empty_channels(st)
    test_the_median_in_the_first_and_in_the_last_bin(st)
    for bits in BOUNDARIES:
        test_statistics_on_the_digit_boundaries_of_the_radix_rounds(st, bits)
    test_statistics_of_more_rows_than_one_sweep_of_the_grid_covers(st)


# ---- 2. the stretch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", list(DEPTHS))
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_stretch_of_sizes_channels_curves_and_colour_modes(st, cn, depth):
    rng = np.random.default_rng(100 + cn + depth)
    for k, ((w, h), curve, colour) in enumerate(itertools.product(SMALL + SIZES, (STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE), (0, 1))):
        if (w, h) in SIZES and (k // 6 + curve + colour) % 3:                   # every small size fully; of the larger, every size under two of the six
            continue
        d = _image(rng, h, w, cn)
        p, kw = _random_stretch(rng, curve, colour, depth, TABLES[(2, 37, 65536)[k % 3]] if curve == STRETCH_TABLE else None)
        _check_stretch(st, d, p, kw, padded=bool(k & 1), device=bool(k & 2), what=(w, h, cn, depth, curve, colour))


@pytest.mark.parametrize("curve", [STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE])
def test_stretch_at_the_edges_of_the_definition(st, curve):
    rng = np.random.default_rng(40 + curve)
    black, white = F(0.015625), F(0.765625)
    h, w = 5, 67
    d = _image(rng, h, w, 3)
    d[0, :12] = np.array([black, white, np.nextafter(black, F(-1)), np.nextafter(black, F(1)), np.nextafter(white, F(0)), np.nextafter(white, F(2)), -5.0, 5.0,
                          np.nan, np.inf, -np.inf, -0.0], F)[:, None]
    d[1, :4] = black                                                           # L = 0 in colour mode: every x is 0
    d[1, 4:8] = [black, black, -1.0]                                           # ... and with channels below black
    d[1, 8] = [np.nan, np.nan, np.nan]
    d[2, :5] = [[white, black, black], [black, white, black], [white, white, white], [np.inf, 0.3, 0.1], [0.4, np.nan, 0.2]]
    for colour, depth in itertools.product((0, 1), DEPTHS):
        tab = TABLES[65536] if colour else TABLES[2]
        for mid in (0.5, 0.01, 0.25, 0.99):
            kw = dict(curve=curve, colour=colour, out_depth=depth, black=black, white=white, midtone=mid, out_scale=1.0, tab=tab if curve == STRETCH_TABLE else None)
            p = StretchParameters(curve=curve, colour=colour, out_depth=depth, black=float(black), white=float(white), midtone=mid, table=kw["tab"])
            got = _check_stretch(st, d, p, kw, device=bool(colour), what=(curve, colour, depth, mid))
            full = {DEPTH_U8: 255, DEPTH_U16: 65535, DEPTH_F32: 1.0}[depth]
            assert got[0, 0, 0] == 0 and abs(float(got[0, 1, 0]) - full) <= full * 2.0 ** -23 and got[0, 8, 0] == 0 and got[0, 10, 0] == 0
            if colour:
                assert not got[1, :9].any()
    # x exactly 1 reads the last interval of the table (i = K - 1), with 2 and with 65536 knots
    if curve == STRETCH_TABLE:
        ones = np.full((3, 5, 3), 1.0, F)
        for knots in (2, 65536):
            got = st.stretch_image(ones, StretchParameters(curve=STRETCH_TABLE, table=TABLES[knots]))
            assert (_np(got) == 1.0).all()
        ramp = np.linspace(0, 1, 4099, dtype=F).reshape(1, 4099)
        for knots, kind in ((2, CURVE_GAMMA), (65536, CURVE_GAMMA), (65536, CURVE_ASINH)):
            tab = stretch_table(kind, 2.2, knots)
            _check_stretch(st, ramp, StretchParameters(curve=STRETCH_TABLE, table=tab, out_depth=DEPTH_U16), dict(curve=STRETCH_TABLE, out_depth=DEPTH_U16, tab=tab))


def test_rounding_half_to_even_and_saturation(st):
    k8 = np.arange(255, dtype=np.float64) + 0.5
    half8 = (k8 / 255).astype(F)
    half8 = half8[(half8 * F(255)).astype(F) == k8.astype(F)]                    # those whose product lands on .5 exactly
    k16 = np.arange(0, 65535, 97, dtype=np.float64) + 0.5
    half16 = (k16 / 65535).astype(F)
    half16 = half16[(half16 * F(65535)).astype(F) == k16.astype(F)]
    assert half8.size > 50 and half16.size > 50 and ((half8 * F(255)).astype(F) % 1 == 0.5).all()
    for depth, vals in ((DEPTH_U8, half8), (DEPTH_U16, half16)):
        d = np.concatenate([vals, [0.0, 1.0, 1.5, -0.5, np.nan, np.inf]]).astype(F).reshape(1, -1)
        p, kw = StretchParameters(curve=STRETCH_LINEAR, out_depth=depth), dict(curve=STRETCH_LINEAR, out_depth=depth)
        got = _check_stretch(st, d, p, kw, what=depth)
        if depth == DEPTH_U8:
            assert (got[0, :vals.size, 0] % 2 == 0).all()                        # ties go to the even neighbour
        full = 255 if depth == DEPTH_U8 else 65535
        assert got[0, -6:, 0].tolist() == [0, full, full, 0, 0, full]


@pytest.mark.parametrize("device", [False, True])
def test_outputs_the_caller_holds(st, device):
    rng = np.random.default_rng(50 + device)
    h, w = 33, 65
    for cn, (depth, dtype) in itertools.product((1, 3, 4), DEPTHS.items()):
        d = _image(rng, h, w, cn)
        d3 = d if cn > 1 else d[..., None]
        p, kw = _random_stretch(rng, STRETCH_MTF, int(cn == 3), depth)
        want = sr.stretch(d, **kw)
        for pad_in, pad_out in itertools.product((False, True), repeat=2):
            src = _place(d3.copy(), pad_in, device)
            out = _place(np.full((h, w, cn), 77, dtype), pad_out, device)
            assert st.stretch_image(src, p, out=out) is out
            _same_image(out, want, (cn, depth, pad_in, pad_out))
            assert _np(src).tobytes() == d3.tobytes()                            # the input is left as it was
            if depth == DEPTH_F32:                                              # in place: same pointer, same stride
                assert st.stretch_image(src, p, out=src) is src
                _same_image(src, want, (cn, pad_in, "in place"))
        if not device:                                                          # only pixel bytes are written
            big = np.full((h, w + 3, cn), 77, dtype)
            st.stretch_image(d3, p, out=big[:, :w])
            assert big[:, :w].tobytes() == want.tobytes() and (big[:, w:] == 77).all()
    if device:                                                                  # alpha: clamped, no black point and no curve
        d = _image(rng, 5, 9, 4)
        d[..., 3] = np.array([-1.0, 0.0, 0.25, 1.0, 2.0, np.nan, np.inf, -np.inf, 0.75], F)[None, :]
        got = _np(st.stretch_image(d, StretchParameters(black=0.01, white=0.5, midtone=0.1, out_scale=2.0)))
        assert got[0, :, 3].tolist() == [0.0, 0.0, 0.5, 2.0, 2.0, 0.0, 2.0, 0.0, 1.5]


@functools.lru_cache(maxsize=None)
def _tall_stretch():
    rng = np.random.default_rng(60)
    d = (0.02 + 0.01 * rng.standard_normal((262150, 5))).astype(F)
    kw = dict(curve=STRETCH_MTF, out_depth=DEPTH_U8, black=0.005, white=0.9, midtone=0.05)
    return d, sr.stretch(d, **kw)


def test_stretch_of_more_rows_than_one_sweep_of_the_grid_covers(st):
    """65535 workgroup rows cover 262 140 rows: 262 150 need a second sweep"""
    d, want = _tall_stretch()
    _same_image(st.stretch_image(d, StretchParameters(out_depth=DEPTH_U8, black=0.005, white=0.9, midtone=0.05)), want)


# ---- 3. the whole form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_the_whole_form_equals_its_parts(st, cn):
    rng = np.random.default_rng(70 + cn)
    h, w = 33, 129
    d = _image(rng, h, w, cn)
    mask = (rng.random((h, w)) - 0.3).astype(F)
    tab = TABLES[37]
    for k, (masked, linked, white_mode, (curve, colour, depth)) in enumerate(itertools.product((False, True), (0, 1), (0, 1, 2), ((STRETCH_MTF, 0, DEPTH_F32), (STRETCH_TABLE, 1, DEPTH_U16),
                                                                                                                           (STRETCH_LINEAR, 0, DEPTH_U8)))):
        auto = AutoStretchParameters(shadows_clip=-2.0, target_background=0.2, linked=linked, white_mode=white_mode, white=0.9, white_quantile=0.97)
        src = _place(d, bool(k & 1), bool(k & 2))
        m = mask if masked else None
        got, stats, used = st.auto_stretch_image(src, auto, curve=curve, colour=colour, out_depth=depth, out_scale=0.5, table=tab, mask=m, return_stats=True, return_params=True)
        # the parts, through the engine
        s2 = st.image_stats(src, mask=m, quantiles=(0.97,) if white_mode == 2 else ())
        assert stats.tobytes() == s2.tobytes()
        rule = stretch_auto(s2 if cn < 4 else np.concatenate([s2, np.zeros(1, STAT_DTYPE)]), auto)
        for name in ("black", "white", "midtone"):
            assert getattr(used, name).tobytes() == getattr(rule, name).tobytes()
        assert (used.curve, used.colour, used.out_depth, used.out_scale) == (curve, colour, depth, 0.5)
        rule.curve, rule.colour, rule.out_depth, rule.out_scale, rule.table = curve, colour, depth, 0.5, tab
        _same_image(got, _np(st.stretch_image(src, rule)), (k, "parts"))
        # and the restatement
        want, wst, _ = sr.auto_stretch(d, m, curve, colour, depth, 0.5, tab, 0.97, shadows_clip=-2.0, target_background=0.2, linked=linked, white_mode=white_mode, white=0.9)
        assert stats.tobytes() == wst.tobytes()
        _same_image(got, want, (k, "restatement"))
    plain = st.auto_stretch_image(d)
    _same_image(plain, sr.auto_stretch(d)[0])


# ---- 4. refusals that need a context --------------------------------------------------------------------------------
def test_refusals(st):
    import ctypes as C
    from libstacker_rs_amd import _ffi
    rng = np.random.default_rng(9)
    h, w = 20, 30
    d = _image(rng, h, w, 3, special=False)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(curve=3), dict(curve=-1), dict(colour=2), dict(colour=-1), dict(out_scale=nan), dict(out_scale=inf), dict(black=nan), dict(black=[0.0, inf]),
                dict(white=nan), dict(white=[1.0, 1.0, -inf]), dict(white=0.0), dict(black=0.5, white=0.25), dict(black=[0.0, 0.0, 2.0]), dict(midtone=0.0), dict(midtone=1.0),
                dict(midtone=nan), dict(midtone=[0.5, 0.5, -0.1]), dict(curve=STRETCH_TABLE, table=[0.0, 0.5, nan]), dict(curve=STRETCH_TABLE, table=[0.0, 0.5, 1.5]),
                dict(curve=STRETCH_TABLE, table=[0.0, -0.1, 1.0]), dict(curve=STRETCH_TABLE, table=[0.0, inf, 1.0]), dict(black=-3e38, white=3e38)):
        with pytest.raises(InvalidParams):
            st.stretch_image(d, StretchParameters(**bad))
    st.stretch_image(d, StretchParameters(curve=STRETCH_LINEAR, midtone=0.0))    # the midtone is read under MTF alone
    st.stretch_image(d[..., 0], StretchParameters(black=[0.0, nan, nan, nan]))   # the entries of channels the image does not have are not read

    class Reserved(StretchParameters):
        def _c(self):
            c = super()._c()
            c.reserved = 1
            return c
    with pytest.raises(InvalidParams):
        st.stretch_image(d, Reserved())
    for q in ([nan], [-0.1], [1.1], [inf], [0.5, 2.0]):
        with pytest.raises(InvalidParams):
            st.image_stats(d, quantiles=q)
    with pytest.raises(InvalidParams):
        st.image_stats(np.ones((h, w, 2), np.float32))                          # two channels
    with pytest.raises(InvalidParams):
        st.stretch_image(np.ones((h, w, 2), np.float32))
    for bad in (dict(shadows_clip=0.5), dict(target_background=0.0), dict(target_background=1.0), dict(white=nan), dict(linked=2), dict(white_mode=3),
                dict(white_quantile=1.5)):
        with pytest.raises(InvalidParams):
            st.auto_stretch_image(d, AutoStretchParameters(**bad))
    with pytest.raises(InvalidParams):
        st.auto_stretch_image(d, curve=7)
    with pytest.raises(InvalidParams):
        st.auto_stretch_image(d, out_scale=nan)
    # the output: geometry, location, depth, overlaps
    p = StretchParameters()
    for out in (np.zeros((h, w + 1, 3), F), np.zeros((h + 1, w, 3), F)[:h + 1], np.zeros((h, w), F), np.zeros((h, w, 4), F)):
        with pytest.raises(InvalidParams):
            st.stretch_image(d, p, out=out)
    import torch
    with pytest.raises(InvalidParams):
        st.stretch_image(d, p, out=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"))          # another location
    buf = np.zeros((h + 1, w, 3), F)
    buf[:h] = d
    with pytest.raises(InvalidParams):
        st.stretch_image(buf[:h], p, out=buf[1:])                               # shifted by a row
    wide = np.zeros((h, 2 * w, 3), F)
    with pytest.raises(InvalidParams):
        st.stretch_image(wide[:, :w], p, out=wide.reshape(2 * h, w, 3)[:h])     # the same pointer, another stride
    bytes_ = np.zeros((h, w, 3), F)
    with pytest.raises(InvalidParams):                                          # an 8-bit output over the image: only f32 may be in place
        st.stretch_image(bytes_, StretchParameters(out_depth=DEPTH_U8), out=bytes_.view(np.uint8).reshape(h, w * 4, 3)[:, :w])
    both = torch.zeros((h + 1, w, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(InvalidParams):
        st.stretch_image(both[:h], p, out=both[1:])
    img = _ffi.ImageF32(d.ctypes.data, w, h, 3, 0, 0)
    o = _ffi.ImageOut(np.zeros((h, w, 3), np.uint16).ctypes.data, w, h, 3, 16, 0, 0)
    pc = p._c()
    assert st._lib.stk_stretch(st._h, C.byref(img), C.byref(pc), None, 0, C.byref(o)) == 2              # the output's depth is not the parameters'
    assert st._lib.stk_stretch(st._h, C.byref(img), None, None, 0, C.byref(o)) == 2 and st._lib.stk_stretch(st._h, C.byref(img), C.byref(pc), None, 0, None) == 2
    keep = np.zeros((h, w, 3), np.uint16)
    o16 = _ffi.ImageOut(keep.ctypes.data, w, h, 3, 16, 0, w * 6 + 1)
    pc.out_depth = 16
    assert st._lib.stk_stretch(st._h, C.byref(img), C.byref(pc), None, 0, C.byref(o16)) == 2            # a stride that is no multiple of the element
    o16.row_stride_bytes = w * 6 - 2
    assert st._lib.stk_stretch(st._h, C.byref(img), C.byref(pc), None, 0, C.byref(o16)) == 2            # ... or shorter than a row
    recs = np.zeros(4, STAT_DTYPE)
    assert st._lib.stk_image_stats(st._h, C.byref(img), None, 0, 0, None, 0, None) == 2
    assert st._lib.stk_image_stats(st._h, C.byref(img), None, 0, 0, None, 1, recs.ctypes.data_as(C.POINTER(_ffi.ImageStat))) == 2     # a count without quantiles
    assert st._lib.stk_image_stats(st._h, C.byref(img), None, 0, 0, None, 5, recs.ctypes.data_as(C.POINTER(_ffi.ImageStat))) == 2
    assert st._lib.stk_image_stats(st._h, C.byref(img), C.c_void_p(d.ctypes.data), 2, 0, None, 0, recs.ctypes.data_as(C.POINTER(_ffi.ImageStat))) == 2    # a mask stride below a row
    assert st._lib.stk_image_stats(st._h, C.byref(img), C.c_void_p(d.ctypes.data), 0, 5, None, 0, recs.ctypes.data_as(C.POINTER(_ffi.ImageStat))) == 2    # a mask location
    over = _ffi.ImageF32(recs.ctypes.data, 5, 2, 3, 0, 0)                        # the records over the image
    assert st._lib.stk_image_stats(st._h, C.byref(over), None, 0, 0, None, 0, recs.ctypes.data_as(C.POINTER(_ffi.ImageStat))) == 2
    huge = _ffi.ImageF32(d.ctypes.data, 1 << 16, 1 << 15, 1, 0, 0)               # width * height = 2^31
    assert st._lib.stk_image_stats(st._h, C.byref(huge), None, 0, 0, None, 0, recs.ctypes.data_as(C.POINTER(_ffi.ImageStat))) == 2
    # the context is still good
    dev = torch.from_numpy(d).cuda()
    assert st.image_stats(dev).tobytes() == sr.stats(d).tobytes()
    _same_image(st.stretch_image(dev, p), sr.stretch(d))


# ---- 5. history independence ----------------------------------------------------------------------------------------
def test_the_same_bits_whatever_the_context_held(st):
    rng = np.random.default_rng(5)
    d = _image(rng, 50, 70, 3)
    mask = (rng.random((50, 70)) - 0.2).astype(F)
    p, _ = _random_stretch(rng, STRETCH_TABLE, 1, DEPTH_U16, TABLES[37])

    def run(s):
        out, stats, used = s.auto_stretch_image(d, AutoStretchParameters(white_mode=2), mask=mask, return_stats=True, return_params=True)
        return (out.tobytes() + stats.tobytes() + used.black.tobytes() + used.midtone.tobytes() + s.image_stats(d, quantiles=(0.1, 0.5, 0.9, 1.0)).tobytes()
                + s.stretch_image(d, p).tobytes())
    a = run(st)
    assert run(st) == a
    for byte in (0x00, 0xFF, 0x7F):
        st.set_option("debug_poison", byte)
        assert st.timing()["debug_poison_bytes"] > 0
        assert run(st) == a, "after debug_poison 0x%02X" % byte
    st.image_stats(_image(rng, 90, 150, 4), quantiles=(0.3,))                    # other counts, other prefixes
    assert run(st) == a
    st.wavelet_image(np.abs(_image(rng, 60, 80, 3, special=False)), WaveletParameters(levels=3, thresholds=2.0))
    assert run(st) == a
    fresh = Stacker(0)
    assert run(fresh) == a
    fresh.close()
    st.image_stats(d)
    t = st.timing()
    assert t["finalize_ms"] > 0.0 and t["prep_ms"] > 0.0

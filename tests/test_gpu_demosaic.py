"""Colour-filter mosaics on the GPU (include/stacker.h, "colour-filter mosaics"): stk_demosaic and stk_cfa_mask against the
numpy restatement (demosaic_restate.py), == on bytes (f32 with NaNs: equal bits where finite, NaN exactly where the
restatement has NaN), over shapes that straddle the 64 x 16 tile, the 2 x 2 cell and the reflection; padded and misaligned
rows in and out with every non-pixel byte checked; independence of what the context held before; stream ordering into
ecc_match; Bayer drizzle as the composition it is defined to be; every refusal; calibrate -> demosaic against the
restatements composed."""
import ctypes as C
import itertools

import numpy as np
import pytest

import calibrate_restate as cr
import demosaic_restate as dr
from libstacker_rs_amd import (CalibrationParameters, DrizzleParameters, EccMatchParameters, MotionType, Stacker, _ffi, synth)
from test_gpu_calibrate import SENTINEL, _dev, _np, _views

pytestmark = pytest.mark.gpu

F = np.float32
DT = dr.DTYPES
SHAPES = [(3, 3), (4, 3), (5, 4), (63, 15), (64, 16), (65, 17), (67, 33), (131, 97), (200, 50)]         # w x h
DEPTHS = [(8, 8), (8, 32), (16, 16), (16, 32), (32, 32)]
NS = (1, 3, 5)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _mosaics(depth, n, w, h, seed=0):
    rng = np.random.default_rng(seed * 7919 + depth * 131 + n + w * 3 + h)
    if depth == 32:
        return rng.normal(100, 60, (n, h, w)).astype(F)
    return rng.integers(0, (1 << depth), (n, h, w)).astype(DT[depth])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth,od", DEPTHS)
def test_every_shape_pattern_and_method_is_the_restatement(st, depth, od, device):
    for k, ((w, h), pattern, method) in enumerate(itertools.product(SHAPES, dr.PATTERNS, dr.METHODS)):
        n = NS[(k // 16 + k) % 3]                                    # every n with every shape, pattern and method over the grid
        m = _mosaics(depth, n, w, h, k)
        got = _np(st.demosaic(_dev(m) if device else m, pattern, method, out_depth=od))
        assert dr.same_bits(got, dr.demosaic(m, pattern, method, od)), (w, h, pattern, method, n)


def test_every_n_meets_every_method_and_pattern(st):
    for n, pattern, method in itertools.product(NS, dr.PATTERNS, dr.METHODS):
        m = _mosaics(16, n, 67, 33, n)
        assert dr.same_bits(_np(st.demosaic(_dev(m), pattern, method)), dr.demosaic(m, pattern, method)), (n, pattern, method)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("depth,od", DEPTHS)
def test_padded_and_misaligned_rows_in_and_out(st, depth, od, device):
    """Odd base offsets and strides that are no multiple of 4 (in elements: 1, 2, 3 and 5, 3, 1, 7), sentinels in whole
    buffers: only pixel bytes change, the planes and their padding not at all."""
    layouts = [(1, 5, 1, 5), (2, 3, 3, 1), (0, 0, 1, 7), (3, 1, 0, 0)]
    for k, ((w, h), layout, method) in enumerate(itertools.product([(65, 17), (5, 4), (64, 16)], layouts, dr.METHODS)):
        io, ip, oo, op = layout
        pattern, n = k % 4, NS[k % 3]
        m = _mosaics(depth, n, w, h, 100 + k)
        fin, ibuf, _ = _views(m[..., None], io, ip, device)
        before = _np(ibuf).copy()
        ow, oh = (w // 2, h // 2) if method == dr.SUPERPIXEL else (w, h)
        outs, obuf, fill = _views(np.zeros((n, oh, ow, 3), DT[od]), oo, op, device)
        assert st.demosaic(fin, pattern, method, out_depth=od, out=outs) is outs
        want = dr.demosaic(m, pattern, method, od)
        assert dr.same_bits(np.stack([_np(o) for o in outs]), want), (w, h, layout, method)
        wbuf = fill(want)
        gbuf = _np(obuf)
        if od == 32:                                                # NaN-free inputs: bytes throughout
            assert not np.isnan(want).any()
        assert np.array_equal(gbuf, wbuf), (w, h, layout, method)
        assert np.array_equal(_np(ibuf), before)


@pytest.mark.parametrize("depth", [8, 16])
def test_extremes(st, depth):
    top = (1 << depth) - 1
    yy, xx = np.mgrid[0:33, 0:67]
    boards = np.stack([((xx + yy) & 1) * top, ((xx + yy + 1) & 1) * top, (xx & 1) * top, (yy & 1) * top,
                       (((xx >> 1) + (yy >> 1)) & 1) * top, np.full_like(xx, top)]).astype(DT[depth])
    spike = np.zeros((2, 33, 67), DT[depth])
    spike[0, 16, 30] = spike[0, 0, 0] = spike[0, 32, 66] = spike[0, 15, 63] = top
    spike[1] = top - spike[0]
    m = np.concatenate([boards, spike])
    for od, pattern, method in itertools.product((depth, 32), dr.PATTERNS, dr.METHODS):
        assert dr.same_bits(_np(st.demosaic(_dev(m), pattern, method, out_depth=od)), dr.demosaic(m, pattern, method, od)), (od, pattern, method)


def test_non_finite_f32(st):
    m = _mosaics(32, 3, 67, 33, 5)
    m[0, 10, 20], m[0, 0, 0], m[1, 32, 66], m[1, 16, 63], m[2, 5, 5], m[2, 6, 6] = np.nan, np.inf, -np.inf, np.nan, 3e38, -3e38
    for device, pattern, method in itertools.product((False, True), dr.PATTERNS, dr.METHODS):
        got = _np(st.demosaic(_dev(m) if device else m, pattern, method))
        want = dr.demosaic(m, pattern, method)
        assert np.isnan(want).any() and dr.same_bits(got, want), (device, pattern, method)


# ---- independence of what the context held, in the manner of test_gpu_history.py ---------------------------------------------
def _cases():
    m8, m16, mf = _mosaics(8, 3, 131, 97, 1), _mosaics(16, 5, 67, 33, 2), _mosaics(32, 3, 65, 17, 3)
    return [("u8 MHC host", lambda s: s.demosaic(m8, dr.GRBG, dr.MHC)), ("u8 MHC resident", lambda s: s.demosaic(_dev(m8), dr.GRBG, dr.MHC)),
            ("u16 HA to f32 host", lambda s: s.demosaic(m16, dr.BGGR, dr.HA, out_depth=32)),
            ("u16 HA to f32 resident", lambda s: s.demosaic(_dev(m16), dr.BGGR, dr.HA, out_depth=32)),
            ("f32 bilinear host", lambda s: s.demosaic(mf, dr.RGGB, dr.BILINEAR)), ("f32 superpixel resident", lambda s: s.demosaic(_dev(mf), dr.GBRG, dr.SUPERPIXEL)),
            ("mask host", lambda s: s.cfa_mask(131, 97, dr.GBRG, 1)), ("mask resident", lambda s: s.cfa_mask(131, 97, dr.GBRG, 1, device=True))]


def test_results_do_not_depend_on_what_the_context_held(st):
    cases = _cases()
    fresh = []
    for name, run in cases:
        s = Stacker(0)                                              # a context made for the call alone
        fresh.append(_np(run(s)).tobytes())
        s.close()
    neighbour = _mosaics(16, 2, 200, 50, 9)
    for (name, run), want in zip(cases, fresh):
        for byte in (0xFF, 0x7F):
            st.set_option("debug_poison", byte)
            assert _np(run(st)).tobytes() == want, (name, "after debug_poison 0x%02X" % byte)
        st.demosaic(neighbour, dr.RGGB, dr.HA, out_depth=32)       # another geometry, host-fed: ctx->frames and ctx->local regrow
        st.cfa_mask(7, 5, 0, 0)
        assert _np(run(st)).tobytes() == want, (name, "after a neighbour call")
        st.demosaic(_dev(neighbour), dr.BGGR, dr.MHC)
        assert _np(run(st)).tobytes() == want, (name, "after a resident neighbour call")


def test_device_outputs_go_straight_into_ecc_match(st):
    """The outputs of a resident demosaic handed on without a host round trip give the bits their host copies give on a
    fresh context: the call is complete when it returns."""
    frames, _ = synth.make_stack(3, 256, 192)
    mosaics = np.stack([dr.mosaic_of(f, dr.RGGB) for f in frames.numpy()])
    params = EccMatchParameters(MotionType.Homography, 50, 1e-4, 5)
    bgr = st.demosaic(_dev(mosaics), dr.RGGB, dr.MHC)
    image, stats = st.ecc_match(bgr, params, return_stats=True)
    assert dr.same_bits(_np(bgr), dr.demosaic(mosaics, dr.RGGB, dr.MHC))
    fresh = Stacker(0)
    image2, stats2 = fresh.ecc_match(_np(bgr), params, return_stats=True)
    fresh.close()
    assert _np(image).tobytes() == _np(image2).tobytes()
    assert [np.asarray(s["warp"]).tobytes() for s in stats] == [np.asarray(s["warp"]).tobytes() for s in stats2]
    assert [s["iterations"] for s in stats] == [s["iterations"] for s in stats2]


# ---- the mask and Bayer drizzle ----------------------------------------------------------------------------------------------
def test_cfa_mask(st):
    for (w, h), pattern, channel in itertools.product(SHAPES + [(1, 1), (300, 2)], dr.PATTERNS, range(3)):
        want = dr.cfa_mask(w, h, pattern, channel)
        host = st.cfa_mask(w, h, pattern, channel)
        dev = st.cfa_mask(w, h, pattern, channel, device=True)
        assert isinstance(host, np.ndarray) and dev.is_cuda and host.dtype == F
        assert np.array_equal(host, want) and np.array_equal(_np(dev), want), (w, h, pattern, channel)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_cfa_drizzle_stack_is_its_three_drizzles(st, device):
    n, w, h, pattern = 3, 67, 33, dr.GRBG
    m = _mosaics(8, n, w, h, 4)
    warps = np.tile(np.eye(3), (n, 1, 1))
    warps[1, 0, 2], warps[1, 1, 2], warps[2, 0, 2], warps[2, 1, 2] = 0.4, -0.7, -1.3, 0.6
    dz = DrizzleParameters(scale=2.0, pixfrac=0.6)
    put = _dev if device else (lambda a: a)
    image, den = st.cfa_drizzle_stack(put(m), warps, pattern, dz)
    image, den = _np(image), _np(den)
    assert image.shape == den.shape == (2 * h, 2 * w, 3)
    garbage = np.random.default_rng(8).integers(0, 256, m.shape).astype(np.uint8)
    for c in range(3):
        mask = dr.cfa_mask(w, h, pattern, c)
        one, one_den = st.drizzle_stack(put(m), warps, dz, maps=[put(mask)] * n, return_den=True)
        assert _np(one).reshape(2 * h, 2 * w).tobytes() == image[..., c].tobytes() and _np(one_den).tobytes() == den[..., c].tobytes()
        other = np.where(mask > 0, m, garbage)                      # every sample of the other colours replaced
        image_g, den_g = st.cfa_drizzle_stack(put(other), warps, pattern, dz)
        assert _np(image_g)[..., c].tobytes() == image[..., c].tobytes() and _np(den_g)[..., c].tobytes() == den[..., c].tobytes()
    # identity warps, scale 1, pixfrac 1: den is n at own-colour sites and 0 elsewhere, and the image is the mean there
    same = np.repeat(m[:1], n, 0)
    image, den = st.cfa_drizzle_stack(put(same), np.tile(np.eye(3), (n, 1, 1)), pattern, DrizzleParameters(scale=1.0, pixfrac=1.0), alpha=1.0)
    image, den = _np(image), _np(den)
    for c in range(3):
        own = dr.cfa_mask(w, h, pattern, c) > 0
        assert np.array_equal(den[..., c], np.where(own, F(n), F(0)))
        assert np.array_equal(image[..., c][own], same[0][own].astype(F))
    assert [int(round(float(den[..., c].sum() / n))) for c in range(3)] == [int(dr.cfa_mask(w, h, pattern, c).sum()) for c in range(3)]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(st):
    lib, ctx = st._lib, st._h
    INVALID, NOT_IMPLEMENTED = 2, 7
    plane = np.zeros((2, 5, 40), np.uint8)                           # rows of 7 inside rows of 40: room for every stride below
    out = np.zeros((2, 5, 7, 3), F)

    def call(n=2, w=7, h=5, depth=8, location=0, pattern=0, stride=0, method=1, od=8, ostride=0, data=True, outs=True, ptrs=None, optrs=None, mosaic=True):
        ptrs = ptrs if ptrs is not None else [plane[i].ctypes.data for i in range(2)]
        optrs = optrs if optrs is not None else [out[i].ctypes.data for i in range(2)]
        pa = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        oa = (C.c_void_p * max(len(optrs), 1))(*optrs)
        mo = _ffi.Mosaic(C.cast(pa, C.POINTER(C.c_void_p)) if data else None, n, w, h, depth, location, pattern, stride)
        status = lib.stk_demosaic(ctx, C.byref(mo) if mosaic else None, method, od, C.cast(oa, C.c_void_p) if outs else None, ostride)
        return status, lib.stk_last_error(ctx)

    assert call()[0] == 0
    bad = [dict(mosaic=False), dict(data=False), dict(outs=False), dict(ptrs=[plane[0].ctypes.data, None]), dict(optrs=[None, out[1].ctypes.data]),
           dict(n=0), dict(pattern=4), dict(pattern=-1), dict(method=4), dict(method=-1), dict(depth=12), dict(depth=0), dict(location=2),
           dict(od=16), dict(depth=16, od=8), dict(depth=32, od=8), dict(depth=32, od=16), dict(w=2), dict(h=2), dict(w=2, h=2, method=0), dict(w=1, method=3),
           dict(h=1, method=3), dict(stride=6), dict(depth=16, od=16, stride=15), dict(ostride=20), dict(od=32, ostride=7 * 12 + 2),
           dict(optrs=[plane[0].ctypes.data + 3, out[1].ctypes.data]), dict(optrs=[out[0].ctypes.data, plane[0].ctypes.data + 4 * 40 + 6], stride=40)]
    for kw in bad:
        status, msg = call(**kw)
        assert status == INVALID and msg, (kw, status, msg)
    big = np.zeros(4 * 40 + 7 + 5 * 7 * 3, np.uint8)                  # a plane with padded rows and, right behind its last sample, the output
    assert call(n=1, ptrs=[big.ctypes.data], optrs=[big.ctypes.data + 4 * 40 + 7], stride=40)[0] == 0
    assert call(n=1, ptrs=[big.ctypes.data], optrs=[big.ctypes.data + 4 * 40 + 6], stride=40)[0] == INVALID
    many = [plane[0].ctypes.data] * 65536
    status, msg = call(n=65536, ptrs=many, optrs=[out[0].ctypes.data] * 65536)
    assert status == NOT_IMPLEMENTED and msg, (status, msg)
    status, msg = call(w=3, h=65535 * 16 + 1)
    assert status == NOT_IMPLEMENTED and msg, (status, msg)
    assert call(w=4, h=65535 * 8 + 2, method=3)[0] == NOT_IMPLEMENTED
    mask = np.zeros((5, 7), F)
    p = C.c_void_p(mask.ctypes.data)
    assert lib.stk_cfa_mask(ctx, 7, 5, 3, 2, p, 0) == 0
    for args in [(7, 5, 0, 0, None, 0), (0, 5, 0, 0, p, 0), (7, 0, 0, 0, p, 0), (7, 5, 4, 0, p, 0), (7, 5, -1, 0, p, 0), (7, 5, 0, 3, p, 0),
                 (7, 5, 0, -1, p, 0), (7, 5, 0, 0, p, 2)]:
        assert lib.stk_cfa_mask(ctx, *args) == INVALID and lib.stk_last_error(ctx), args


# ---- the pipeline ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_calibrate_then_demosaic_is_the_restatements_composed(st, device):
    n, w, h, pattern = 3, 67, 33, dr.GBRG
    rng = np.random.default_rng(12)
    raw = rng.integers(0, 65536, (n, h, w, 1)).astype(np.uint16)
    bias = rng.uniform(0, 500, (h, w, 1)).astype(F)
    dark = rng.uniform(0, 300, (h, w, 1)).astype(F)
    flat = rng.uniform(0.5, 1.5, (h, w, 1)).astype(F)
    defects = (rng.random((h, w)) < 0.05).astype(np.uint8)
    defects[0, 0] = defects[h - 1, w - 1] = 1
    kw = dict(dark_scale=np.array([0.5, 1.0, 2.0], F), flat_mean=[1.0, 1.0, 1.0, 1.0], flat_min=0.25, pedestal=16.0)
    put = _dev if device else (lambda a: a)
    cal = CalibrationParameters(bias=put(bias), dark=put(dark), flat=put(flat), defects=put(defects), defect_step=2, out_depth=32, **kw)
    calibrated = st.calibrate(put(raw), cal)
    want_cal = cr.calibrate_restate(raw, bias, dark, flat, kw["dark_scale"], kw["flat_mean"], kw["flat_min"], kw["pedestal"], defects, 2, 32)
    assert cr.same_bits(_np(calibrated), want_cal)
    for method in dr.METHODS:
        got = _np(st.demosaic(calibrated, pattern, method))
        assert dr.same_bits(got, dr.demosaic(want_cal[..., 0], pattern, method)), method

"""Star measurement on the GPU (include/stacker.h, stk_star_measure_params): stk_star_measure against the numpy restatement
(tests/star_measure_restate.py) on every field of stk_star_shape, bit for bit, over depth x channels x size x placement x row
layout x ring geometry x stars per frame; the frame's edges; saturation and min_pixels; the header's consequences, engine
against engine; the same bits on a second call, after an unrelated call and on a caller's stream;
stk_star_match_quality_weighted against its five parts; the quality weights' effect on a stack; the refusals."""
import itertools

import numpy as np
import pytest

import libstacker_rs_amd as ls
import star_measure_restate as sm
from libstacker_rs_amd import (STAR_DTYPE, InvalidParams, NotEnoughFiles, Stacker, StarDeepParameters, StarMeasureParameters, StarParameters,
                               StarQualityParameters, synth)
from test_cpu_star_measure import quality_stack
from test_gpu_star_deep import F32, POPULATIONS, _frame, _np, _place, _speckle, _two_populations

pytestmark = pytest.mark.gpu
RINGS = [(2, 3, 3), (7, 10, 14), (12, 13, 16)]
SIZES = [(130, 70), (64, 64), (200, 129)]
COUNTS = [(130, 0, 5), (1, 3, 4), (4, 130, 1)]                             # stars per frame of the three frames of one launch


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _stars(pairs):
    s = np.zeros(len(pairs), STAR_DTYPE)
    if len(pairs):
        p = np.asarray(pairs).reshape(-1, 2)
        s["px"], s["py"] = p[:, 0], p[:, 1]
        s["x"], s["y"], s["flux"], s["peak"], s["npix"] = -1.0, 1e9, np.nan, -7, 12345      # only px and py are read
    return s


def _random_stars(rng, w, h, R, count):
    """`count` positions, most with the aperture inside the frame, about one in eight anywhere in or around it"""
    px, py = rng.integers(R, w - R, count), rng.integers(R, h - R, count)
    wild = rng.random(count) < 0.125
    px[wild], py[wild] = rng.integers(-3, w + 3, int(wild.sum())), rng.integers(-3, h + 3, int(wild.sum()))
    return _stars(np.stack([px, py], 1))


def _same(got, want, where=""):
    assert len(got) == len(want), (where, len(got), len(want))
    if got.tobytes() != want.tobytes():
        for f in got.dtype.names:
            bad = np.nonzero(~((got[f] == want[f]) | ((got[f] != got[f]) & (want[f] != want[f]))))[0]
            assert not len(bad), (where, f, int(bad[0]), got[bad[0]], want[bad[0]])
        raise AssertionError((where, "bytes differ"))


def _check(st, frames, stars, mp, deep, device, padded):
    got = st.star_measure([_place(f, padded, device) for f in frames], stars, mp, deep)
    measured = 0
    for k, (f, s) in enumerate(zip(frames, stars)):
        want = sm.measure(f, s, mp, deep)
        _same(got[k], want, "frame %d" % k)
        measured += int((want["flags"] == 0).sum())
    return got, measured


# depth x channels, each at the three sizes; ring geometry, placement, row layout and the stars per frame rotate
CASES = []
for i, (depth, cn) in enumerate(itertools.product((8, 16, 32), (1, 3, 4))):
    for j, (w, h) in enumerate(SIZES):
        CASES.append((depth, cn, w, h, RINGS[(i + j) % 3], (i + j) % 2, (i // 3 + i + j + 1) % 2, COUNTS[(i + 2 * j) % 3]))


@pytest.mark.parametrize("case", CASES, ids=["d%d-c%d-%dx%d-r%d-%s-%s-n%d" % (c[0], c[1], c[2], c[3], c[4][0], "dev" if c[5] else "host", "padded" if c[6] else "tight", c[7][0])
                                             for c in CASES])
def test_measure_equals_the_restatement(st, case):
    depth, cn, w, h, (R, Ri, Ro), device, padded, counts = case
    rng = np.random.default_rng(100000 * depth + 1000 * w + 10 * cn + R)
    keys = [_speckle(rng, h, w, depth) for _ in counts]
    keys[1] = keys[1] // 64 * 64                                            # many ties in the ring
    keys[2][:, : w // 2] = keys[2][0, 0]                                    # a plateau over half the frame: MAD 0 in its rings
    frames = [_frame(k, depth, cn, rng) for k in keys]
    stars = [_random_stars(rng, w, h, R, c) for c in counts]
    sat = 200 if depth == 8 else 40000
    total = 0
    for mp in (StarMeasureParameters(radius=R, ring_inner=Ri, ring_outer=Ro, min_pixels=1),
               StarMeasureParameters(radius=R, ring_inner=Ri, ring_outer=Ro, kappa=0.5, min_contrast=3, min_pixels=4, saturation=sat)):
        got, measured = _check(st, frames, stars, mp, F32, device, padded)
        total += measured
        assert [len(g) for g in got] == list(counts)
    assert total >= max(sum(counts) // 16, 2)                               # the case does exercise the sums and the derived values
    if depth > 8:                                                           # the ring's keys span several high bytes
        k = sm.sd.key(frames[0], F32)
        assert len(np.unique(k >> 8)) > 8


@pytest.mark.parametrize("depth,cn", [(8, 3), (16, 1), (32, 4)])
def test_edges_of_the_frame(st, depth, cn):
    w, h = 70, 50
    rng = np.random.default_rng(depth)
    f = _frame(_speckle(rng, h, w, depth), depth, cn, rng)
    for (R, Ri, Ro), device in zip(RINGS, (0, 1, 0)):
        mp = StarMeasureParameters(radius=R, ring_inner=Ri, ring_outer=Ro, min_pixels=1)
        inside = [(R, 25), (w - 1 - R, 25), (R, R), (w - 1 - R, R), (R, h - 1 - R), (w - 1 - R, h - 1 - R), (35, 25)]
        got, _ = _check(st, [f], [_stars(inside)], mp, F32, device, 1)
        dy, dx = np.mgrid[-Ro:Ro + 1, -Ro:Ro + 1]
        for s, (px, py) in zip(got[0], inside):                             # n_ring counted here, not taken from the restatement
            ring = (dx * dx + dy * dy >= Ri * Ri) & (dx * dx + dy * dy <= Ro * Ro) & (px + dx >= 0) & (px + dx < w) & (py + dy >= 0) & (py + dy < h)
            assert s["flags"] & 1 == 0 and s["n_ring"] == int(ring.sum()), (px, py)
        full = got[0][-1]["n_ring"]
        assert got[0][0]["n_ring"] < full and got[0][2]["n_ring"] < got[0][0]["n_ring"]
        # hand-planted entries outside: bit 0 and zeros, the other stars of the list unchanged
        outside = [(R - 1, 25), (-1, 25), (w, 25), (35, h + 5), (35, -2000000000), (2000000000, 25), (35, h - R)]
        mixed = [outside[0], inside[0], outside[1], outside[2], inside[6], outside[3], inside[2], outside[4], outside[5], inside[5], outside[6]]
        got2, _ = _check(st, [f], [_stars(mixed)], mp, F32, device, 0)
        for s, p in zip(got2[0], mixed):
            if p in outside:
                z = np.zeros((), ls.SHAPE_DTYPE)
                z["px"], z["py"], z["flags"] = p[0], p[1], 1
                assert s.tobytes() == z.tobytes(), p
            else:
                assert s.tobytes() == got[0][inside.index(p)].tobytes(), p


@pytest.mark.parametrize("ring", [RINGS[0], RINGS[2]], ids=["ro3", "ro16"])
@pytest.mark.parametrize("below", [0, 1], ids=["k", "k-1"])
def test_ring_median_rank_on_a_bin_boundary_and_extreme_keys(st, ring, below):
    """The selection's edge `x >= k && x - s < k` in a wave: the ring of the star at the centre of a 48 x 48 frame (the
    smallest ring, 4 pixels, and the largest radius) holds exactly k, or k - 1, keys in the lower of two high-byte bins, so bg
    is the last key of one bin or the first of the next. Second population set: the lower keys are all 0 and 65535 is
    present, so that |K - bg| reaches bin 255 of both levels."""
    R, Ri, Ro = ring
    rng = np.random.default_rng(10 * Ro + below)
    y, x = np.mgrid[0:48, 0:48]
    d2 = (x - 24) ** 2 + (y - 24) ** 2
    in_ring = (d2 >= Ri * Ri) & (d2 <= Ro * Ro)
    n = int(in_ring.sum())
    k = (n + 1) // 2
    assert (n == 4) if Ro == 3 else (n > 128)                                   # one key in four lanes; several keys in every lane
    mp = StarMeasureParameters(radius=R, ring_inner=Ri, ring_outer=Ro, kappa=1.0, min_contrast=1, min_pixels=1)
    for low, mid, top in POPULATIONS:
        K = mid + rng.integers(0, 256, (48, 48))
        K[d2 <= R * R] = np.maximum(mid + 8000 - 60 * d2[d2 <= R * R], mid)   # a star in the aperture
        K[in_ring] = _two_populations(rng, n, k - below, low, mid, top)
        f = K.astype(np.uint16)
        want = sm.measure(f, _stars([(24, 24)]), mp)[0]                     # the restatement alone: the rank does fall on the boundary
        assert want["n_ring"] == n and want["bg"] >> 8 == (mid if below else low) >> 8 and (K[in_ring].min() >> 8, K[in_ring].max()) == (low >> 8, top)
        for device, padded in ((1, 0), (0, 1)):
            _check(st, [f], [_stars([(24, 24)])], mp, None, device, padded)


def test_frames_narrower_than_the_ring(st):
    """5 x 5: the aperture of R = 2 fits at the centre alone, no ring pixel lies inside the frame: n_ring 0, bg 0, mad 0"""
    f = np.arange(25, dtype=np.uint16).reshape(5, 5) * 1000
    got, _ = _check(st, [f], [_stars([(2, 2), (1, 2), (2, 3)])], StarMeasureParameters(radius=2, ring_inner=3, ring_outer=16, min_pixels=1), None, 0, 0)
    assert got[0]["flags"].tolist() == [0, 1, 1] and (got[0][0]["n_ring"], got[0][0]["bg"], got[0][0]["peak"]) == (0, 0, 22000)


def test_saturation_and_min_pixels_flags(st):
    f, truth = sm.make_field(200, 150, 40, 1.6, seed=5, peaks=(400.0, 120000.0))
    lists = st.star_detect_deep([f], StarParameters())
    for mp in (StarMeasureParameters(saturation=65535), StarMeasureParameters(saturation=30000, min_pixels=70), StarMeasureParameters(min_pixels=400),
               StarMeasureParameters(min_contrast=65535)):
        got, _ = _check(st, [f], lists, mp, None, 1, 0)
        flags = got[0]["flags"]
        if mp.saturation:
            assert ((flags & 2) != 0).sum() >= 2 and ((flags & 2) == 0).sum() >= 10
            assert (((flags & 2) != 0) == (got[0]["peak"] >= mp.saturation)).all()
        if mp.min_pixels == 70:                                             # the middle of the restated npix of this field: 20 .. 112
            assert ((flags & 4) != 0).sum() >= 5 and ((flags & 4) == 0).sum() >= 5
        if mp.min_pixels == 400 or mp.min_contrast == 65535:
            assert ((flags & 4) != 0).all()
        assert (((flags & 4) != 0) == ((got[0]["npix"] < mp.min_pixels) | (got[0]["S"] == 0))).all()


def test_consequences_engine_against_engine(st):
    rng = np.random.default_rng(11)
    g = rng.integers(0, 24, (70, 130)).astype(np.uint8)
    pts = [(int(x), int(y)) for y, x in zip(rng.integers(8, 62, 12), rng.integers(8, 122, 12))]
    for x, y in pts:
        g[y - 1:y + 2, x - 1:x + 2] = rng.integers(60, 256)
    mp = StarMeasureParameters(radius=4, ring_inner=5, ring_outer=7, min_pixels=2)
    a = st.star_measure([g], [_stars(pts)], mp)[0]
    b = st.star_measure([g.astype(np.uint16)], [_stars(pts)], mp)[0]       # the one-channel u16 frame with the same values
    assert a.tobytes() == b.tobytes() and (a["flags"] == 0).sum() >= 8
    f16, _ = sm.make_field(200, 150, 40, 1.8, seed=6)
    lists = st.star_detect_deep([f16], StarParameters())
    a = st.star_measure([f16], lists)[0]
    b = st.star_measure([f16.astype(np.float32)], lists, None, StarDeepParameters(1.0))[0]   # an f32 frame holding the u16 values
    assert a.tobytes() == b.tobytes() and (a["flags"] == 0).sum() >= 20
    unit = (f16.astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    c = st.star_measure([unit], lists, None, StarDeepParameters(65535.0))[0]
    assert c.tobytes() == a.tobytes()


def test_same_bits_again_after_another_call_and_on_a_callers_stream(st):
    import torch
    rng = np.random.default_rng(3)
    frames = [_frame(_speckle(rng, 129, 200, 16), 16, 3, rng) for _ in range(3)]
    stars = [_random_stars(rng, 200, 129, 7, c) for c in (1300, 2, 40)]     # beyond detection's cap of 1024 stars
    dev = [torch.from_numpy(f).cuda() for f in frames]
    first = st.star_measure(dev, stars)
    assert sum(int((s["flags"] == 0).sum()) for s in first) > 50
    _same(first[0][-25:], sm.measure(frames[0], stars[0][-25:]), "the last stars of the long list")
    again = st.star_measure(dev, stars)
    # an unrelated call that uses the same workspaces with other contents, then a shorter list in the same slots
    other = [_frame(_speckle(rng, 70, 130, 8), 8, 1, rng) for _ in range(5)]
    st.star_detect_deep(other, StarParameters(min_pixels=1, max_stars=1024))
    st.star_measure(other, [_random_stars(rng, 130, 70, 2, 200) for _ in other], StarMeasureParameters(radius=2, ring_inner=3, ring_outer=4))
    third = st.star_measure(frames, stars)                                  # host frames this time
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        bound = Stacker(0)
        bound.use_torch_stream()
        fourth = bound.star_measure(dev, stars)
        bound.close()
    for other_result in (again, third, fourth):
        assert [a.tobytes() for a in other_result] == [a.tobytes() for a in first]


# ---- stk_star_match_quality_weighted against its parts --------------------------------------------------------------
def _blurred_stack(cn=3):
    """6 frames of one field, u16, 240 x 180, small known shifts; frames 2 and 4 blurred (sigma 2.8 against 1.5)"""
    shifts = [(0.0, 0.0), (1.5, -2.0), (-2.25, 1.0), (3.0, 2.5), (-1.0, -3.5), (2.0, 0.5)]
    sig = [1.5, 1.5, 2.8, 1.5, 2.8, 1.5]
    return [sm.make_field(240, 180, 40, s, seed=31, noise_seed=200 + i, channels=cn, shift=sh)[0] for i, (s, sh) in enumerate(zip(sig, shifts))], shifts


@pytest.mark.parametrize("device,coverage", [(0, True), (1, False)])
def test_match_quality_weighted_equals_its_parts(st, device, coverage):
    import torch
    frames, shifts = _blurred_stack()
    files = [torch.from_numpy(f).cuda() for f in frames] if device else frames
    sp, mp = StarParameters(), StarMeasureParameters()
    qp = StarQualityParameters(fwhm_max=5.0, fwhm_power=2, snr_power=1)
    u = np.array([1.0, 2.0, 1.0, 0.5, 1.0, 1.0], np.float32)
    dropped, rejected, out, cov, applied, quality, stats = st.star_match_quality_weighted(
        files, sp, None, mp, qp, coverage=coverage, weights=u, return_coverage=True, return_applied=True, return_quality=True, return_stats=True)
    # 1. the alignment
    d2, stats2 = st.star_align_deep(files, sp)
    assert dropped == d2 == 0 and [s["status"] for s in stats] == [0] * 6
    for a, b, sh in zip(stats, stats2, shifts):
        assert np.array_equal(a["warp"], b["warp"]) and a["n_inliers"] == b["n_inliers"]
        assert min(synth.corner_error(a["warp"], np.array([[1, 0, k * sh[0]], [0, 1, k * sh[1]], [0, 0, 1.0]]), 240, 180) for k in (1, -1)) <= 0.5
    # 2. - 3. detection, measurement, quality
    lists = st.star_detect_deep(files, sp)
    shapes = st.star_measure(files, lists, mp)
    q = ls.star_frame_quality(shapes)
    assert q.tobytes() == quality.tobytes()
    # 4. the weights: the two blurred frames fail fwhm_max
    w, inc, rej = ls.star_quality_weights(q, qp, reference=0, include=[s["status"] == 0 for s in stats], weights=u)
    assert rejected == rej == 2 and inc.tolist() == [1, 1, 0, 1, 0, 1]
    assert [a["weight"] for a in applied] == [float(x) for x in w] and w[2] == w[4] == 0.0 and w[1] > 0
    assert all(a["gain"].tolist() == [1.0] * 3 and a["offset"].tolist() == [0.0] * 3 for a in applied)
    # 5. the fold
    want, wcov = st.weighted_stack(files, [s["warp"] for s in stats], weights=w, include=inc, coverage=coverage, alpha=1.0 / 65535.0, return_coverage=True)
    assert np.array_equal(_np(out), _np(want)) and np.array_equal(_np(cov), _np(wcov))
    assert float(_np(out).max()) > 0.05


def test_quality_weights_sharpen_the_stack(st):
    """8 unmoved frames, two at sigma 1.3 and six at 2.6: the weighted stack's stars are narrower than the equal mean's.
    Measured on the MI355X: see DESIGN §4.30."""
    sig, frames = quality_stack()
    n = len(frames)
    lists = st.star_detect_deep(frames, StarParameters())
    shapes = st.star_measure(frames, lists)
    for f, l, s in zip(frames[:2], lists[:2], shapes[:2]):
        assert s.tobytes() == sm.measure(f, l).tobytes()
    q = ls.star_frame_quality(shapes)
    w, inc, rej = ls.star_quality_weights(q, StarQualityParameters(fwhm_power=2), reference=0)
    assert inc.all() and rej == 0 and w[:2].min() > 2.5 * w[2:].max()
    eye = [np.eye(3)] * n
    res = []
    for wts in (w, np.ones(n, np.float32)):
        img = _np(st.weighted_stack(frames, eye, weights=wts, alpha=1.0))    # ADU
        f = np.ascontiguousarray(img[..., 0] if img.ndim == 3 else img)
        deep = StarDeepParameters(1.0)
        stars = st.star_detect_deep([f], StarParameters(), deep)
        res.append(float(ls.star_frame_quality(st.star_measure([f], stars, None, deep))[0]["fwhm"]))
    print("median FWHM on the weighted stack %.3f px, on the equal mean %.3f px, ratio %.3f" % (res[0], res[1], res[0] / res[1]))
    assert res[0] < 0.95 * res[1]


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals(st):
    f, _ = sm.make_field(200, 150, 40, 1.6, seed=5, channels=3)
    frames = [f, f]
    lists = st.star_detect_deep(frames, StarParameters())
    M = StarMeasureParameters
    for kw in (dict(radius=1), dict(radius=13), dict(radius=10, ring_inner=10), dict(ring_inner=16, ring_outer=16), dict(ring_outer=9), dict(ring_outer=17),
               dict(kappa=-1.0), dict(kappa=float("nan")), dict(kappa=float("inf")), dict(min_contrast=0), dict(min_contrast=65536), dict(min_pixels=0),
               dict(saturation=-1), dict(saturation=65536)):
        with pytest.raises(InvalidParams):
            st.star_measure(frames, lists, M(**kw))
        with pytest.raises(InvalidParams):
            st.star_match_quality_weighted(frames, measure=M(**kw))

    class Reserved(StarMeasureParameters):
        def _c(self):
            c = super()._c()
            c.reserved = 1
            return c
    with pytest.raises(InvalidParams):
        st.star_measure(frames, lists, Reserved())
    okf = [x.astype(np.float32) for x in frames]
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(InvalidParams):
            st.star_measure(okf, lists, None, StarDeepParameters(f32_scale=scale))
        with pytest.raises(InvalidParams):
            st.star_match_quality_weighted(okf, deep=StarDeepParameters(f32_scale=scale))
    assert len(st.star_measure(frames, lists, None, StarDeepParameters(f32_scale=0.0))) == 2       # not read at depth 16
    import ctypes as C
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import _Marshalled
    m = _Marshalled(frames)
    dp, mp = StarDeepParameters()._c(), M()._c()
    tab, cnt, shp = np.zeros((2, 8), STAR_DTYPE), np.zeros(2, np.int32), np.zeros((2, 8), ls.SHAPE_DTYPE)
    sp = shp.ctypes.data_as(C.POINTER(_ffi.StarShape))
    call = lambda *a: st._lib.stk_star_measure(st._h, C.byref(m.c_frames), *a)
    tp, cp = C.c_void_p(tab.ctypes.data), C.c_void_p(cnt.ctypes.data)
    assert call(C.byref(dp), C.byref(mp), tp, cp, 8, sp) == 0
    assert call(None, C.byref(mp), tp, cp, 8, sp) == 2 and call(C.byref(dp), None, tp, cp, 8, sp) == 2
    assert call(C.byref(dp), C.byref(mp), None, cp, 8, sp) == 2 and call(C.byref(dp), C.byref(mp), tp, None, 8, sp) == 2
    assert call(C.byref(dp), C.byref(mp), tp, cp, 8, None) == 2
    assert call(C.byref(dp), C.byref(mp), tp, cp, 0, sp) == 2 and call(C.byref(dp), C.byref(mp), tp, cp, 4097, sp) == 2
    for bad in (-1, 9):
        cnt[1] = bad
        assert call(C.byref(dp), C.byref(mp), tp, cp, 8, sp) == 2
    with pytest.raises(NotEnoughFiles):
        st.star_measure([], [])
    # the whole-stack form: the parts' refusals
    Q = StarQualityParameters
    for q in (Q(fwhm_power=5), Q(ecc_power=-1), Q(snr_power=5), Q(min_measured=0), Q(fwhm_max=-1.0), Q(ecc_max=float("nan"))):
        with pytest.raises(InvalidParams):
            st.star_match_quality_weighted(frames, quality=q)
    for kw in (dict(alpha=float("nan")), dict(alpha=float("inf")), dict(params=StarParameters(radius=8)), dict(params=StarParameters(border_mode=7)),
               dict(params=StarParameters(border_mode=ls.BORDER_REPLICATE)),           # coverage = 1 needs BORDER_CONSTANT 0
               dict(weights=[1.0, -1.0]), dict(weights=[0.0, 0.0])):
        with pytest.raises(InvalidParams):
            st.star_match_quality_weighted(frames, **kw)
    with pytest.raises(NotEnoughFiles):
        st.star_match_quality_weighted(frames[:1])
    blank = np.full_like(f, 2000)
    with pytest.raises(InvalidParams, match="All images discarded"):
        st.star_match_quality_weighted([f, blank])
    # the reference frame without a measured star: the weights' refusal
    with pytest.raises(InvalidParams, match="star quality weights"):
        st.star_match_quality_weighted(frames, measure=M(min_contrast=65535))
    # the context is still usable
    dropped, rejected, out = st.star_match_quality_weighted(frames, coverage=False, params=StarParameters(border_mode=ls.BORDER_REPLICATE))
    assert (dropped, rejected) == (0, 0) and np.isfinite(_np(out)).all()

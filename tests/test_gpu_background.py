"""The background model on the GPU (include/stacker.h, stk_background_params): stk_background_cells against the numpy
restatement (tests/background_restate.py) in every field, over depths, channel counts, steps, clip rounds, masks, host and
device frames and padded, misaligned rows; special contents; stk_background_apply against the restatement bit for bit on
both of its paths; stk_background_flatten against its three parts; determinism; the CPU tests' planar and quality values on
the device; and the pipeline check: flattening does not cost star detection a star and puts the sky at the target."""
import itertools

import numpy as np
import pytest

import background_restate as br
from libstacker_rs_amd import BG_MEAN, BG_MODE, BackgroundParameters, InvalidParams, Stacker, StarDeepParameters, StarParameters, background_estimate
from test_cpu_background import PLANAR, QUALITY_BAR, planar_frame, planar_params, quality_params
from test_gpu_star_deep import POPULATIONS, _place, _two_populations

pytestmark = pytest.mark.gpu
DTYPES = {8: np.uint8, 16: np.uint16, 32: np.float32}
PAIRS = [(8, 8), (8, 32), (16, 16), (16, 32), (32, 32)]
SCALE = 16.0                                                              # the f32 cases: keys = rint(16 v)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _sky(rng, h, w, depth, cn):
    """A sky frame: a gradient, noise and a few bright blobs, per channel its own level; at depth 16 / 32 the keys of most
    windows straddle a high-byte boundary (2048); a fourth channel is noise."""
    y, x = np.mgrid[0:h, 0:w]
    base, sig, top = (100.0, 5.0, 255) if depth == 8 else (2000.0, 40.0, 65535)
    planes = []
    for c in range(min(cn, 3)):
        f = base * (1 + 0.1 * c) + 0.3 * sig * x / 8 + 0.2 * sig * y / 8 + rng.normal(0, sig, (h, w))
        for _ in range(6):
            sx, sy = rng.uniform(0, w), rng.uniform(0, h)
            f += 30 * sig * np.exp(-((x - sx) ** 2 + (y - sy) ** 2) / 4.5)
        planes.append(f)
    if cn == 4:
        planes.append(rng.uniform(0, top, (h, w)))
    f = np.stack(planes, -1) if cn > 1 else planes[0]
    if depth == 32:
        return (f / SCALE).astype(np.float32)
    return np.clip(np.rint(f), 0, top).astype(DTYPES[depth])


def _fields_equal(got, want, what):
    for name in ("n", "kept", "med", "mad", "lo", "hi", "sum", "sum2", "reserved"):
        assert (got[name] == want[name]).all(), (what, name, np.argwhere(got[name] != want[name])[:3].tolist())


# ---- 1. the records against the restatement -------------------------------------------------------------------------
#          (w, h, step, n, clip_iters, mask, device, padded)
CELL_CASES = [(150, 100, 32, 3, 3, 1, 1, 0), (150, 100, 16, 1, 0, 0, 0, 1), (70, 70, 16, 17, 1, 1, 1, 1), (257, 130, 64, 1, 5, 1, 0, 0),
              (257, 130, 128, 1, 3, 0, 1, 0), (3, 3, 16, 3, 3, 0, 0, 0), (3, 3, 128, 1, 1, 1, 1, 1), (70, 70, 32, 1, 5, 0, 1, 0)]


@pytest.mark.parametrize("depth,cn", list(itertools.product((8, 16, 32), (1, 3, 4))))
def test_cells_equal_the_restatement(st, depth, cn):
    rng = np.random.default_rng(100 * depth + cn)
    for w, h, step, n, clip, masked, device, padded in CELL_CASES:
        p = BackgroundParameters(step=step, clip_iters=clip, kappa=2.5, f32_scale=SCALE)
        frames = [_sky(rng, h, w, depth, cn) for _ in range(min(n, 3))]
        frames = (frames * 6)[:n]                                            # 17 frames: the first three, repeated
        mask = None
        if masked:
            mask = (rng.random((h, w)) < 0.1).astype(np.uint8)
            ax, bx = br.window(1, step, w)
            ay, by = br.window(min(1, br.grid(w, h, step)[1] - 1), step, h)
            if ax <= bx:
                mask[ay:by + 1, ax:bx + 1] = 255                             # the window of node (1, 1), or (0, 1), fully masked
        m = mask
        if masked and device:
            import torch
            m = torch.from_numpy(mask).cuda()
        got = st.background_cells([_place(f, padded, device) for f in frames], p, m)
        gw, gh = br.grid(w, h, step)
        assert got.shape == (n, gh, gw, min(cn, 3))
        want = [br.cells_restate(f, p, mask) for f in frames[:3]]
        for i in range(n):
            _fields_equal(got[i], want[i % 3], (w, h, step, i))
        if masked and bx >= ax and w > 3:
            assert (got[0]["n"][min(1, gh - 1), 1] == 0).all() and (got[0]["n"] > 0).any()
        if w > 3 and clip >= 3 and not masked:                               # the clip does something, and something is left
            assert (got["kept"] < got["n"]).any() and (got["kept"][:, :-1, :-1] > 0).all()
        assert (got["n"][:, -1, -1] == 0).all() or w == 257 or w == 3        # last nodes beyond the frame: empty windows


# ---- 2. special contents --------------------------------------------------------------------------------------------
def test_special_contents(st):
    w, h, step = 70, 50, 32
    p = BackgroundParameters(step=step, clip_iters=3, kappa=3.0, f32_scale=SCALE)

    def both(frame, mask=None, params=p):
        got = st.background_cells([frame], params, mask)[0]
        _fields_equal(got, br.cells_restate(frame, params, mask), "special")
        return got
    c = both(np.full((h, w), 1234, np.uint16))                               # constant: mad 0, d = 1
    live = c["n"] > 0
    assert (c["mad"][live] == 0).all() and (c["lo"][live] == 1233).all() and (c["hi"][live] == 1235).all() and (c["kept"] == c["n"]).all()
    c = both(np.zeros((h, w, 3), np.uint16))                                 # all keys 0
    assert (c["med"] == 0).all() and (c["sum2"] == 0).all() and (c["lo"] == 0).all()
    c = both(np.full((h, w, 3), 65535, np.uint16))                           # all keys 65535: the top bin of both levels
    live = c["n"] > 0
    assert (c["med"][live] == 65535).all() and (c["hi"][live] == 65535).all() and (c["sum2"][live] == c["n"][live].astype(np.uint64) * np.uint64(65535 * 65535)).all()
    both(np.full((h, w), 255, np.uint8))
    f = np.full((h, w), 100.0, np.float32)                                   # f32: NaN, +-inf, negatives and values beyond the clamp
    f[::3, ::4], f[1::5, ::3], f[2::7, 1::2], f[::2, 3::5], f[5::6, ::7] = np.nan, np.inf, -np.inf, -7.5, 1e9
    c = both(f)
    assert c["n"][0, 0, 0] == 17 * 17 and c["lo"][0, 0, 0] >= 0
    c = both(f, params=BackgroundParameters(step=step, clip_iters=0, f32_scale=SCALE))
    assert int(c["sum"][0, 0, 0]) == int(br.keys_of(f, SCALE)[:17, :17].sum())
    rng = np.random.default_rng(5)                                           # keys 255 / 256: a high-byte boundary in every window
    f = (255 + (rng.random((h, w, 4)) < 0.5)).astype(np.uint16)
    c = both(f)
    assert set(np.unique(c["med"][c["n"] > 0]).tolist()) <= {255, 256}
    c = both(f.astype(np.float32) / np.float32(SCALE))
    mask = np.ones((h, w), np.uint8)                                         # a window with n = 1
    mask[32, 32] = 0
    c = both(_sky(rng, h, w, 16, 3), mask)
    assert (c["n"][1, 1] == 1).all() and (c["kept"][1, 1] == 1).all() and (c["mad"][1, 1] == 0).all() and c["n"].sum() == 3


@pytest.mark.parametrize("below", [0, 1], ids=["k", "k-1"])
def test_median_rank_on_a_bin_boundary_and_extreme_keys(st, below):
    """The selection's edge `x >= k && x - v < k` at the smallest step: the 17 x 17 window of node (1, 1) of a 33 x 33 frame
    holds exactly k = 145, or k - 1, keys in the lower of two high-byte bins. Second population set: the lower keys are all 0
    and 65535 is present, so that |K - med| reaches bin 255 of both levels."""
    rng = np.random.default_rng(50 + below)
    for low, mid, top in POPULATIONS:
        K = mid + rng.integers(0, 256, (33, 33))
        K[8:25, 8:25] = _two_populations(rng, 289, 145 - below, low, mid, top).reshape(17, 17)
        for clip in (0, 2):
            p = BackgroundParameters(step=16, clip_iters=clip, kappa=2.5)
            want = br.cells_restate(K.astype(np.uint16), p)
            assert want.shape == (3, 3, 1) and want["n"][1, 1, 0] == 289
            if clip == 0:                                                    # the restatement alone: the rank does fall on the boundary
                assert want["med"][1, 1, 0] >> 8 == (mid if below else low) >> 8 and (K[8:25, 8:25].min() >> 8, K.max()) == (low >> 8, top)
            for device in (0, 1):
                _fields_equal(st.background_cells([_place(K.astype(np.uint16), device, device)], p)[0], want, (low, clip, device))


def test_one_key_no_key_and_rounds_that_stop_on_their_first_pick(st):
    """At the smallest step, 33 x 33: a constant frame, whose second round keeps the first round's set and so stops on its
    first pick (kept = n, lo and hi one key either side); every pixel but one masked: one window of one key; every pixel
    masked: records of zeros."""
    p = BackgroundParameters(step=16, clip_iters=2, kappa=2.5)
    f = np.full((33, 33, 3), 40000, np.uint16)
    want = br.cells_restate(f, p)
    assert (want["kept"] == want["n"]).all() and (want["n"] > 0).all() and (want["lo"] == 39999).all() and (want["hi"] == 40001).all()
    _fields_equal(st.background_cells([f], p)[0], want, "constant")
    rng = np.random.default_rng(9)
    f = rng.integers(0, 65536, (33, 33, 3)).astype(np.uint16)
    mask = np.ones((33, 33), np.uint8)
    got = st.background_cells([f], p, mask)[0]
    assert got.tobytes() == np.zeros_like(got).tobytes()
    _fields_equal(got, br.cells_restate(f, p, mask), "empty")
    mask[20, 11] = 0                                                         # inside the window of node (1, 1) alone
    want = br.cells_restate(f, p, mask)
    assert want["n"].sum() == 3 and (want["n"][1, 1] == 1).all() and (want["med"][1, 1] == f[20, 11]).all() and (want["mad"][1, 1] == 0).all()
    _fields_equal(st.background_cells([f], p, mask)[0], want, "one key")


# ---- 3. apply against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,out_depth", PAIRS)
def test_apply_equals_the_restatement(st, depth, out_depth):
    rng = np.random.default_rng(10 * depth + out_depth)
    level = 100.0 if depth == 8 else 2000.0
    saturated = False
    for i, (w, step) in enumerate(itertools.product((63, 64, 65, 130), (16, 64, 128))):
        cn, device = (3, 1, 4)[(i + i // 3) % 3], i % 5 != 1                  # every channel count meets every step
        h, n = 37, 3
        gw, gh = br.grid(w, h, step)
        cc = min(cn, 3)
        frames = [(_sky(rng, h, w, depth, cn) * (SCALE if depth == 32 else 1)).astype(DTYPES[depth]) for _ in range(n)]
        planes = [(level + rng.normal(0, 0.2 * level, (gh, gw, cc))).astype(np.float32), None, (rng.normal(0, level, (gh, gw, cc))).astype(np.float32)]
        target = (0.25 * level, 7.5, -3.0, 11.0)
        got = _np(st.background_apply([_place(f, 0, device) for f in frames], planes, step, target, out_depth))
        assert got.shape == (n, h, w, cn) and got.dtype == DTYPES[out_depth]
        for k in range(n):
            want = br.apply_restate(frames[k], planes[k], step, target, out_depth)
            assert got[k].tobytes() == want.tobytes(), (w, step, cn, device, k, np.argwhere(got[k] != want)[:3].tolist())
            if cn == 4:                                                      # alpha is untouched
                assert (got[k][..., 3].astype(np.float64) == frames[k][..., 3]).all()
            saturated = saturated or bool((want[..., :cc] == 0).any())
    assert saturated or out_depth == 32                                      # the integer outputs met their lower bound somewhere


def test_apply_zero_planes_padding_and_strided_rows(st):
    rng = np.random.default_rng(8)
    w, h, cn, step = 65, 21, 4, 64
    gw, gh = br.grid(w, h, step)
    for depth in (8, 16, 32):
        frames = [_sky(rng, h, w, depth, cn) for _ in range(2)]
        zero = [np.zeros((gh, gw, 3), np.float32), None]
        for device, padded in itertools.product((0, 1), (0, 1)):
            placed = [_place(f, padded, device) for f in frames]
            got = _np(st.background_apply(placed, zero, step, (0.0,) * 4, 32))
            assert got.dtype == np.float32 and (got == np.stack(frames).astype(np.float32)).all()
            # the caller's padded outputs: the padding keeps its contents
            row = w * cn + 5
            if device:
                import torch
                big = torch.from_numpy(np.full((2, h, row), 77, DTYPES[depth])).cuda()
                outs = [big[i][:, :w * cn].unflatten(1, (w, cn)) for i in range(2)]
            else:
                big = np.full((2, h, row), 77, DTYPES[depth])
                outs = [big[i][:, :w * cn].reshape(h, w, cn) for i in range(2)]
                assert all(np.shares_memory(o, big) for o in outs)
            st.background_apply(placed, zero, step, (1.0, 2.0, 3.0, 4.0), None, out=outs)
            b = _np(big)
            assert (b[:, :, w * cn:] == 77).all()
            want = np.stack([br.apply_restate(f, None, step, (1.0, 2.0, 3.0, 4.0), depth) for f in frames])
            assert b[:, :, :w * cn].reshape(2, h, w, cn).tobytes() == want.tobytes()
    with pytest.raises(InvalidParams):
        st.background_apply(frames, zero, step, (0.0,) * 4, 16)                # f32 frames flatten to f32 only
    with pytest.raises(InvalidParams):
        st.background_apply(frames, zero, 48)
    with pytest.raises(InvalidParams):
        st.background_apply(frames, zero, step, (0.0, float("nan"), 0.0, 0.0))
    f32 = np.stack(frames)
    with pytest.raises(InvalidParams):
        st.background_apply(f32, zero, step, out=[f32[0], f32[1]])            # an output over a frame


# ---- 4. the whole-stack form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, 1])
def test_flatten_equals_its_parts(st, device):
    rng = np.random.default_rng(21 + device)
    for depth, cn, step, out_depth in ((16, 3, 32, None), (8, 4, 16, 32), (32, 1, 64, None)):
        w, h, n = 150, 100, 3
        p = BackgroundParameters(step=step, clip_iters=3, f32_scale=SCALE, estimator=BG_MODE, target=(300.0, 310.0, 320.0, 0.0) if depth != 8 else (30.0,) * 4,
                                 out_depth=out_depth)
        frames = [_sky(rng, h, w, depth, cn) for _ in range(n)]
        mask = (rng.random((h, w)) < 0.05).astype(np.uint8)
        placed = [_place(f, 0, device) for f in frames]
        out, planes, rms, cells = st.background_flatten(placed, p, mask, return_planes=True, return_rms=True, return_cells=True)
        parts_cells = st.background_cells(placed, p, mask)
        assert cells.tobytes() == parts_cells.tobytes()
        est = [background_estimate(w, h, cn, depth, parts_cells[i], p, return_rms=True) for i in range(n)]
        assert planes.tobytes() == np.stack([e[0] for e in est]).tobytes() and rms.tobytes() == np.stack([e[1] for e in est]).tobytes()
        parts_out = st.background_apply(placed, [e[0] for e in est], step, p.target, out_depth)
        assert _np(out).tobytes() == _np(parts_out).tobytes() and _np(out).dtype == DTYPES[out_depth or depth]
        assert _np(st.background_flatten(placed, p, mask)).tobytes() == _np(out).tobytes()
        # and the restatement of the three parts
        want = br.flatten_restate(frames[1], p, mask)
        assert _np(out)[1].tobytes() == want[0].tobytes() and planes[1].tobytes() == want[1].tobytes() and rms[1].tobytes() == want[2].tobytes()
    img, plane = st.flatten_image(placed[0], p, mask, return_plane=True)            # the f32 one-channel stack of the last round
    assert _np(img).tobytes() == _np(out)[0].tobytes() and plane.tobytes() == planes[0].tobytes()


# ---- 5. determinism, the CPU tests' values, the pipeline ------------------------------------------------------------
def test_same_bits_on_every_call_and_after_an_unrelated_call(st):
    rng = np.random.default_rng(31)
    frames = [_sky(rng, 100, 150, 16, 3) for _ in range(3)]
    p = BackgroundParameters(step=32, target=(500.0,) * 4)
    a = st.background_flatten(frames, p, return_planes=True, return_cells=True)
    b = st.background_flatten(frames, p, return_planes=True, return_cells=True)
    st.stack_sharpness([_sky(rng, 80, 90, 8, 3) for _ in range(2)])
    c = st.background_flatten(frames, p, return_planes=True, return_cells=True)
    fresh = Stacker(0)
    d = fresh.background_flatten(frames, p, return_planes=True, return_cells=True)
    fresh.close()
    for other in (b, c, d):
        assert all(_np(x).tobytes() == _np(y).tobytes() for x, y in zip(a, other))


@pytest.mark.parametrize("w,h,step", PLANAR)
def test_a_plane_is_flattened_exactly(st, w, h, step):
    K = planar_frame(w, h)
    p = planar_params(step)
    out, planes, cells = st.background_flatten([K], p, return_planes=True, return_cells=True)
    assert cells[0].tobytes() == br.cells_restate(K, p).tobytes()
    assert (br.level_at_pixels(planes[0], w, h, step)[..., 0] == K).all()
    assert (out[0] == 500).all() and out.dtype == np.uint16


def test_quality_seed_and_pipeline(st):
    """One quality seed gives the CPU test's value (the records are the restatement's, so is the plane). Then the pipeline on
    the 256 x 192 field: after flattening to u16 at target 1000 star detection keeps at least as many stars as on the raw
    frame, and the noise pass's per-frame median is within 2 ADU of 1000 (on the restatement: 1000, see the print)."""
    w, h, seed = 256, 192, 2
    f, bg = br.scene(w, h, seed)
    p = quality_params(BG_MEAN, True)
    p.target = (1000.0,) * 4
    out, planes = st.background_flatten([f], p, return_planes=True)
    want = br.flatten_restate(f, p)
    assert planes[0].tobytes() == want[1].tobytes() and out[0].tobytes() == want[0].tobytes()
    err = br.level_error(br.level_at_pixels(planes[0], w, h, 32)[..., 0], bg)
    rest_median = float(np.median(want[0]))
    print("level error %.4f (bar %.4f); median of the restated flattened frame %.1f" % (err, QUALITY_BAR[BG_MEAN], rest_median))
    assert err <= QUALITY_BAR[BG_MEAN] and abs(rest_median - 1000.0) <= 2.0
    sp = StarParameters(radius=4, kappa=4.0, min_pixels=3, max_stars=500)
    raw = st.star_detect_deep([f], sp, StarDeepParameters())[0]
    flat = st.star_detect_deep([out[0]], sp, StarDeepParameters())[0]
    print("stars on the raw frame %d, on the flattened frame %d" % (len(raw), len(flat)))
    assert len(flat) >= len(raw) > 0
    med = int(st.stack_noise([out[0]])[0, 0]["median"])
    assert abs(med - 1000) <= 2, med

"""Drizzle integration (include/stacker.h, stk_drizzle_params) on the GPU: stk_drizzle_stack against the numpy restatement
(drizzle_restate.py) — bit for bit where every operation is exact, within a bound computed from the f64 restatement
elsewhere —, against the weighted combine it reduces to, the whole-stack forms against their parts, strided frames, the
quality gain on the device, and every refusal. Frames are 27 x 35 to 40 x 56, outputs 45 x 67 and the like: no width is a
multiple of 64, several blocks per launch."""
import ctypes as C
import itertools

import numpy as np
import pytest

import drizzle_restate as dr
from libstacker_rs_amd import (RANSAC, DrizzleParameters, EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType,
                               Stacker, synth)

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
LOC = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def shift(sx, sy):
    M = np.eye(3)
    M[0, 2], M[1, 2] = sx, sy
    return M


def place(frames, device):
    if not device:
        return frames
    import torch
    return [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run(st, frames, warps, dz, shape, device, **kw):
    out, den = st.drizzle_stack(place(frames, device), warps, dz, out_shape=shape, return_den=True, **kw)
    return host(out), host(den)


# ---- 1. the exact case ----------------------------------------------------------------------------------------------------
EX_H, EX_W, EX_OUT = 27, 35, (45, 67)
EX_DZ = DrizzleParameters(scale=2.0, pixfrac=0.5, origin_x=-1.5, origin_y=-0.75, fill=-3.0)
_EXACT = {}


def exact_case(cn):
    """(integer frames 9 x h x w x cn, warps, per N the f64 restatement): computed once, shared by every dtype and location."""
    if cn not in _EXACT:
        rng = np.random.default_rng(100 + cn)
        vals = rng.integers(0, 256, (9, EX_H, EX_W, cn))
        warps = [shift(0, 0)] + [shift(*(rng.integers(-20, 21, 2) / 8.0)) for _ in range(8)]
        As = [dr.grid_matrix(M, False, EX_DZ.scale, EX_DZ.origin_x, EX_DZ.origin_y) for M in warps]
        refs = {n: dr.drizzle(vals[:n], As[:n], False, 1.0, 2.0, 0.5, EX_DZ.fill, *EX_OUT) for n in range(1, 10)}
        _EXACT[cn] = (vals, warps, refs)
    return _EXACT[cn]


@LOC
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
@pytest.mark.parametrize("cn", [1, 3, 4])
def test_exact_case_is_the_f64_restatement_bit_for_bit(st, cn, dtype, device):
    """u8 values, alpha = 1, translations and origin in multiples of 1/8 px, s = 2, p = 0.5: d is a multiple of 1/8,
    hx = hp = 1/4, every 1-D overlap a multiple of 1/8 and every weight of 1/64 (a fortiori of 1/256); the sums of at most
    81 products weight x integer < 2^8 are exact in f32. So den is the f64 restatement's exactly and out is
    f32(num64 / den64) exactly (rounding an f64 quotient of two f32 values to f32 rounds once), fill where den = 0."""
    vals, warps, refs = exact_case(cn)
    frames = [v.astype(dtype) for v in vals]
    holes = 0
    for n in range(1, 10):
        ro, rd = refs[n]
        for aff in (False, True):
            out, den = run(st, frames[:n], warps[:n], EX_DZ, EX_OUT, device, alpha=1.0, is_affine=aff)
            assert out.shape == EX_OUT + (cn,) and den.shape == EX_OUT
            assert np.array_equal(den, rd.astype(F)) and np.array_equal(rd.astype(F).astype(np.float64), rd), (n, aff)
            assert np.array_equal(out, ro.astype(F)), (n, aff)
            assert np.array_equal(out[den == 0], np.full(((den == 0).sum(), cn), EX_DZ.fill, F))
        holes += int((rd == 0).sum())
    assert holes > 0 and (refs[9][1] > 0).mean() > 0.5           # both answers occur


# ---- 2. the general case ----------------------------------------------------------------------------------------------------
def rot(deg, cx, cy, tx=0.0, ty=0.0):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1.0]])


KINDS = ["rot30-affine", "homography", "canvas", "small-affine"]
FORMATS = [(np.uint8, 3, 1.0 / 255.0), (np.uint16, 1, 1.0 / 65535.0), (np.float32, 4, 1.0)]
GENERAL = [(s, p, KINDS[i % 4], FORMATS[i % 3], i) for i, (s, p) in enumerate(itertools.product((1.0, 1.5, 2.0, 3.0), (0.3, 0.7, 1.0)))]
_GENERAL = {}


def general_case(case):
    """Inputs and the reference of one general case, once for both locations: frames, warps, call arguments, the f64
    restatement (out, den) and its coordinate terms."""
    s, p, kind, (dtype, cn, alpha), idx = case
    if idx in _GENERAL:
        return _GENERAL[idx]
    rng = np.random.default_rng(200 + idx)
    h, w, n = (31, 45, 5) if idx % 2 else (40, 56, 4)
    scale = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}[dtype]
    frames = [np.rint(rng.random((h, w, cn)) * scale).astype(dtype) if dtype != np.float32 else rng.random((h, w, cn)).astype(F)
              for _ in range(n)]
    affine = kind in ("rot30-affine", "small-affine")
    if kind == "rot30-affine":          # all three taps per axis live
        warps = [rot(30.0 * (1 if k % 2 else -1), w / 2, h / 2, *rng.uniform(-2, 2, 2)) if k else np.eye(3) for k in range(n)]
    elif kind == "homography":
        warps = []
        for k in range(n):
            M = rot(rng.uniform(-4, 4), w / 2, h / 2, *rng.uniform(-3, 3, 2))
            M[2, :2] = rng.normal(0, 4e-4, 2)
            warps.append(M)
    elif kind == "canvas":
        warps = [shift(*rng.uniform(-6, 6, 2)) for _ in range(n)]
    else:
        warps = [rot(rng.uniform(-3, 3), w / 2, h / 2, *rng.uniform(-4, 4, 2)) for _ in range(n)]
    dz = DrizzleParameters(scale=s, pixfrac=p, fill=0.25)
    oh, ow = dz.out_shape(h, w)
    if kind == "canvas":                # an output larger than the scaled frame around a negative origin
        dz = DrizzleParameters(scale=s, pixfrac=p, origin_x=-4.5, origin_y=-2.25, fill=0.25)
        oh, ow = oh + int(7 * s), ow + int(11 * s)
    oh, ow = oh | 1, ow | 1             # odd in both axes
    kw = {}
    include = None
    if idx % 2:
        include = [1] * n
        include[1 + idx % (n - 1)] = 0
        kw["include"] = include
    if idx % 3 == 0:
        kw.update(gain=rng.uniform(0.5, 1.5, (n, cn)).astype(F), offset=rng.uniform(0.0, 0.1, (n, cn)).astype(F),
                  weights=rng.uniform(0.25, 2.0, n).astype(F))
    maps = None
    if idx % 2 == 0:
        maps = []
        for k in range(n):
            m = rng.uniform(0.5, 2.0, (h, w)).astype(F)
            m[rng.random((h, w)) < 0.15] = 0.0              # bad pixels
            maps.append(None if k == 2 else m)
        kw["maps"] = maps
    sel = [k for k in range(n) if include is None or include[k]]
    As = [dr.grid_matrix(warps[k], affine, s, dz.origin_x, dz.origin_y) for k in sel]
    rk = dict(gain=None if "gain" not in kw else kw["gain"][sel], offset=None if "offset" not in kw else kw["offset"][sel],
              weights=None if "weights" not in kw else kw["weights"][sel], maps=None if maps is None else [maps[k] for k in sel])

    def call(du, dv):
        return dr.drizzle([frames[k] for k in sel], As, affine, alpha, s, p, dz.fill, oh, ow, du=du, dv=dv, **rk)
    ro, rd, eo, ed = dr.coordinate_term(call, As, oh, ow, affine)
    vmax = max(float(np.abs(np.asarray(f, np.float64)).max()) for f in frames) * float(F(alpha))
    sample = vmax * (1.0 if "gain" not in kw else float(kw["gain"].max())) + (0.0 if "offset" not in kw else float(kw["offset"].max()))
    wmap = max((1.0 if "weights" not in kw else float(kw["weights"][k])) * (1.0 if maps is None or maps[k] is None else float(maps[k].max()))
               for k in sel)
    _GENERAL[idx] = (frames, warps, dz, (oh, ow), dict(kw, is_affine=affine, alpha=alpha), len(sel), ro, rd, eo, ed, sample, wmap)
    return _GENERAL[idx]


@LOC
@pytest.mark.parametrize("case", GENERAL, ids=[f"s{c[0]}-p{c[1]}-{c[2]}-{np.dtype(c[3][0]).name}c{c[3][1]}" for c in GENERAL])
def test_general_case_against_the_f64_restatement(st, case, device):
    """The bound is the sum of two terms, both from the reference.
    Rounding: out is a ratio of two sums of at most 9 N products with weights >= 0 and (here) samples >= 0, so accumulating
    them in order costs at most 9 N u relative to the sum of the terms' magnitudes (u = 2^-24), which for the ratio is at
    most max |sample|; on the way from the coordinates to the output a term passes through at most 16 further rounded
    operations (d -+ hx, a -+ hp, the min - max difference and the clamp, per axis; ox oy; the map; alpha; wgt t; s g, o k,
    their sum, w x, the add into num; the division): (9 N + 16) u max |sample|.
    den has no ratio to cancel the weights' own errors, and those are absolute, not relative to the weight: d -+ hx and
    a -+ hp are below 2 in magnitude, so each is off by at most u, and so is their clamped difference: 3 u per 1-D overlap.
    A tap's wgt = ox oy (both <= 1) is then off by at most 3 u + 3 u + u, its product with the map and the add into k cost
    u each: 9 u per tap, 81 u per entry, times w_i and the largest map value; w k, the add into den and the slack of the
    second-order terms: (81 N + 16) u max (w_i max map_i).
    Coordinates: the engine's f32 (u, v) differ from the f64 ones by at most 3 ulp of the largest coordinate magnitude; the
    term is the largest change of the f64 restatement when its coordinates move by that much along either axis or both,
    every entry on its own, since the entries' coordinate errors are independent (drizzle_restate.coordinate_term).
    Pixels whose reference den is below 1e-3 of the median den (a sliver of one drop) are compared on den only — at most
    1 % of the output — and there out must be fill wherever the engine's den is 0."""
    frames, warps, dz, shape, kw, n, ro, rd, eo, ed, sample, wmap = general_case(case)
    out, den = run(st, frames, warps, dz, shape, device, **kw)
    r, rden = (9 * n + 16) * U, (81 * n + 16) * U
    med = float(np.median(rd[rd > 0]))
    low = rd < 1e-3 * med
    thin = low & (rd > 0)
    derr = np.abs(den.astype(np.float64) - rd) / (rden * wmap + ed)
    oerr = (np.abs(out.astype(np.float64) - ro).max(axis=2) / (r * sample + eo))[~low]
    print(f"den error / bound {derr.max():.3f}, out error / bound {oerr.max():.3f} (out bound: rounding {r * sample:.3e}, coordinate "
          f"median {np.median(eo):.3e} max {eo[~low].max():.3e}; den bound: rounding {rden * wmap:.3e}); thin share "
          f"{thin.mean():.4f}, holes {(rd == 0).mean():.3f}")
    assert thin.mean() <= 0.01
    assert (~low).mean() > 0.3
    assert derr.max() <= 1
    assert oerr.max() <= 1
    assert np.array_equal(out[low & (den == 0)], np.full(((low & (den == 0)).sum(), out.shape[2]), dz.fill, F))


# ---- 3. s = 1, p = 1, translations: the weighted combine with coverage = 1 ---------------------------------------------
def test_scale_1_pixfrac_1_is_the_weighted_combine(st):
    """Not bit for bit (the operation order differs): within the general case's two-term bound, computed from the f64
    restatement, of the weighted combine's image and coverage, and of the restatement itself."""
    rng = np.random.default_rng(31)
    h, w, n = 31, 45, 6
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    warps = [shift(*rng.uniform(-5, 5, 2)) for _ in range(n)]
    gain, offset, weights = rng.uniform(0.5, 1.5, (n, 3)).astype(F), rng.uniform(0, 0.1, (n, 3)).astype(F), rng.uniform(0.5, 2, n).astype(F)
    dz = DrizzleParameters(scale=1.0, pixfrac=1.0)
    out, den = run(st, frames, warps, dz, (h, w), False, gain=gain, offset=offset, weights=weights)
    ref, cov = st.weighted_stack(frames, warps, gain, offset, weights, coverage=True, return_coverage=True)
    As = [dr.grid_matrix(M, False, 1.0) for M in warps]

    def call(du, dv):
        return dr.drizzle(frames, As, False, 1.0 / 255.0, 1.0, 1.0, 0.0, h, w, gain=gain, offset=offset, weights=weights, du=du, dv=dv)
    ro, rd, eo, ed = dr.coordinate_term(call, As, h, w, False)
    r, rden = (9 * n + 16) * U, (81 * n + 16) * U * float(weights.max())
    sample = float(F(1.0 / 255.0)) * 255.0 * float(gain.max()) + float(offset.max())
    ok = rd >= 1e-3 * np.median(rd[rd > 0])
    assert ok.mean() > 0.95
    assert (np.abs(den.astype(np.float64) - cov) <= rden + ed).all()
    assert (np.abs(out.astype(np.float64) - ref).max(axis=2) <= r * sample + eo)[ok].all()
    assert (np.abs(out.astype(np.float64) - ro).max(axis=2) <= r * sample + eo)[ok].all()


# ---- 4. the whole-stack forms equal their parts ------------------------------------------------------------------------------
def _stats_equal(a, b):
    for x, y in zip(a, b):
        assert x["status"] == y["status"] and x["iterations"] == y["iterations"] and x["rho"] == y["rho"]
        assert x["n_matches"] == y["n_matches"] and np.array_equal(x["warp"], y["warp"])


def test_ecc_match_drizzle_equals_its_parts(st):
    frames, _ = synth.make_stack(4, 128, 96)
    dev = frames.cuda()
    dz = DrizzleParameters(scale=1.5, pixfrac=0.7, origin_x=-2.0, origin_y=1.0, fill=0.5)
    shape = (151, 197)
    out, den, stats = st.ecc_match_drizzle(dev, ECC, dz, out_shape=shape, return_den=True, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    _stats_equal(stats, pstats)
    ref, rden = st.drizzle_stack(dev, [s["warp"] for s in stats], dz, out_shape=shape, return_den=True)
    assert np.array_equal(host(out), host(ref)) and np.array_equal(host(den), host(rden))
    assert float(host(den).max()) > 0 and np.isfinite(host(out)).all()
    hout, hden = st.ecc_match_drizzle(frames.numpy(), ECC, dz, out_shape=shape, return_den=True)       # host-fed: the same bits
    assert isinstance(hout, np.ndarray) and np.array_equal(hout, host(out)) and np.array_equal(hden, host(den))
    multi = Stacker(devices=[0, 0])                      # a multi-device context runs the call on its first device
    try:
        mo = multi.ecc_match_drizzle(dev, ECC, dz, out_shape=shape)
    finally:
        multi.close()
    assert np.array_equal(host(mo), host(out))


def test_keypoint_match_drizzle_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(3, 640, 480)
    frames = frames.numpy()
    stack = [frames[0], frames[1], np.full_like(frames[0], 128), frames[2]]       # featureless: dropped
    dz = DrizzleParameters(scale=1.5, pixfrac=0.6)
    dropped, out, den, stats = st.keypoint_match_drizzle(stack, KP, dz, return_den=True, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    _stats_equal(stats, pstats)
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    ref, rden = st.drizzle_stack(stack, warps, dz, include=include, return_den=True)
    assert out.shape == (720, 960, 3) and np.array_equal(out, ref) and np.array_equal(den, rden)
    # the dropped frame is absent from den: with it (through the identity) the weight image is larger everywhere it covers
    with_it, wden = st.drizzle_stack(stack, warps, dz, return_den=True)
    assert (wden >= den).all() and (wden > den).mean() > 0.9


# ---- 5. strided frames ------------------------------------------------------------------------------------------------------
def window(frame, device):
    """The frame as a window of a larger canvas: two columns to its left, three to its right, a row above and two below."""
    h, w, cn = frame.shape
    canvas = np.full((h + 3, w + 5, cn), 77, frame.dtype)
    canvas[1:1 + h, 2:2 + w] = frame
    if device:
        import torch
        view = torch.from_numpy(canvas).cuda()[1:1 + h, 2:2 + w]
        assert not view.is_contiguous()
        return view
    view = canvas[1:1 + h, 2:2 + w]
    assert not view.flags.c_contiguous
    return view


@LOC
@pytest.mark.parametrize("fmt", FORMATS, ids=["u8c3", "u16c1", "f32c4"])
def test_windows_of_a_canvas_give_the_packed_bits(st, fmt, device):
    from libstacker_rs_amd.api import _Marshalled
    dtype, cn, alpha = fmt
    rng = np.random.default_rng(5)
    h, w, n = 27, 35, 4
    frames = [rng.integers(0, 200, (h, w, cn)).astype(dtype) for _ in range(n)]
    warps = [rot(rng.uniform(-5, 5), w / 2, h / 2, *rng.uniform(-3, 3, 2)) for _ in range(n)]
    dz = DrizzleParameters(scale=2.0, pixfrac=0.7)
    tight = run(st, frames, warps, dz, (55, 71), device, alpha=alpha)
    views = [window(f, device) for f in frames]
    assert _Marshalled(views).c_frames.row_stride_bytes == (w + 5) * cn * np.dtype(dtype).itemsize       # handed over where they lie
    out, den = st.drizzle_stack(views, warps, dz, out_shape=(55, 71), return_den=True, alpha=alpha)
    assert np.array_equal(host(out), tight[0]) and np.array_equal(host(den), tight[1])


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------
def test_the_same_bits_on_every_call_and_under_warp_tune(st):
    frames, warps, dz, shape, kw = general_case(GENERAL[4])[:5]
    a = run(st, frames, warps, dz, shape, True, **kw)
    b = run(st, frames, warps, dz, shape, True, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for tune in (1, 2):
        st.set_option("warp_tune", tune)
        try:
            c = run(st, frames, warps, dz, shape, True, **kw)
        finally:
            st.set_option("warp_tune", 0)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    st.set_option("warp_interpolation", 2)               # ignored: drizzle does not interpolate
    try:
        c = run(st, frames, warps, dz, shape, True, **kw)
    finally:
        st.set_option("warp_interpolation", 1)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


# ---- 7. the quality gain on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quality_on_the_device(st, seed):
    """test_cpu_drizzle's stack through the engine: the RMS error of the GPU result against the point-sampled scene is
    within 1 % of the f64 restatement's own."""
    frames, warps, scene = dr.quality_stack(seed)
    truth, inner = dr.quality_truth(scene, 2)
    dz = DrizzleParameters(scale=2.0, pixfrac=0.5)
    out, den = run(st, list(frames), warps, dz, (2 * dr.QH, 2 * dr.QW), True, alpha=1.0)
    As = [dr.grid_matrix(M, False, 2.0) for M in warps]
    ro, _ = dr.drizzle(frames, As, False, 1.0, 2.0, 0.5, 0.0, 2 * dr.QH, 2 * dr.QW)
    e_gpu, e_ref = dr.rms(out[..., 0], truth, inner), dr.rms(ro[..., 0], truth, inner)
    yard, _ = dr.bilinear_mean64(frames, warps, 2)
    print(f"seed {seed}: gpu {e_gpu:.5f}, f64 restatement {e_ref:.5f}, bilinear yardstick {dr.rms(yard, truth, inner):.5f}")
    assert den[inner].min() >= 1.0
    assert abs(e_gpu / e_ref - 1.0) <= 0.01


# ---- 8. errors: refused on the host, nothing is launched ----------------------------------------------------------------------
def test_invalid_arguments_are_rejected(st):
    rng = np.random.default_rng(9)
    h, w, n = 27, 35, 3
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    Is = [np.eye(3)] * n
    nan, inf = float("nan"), float("inf")
    bad = [(dict(scale=0.99), "scale"), (dict(scale=4.01), "scale"), (dict(scale=nan), "scale"), (dict(scale=inf), "scale"),
           (dict(pixfrac=0.0), "pixfrac"), (dict(pixfrac=-0.5), "pixfrac"), (dict(pixfrac=1.01), "pixfrac"), (dict(pixfrac=nan), "pixfrac"),
           (dict(origin_x=nan), "origin"), (dict(origin_y=inf), "origin"), (dict(origin_x=-inf), "origin"),
           (dict(fill=nan), "fill"), (dict(fill=inf), "fill")]
    for kw, field in bad:
        dz = DrizzleParameters(**kw)
        shape = (40, 50)
        with pytest.raises(InvalidParams, match=field):
            st.drizzle_stack(frames, Is, dz, out_shape=shape)
        with pytest.raises(InvalidParams, match=field):
            st.ecc_match_drizzle(frames, ECC, dz, out_shape=shape)
        with pytest.raises(InvalidParams, match=field):
            st.keypoint_match_drizzle(frames, KP, dz, out_shape=shape)
    dz = DrizzleParameters()
    for shape in ((1, 32769), (32769, 1)):
        with pytest.raises(InvalidParams, match="32768"):
            st.drizzle_stack(frames, Is, dz, out_shape=shape)
    for kw, field in ((dict(weights=[0, 0, 0]), "weight"), (dict(weights=[1, -1, 1]), "weight"), (dict(weights=[1, nan, 1]), "weight"),
                      (dict(weights=[1, inf, 1]), "weight"), (dict(gain=np.array([[1, 1, 1], [1, nan, 1], [1, 1, 1]])), "gain"),
                      (dict(offset=np.array([[0, 0, 0], [0, 0, 0], [0, 0, inf]])), "offset"),
                      (dict(weights=[0, 1, 0], include=[1, 0, 1]), "weight"), (dict(include=[0, 0, 0]), "included")):
        with pytest.raises(InvalidParams, match=field):
            st.drizzle_stack(frames, Is, dz, **kw)
    st.drizzle_stack(frames, Is, dz, weights=[0, 1, 0])          # one positive weight is enough
    st.set_option("warp_subpixel_bits", 5)
    try:
        for call in (lambda: st.drizzle_stack(frames, Is, dz), lambda: st.ecc_match_drizzle(frames, ECC, dz),
                     lambda: st.keypoint_match_drizzle(frames, KP, dz)):
            with pytest.raises(InvalidParams, match="warp_subpixel_bits"):
                call()
    finally:
        st.set_option("warp_subpixel_bits", 0)


def test_reserved_packing_and_null_pointers_are_rejected(st):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    rng = np.random.default_rng(10)
    frames = [rng.integers(0, 256, (27, 35, 3), dtype=np.uint8) for _ in range(3)]
    m = _Marshalled(frames)
    out = np.empty((45, 80, 3), np.float32)
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    dz, ep, kp = DrizzleParameters()._c(), ECC._c(), KP._c()
    dropped = C.c_int32(0)

    def image(width=67, channels=3, stride=0, data=out.ctypes.data):
        return _ffi.ImageF32(data, width, 45, channels, HOST, stride)
    good = image()
    bad = DrizzleParameters()._c()
    bad.reserved = 1
    for p, img, mp, word in ((bad, good, Mp, b"reserved"), (dz, image(stride=80 * 12), Mp, b"tightly packed"),
                             (dz, image(channels=1), Mp, b"channels"), (dz, image(data=None), Mp, b"null output"),
                             (dz, image(width=0), Mp, b"32768"), (dz, good, None, b"null matrix")):
        assert lib.stk_drizzle_stack(h, fr, mp, None, 0, 1.0 / 255, C.byref(p), None, None, C.byref(img), None) == 2
        assert word in lib.stk_last_error(h), word
    assert lib.stk_drizzle_stack(h, fr, Mp, None, 0, 1.0 / 255, None, None, None, C.byref(good), None) == 2
    assert lib.stk_drizzle_stack(h, fr, Mp, None, 0, 1.0 / 255, C.byref(dz), None, None, None, None) == 2
    assert lib.stk_drizzle_stack(None, fr, Mp, None, 0, 1.0 / 255, C.byref(dz), None, None, C.byref(good), None) == 2
    assert lib.stk_ecc_match_drizzle(h, fr, C.byref(ep), 0.0, C.byref(bad), C.byref(good), None, None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    assert lib.stk_keypoint_match_drizzle(h, fr, C.byref(kp), 0.0, C.byref(bad), C.byref(good), C.byref(dropped), None, None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    assert lib.stk_ecc_match_drizzle(h, fr, C.byref(ep), 0.0, None, C.byref(good), None, None) == 2
    assert lib.stk_keypoint_match_drizzle(h, fr, None, 0.0, C.byref(dz), C.byref(good), C.byref(dropped), None, None) == 2
    assert lib.stk_drizzle_stack(h, fr, Mp, None, 0, 1.0 / 255, C.byref(dz), None, None, C.byref(good), None) == 0

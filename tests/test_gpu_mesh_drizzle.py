"""Mesh-displaced drizzle (include/stacker.h, the block after stk_drizzle_params) on the GPU: stk_mesh_drizzle_stack against
stk_drizzle_stack where the fields are NULL or zero, against the numpy restatement (mesh_drizzle_restate.py) — bit for bit
where every operation is exact, within a bound computed from the f64 restatement elsewhere —, the whole-stack forms against
their parts, strided frames, masks, repeatability, the quality on the device, and every refusal. Frames are 65 x 53: with
step 8 the grid is 9 x 8, the last node column exactly on the last image column and the last node row beyond the edge; the
outputs (65 x 53 to 260 x 212, canvases a little larger) are no multiple of 64 wide and several blocks."""
import ctypes as C

import numpy as np
import pytest

import drizzle_restate as dr
import mesh_drizzle_restate as mr
from libstacker_rs_amd import (RANSAC, DrizzleParameters, EccMatchParameters, InvalidParams, KeyPointMatchParameters, MeshParameters,
                               MotionType, NotImplementedYet, Stacker, mesh_grid, synth)

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
H, W, STEP = 53, 65, 8
GW, GH = 9, 8
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
MP = MeshParameters(step=16, radius=8, max_iters=6, epsilon=0.01, max_shift=4.0, min_eig=1.0, fill=2)
LOC = pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
FORMATS = [(dt, cn) for dt in (np.uint8, np.uint16, np.float32) for cn in (1, 3, 4)]
FMT_IDS = [f"{np.dtype(dt).name}c{cn}" for dt, cn in FORMATS]
ALPHA = {np.uint8: 1.0 / 255.0, np.uint16: 1.0 / 65535.0, np.float32: 1.0}


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def shift(sx, sy):
    M = np.eye(3)
    M[0, 2], M[1, 2] = sx, sy
    return M


def rot(deg, cx, cy, tx=0.0, ty=0.0):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, cx - c * cx + s * cy + tx], [s, c, cy - s * cx - c * cy + ty], [0, 0, 1.0]])


def place(xs, device):
    if not device:
        return xs
    import torch
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def run(st, frames, warps, fields, dz, shape, device, step=STEP, **kw):
    if kw.get("maps") is not None:
        kw = dict(kw, maps=place(kw["maps"], device))
    out, den = st.mesh_drizzle_stack(place(frames, device), warps, place(fields, device), step, dz, out_shape=shape, return_den=True, **kw)
    return host(out), host(den)


def run_plain(st, frames, warps, dz, shape, device, **kw):
    if kw.get("maps") is not None:
        kw = dict(kw, maps=place(kw["maps"], device))
    out, den = st.drizzle_stack(place(frames, device), warps, dz, out_shape=shape, return_den=True, **kw)
    return host(out), host(den)


def random_frames(rng, n, dtype, cn):
    if dtype == np.float32:
        return [rng.random((H, W, cn)).astype(F) for _ in range(n)]
    return [rng.integers(0, np.iinfo(dtype).max + 1, (H, W, cn)).astype(dtype) for _ in range(n)]


def smooth_field(rng, amp):
    """A gh x gw x 2 field of one cosine per component: up to `amp` px, wavelengths of 60 to 110 px (slopes up to 0.3)."""
    j, k = np.mgrid[0:GH, 0:GW].astype(np.float64) * STEP
    D = np.zeros((GH, GW, 2), F)
    for c in range(2):
        lam, th, ph = rng.uniform(60, 110), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        D[..., c] = amp * np.cos(2 * np.pi * (np.cos(th) * k + np.sin(th) * j) / lam + ph)
    return D


# ---- 1. NULL and zero fields are stk_drizzle_stack, bit for bit -----------------------------------------------------------
GRIDS = [(DrizzleParameters(scale=1.0, pixfrac=1.0, fill=0.25), (H, W)),
         (DrizzleParameters(scale=2.0, pixfrac=0.7, fill=0.25), (2 * H, 2 * W)),
         (DrizzleParameters(scale=3.0, pixfrac=0.4, fill=0.25), (3 * H, 3 * W)),
         (DrizzleParameters(scale=1.5, pixfrac=0.8, origin_x=-4.5, origin_y=-2.25, fill=0.25), (97, 121))]      # a canvas


@LOC
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
def test_null_and_zero_fields_are_plain_drizzle(st, fmt, device):
    """Every depth and channel count, an affine table with a 30 degree rotation and a perspective one, with and without
    maps and records, N = 3 and 4, the four output grids in turn: all-NULL, all-zero and mixed field tables return
    stk_drizzle_stack's image and weight image to the bit (the plain kernels on one side, the mesh kernels on the other)."""
    dtype, cn = fmt
    idx = FORMATS.index(fmt)
    rng = np.random.default_rng(300 + idx)
    zero = np.zeros((GH, GW, 2), F)
    for v, (aff, with_maps) in enumerate(((True, False), (True, True), (False, False), (False, True))):
        n = 3 + (idx + v) % 2
        dz, shape = GRIDS[(idx + v) % 4]
        frames = random_frames(rng, n, dtype, cn)
        warps = [rot(30.0 * (1 if k % 2 else -1) if aff else rng.uniform(-4, 4), W / 2, H / 2, *rng.uniform(-3, 3, 2)) if k else np.eye(3)
                 for k in range(n)]
        if not aff:
            for M in warps[1:]:
                M[2, :2] = rng.normal(0, 4e-4, 2)
        kw = dict(is_affine=aff, alpha=ALPHA[dtype])
        if with_maps:
            maps = [rng.uniform(0.5, 2.0, (H, W)).astype(F) for _ in range(n)]
            maps[0][rng.random((H, W)) < 0.15] = 0.0
            maps[1] = None
            kw.update(maps=maps, gain=rng.uniform(0.5, 1.5, (n, cn)).astype(F), offset=rng.uniform(0, 0.1, (n, cn)).astype(F),
                      weights=rng.uniform(0.25, 2.0, n).astype(F))
        ref = run_plain(st, frames, warps, dz, shape, device, **kw)
        assert (ref[1] > 0).mean() > 0.3
        for fields in ([None] * n, [zero] * n, [zero, None, zero] + [None] * (n - 3)):
            got = run(st, frames, warps, fields, dz, shape, device, **kw)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (aff, with_maps)


# ---- 2. the exact cases ---------------------------------------------------------------------------------------------------
EXACT = [(1.0, 1.0, (0.0, 0.0), (H, W)), (2.0, 0.5, (-1.5, -0.75), (2 * H + 5, 2 * W + 7)), (4.0, 0.5, (0.0, 0.0), (4 * H, 4 * W))]
_EXACT = {}


def exact_case(gi, cn):
    """(integer frames 9 x h x w x cn, warps, fields, per N the f64 restatement): once for every dtype and location."""
    if (gi, cn) not in _EXACT:
        s, p, origin, (oh, ow) = EXACT[gi]
        rng = np.random.default_rng(400 + 10 * gi + cn)
        vals = rng.integers(0, 256, (9, H, W, cn))
        warps = [shift(0, 0)] + [shift(*(rng.integers(-20, 21, 2) / 8.0)) for _ in range(8)]
        fields = [None]
        for k in range(1, 9):
            D = np.zeros((GH, GW, 2), F)
            D[..., 0], D[..., 1] = rng.integers(-16, 17, 2) / 8.0
            fields.append(None if k == 4 else D)
        As = [dr.grid_matrix(M, False, s, *origin) for M in warps]
        terms = [mr.entry_terms(vals[k], As[k], False, 1.0, p, oh, ow, fields[k], STEP, s, *origin) for k in range(9)]
        refs = {n: mr.combine(terms[:n], -3.0) for n in range(1, 10)}
        _EXACT[(gi, cn)] = (vals, warps, fields, refs)
    return _EXACT[(gi, cn)]


@LOC
@pytest.mark.parametrize("fmt", FORMATS, ids=FMT_IDS)
@pytest.mark.parametrize("gi", [0, 1, 2], ids=["s1-p1", "s2-p0.5-canvas", "s4-p0.5"])
def test_exact_case_is_the_f64_restatement_bit_for_bit(st, gi, fmt, device):
    """u8 values, alpha = 1, translations and origins in multiples of 1/8 px, per-frame constant fields in multiples of 1/8 px
    (so s d is a multiple of 1/8 too, the lerp of equal node values is that value and every slope is exactly 0), s = 1, 2, 4
    with p = 1, 0.5, 0.5: the displaced coordinate, u, d and the half-extents hx = 1 / (2 s), hp = p / 2 are multiples of
    1/8, every 1-D overlap is a multiple of 1/8 and every weight of 1/64; the sums of at most 81 products weight x integer
    < 2^8 are exact in f32. So den is the f64 restatement's exactly and out is f32(num64 / den64), fill where den = 0. An
    affine table (the kernel's per-pixel footprint for displaced entries, the host's table for the others) and a
    perspective one give the same bits. N = 1 .. 9."""
    dtype, cn = fmt
    s, p, origin, shape = EXACT[gi]
    vals, warps, fields, refs = exact_case(gi, cn)
    frames = [v.astype(dtype) for v in vals]
    dz = DrizzleParameters(scale=s, pixfrac=p, origin_x=origin[0], origin_y=origin[1], fill=-3.0)
    holes = 0
    for n in range(1, 10):
        ro, rd = refs[n]
        for aff in (False, True):
            out, den = run(st, frames[:n], warps[:n], fields[:n], dz, shape, device, alpha=1.0, is_affine=aff)
            assert out.shape == shape + (cn,) and den.shape == shape
            assert np.array_equal(den, rd.astype(F)) and np.array_equal(rd.astype(F).astype(np.float64), rd), (n, aff)
            assert np.array_equal(out, ro.astype(F)), (n, aff)
        holes += int((rd == 0).sum())
    assert (refs[9][1] > 0).mean() > 0.5 and (holes > 0 or p == 1.0)
    if gi == 1 and fmt == FORMATS[0]:      # the fields did something: the plain drizzle of the same stack differs
        assert not np.array_equal(run_plain(st, frames, warps, dz, shape, device, alpha=1.0)[1], refs[9][1].astype(F))


# ---- 3. the general cases -------------------------------------------------------------------------------------------------
GENERAL = [(1.0, 1.0, "rot30-affine", (np.uint8, 3)), (2.0, 0.7, "homography", (np.uint16, 1)), (3.0, 0.5, "canvas", (np.float32, 4)),
           (2.0, 0.5, "rot30-affine", (np.float32, 1)), (3.0, 0.6, "homography", (np.uint8, 4)), (1.5, 0.8, "canvas", (np.uint16, 3))]
_GENERAL = {}


def general_case(idx):
    """Inputs and the reference of one general case, once for both locations."""
    if idx in _GENERAL:
        return _GENERAL[idx]
    s, p, kind, (dtype, cn) = GENERAL[idx]
    alpha = ALPHA[dtype]
    rng = np.random.default_rng(500 + idx)
    n = 3 + idx % 2
    frames = random_frames(rng, n, dtype, cn)
    affine = kind != "homography"
    if kind == "rot30-affine":
        warps = [rot(30.0 * (1 if k % 2 else -1), W / 2, H / 2, *rng.uniform(-2, 2, 2)) if k else np.eye(3) for k in range(n)]
    elif kind == "homography":
        warps = []
        for k in range(n):
            M = rot(rng.uniform(-4, 4), W / 2, H / 2, *rng.uniform(-3, 3, 2))
            M[2, :2] = rng.normal(0, 4e-4, 2)
            warps.append(M)
    else:
        warps = [shift(*rng.uniform(-6, 6, 2)) for _ in range(n)]
    origin = (-4.5, -2.25) if kind == "canvas" else (0.0, 0.0)
    dz = DrizzleParameters(scale=s, pixfrac=p, origin_x=origin[0], origin_y=origin[1], fill=0.25)
    oh, ow = dz.out_shape(H, W)
    if kind == "canvas":
        oh, ow = oh + int(7 * s), ow + int(11 * s)
    oh, ow = oh | 1, ow | 1
    fields = [None if k == 0 else smooth_field(rng, 3.0 if k == 1 else rng.uniform(1.0, 3.0)) for k in range(n)]
    kw = {}
    gain = offset = weights = maps = None
    if idx % 3 == 0:
        gain, offset, weights = rng.uniform(0.5, 1.5, (n, cn)).astype(F), rng.uniform(0, 0.1, (n, cn)).astype(F), rng.uniform(0.25, 2.0, n).astype(F)
        kw.update(gain=gain, offset=offset, weights=weights)
    if idx % 2 == 0:
        maps = []
        for k in range(n):
            m = rng.uniform(0.5, 2.0, (H, W)).astype(F)
            m[rng.random((H, W)) < 0.15] = 0.0
            maps.append(None if k == 2 else m)
        kw["maps"] = maps
    As = [dr.grid_matrix(M, affine, s, *origin) for M in warps]
    delta, eh, bias = mr.probe_sizes(As, fields, affine, oh, ow, W, H, STEP, s, *origin)

    def entry(i, **probe):
        return mr.entry_terms(frames[i], As[i], affine, alpha, p, oh, ow, fields[i], STEP, s, *origin,
                              None if maps is None else maps[i], **probe)

    def finish(terms):
        return mr.combine(terms, dz.fill, gain, offset, weights)
    ro, rd, eo, ed = mr.bound_terms(entry, n, finish, delta, eh, bias)
    vmax = max(float(np.abs(np.asarray(f, np.float64)).max()) for f in frames) * float(F(alpha))
    sample = vmax * (1.0 if gain is None else float(gain.max())) + (0.0 if offset is None else float(offset.max()))
    wmap = max((1.0 if weights is None else float(weights[k])) * (1.0 if maps is None or maps[k] is None else float(maps[k].max()))
               for k in range(n))
    _GENERAL[idx] = (frames, warps, fields, dz, (oh, ow), dict(kw, is_affine=affine, alpha=alpha), n, ro, rd, eo, ed, sample, wmap,
                     (delta, eh, bias))
    return _GENERAL[idx]


@LOC
@pytest.mark.parametrize("idx", range(len(GENERAL)), ids=[f"s{c[0]}-p{c[1]}-{c[2]}-{np.dtype(c[3][0]).name}c{c[3][1]}" for c in GENERAL])
def test_general_case_against_the_f64_restatement(st, idx, device):
    """Smooth fields of up to 3 px (slopes up to 0.3) on a 30 degree rotation, homographies and a canvas. The bound is
    test_gpu_drizzle's, both parts from the reference alone:
    Rounding: (9 N + 16) u max |sample| for the image and (81 N + 16) u max (w_i max map_i) for den, as derived there.
    Coordinates: the largest change of the f64 restatement when one entry's source coordinates move by delta, every entry on
    its own, summed. delta is drizzle's 3 ulp of the largest coordinate, widened by what the field sample and Xd add
    (mesh_drizzle_restate.probe_sizes: the two roundings of x0, six of the lerp, those of s d and X + s d, carried through
    the local Jacobian). The field sample also feeds the footprint and takes two decisions from x0, so the same procedure
    moves the half-extents by eh (the slopes' and the Jacobian product's roundings) and the decision coordinate by bias (an
    f32 x0 within 2 ulp of a node column, or of the frame's edge, may fall into the neighbouring cell or count as clamped,
    where the slope differs).
    Every pixel is compared on den. Every pixel is compared on the image: where the reference den is below 1e-3 of the median
    (a sliver of a drop) the quotient magnifies den's own allowance E, so the bound gains 2 max |sample| E / (den - E); where
    den <= 2 E it cannot be told from 0, and there out must be fill if the engine's den is 0 and a weighted mean of samples
    (|out| <= max |sample| (1 + 1e-5)) otherwise.
    Measured on an MI355X, the worst fraction of the bound reached over the six cases (host and device alike): den 0.104,
    image 0.232, both at scale 3, pixfrac 0.6 under homographies; the other cases 0.06 - 0.10 and 0.05 - 0.20."""
    frames, warps, fields, dz, shape, kw, n, ro, rd, eo, ed, sample, wmap, probes = general_case(idx)
    out, den = run(st, frames, warps, fields, dz, shape, device, **kw)
    r, rden = (9 * n + 16) * U, (81 * n + 16) * U
    med = float(np.median(rd[rd > 0]))
    E = rden * wmap + ed
    derr = np.abs(den.astype(np.float64) - rd) / E
    low = rd < 1e-3 * med
    nil = low & (rd <= 2 * E)
    bound = r * sample + eo
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(low & ~nil, bound + 2 * sample * E / (rd - E), bound)
    oerr = np.abs(out.astype(np.float64) - ro).max(axis=2) / bound
    print(f"den error / bound {derr.max():.3f}, out error / bound {oerr[~nil].max():.3f} (delta {probes[0]:.3e}, eh {probes[1]:.3e}, bias "
          f"{probes[2]:.3e}; out bound: rounding {r * sample:.3e}, probes median {np.median(eo):.3e} max {eo[~low].max():.3e}; den bound: "
          f"rounding {rden * wmap:.3e}, probes max {ed.max():.3e}); sliver share {(low & (rd > 0)).mean():.4f}, holes {(rd == 0).mean():.3f}")
    assert (~low).mean() > 0.3
    assert derr.max() <= 1
    assert oerr[~nil].max() <= 1
    empty = nil & (den == 0)
    assert np.array_equal(out[empty], np.full((empty.sum(), out.shape[2]), dz.fill, F))
    assert (np.abs(out[nil & (den > 0)]) <= sample * (1 + 1e-5)).all()
    # the fields matter: the plain drizzle of the same stack is far outside the bound
    plain = run_plain(st, frames, warps, dz, shape, device, **kw)
    assert (np.abs(plain[1].astype(np.float64) - rd) / E).max() > 100


# ---- 4. the whole-stack forms equal their parts ---------------------------------------------------------------------------
def _stats_equal(a, b):
    for x, y in zip(a, b):
        assert x["status"] == y["status"] and x["iterations"] == y["iterations"] and x["rho"] == y["rho"]
        assert x["n_matches"] == y["n_matches"] and np.array_equal(x["warp"], y["warp"])


def test_ecc_match_local_aligned_drizzle_equals_its_parts(st):
    frames, _ = synth.make_stack(4, 128, 96)
    dev = frames.cuda()
    dz = DrizzleParameters(scale=1.5, pixfrac=0.7, origin_x=-2.0, origin_y=1.0, fill=0.5)
    shape = (151, 197)
    out, den, stats = st.ecc_match_local_aligned_drizzle(dev, ECC, MP, dz, out_shape=shape, return_den=True, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    _stats_equal(stats, pstats)
    warps = [s["warp"] for s in stats]
    fields, status = st.local_align(dev, warps, MP, return_status=True)
    assert (host(status)[1:] > 0).any() and (host(fields)[1:] != 0).any()
    ref, rden = st.mesh_drizzle_stack(dev, warps, fields, MP.step, dz, out_shape=shape, return_den=True)
    assert np.array_equal(host(out), host(ref)) and np.array_equal(host(den), host(rden))
    assert float(host(den).max()) > 0 and np.isfinite(host(out)).all()
    plain = st.drizzle_stack(dev, warps, dz, out_shape=shape)
    assert not np.array_equal(host(plain), host(out))
    hout, hden = st.ecc_match_local_aligned_drizzle(frames.numpy(), ECC, MP, dz, out_shape=shape, return_den=True)    # host-fed: the same bits
    assert isinstance(hout, np.ndarray) and np.array_equal(hout, host(out)) and np.array_equal(hden, host(den))
    multi = Stacker(devices=[0, 0])                      # a multi-device context runs the call on its first device
    try:
        mo = multi.ecc_match_local_aligned_drizzle(dev, ECC, MP, dz, out_shape=shape)
    finally:
        multi.close()
    assert np.array_equal(host(mo), host(out))


def test_keypoint_match_local_aligned_drizzle_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(3, 640, 480)
    frames = frames.numpy()
    stack = [frames[0], frames[1], np.full_like(frames[0], 128), frames[2]]       # featureless: dropped
    dz = DrizzleParameters(scale=1.5, pixfrac=0.6)
    mp = MeshParameters(step=32, radius=8, max_iters=6, epsilon=0.01, max_shift=4.0, min_eig=1.0, fill=2)
    dropped, out, den, stats = st.keypoint_match_local_aligned_drizzle(stack, KP, mp, dz, return_den=True, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    _stats_equal(stats, pstats)
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    fields = st.local_align(stack, warps, mp, include)
    ref, rden = st.mesh_drizzle_stack(stack, warps, fields, mp.step, dz, include=include, return_den=True)
    assert out.shape == (720, 960, 3) and np.array_equal(out, ref) and np.array_equal(den, rden)


# ---- 5. strided frames, masks, repeatability ------------------------------------------------------------------------------
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
@pytest.mark.parametrize("fmt", [(np.uint8, 3), (np.uint16, 1), (np.float32, 4)], ids=["u8c3", "u16c1", "f32c4"])
def test_windows_of_a_canvas_give_the_packed_bits(st, fmt, device):
    dtype, cn = fmt
    rng = np.random.default_rng(6)
    n = 4
    frames = [rng.integers(0, 200, (H, W, cn)).astype(dtype) for _ in range(n)]
    warps = [rot(rng.uniform(-5, 5), W / 2, H / 2, *rng.uniform(-3, 3, 2)) for _ in range(n)]
    fields = [None] + [smooth_field(rng, 2.0) for _ in range(n - 1)]
    dz = DrizzleParameters(scale=2.0, pixfrac=0.7)
    tight = run(st, frames, warps, fields, dz, (106, 130), device, alpha=ALPHA[dtype])
    views = [window(f, device) for f in frames]
    out, den = st.mesh_drizzle_stack(views, warps, place(fields, device), STEP, dz, out_shape=(106, 130), return_den=True,
                                     alpha=ALPHA[dtype])
    assert np.array_equal(host(out), tight[0]) and np.array_equal(host(den), tight[1])


def test_masked_pixels_are_never_read_and_two_calls_agree(st):
    """A pixel whose map value is 0 is never read: NaN there changes nothing. Records are the plain drizzle's: doubling
    every weight doubles den and leaves the image's bits. Two calls return the same bits."""
    rng = np.random.default_rng(7)
    n = 4
    frames = [rng.random((H, W, 3)).astype(F) for _ in range(n)]
    warps = [rot(rng.uniform(-5, 5), W / 2, H / 2, *rng.uniform(-3, 3, 2)) for _ in range(n)]
    fields = [None] + [smooth_field(rng, 3.0) for _ in range(n - 1)]
    maps = [(rng.random((H, W)) > 0.2).astype(F) for _ in range(n)]
    poisoned = [np.where(m[..., None] > 0, f, np.nan).astype(F) for f, m in zip(frames, maps)]
    dz = DrizzleParameters(scale=2.0, pixfrac=0.7, fill=-1.0)
    a = run(st, frames, warps, fields, dz, (106, 130), True, maps=maps, alpha=1.0)
    b = run(st, poisoned, warps, fields, dz, (106, 130), True, maps=maps, alpha=1.0)
    c = run(st, frames, warps, fields, dz, (106, 130), True, maps=maps, alpha=1.0)
    assert np.isfinite(a[0]).all() and (a[1] == 0).any() and (a[1] > 0).mean() > 0.5
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    d = run(st, frames, warps, fields, dz, (106, 130), True, maps=maps, alpha=1.0, weights=[2.0] * n)
    assert np.array_equal(d[1], 2 * a[1]) and np.array_equal(d[0], a[0])
    e = run(st, frames, warps, fields, dz, (106, 130), False, maps=maps, alpha=1.0)          # host-fed: the same bits
    assert np.array_equal(a[0], e[0]) and np.array_equal(a[1], e[1])


# ---- 6. the quality on the device -------------------------------------------------------------------------------------------
def test_quality_on_the_device(st):
    """test_cpu_mesh_drizzle's quality stack at (2, 0.7) through the engine, with the restated fields: the RMS error against
    the point-sampled scene is within 1 % of the f64 restatement's own."""
    from test_cpu_mesh import QM, quality_mesh_restated, quality_mesh_stack
    from test_cpu_mesh_drizzle import quality_truth
    _, frames, _ = quality_mesh_stack()
    fields = quality_mesh_restated(frames)[2]
    truth, inner = quality_truth(2.0)
    oh, ow = truth.shape
    n = len(frames)
    fr = [f[..., None] for f in frames]
    dz = DrizzleParameters(scale=2.0, pixfrac=0.7)
    out, den = st.mesh_drizzle_stack(fr, [np.eye(3)] * n, fields, QM["mesh"].step, dz, out_shape=(oh, ow), alpha=1.0, is_affine=True,
                                     return_den=True)
    As = [dr.grid_matrix(np.eye(3), True, 2.0)] * n
    ro, _ = mr.mesh_drizzle(fr, As, True, 1.0, 2.0, 0.7, 0.0, oh, ow, fields, QM["mesh"].step)
    e_gpu, e_ref = dr.rms(out[..., 0], truth, inner), dr.rms(ro[..., 0], truth, inner)
    plain = st.drizzle_stack(fr, [np.eye(3)] * n, dz, out_shape=(oh, ow), alpha=1.0, is_affine=True)
    print(f"quality stack at (2, 0.7): gpu {e_gpu:.5f}, f64 restatement {e_ref:.5f}, plain drizzle on the device "
          f"{dr.rms(plain[..., 0], truth, inner):.5f}, smallest interior den {den[inner].min():.3f}")
    assert den[inner].min() > 0
    assert abs(e_gpu / e_ref - 1.0) <= 0.01


# ---- 7. errors: refused on the host, nothing is launched ------------------------------------------------------------------
def test_invalid_arguments_are_rejected(st):
    rng = np.random.default_rng(9)
    n = 3
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    Is = [np.eye(3)] * n
    zero = [np.zeros((GH, GW, 2), F)] * n
    nan, inf = float("nan"), float("inf")
    bad = [(dict(scale=0.99), "scale"), (dict(scale=4.01), "scale"), (dict(scale=nan), "scale"), (dict(pixfrac=0.0), "pixfrac"),
           (dict(pixfrac=1.01), "pixfrac"), (dict(pixfrac=nan), "pixfrac"), (dict(origin_x=nan), "origin"), (dict(origin_y=inf), "origin"),
           (dict(fill=nan), "fill"), (dict(fill=inf), "fill")]
    for kw, field in bad:
        dz = DrizzleParameters(**kw)
        with pytest.raises(InvalidParams, match=field):
            st.mesh_drizzle_stack(frames, Is, zero, STEP, dz, out_shape=(40, 50))
        with pytest.raises(InvalidParams, match=field):
            st.ecc_match_local_aligned_drizzle(frames, ECC, MP, dz, out_shape=(40, 50))
        with pytest.raises(InvalidParams, match=field):
            st.keypoint_match_local_aligned_drizzle(frames, KP, MP, dz, out_shape=(40, 50))
    dz = DrizzleParameters()
    for shape in ((1, 32769), (32769, 1)):
        with pytest.raises(InvalidParams, match="32768"):
            st.mesh_drizzle_stack(frames, Is, zero, STEP, dz, out_shape=shape)
    for kw, field in ((dict(weights=[0, 0, 0]), "weight"), (dict(weights=[1, -1, 1]), "weight"), (dict(weights=[1, nan, 1]), "weight"),
                      (dict(gain=np.array([[1, 1, 1], [1, nan, 1], [1, 1, 1]])), "gain"),
                      (dict(offset=np.array([[0, 0, 0], [0, 0, 0], [0, 0, inf]])), "offset"), (dict(include=[0, 0, 0]), "included")):
        with pytest.raises(InvalidParams, match=field):
            st.mesh_drizzle_stack(frames, Is, zero, STEP, dz, **kw)
    # the mesh side: a step that is no power of two in 8 .. 256, planes of another grid, a wrong count
    for step in (0, 4, 12, 512):
        with pytest.raises(InvalidParams, match="step"):
            st.mesh_drizzle_stack(frames, Is, zero, step, dz)
    with pytest.raises(InvalidParams, match="gh x gw x 2"):
        st.mesh_drizzle_stack(frames, Is, zero, 16, dz)
    with pytest.raises(InvalidParams, match="one field per frame"):
        st.mesh_drizzle_stack(frames, Is, zero[:2], STEP, dz)
    assert mesh_grid(W, H, STEP) == (GW, GH)
    for kw in (dict(step=12), dict(radius=1), dict(radius=33), dict(max_iters=0), dict(epsilon=-1.0), dict(max_shift=0.0),
               dict(max_shift=65.0), dict(min_eig=-1.0), dict(fill=17)):
        mp = MeshParameters(**kw)
        with pytest.raises(InvalidParams, match="mesh"):
            st.ecc_match_local_aligned_drizzle(frames, ECC, mp, dz)
        with pytest.raises(InvalidParams, match="mesh"):
            st.keypoint_match_local_aligned_drizzle(frames, KP, mp, dz)
    deep = [f.astype(np.uint16) * 257 for f in frames]
    with pytest.raises(NotImplementedYet):
        st.ecc_match_local_aligned_drizzle(deep, ECC, MP, dz)
    with pytest.raises(NotImplementedYet):
        st.keypoint_match_local_aligned_drizzle(deep, KP, MP, dz)
    st.mesh_drizzle_stack(deep, Is, zero, STEP, dz, alpha=1.0 / 65535.0)          # the caller-held form takes any depth
    st.set_option("warp_subpixel_bits", 5)
    try:
        for call in (lambda: st.mesh_drizzle_stack(frames, Is, zero, STEP, dz), lambda: st.ecc_match_local_aligned_drizzle(frames, ECC, MP, dz),
                     lambda: st.keypoint_match_local_aligned_drizzle(frames, KP, MP, dz)):
            with pytest.raises(InvalidParams, match="warp_subpixel_bits"):
                call()
    finally:
        st.set_option("warp_subpixel_bits", 0)
    st.set_option("warp_interpolation", 2)               # ignored: drizzle does not interpolate
    try:
        a = st.mesh_drizzle_stack(frames, Is, zero, STEP, dz)
    finally:
        st.set_option("warp_interpolation", 1)
    assert np.array_equal(a, st.drizzle_stack(frames, Is, dz))


def test_reserved_packing_and_null_pointers_are_rejected(st):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    rng = np.random.default_rng(10)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3)]
    m = _Marshalled(frames)
    out = np.empty((45, 80, 3), np.float32)
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    zero = np.zeros((GH, GW, 2), F)
    fp = (C.c_void_p * 3)(None, zero.ctypes.data, None)
    Fp = C.cast(fp, C.c_void_p)
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    dz, ep, kp, mp = DrizzleParameters()._c(), ECC._c(), KP._c(), MP._c()
    dropped = C.c_int32(0)

    def image(width=67, channels=3, stride=0, data=out.ctypes.data):
        return _ffi.ImageF32(data, width, 45, channels, HOST, stride)
    good = image()
    bad = DrizzleParameters()._c()
    bad.reserved = 1
    badm = MP._c()
    badm.reserved = 1
    for p, img, mat, fld, word in ((bad, good, Mp, Fp, b"reserved"), (dz, image(stride=80 * 12), Mp, Fp, b"tightly packed"),
                                   (dz, image(channels=1), Mp, Fp, b"channels"), (dz, image(data=None), Mp, Fp, b"null output"),
                                   (dz, image(width=0), Mp, Fp, b"32768"), (dz, good, None, Fp, b"null matrix"),
                                   (dz, good, Mp, None, b"null fields")):
        assert lib.stk_mesh_drizzle_stack(h, fr, mat, None, 0, 1.0 / 255, C.byref(p), None, None, fld, STEP, C.byref(img), None) == 2
        assert word in lib.stk_last_error(h), word
    assert lib.stk_mesh_drizzle_stack(h, fr, Mp, None, 0, 1.0 / 255, None, None, None, Fp, STEP, C.byref(good), None) == 2
    assert lib.stk_mesh_drizzle_stack(h, fr, Mp, None, 0, 1.0 / 255, C.byref(dz), None, None, Fp, STEP, None, None) == 2
    assert lib.stk_mesh_drizzle_stack(None, fr, Mp, None, 0, 1.0 / 255, C.byref(dz), None, None, Fp, STEP, C.byref(good), None) == 2
    for pm, pd, word in ((mp, bad, b"reserved"), (badm, dz, b"reserved"), (None, dz, b"null mesh"), (mp, None, b"null drizzle")):
        pmr = None if pm is None else C.byref(pm)
        pdr = None if pd is None else C.byref(pd)
        assert lib.stk_ecc_match_local_aligned_drizzle(h, fr, C.byref(ep), 0.0, pmr, pdr, C.byref(good), None, None) == 2
        assert word in lib.stk_last_error(h), word
        assert lib.stk_keypoint_match_local_aligned_drizzle(h, fr, C.byref(kp), 0.0, pmr, pdr, C.byref(good), C.byref(dropped), None, None) == 2
        assert word in lib.stk_last_error(h), word
    assert lib.stk_keypoint_match_local_aligned_drizzle(h, fr, None, 0.0, C.byref(mp), C.byref(dz), C.byref(good), C.byref(dropped), None, None) == 2
    assert lib.stk_ecc_match_local_aligned_drizzle(None, fr, C.byref(ep), 0.0, C.byref(mp), C.byref(dz), C.byref(good), None, None) == 2
    # a NULL entry of an included frame is allowed: no displacement
    assert lib.stk_mesh_drizzle_stack(h, fr, Mp, None, 0, 1.0 / 255, C.byref(dz), None, None, Fp, STEP, C.byref(good), None) == 0

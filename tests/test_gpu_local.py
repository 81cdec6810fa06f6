"""Per-pixel weight maps and local-sharpness stacking on the GPU: stk_local_sharpness / stk_local_weighted_stack /
stk_ecc_match_local_weighted / stk_keypoint_match_local_weighted against the numpy restatements of the definition
(test_cpu_local.local_sharpness_restate and local_weighted_restate). The samples and kappa come from the engine's own
single-frame warp as in test_gpu_weighted.py; omega from the same warp of the map replicated to three f32 channels under
BORDER_CONSTANT 0 with alpha = 1, always linear."""
import ctypes as C
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, LocalParameters, MotionType, NotImplementedYet, Stacker, WeightParameters,
                               synth)
from test_cpu_local import (QS, interior_rms, local_sharpness_restate, local_weighted_restate, quality_stack,
                            quality_stack_restated)
from test_cpu_weighted import LINEAR
from test_gpu_clip import CASES
from test_gpu_weighted import engine_kappa, engine_samples, random_frames, shifted_warps

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
_ALPHA = {np.uint8: 1.0 / 255.0, np.uint16: 1.0 / 65535.0, np.float32: 1.0}
_CASE_IDS = [f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[5]}-{c[8][0]}x{c[8][1]}" for c in CASES]


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


# ---- 1. the map, bit for bit ------------------------------------------------------------------------------------------
# (h, w, channels, radius, threshold, layout): every value of every axis, every tiny size at radius 15
MAP_CASES = [
    (1, 1, 1, 15, 0, "host"), (1, 1, 3, 1, 16, "device"), (1, 1, 4, 4, 0, "list3"),
    (1, 17, 3, 15, 0, "host"), (1, 17, 4, 4, 16, "device"),
    (33, 1, 1, 15, 16, "host"), (33, 1, 3, 4, 0, "pad5"),
    (5, 3, 3, 15, 0, "device"), (5, 3, 4, 1, 16, "host"), (5, 3, 1, 15, 16, "list3"),
    (64, 64, 3, 4, 16, "device"), (64, 64, 1, 15, 0, "host"), (64, 64, 4, 1, 0, "device"), (64, 64, 3, 15, 16, "pad5"),
    (64, 64, 1, 4, 16, "device"), (64, 64, 3, 4, 0, "const"),
    (63, 65, 3, 4, 0, "host"), (63, 65, 1, 1, 16, "device"), (63, 65, 4, 15, 0, "list3"), (63, 65, 1, 4, 16, "pad5"),
    (70, 130, 3, 15, 16, "device"), (70, 130, 4, 4, 0, "host"), (70, 130, 1, 1, 0, "pad5"), (70, 130, 3, 1, 16, "list3"),
    (70, 130, 1, 15, 16, "const"),
    (37, 641, 3, 4, 16, "device"), (37, 641, 3, 15, 0, "host"), (37, 641, 3, 1, 0, "list3"),       # a row of 1923 bytes: the byte route
    (64, 128, 3, 4, 16, "device"), (128, 64, 4, 15, 0, "device"),                                # whole tiles only: the dword route
]


def _padded(frame, pad, device):
    """The frame as a row-strided view of a buffer whose rows are `pad` bytes longer."""
    h, w, cn = frame.shape
    if device:
        import torch
        big = torch.zeros((h, w * cn + pad), dtype=torch.uint8, device="cuda")
        big[:, :w * cn] = torch.from_numpy(frame.reshape(h, w * cn)).cuda()
        view = big[:, :w * cn].unflatten(1, (w, cn))
        assert not view.is_contiguous() and view.stride(0) == w * cn + pad
        return view
    big = np.zeros((h, w * cn + pad), np.uint8)
    big[:, :w * cn] = frame.reshape(h, w * cn)
    view = big[:, :w * cn].reshape(h, w, cn)
    assert np.shares_memory(view, big) and view.strides[0] == w * cn + pad
    return view


@pytest.mark.parametrize("case", MAP_CASES, ids=[f"{c[0]}x{c[1]}c{c[2]}-r{c[3]}-t{c[4]}-{c[5]}" for c in MAP_CASES])
def test_map_matches_restatement(st, case):
    import torch
    h, w, cn, radius, thr, layout = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    n = 3 if layout == "list3" else 2
    frames = [rng.integers(0, 256, (h, w, cn), dtype=np.uint8) for _ in range(n)]
    if layout == "const":
        frames[1] = np.full((h, w, cn), 91, np.uint8)
    ref = np.stack([local_sharpness_restate(f, radius, thr) for f in frames])
    lp = LocalParameters(radius, thr)
    if layout in ("host", "const"):
        got = st.local_sharpness(frames, lp)
        dgot = st.local_sharpness(torch.from_numpy(np.stack(frames)).cuda(), lp).cpu().numpy()
        assert np.array_equal(dgot, ref)
    elif layout == "device":
        got = st.local_sharpness(torch.from_numpy(np.stack(frames)).cuda(), lp).cpu().numpy()
    elif layout == "pad5":
        got = st.local_sharpness([_padded(f, 5, False) for f in frames], lp)
        dgot = st.local_sharpness([_padded(f, 5, True) for f in frames], lp).cpu().numpy()
        assert np.array_equal(dgot, ref)
    else:
        # three frames in one device buffer, unevenly spaced, the second at an odd address
        fb = h * w * cn
        offs = [0, fb + 1, 3 * fb + 8]
        big = torch.zeros(4 * fb + 16, dtype=torch.uint8, device="cuda")
        views = []
        for f, o in zip(frames, offs):
            big[o:o + fb] = torch.from_numpy(f.reshape(-1)).cuda()
            views.append(big[o:o + fb].view(h, w, cn))
        got = st.local_sharpness(views, lp).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (n, h, w)
    assert np.array_equal(got, ref)
    if layout == "const":
        assert (got[1] == 0).all()
    assert st.timing()["prep_ms"] > 0


# ---- 2. the fold against the restatement, bit for bit ------------------------------------------------------------------
def engine_omega(st, maps, warps, idx, is_affine):
    """omega_i: channel 0 of the engine's LINEAR sample of map_i replicated to three f32 channels, BORDER_CONSTANT 0, alpha 1."""
    return np.stack([np.asarray(st.warp_accumulate(np.repeat(maps[i][..., None], 3, axis=2), warps[i], acc=None, is_affine=is_affine,
                                                   border_mode=BORDER_CONSTANT, border_value=(0, 0, 0, 0), alpha=1.0))[..., 0] for i in idx])


def _fold_case(st, case, interp, n=9, reach=6.0):
    import torch
    dtype, cn, affine, border, _, sub, _, _, (h, w) = case
    rng = np.random.default_rng(zlib.crc32(("local" + str(case)).encode()))
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine, reach=reach)
    include = [1] * n
    include[4] = 0
    idx = [i for i in range(n) if include[i]]
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(np.float32)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(np.float32)
    wt = rng.uniform(0.0, 2.0, n).astype(np.float32)
    wt[2] = 0.0
    maps = rng.integers(0, 5000, (n, h, w)).astype(np.float32)
    maps[3] = 0.0
    kw = dict(is_affine=affine, border_mode=border, border_value=(0, 0, 0, 0), alpha=_ALPHA[dtype])
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    st.set_option("warp_subpixel_bits", sub)
    try:
        if border != BORDER_CONSTANT:
            with pytest.raises(InvalidParams, match="BORDER_CONSTANT"):
                st.local_weighted_stack(frames, warps, maps, g, o, wt, include, **kw)
            return
        # kappa and omega are the linear fold's, whatever warp_interpolation says; the samples follow the option
        kappa = engine_kappa(st, (h, w), warps, idx, affine)
        omega = engine_omega(st, maps, warps, idx, affine)
        st.set_option("warp_interpolation", interp)
        samples = engine_samples(st, frames, warps, idx, **kw)
        got = {}
        for power, floor in ((1, 0.0), (2, 1.0), (4, 1.0), (4, 0.0), (1, 1.0), (2, 0.0)):
            got[(power, floor)] = st.local_weighted_stack(frames, warps, maps, g, o, wt, include, floor=floor, power=power,
                                                          return_coverage=True, **kw)
        dout, dden = st.local_weighted_stack(dframes, warps, torch.from_numpy(maps).cuda(), g, o, wt, include, floor=1.0, power=2,
                                             return_coverage=True, **kw)
        only = st.local_weighted_stack(frames, warps, maps, g, o, wt, include, floor=1.0, power=2, **kw)
    finally:
        st.set_option("warp_interpolation", 1)
        st.set_option("warp_subpixel_bits", 0)
    rim = ((kappa >= 0) & (kappa < 1)).mean()
    assert rim >= 0.03, rim
    assert (omega >= 0).all() and (omega[idx.index(3)] == 0).all() and omega.max() > 1000
    for (power, floor), (out, den) in got.items():
        ref, ref_den = local_weighted_restate(samples, kappa, omega, g[idx], o[idx], wt[idx], floor, power)
        assert np.array_equal(den, ref_den), (power, floor)
        assert np.array_equal(out, ref, equal_nan=True), (power, floor)
        assert np.isfinite(ref_den).all() and (ref_den > 0).any()
    ref, ref_den = local_weighted_restate(samples, kappa, omega, g[idx], o[idx], wt[idx], 1.0, 2)
    assert np.array_equal(dden.cpu().numpy(), ref_den) and np.array_equal(dout.cpu().numpy(), ref, equal_nan=True)
    assert np.array_equal(only, got[(2, 1.0)][0], equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=_CASE_IDS)
def test_local_weighted_stack_matches_restatement(st, case):
    _fold_case(st, case, 1)


def test_local_weighted_stack_cubic_samples_linear_weights(st):
    case = CASES[0]
    assert case[5] == 0                     # cubic is defined on exact coordinates only
    _fold_case(st, case, 2)


# launch_local_fold at every cell of depth x channels x interpolation x motion model (the one (depth, cn) ladder decides the
# kernel). 70 x 6: the 64-wide and the 4-row tile both have a ragged second tile; 5 frames, 4 of them included, shifts of up to 2 px so
# that every frame keeps rows inside.
@pytest.mark.parametrize("interp", [1, 2], ids=["linear", "cubic"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "persp"])
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_local_weighted_stack_at_every_launcher_cell(st, dtype, cn, affine, interp):
    _fold_case(st, (dtype, cn, affine, BORDER_CONSTANT, None, 0, None, None, (6, 70)), interp, n=5, reach=2.0)


def test_null_records_mean_unit_records(st):
    rng = np.random.default_rng(8)
    frames = random_frames(rng, 4, 33, 70, 3, np.uint8)
    warps = shifted_warps(rng, 4, False)
    maps = rng.integers(0, 5000, (4, 33, 70)).astype(np.float32)
    a = st.local_weighted_stack(frames, warps, maps)
    b = st.local_weighted_stack(frames, warps, maps, np.ones((4, 3)), np.zeros((4, 3)), np.ones(4))
    assert np.array_equal(a, b)


# ---- 3. a constant scene on the rim -------------------------------------------------------------------------------------
def test_constant_scene_comes_back_constant_on_the_rim(st):
    rng = np.random.default_rng(11)
    n, h, w = 9, 48, 80
    frames = [np.full((h, w, 3), 153, np.uint8) for _ in range(n)]
    v = np.float32(153) * np.float32(1.0 / 255.0)
    warps = []
    for _ in range(n):
        M = np.eye(3)
        M[:2, 2] = rng.uniform(1.0, 6.0, 2)
        warps.append(M)
    maps = st.local_sharpness(frames, LocalParameters())
    assert (maps == 0).all()
    for power in (1, 2, 3, 4):
        out, den = st.local_weighted_stack(frames, warps, maps, floor=1.0, power=power, return_coverage=True)
        cov = den > 0
        assert (~cov).any() and (den[cov] < n).any() and (den == n).any()
        rel = np.abs(out[cov].astype(np.float64) - float(v)) / float(v)
        print("constant scene, power", power, ": max relative error", rel.max() / 2.0 ** -24, "x 2^-24")
        # the issue's bound: about twice what an f32 prototype of this case measured (3.4 x 2^-24)
        assert rel.max() <= 8 * 2.0 ** -24
        assert (out[~cov] == 0).all()
        zero = st.local_weighted_stack(frames, warps, maps, floor=0.0, power=power)
        assert (zero == 0).all()


# ---- 4. ground truth ------------------------------------------------------------------------------------------------------
def test_quality_stack_through_the_engine(st):
    scene, frames = quality_stack()
    bgr = [np.repeat(f[..., None], 3, axis=2) for f in frames]
    I = [np.eye(3)] * len(bgr)
    lp = LocalParameters(QS["radius"], QS["threshold"], QS["power"], QS["floor"])
    maps = st.local_sharpness(bgr, lp)
    out = st.local_weighted_stack(bgr, I, maps, floor=lp.floor, power=lp.power)
    mean = st.local_weighted_stack(bgr, I, np.zeros_like(maps), floor=1.0, power=1)
    ref, _ = quality_stack_restated(frames)
    r_engine, r_ref = interior_rms(out[..., 0] * 255.0, scene), interior_rms(ref, scene)
    r_mean = interior_rms(mean[..., 0] * 255.0, scene)
    print("quality stack: RMS engine", r_engine, "restatement", r_ref, "plain mean", r_mean)
    assert abs(r_engine - r_ref) <= 0.01 * r_ref
    assert r_engine <= 0.45 * r_mean
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])


# ---- 5. composition, bit for bit ----------------------------------------------------------------------------------------
def _stats_equal(a, b):
    for x, y in zip(a, b):
        assert x["status"] == y["status"] and x["iterations"] == y["iterations"] and x["rho"] == y["rho"]
        assert x["n_matches"] == y["n_matches"] and np.array_equal(x["warp"], y["warp"])


@pytest.fixture(scope="module")
def small_stack():
    frames, _ = synth.make_stack(6, 128, 96)
    return frames.numpy()


def test_ecc_match_local_weighted_equals_its_parts(st, small_stack):
    import torch
    host = small_stack
    dev = torch.from_numpy(host).cuda()
    lp = LocalParameters(3, 8, 3, 0.5)
    wp = WeightParameters(LINEAR, True, 2)
    weights = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0]
    out, den, applied, stats = st.ecc_match_local_weighted(dev, ECC, lp, wp, weights, return_stats=True, return_coverage=True,
                                                           return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    _stats_equal(stats, pstats)
    warps = [s["warp"] for s in stats]
    maps = st.local_sharpness(dev, lp)
    ref, ref_den = st.local_weighted_stack(dev, warps, maps, applied=applied, floor=lp.floor, power=lp.power, return_coverage=True)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.array_equal(den.cpu().numpy(), ref_den.cpu().numpy())
    assert [a["weight"] for a in applied] == weights and applied[0]["gain"].tolist() == [1, 1, 1]
    assert float(maps.max()) > 0 and np.isfinite(out.cpu().numpy()).all()
    # the weighted call's records: the normalisation is the existing moments pass
    _, wapplied = st.ecc_match_weighted(dev, ECC, wp, weights, return_applied=True)
    for a, b in zip(applied, wapplied):
        assert np.array_equal(a["gain"], b["gain"]) and np.array_equal(a["offset"], b["offset"]) and a["flags"] == b["flags"]
    # host-fed: the same bits, outputs on the host
    hout, hden = st.ecc_match_local_weighted(host, ECC, lp, wp, weights, return_coverage=True)
    assert np.array_equal(hout, out.cpu().numpy()) and np.array_equal(hden, den.cpu().numpy())
    # maps from the full-size frames under scale_down_width too
    sout, sapp, sstats = st.ecc_match_local_weighted(dev, ECC, lp, wp, weights, scale_down_width=96.0, return_stats=True,
                                                     return_applied=True)
    sref = st.local_weighted_stack(dev, [s["warp"] for s in sstats], maps, applied=sapp, floor=lp.floor, power=lp.power)
    assert np.array_equal(sout.cpu().numpy(), sref.cpu().numpy())
    # a multi-device context runs the call on its first device: the single-device bits
    multi = Stacker(devices=[0, 0])
    try:
        mo = multi.ecc_match_local_weighted(dev, ECC, lp, wp, weights)
    finally:
        multi.close()
    assert np.array_equal(mo.cpu().numpy(), out.cpu().numpy())


def test_keypoint_match_local_weighted_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 640, 480)
    frames = frames.numpy()
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    weights = [1.0, 2.0, 3.0, 0.5, 1.0]
    lp = LocalParameters()
    wp = WeightParameters(LINEAR, True, 2)
    dropped, out, den, applied, stats = st.keypoint_match_local_weighted(stack, KP, lp, wp, weights, return_stats=True,
                                                                         return_coverage=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[2]["status"] == 1
    _stats_equal(stats, pstats)
    assert applied[2]["weight"] == 0.0 and applied[2]["gain"].tolist() == [1, 1, 1] and applied[2]["offset"].tolist() == [0, 0, 0]
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    maps = st.local_sharpness(stack, lp)
    ref, ref_den = st.local_weighted_stack(stack, warps, maps, applied=applied, include=include, floor=lp.floor, power=lp.power,
                                           return_coverage=True)
    assert np.array_equal(out, ref) and np.array_equal(den, ref_den)


# ---- 6. layout and repeatability ----------------------------------------------------------------------------------------
def test_layout_repeatability_and_options(st, small_stack):
    import torch
    host = small_stack
    lp, wp = LocalParameters(), WeightParameters(LINEAR, True, 0)
    base, bden = st.ecc_match_local_weighted(host, ECC, lp, wp, return_coverage=True)
    again, aden = st.ecc_match_local_weighted(host, ECC, lp, wp, return_coverage=True)
    assert np.array_equal(again, base) and np.array_equal(aden, bden)
    dev = st.ecc_match_local_weighted(torch.from_numpy(host).cuda(), ECC, lp, wp)
    assert np.array_equal(dev.cpu().numpy(), base)
    padded = st.ecc_match_local_weighted([_padded(f, 5, False) for f in host], ECC, lp, wp)
    assert np.array_equal(padded, base)
    dpadded = st.ecc_match_local_weighted([_padded(f, 5, True) for f in host], ECC, lp, wp)
    assert np.array_equal(dpadded.cpu().numpy(), base)
    for name, val, back in (("quantile_band_rows", 7, 0), ("ecc_slots", 4, 0)):
        st.set_option(name, val)
        try:
            other = st.ecc_match_local_weighted(host, ECC, lp, wp)
            omaps = st.local_sharpness(host, lp)
        finally:
            st.set_option(name, back)
        assert np.array_equal(other, base), name
        assert np.array_equal(omaps, st.local_sharpness(host, lp)), name
    # the fold alone: padded rows and device frames give the tight host stack's bits
    rng = np.random.default_rng(6)
    warps = shifted_warps(rng, len(host), False)
    maps = st.local_sharpness(host, lp)
    tight = st.local_weighted_stack(host, warps, maps)
    assert np.array_equal(st.local_weighted_stack([_padded(f, 5, False) for f in host], warps, maps), tight)
    assert np.array_equal(st.local_weighted_stack([_padded(f, 5, True) for f in host], warps, maps).cpu().numpy(), tight)
    assert np.array_equal(st.local_weighted_stack(host, warps, maps), tight)


# ---- 7. errors --------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected(st, small_stack):
    frames = small_stack[:3]
    I = [np.eye(3)] * 3
    maps = np.ones((3, 96, 128), np.float32)
    bad = [(LocalParameters(radius=0), "radius"), (LocalParameters(radius=16), "radius"),
           (LocalParameters(threshold=-1), "threshold"), (LocalParameters(threshold=1021), "threshold"),
           (LocalParameters(power=0), "power"), (LocalParameters(power=5), "power"),
           (LocalParameters(floor=-1.0), "floor"), (LocalParameters(floor=float("nan")), "floor"),
           (LocalParameters(floor=float("inf")), "floor")]
    for lp, field in bad:
        with pytest.raises(InvalidParams, match=field):
            st.local_sharpness(frames, lp)
        with pytest.raises(InvalidParams, match=field):
            st.ecc_match_local_weighted(frames, ECC, lp)
        with pytest.raises(InvalidParams, match=field):
            st.keypoint_match_local_weighted(frames, KP, lp)
    for power, floor, field in ((0, 1.0, "power"), (5, 1.0, "power"), (2, -1.0, "floor"), (2, float("nan"), "floor"),
                                (2, float("inf"), "floor")):
        with pytest.raises(InvalidParams, match=field):
            st.local_weighted_stack(frames, I, maps, floor=floor, power=power)
    for call in (lambda: st.ecc_match_local_weighted(frames, ECC, LocalParameters(), WeightParameters(LINEAR, False)),
                 lambda: st.keypoint_match_local_weighted(frames, KP, LocalParameters(), WeightParameters(LINEAR, False))):
        with pytest.raises(InvalidParams, match="coverage"):
            call()
    with pytest.raises(InvalidParams, match="border_value"):
        st.local_weighted_stack(frames, I, maps, border_value=(0, 0.5, 0, 0))
    with pytest.raises(InvalidParams, match="border_mode"):
        st.local_weighted_stack(frames, I, maps, border_mode=BORDER_REPLICATE)
    with pytest.raises(InvalidParams, match="border_mode"):
        st.keypoint_match_local_weighted(frames, KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9, BORDER_REPLICATE))
    with pytest.raises(InvalidParams, match="weight"):
        st.local_weighted_stack(frames, I, maps, weights=[0, 0, 0])
    with pytest.raises(InvalidParams, match="weight"):
        st.ecc_match_local_weighted(frames, ECC, weights=[1, -1, 1])
    for dtype in (np.uint16, np.float32):
        deep = [f.astype(dtype) for f in frames]
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.local_sharpness(deep)
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.ecc_match_local_weighted(deep, ECC)
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.keypoint_match_local_weighted(deep, KP)
        st.local_weighted_stack(deep, I, maps, alpha=_ALPHA[dtype])          # the fold alone takes any depth
    # under cubic the pair of fold options is checked at the call
    st.set_option("warp_interpolation", 2)
    st.set_option("warp_subpixel_bits", 5)
    try:
        with pytest.raises(InvalidParams, match="warp_subpixel_bits"):
            st.local_weighted_stack(frames, I, maps)
    finally:
        st.set_option("warp_subpixel_bits", 0)
        st.set_option("warp_interpolation", 1)


def test_reserved_and_null_pointers_are_rejected(st, small_stack):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    m = _Marshalled(small_stack[:3])
    out = np.empty((96, 128, 3), np.float32)
    img = _ffi.ImageF32(out.ctypes.data, 128, 96, 3, HOST, 0)
    planes = np.ones((3, 96, 128), np.float32)
    ptrs = (C.c_void_p * 3)(*[planes.ctypes.data + i * planes[0].nbytes for i in range(3)])
    pp = C.cast(ptrs, C.c_void_p)
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    ep, kp, wp, lp = ECC._c(), KP._c(), WeightParameters()._c(), LocalParameters()._c()
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    dropped = C.c_int32(0)
    bad = LocalParameters()._c()
    bad.reserved[1] = 1
    assert lib.stk_local_sharpness(h, fr, C.byref(bad), pp) == 2
    assert b"reserved" in lib.stk_last_error(h)
    assert lib.stk_ecc_match_local_weighted(h, fr, C.byref(ep), 0.0, C.byref(wp), None, C.byref(bad), C.byref(img), None, None, None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    assert lib.stk_local_sharpness(h, fr, None, pp) == 2 and lib.stk_local_sharpness(h, fr, C.byref(lp), None) == 2
    assert lib.stk_ecc_match_local_weighted(h, fr, C.byref(ep), 0.0, C.byref(wp), None, None, C.byref(img), None, None, None) == 2
    assert lib.stk_keypoint_match_local_weighted(h, fr, C.byref(kp), 0.0, None, None, C.byref(lp), C.byref(img), C.byref(dropped), None,
                                                 None, None) == 2
    assert lib.stk_local_weighted_stack(h, fr, None, None, 0, 0, None, 1.0 / 255, None, pp, 1.0, 2, C.byref(img), None) == 2
    assert lib.stk_local_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, None, 1.0, 2, C.byref(img), None) == 2
    assert lib.stk_local_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, pp, 1.0, 2, C.byref(img), None) == 0
    assert lib.stk_local_sharpness(h, fr, C.byref(lp), pp) == 0

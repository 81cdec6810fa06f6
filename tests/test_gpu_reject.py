"""Blot-and-compare rejection maps (include/stacker.h, stk_reject_params) on the GPU: stk_reject_maps against the f32
restatement (reject_restate.py), every map and both counts EXACTLY (every operation of the definition is restated, so
there is no tolerance); tile seams, the frame's edge, strided frames with poisoned padding, degenerate sizes, in-place maps,
determinism, the quality experiment on the device, the whole-stack forms against their parts, and every refusal. Frames are
65 x 53 (w x h): no multiple of the 64 x 16 tile, 2 x 4 tiles."""
import numpy as np
import pytest

import drizzle_restate as dr
import reject_restate as rr
from libstacker_rs_amd import (RANSAC, DrizzleParameters, EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType,
                               RejectParameters, Stacker, WeightParameters, synth)

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 65, 53
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)


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


def place(x, device):
    if x is None or not device:
        return x
    import torch
    if isinstance(x, (list, tuple)):
        return [place(v, device) for v in x]
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def params(**kw):
    base = dict(snr1=4.0, snr2=3.0, scale1=1.2, scale2=0.7, read_noise=0.01, poisson_gain=0.0, min_count=0)
    base.update(kw)
    return RejectParameters(**base)


def run(st, frames, warps, clean, p, device, counts=None, maps=None, **kw):
    maps_d = None if maps is None else [place(m, device) for m in maps]
    out, rej, jud = st.reject_maps(place(list(frames), device), warps, place(clean, device), p, place(counts, device), maps=maps_d,
                                   return_counts=True, **kw)
    return host(out), rej, jud


# ---- 1. every depth, channel count and table kind against the f32 restatement, exactly -----------------------------------
FORMATS = [(np.uint8, 1.0 / 255.0, 255.0), (np.uint16, 1.0 / 65535.0, 65535.0), (np.float32, 1.0, 1.0)]
CASES = [(fi, cn, kind) for fi in range(3) for cn in (1, 3, 4) for kind in ("affine", "perspective")]


def smooth_image(rng, h, w, cn):
    """A smooth image in [0.25, 0.75]: three cosines per channel with periods of 12 pixels and more."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, cn))
    for c in range(cn):
        for _ in range(3):
            fx, fy, ph = rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), rng.uniform(0, 2 * np.pi)
            img[..., c] += np.cos(2 * np.pi * (fx * x + fy * y) + ph) / 12.0
    return (0.5 + img).astype(F)


def general_case(idx):
    """Inputs of case idx: a smooth clean image; frames that are the blotted model (f64 restatement) brought to the frame's
    level and format, plus noise of sigma 0.01, with 4 % of the pixels moved by 0.03 .. 0.2 (outliers from just under the
    grow threshold to far beyond the first) and white noise where the model does not reach. Records, counts, input maps, N and
    the location follow the index so that every combination of the issue's list occurs."""
    fi, cn, kind = CASES[idx]
    dtype, alpha, full = FORMATS[fi]
    rng = np.random.default_rng(700 + idx)
    n = 3 + ((idx // 3) & 1)
    affine = kind == "affine"
    clean = smooth_image(rng, H, W, cn)
    if affine:
        warps = [rot(30.0 * (1 if k % 2 else -1), W / 2, H / 2, *rng.uniform(-2, 2, 2)) if k else np.eye(3) for k in range(n)]
    else:
        warps = []
        for k in range(n):
            M = rot(rng.uniform(-4, 4), W / 2, H / 2, *rng.uniform(-3, 3, 2))
            M[2, 0], M[2, 1] = rng.uniform(-4e-4, 4e-4, 2)
            warps.append(M if k else np.eye(3))
    bits = (idx * 7 + 3) % 16                                 # (0 .. 17 -> every one of the 16 combinations)
    with_records, with_counts, with_maps, device = bool(bits & 1), bool(bits & 2), bool(bits & 4), bool(bits & 8)
    gain = rng.uniform(0.8, 1.25, (n, cn)).astype(F) if with_records else None
    offset = rng.uniform(-0.05, 0.05, (n, cn)).astype(F) if with_records else None
    counts = rng.integers(1, 7, (H, W)).astype(np.int32) if with_counts else None
    p = params(poisson_gain=2e-4 if idx % 3 else 0.0, min_count=2 if with_counts else 0)
    frames = []
    for k in range(n):
        B, valid = rr.blot(clean, warps[k], affine, dtype=np.float64, halo=0)
        v = np.where(valid[..., None], B, rng.uniform(0.2, 0.8, (H, W, cn)))
        v = v + rng.normal(0, 0.01, v.shape)
        hit = rng.random((H, W)) < 0.04
        v = v + hit[..., None] * rng.uniform(0.03, 0.2, (H, W, 1)) * rng.choice([-1.0, 1.0], (H, W, 1))
        if with_records:
            v = (v - offset[k].astype(np.float64)) / gain[k].astype(np.float64)
        v = np.clip(v, 0.0, 1.0) * full
        frames.append(np.rint(v).astype(dtype) if dtype != np.float32 else v.astype(F))
    maps = None
    if with_maps:
        maps = []
        for k in range(n):
            m = rng.uniform(0.25, 2.0, (H, W)).astype(F)
            m[rng.random((H, W)) < 0.1] = 0.0
            maps.append(None if k == 1 else m)
    return dict(frames=frames, warps=warps, affine=affine, alpha=alpha, clean=clean, p=p, counts=counts, gain=gain, offset=offset,
                maps=maps, device=device, n=n)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{np.dtype(FORMATS[f][0]).name}c{c}-{k}" for f, c, k in CASES])
def test_maps_and_counts_equal_the_f32_restatement(st, idx):
    c = general_case(idx)
    ref, rrej, rjud = rr.reject_maps(c["frames"], c["warps"], c["affine"], c["alpha"], c["clean"], c["p"], c["counts"], c["gain"],
                                     c["offset"], c["maps"])
    out, rej, jud = run(st, c["frames"], c["warps"], c["clean"], c["p"], c["device"], c["counts"], c["maps"], gain=c["gain"],
                        offset=c["offset"], is_affine=c["affine"], alpha=c["alpha"])
    assert st.timing()["finalize_ms"] > 0
    print(f"case {idx}: rejected {rrej.tolist()} of judged {rjud.tolist()} of {H * W}")
    for k in range(c["n"]):                                  # both answers occur, and some pixels cannot be compared
        assert 0 < rrej[k] < rjud[k] < H * W
    assert np.array_equal(rej, rrej) and np.array_equal(jud, rjud)
    assert np.array_equal(out, ref)


def test_excluded_frames_are_not_written_and_count_nothing(st):
    c = general_case(3)
    assert c["n"] == 4
    include = [1, 0, 1, 1]
    ref, rrej, rjud = rr.reject_maps(c["frames"], c["warps"], c["affine"], c["alpha"], c["clean"], c["p"], c["counts"], c["gain"],
                                     c["offset"], c["maps"], include=include)
    import torch
    buf = torch.full((c["n"], H, W), 7.0, dtype=torch.float32, device="cuda")
    out, rej, jud = st.reject_maps(place(c["frames"], True), c["warps"], place(c["clean"], True), c["p"], place(c["counts"], True),
                                   gain=c["gain"], offset=c["offset"], include=include, out=buf, is_affine=c["affine"], alpha=c["alpha"],
                                   return_counts=True)
    assert out is buf and rej[1] == 0 and jud[1] == 0 and np.array_equal(rej, rrej) and np.array_equal(jud, rjud)
    got = host(buf)
    assert np.array_equal(got[1], np.full((H, W), 7.0, F)) and np.array_equal(got[[0, 2, 3]], ref[[0, 2, 3]])


# ---- 2. tile seams ------------------------------------------------------------------------------------------------------------
def test_flags_cross_the_tile_seams(st):
    """The tile is 64 x 16: (63, 15), (64, 15), (63, 16), (64, 16) lie in four different tiles around one corner. Frame k has a
    first-pass outlier (+0.05 against 4 x 0.01) at corner k and grow-only values (+0.035) at the other three, each across a
    seam (or the corner) from it: all four are rejected in every frame, nothing else is. Under the forward shift (-2, -2)
    column 64 and row 52 are judged."""
    corners = [(63, 15), (64, 15), (63, 16), (64, 16)]
    clean = np.full((H, W, 1), 0.5, F)
    frames = []
    for k in range(4):
        f = clean.copy()
        for j, (x, y) in enumerate(corners):
            f[y, x] = 0.55 if j == k else 0.535
        frames.append(f)
    warps = [shift(-2, -2)] * 4
    ref, rrej, rjud = rr.reject_maps(frames, warps, False, 1.0, clean, params())
    out, rej, jud = run(st, frames, warps, clean, params(), True, alpha=1.0)
    want = np.ones((H, W), F)
    for x, y in corners:
        want[y, x] = 0
    for k in range(4):
        assert np.array_equal(out[k], want)
    assert np.array_equal(out, ref) and rej.tolist() == [4] * 4 == rrej.tolist() and np.array_equal(jud, rjud)
    assert jud.tolist() == [(W - 2) * (H - 2)] * 4
    # without the outlier the grow-only values stay
    lone = clean.copy()
    for x, y in corners:
        lone[y, x] = 0.535
    out, rej, _ = run(st, [lone], warps[:1], clean, params(), True, alpha=1.0)
    assert rej[0] == 0 and np.array_equal(out[0], np.ones((H, W), F))


# ---- 3. the frame's edge ------------------------------------------------------------------------------------------------------
def edge_case():
    """Frame 0 under the identity (columns 0 .. W - 2, rows 0 .. H - 2 judged): outliers on column 0 and row 0. Frame 1 under
    the forward shift (-2, -2) (columns 2 .. W - 1, rows 2 .. H - 1 judged): outliers on column W - 1 and row H - 1. Every
    other pixel of those edge columns and rows holds a grow-only value: an outlier invented beyond the edge would reject its
    neighbours on the edge."""
    clean = np.full((H, W, 1), 0.5, F)
    a, b = clean.copy(), clean.copy()
    a[:, 0], a[0, :] = 0.535, 0.535
    b[:, W - 1], b[H - 1, :] = 0.535, 0.535
    for y in (0, 7, 16, 30, H - 2):
        a[y, 0] = 0.9
        b[min(y + 2, H - 1), W - 1] = 0.9
    for x in (5, 63, 40):
        a[0, x] = 0.9
        b[H - 1, x + 1] = 0.9
    return [a, b], [np.eye(3), shift(-2, -2)], clean


def window(frame, device, poison):
    """The frame as a window of a larger canvas filled with `poison`."""
    h, w, cn = frame.shape
    canvas = np.full((h + 3, w + 5, cn), poison, frame.dtype)
    canvas[1:1 + h, 2:2 + w] = frame
    if device:
        import torch
        return torch.from_numpy(canvas).cuda()[1:1 + h, 2:2 + w]
    return canvas[1:1 + h, 2:2 + w]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_the_frames_edge_and_poisoned_padding(st, device):
    frames, warps, clean = edge_case()
    ref, rrej, rjud = rr.reject_maps(frames, warps, False, 1.0, clean, params())
    out, rej, jud = run(st, frames, warps, clean, params(), device, alpha=1.0)
    assert np.array_equal(out, ref) and np.array_equal(rej, rrej) and np.array_equal(jud, rjud)
    # the planted outliers and their neighbours along the edge are rejected, the rest of the edge is kept
    assert out[0][7, 0] == 0 and out[0][6, 0] == 0 and out[0][8, 0] == 0 and out[0][10, 0] == 1 and out[0][0, 20] == 1
    assert out[1][9, W - 1] == 0 and out[1][H - 1, 41] == 0 and out[1][H - 1, 20] == 1 and out[1][20, W - 1] == 1
    assert jud.tolist() == [(W - 1) * (H - 1), (W - 2) * (H - 2)]
    # strided: windows of canvases whose padding holds an outlier's value; what lies beyond the edge never reaches a map
    from libstacker_rs_amd.api import _Marshalled
    views = [window(f, device, 9.0) for f in frames]
    assert _Marshalled(views).c_frames.row_stride_bytes == (W + 5) * 4
    sout, srej, sjud = st.reject_maps(views, warps, place(clean, device), params(), alpha=1.0, return_counts=True)
    assert np.array_equal(host(sout), out) and np.array_equal(srej, rej) and np.array_equal(sjud, jud)


# ---- 4. degenerate sizes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_degenerate_sizes(st, device):
    rng = np.random.default_rng(11)
    clean = np.full((3, 5, 3), 0.5, F)
    frames = [np.clip(rng.normal(0.5, 0.02, (3, 5, 3)), 0, 1).astype(F) for _ in range(3)]
    warps = [np.eye(3), shift(1, 0), shift(-1, -1)]
    ref, rrej, rjud = rr.reject_maps(frames, warps, False, 1.0, clean, params())
    out, rej, jud = run(st, frames, warps, clean, params(), device, alpha=1.0)
    assert np.array_equal(out, ref) and np.array_equal(rej, rrej) and np.array_equal(jud, rjud)
    assert 0 < rrej.sum() < rjud.sum() and rjud.tolist() == [8, 6, 8]
    # 1 x 1: nothing is valid, everything is kept: 1, or the input map
    one = [np.full((1, 1, 1), 200, np.uint8), np.full((1, 1, 1), 0, np.uint8)]
    c1 = np.full((1, 1, 1), 0.5, F)
    out, rej, jud = run(st, one, [np.eye(3)] * 2, c1, params(), device)
    assert np.array_equal(out, np.ones((2, 1, 1), F)) and rej.tolist() == [0, 0] and jud.tolist() == [0, 0]
    out, rej, jud = run(st, one, [np.eye(3)] * 2, c1, params(), device, maps=[np.full((1, 1), 0.25, F), None])
    assert out[:, 0, 0].tolist() == [0.25, 1.0] and jud.tolist() == [0, 0]


# ---- 5. in place, and the same bits on every call -----------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_in_place_maps_and_determinism(st, device):
    c = general_case(4)                                   # (records, counts and input maps)
    assert c["maps"] is not None
    planes = np.stack([np.ones((H, W), F) if m is None else m for m in c["maps"]])
    kw = dict(gain=c["gain"], offset=c["offset"], is_affine=c["affine"], alpha=c["alpha"], return_counts=True)
    fr, cl, cn = place(c["frames"], device), place(c["clean"], device), place(c["counts"], device)
    a, arej, ajud = st.reject_maps(fr, c["warps"], cl, c["p"], cn, maps=place(planes, device), **kw)
    b, brej, bjud = st.reject_maps(fr, c["warps"], cl, c["p"], cn, maps=place(planes, device), **kw)
    assert np.array_equal(host(a), host(b)) and np.array_equal(arej, brej) and np.array_equal(ajud, bjud)
    buf = place(planes.copy(), device)
    o, orej, ojud = st.reject_maps(fr, c["warps"], cl, c["p"], cn, maps=buf, out=buf, **kw)
    assert o is buf
    assert np.array_equal(host(buf), host(a)) and np.array_equal(orej, arej) and np.array_equal(ojud, ajud)
    assert 0 < arej.sum() and (host(a)[planes == 0] == 0).all()
    # warp_interpolation is ignored: the model is always bilinear
    st.set_option("warp_interpolation", 2)
    try:
        d, drej, _ = st.reject_maps(fr, c["warps"], cl, c["p"], cn, maps=place(planes, device), **kw)
    finally:
        st.set_option("warp_interpolation", 1)
    assert np.array_equal(host(d), host(a)) and np.array_equal(drej, arej)


# ---- 6. the quality experiment on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quality_on_the_device(st, seed):
    """test_cpu_reject's stack through the engine: median (quantile_stack_weighted) -> reject_maps -> drizzle_stack, with the
    same three assertions. Measured on an MI355X, seeds 1, 2, 3: see DESIGN 4.16."""
    import torch
    bad, good, warps, planted = rr.reject_stack(seed)
    dev = torch.from_numpy(bad).cuda()
    clean, cnt = st.quantile_stack_weighted(dev, warps, 0.5, coverage=True, return_counts=True)
    p = rr.quality_params()
    maps, rej, jud = st.reject_maps(dev, warps, clean, p, cnt, return_counts=True)
    dz = DrizzleParameters(scale=2.0, pixfrac=0.7)
    with_maps = host(st.drizzle_stack(dev, warps, dz, maps=list(maps)))
    without = host(st.drizzle_stack(dev, warps, dz))
    reference = host(st.drizzle_stack(torch.from_numpy(good).cuda(), warps, dz))
    judged = np.stack([rr.blot(host(clean), warps[i], False, host(cnt), p.min_count, halo=0)[1] for i in range(len(bad))])
    assert np.array_equal(judged.sum(axis=(1, 2)), jud) and np.array_equal((host(maps) == 0).sum(axis=(1, 2)), rej)
    hit, false_alarm, ratio, e_with, e_without = rr.quality_measures(host(maps), judged, planted, with_maps * 255.0, without * 255.0,
                                                                     reference * 255.0)
    print(f"seed {seed}: core rejected {hit:.4f}, clean rejected {false_alarm:.6f}, rms {e_with:.4f} / {e_without:.4f} = {ratio:.4f}")
    assert hit >= 0.85
    assert false_alarm <= 0.005
    assert ratio <= 0.3


# ---- 7. the whole-stack forms equal their parts --------------------------------------------------------------------------------
def _stats_equal(a, b):
    for x, y in zip(a, b):
        assert x["status"] == y["status"] and x["iterations"] == y["iterations"] and x["rho"] == y["rho"]
        assert x["n_matches"] == y["n_matches"] and np.array_equal(x["warp"], y["warp"])


def _applied_equal(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x["gain"], y["gain"]) and np.array_equal(x["offset"], y["offset"])
        assert x["weight"] == y["weight"] and x["flags"] == y["flags"]


def streak(frames, k):
    """The stack with a bright streak of three pixels' width across frame k (a numpy copy)."""
    f = np.array(frames)
    h, w = f.shape[1:3]
    for x in range(8, w - 8):
        y = int(0.2 * h + 0.45 * x * h / w)
        f[k, y - 1:y + 2, x] = np.minimum(f[k, y - 1:y + 2, x].astype(np.int32) + 90, 255).astype(np.uint8)
    return f


def rms(a, b):
    return float(np.sqrt(np.mean((host(a).astype(np.float64) - host(b).astype(np.float64)) ** 2)))


def test_ecc_match_drizzle_rejected_equals_its_parts(st):
    import torch
    frames, _ = synth.make_stack(6, 128, 96)
    bad = streak(frames.numpy(), 3)
    dev = torch.from_numpy(bad).cuda()
    dz = DrizzleParameters(scale=1.5, pixfrac=0.7)
    wp, rp = WeightParameters(normalize=3, coverage=True), RejectParameters()
    out, den, maps, rej, applied, stats = st.ecc_match_drizzle_rejected(dev, ECC, dz, rp, wp, return_den=True, return_maps=True,
                                                                        return_rejected=True, return_applied=True, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    # the five parts through the API on the returned stats
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    _stats_equal(stats, pstats)
    _, papplied = st.ecc_match_weighted(dev, ECC, wp, return_applied=True)
    _applied_equal(applied, papplied)
    warps = [s["warp"] for s in stats]
    clean, cnt = st.quantile_stack_weighted(dev, warps, 0.5, applied=applied, coverage=True, return_counts=True)
    pmaps, prej, _ = st.reject_maps(dev, warps, clean, rp, cnt, applied=applied, return_counts=True)
    pout, pden = st.drizzle_stack(dev, warps, dz, applied=applied, maps=list(pmaps), return_den=True)
    assert np.array_equal(host(maps), host(pmaps)) and np.array_equal(rej, prej)
    assert np.array_equal(host(out), host(pout)) and np.array_equal(host(den), host(pden))
    assert rej[3] > 0 and np.isfinite(host(out)).all()
    # nearer the streak-free stack's drizzle than the drizzle without rejection is
    good = st.ecc_match_drizzle(frames.cuda(), ECC, dz)
    plain = st.ecc_match_drizzle(dev, ECC, dz)
    e_rej, e_plain = rms(out, good), rms(plain, good)
    print(f"ecc: rms against the streak-free drizzle: rejected {e_rej * 255:.4f}, plain {e_plain * 255:.4f} grey levels; rejected {rej.tolist()}")
    assert e_rej < e_plain
    # host-fed: the same bits
    hout, hmaps, hrej = st.ecc_match_drizzle_rejected(bad, ECC, dz, rp, wp, return_maps=True, return_rejected=True)
    assert isinstance(hout, np.ndarray) and np.array_equal(hout, host(out)) and np.array_equal(hmaps, host(maps))
    assert np.array_equal(hrej, rej)
    multi = Stacker(devices=[0, 0])                      # a multi-device context runs the call on its first device
    try:
        mo = multi.ecc_match_drizzle_rejected(dev, ECC, dz, rp, wp)
    finally:
        multi.close()
    assert np.array_equal(host(mo), host(out))


def test_keypoint_match_drizzle_rejected_equals_its_parts(st):
    frames, _ = synth.make_stack(5, 640, 480)
    bad = streak(frames.numpy(), 2)
    stack = [bad[0], bad[1], bad[2], np.full_like(bad[0], 128), bad[3], bad[4]]       # featureless: dropped
    dz = DrizzleParameters(scale=1.5, pixfrac=0.7)
    wp, rp = WeightParameters(normalize=1, coverage=True), RejectParameters()
    dropped, out, den, maps, rej, applied, stats = st.keypoint_match_drizzle_rejected(
        stack, KP, dz, rp, wp, return_den=True, return_maps=True, return_rejected=True, return_applied=True, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert dropped == pd == 1 and stats[3]["status"] == 1
    _stats_equal(stats, pstats)
    _, _, papplied = st.keypoint_match_weighted(stack, KP, wp, return_applied=True)
    _applied_equal(applied, papplied)
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    clean, cnt = st.quantile_stack_weighted(stack, warps, 0.5, applied=applied, include=include, coverage=True, return_counts=True)
    pmaps, prej, _ = st.reject_maps(stack, warps, clean, rp, cnt, applied=applied, include=include, return_counts=True)
    pout, pden = st.drizzle_stack(stack, warps, dz, applied=applied, include=include, maps=list(pmaps), return_den=True)
    assert np.array_equal(maps, pmaps) and np.array_equal(rej, prej) and rej[3] == 0 and np.array_equal(maps[3], np.ones((480, 640), F))
    assert np.array_equal(out, pout) and np.array_equal(den, pden)
    assert rej[2] > 0
    good = [frames.numpy()[0], frames.numpy()[1], frames.numpy()[2], stack[3], frames.numpy()[3], frames.numpy()[4]]
    _, gout = st.keypoint_match_drizzle(good, KP, dz)
    _, plain = st.keypoint_match_drizzle(stack, KP, dz)
    e_rej, e_plain = rms(out, gout), rms(plain, gout)
    print(f"keypoint: rms against the streak-free drizzle: rejected {e_rej * 255:.4f}, plain {e_plain * 255:.4f} grey levels; rejected {rej.tolist()}")
    assert e_rej < e_plain


# ---- 8. errors: refused on the host, nothing is launched ----------------------------------------------------------------------
def test_invalid_arguments_are_rejected(st):
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 255, (12, 16, 3)).astype(np.uint8) for _ in range(3)]
    warps = [np.eye(3)] * 3
    clean = np.full((12, 16, 3), 0.5, F)
    for bad in (dict(snr1=0.0), dict(snr2=-1.0), dict(snr1=np.inf), dict(scale1=-0.1), dict(scale2=np.nan), dict(read_noise=-1.0),
                dict(poisson_gain=np.inf), dict(min_count=-1)):
        with pytest.raises(InvalidParams):
            st.reject_maps(frames, warps, clean, params(**bad))
    st.reject_maps(frames, warps, clean, params(read_noise=0.0, poisson_gain=0.0))       # allowed: only the gradient tolerates
    with pytest.raises(InvalidParams):
        st.reject_maps(frames, warps, clean, params(), include=[0, 0, 0])
    with pytest.raises(InvalidParams):
        st.reject_maps(frames, warps, clean, params(), gain=np.full((3, 3), np.nan))
    with pytest.raises(InvalidParams):
        st.reject_maps(frames, warps, clean[:, :, :1], params())
    st.set_option("warp_subpixel_bits", 5)
    try:
        with pytest.raises(InvalidParams):
            st.reject_maps(frames, warps, clean, params())
    finally:
        st.set_option("warp_subpixel_bits", 0)
    stack, _ = synth.make_stack(3, 128, 96)
    with pytest.raises(InvalidParams):                       # coverage must be 1
        st.ecc_match_drizzle_rejected(stack.numpy(), ECC, None, None, WeightParameters(coverage=False))
    with pytest.raises(InvalidParams):
        st.keypoint_match_drizzle_rejected(stack.numpy(), KP, None, params(snr1=0.0))

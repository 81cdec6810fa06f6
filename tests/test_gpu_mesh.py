"""Local alignment on the GPU: stk_local_align / stk_mesh_stack / stk_mesh_local_weighted_stack /
stk_ecc_match_local_aligned / stk_keypoint_match_local_aligned against the numpy restatements of the definition
(test_cpu_mesh: local_align_restate, mesh_fill_restate, mesh_fold_restate) and against their own parts."""
import ctypes as C
import zlib

import numpy as np
import pytest

from interp_restate import F
from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REFLECT, BORDER_REFLECT_101, BORDER_REPLICATE, BORDER_WRAP, RANSAC,
                               EccMatchParameters, InvalidParams, KeyPointMatchParameters, LocalParameters, MeshParameters,
                               MotionType, NotImplementedYet, Stacker, mesh_grid, synth)
from test_cpu_local import local_weighted_restate
from test_cpu_mesh import (QM, _cosines, grid_restate, interior_rms, local_align_restate, mesh_fill_restate, mesh_fold_restate,
                           mesh_mean_restate, quality_mesh_restated, quality_mesh_stack)

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
_ALPHA = {np.uint8: 1.0 / 255.0, np.uint16: 1.0 / 65535.0, np.float32: 1.0}
_SCALE = {np.uint8: 255.0, np.uint16: 65535.0, np.float32: 1.0}


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _padded(frame, pad, device):
    """The frame as a row-strided view of a buffer whose rows are `pad` bytes longer."""
    h, w, cn = frame.shape
    if device:
        import torch
        big = torch.zeros((h, w * cn + pad), dtype=torch.uint8, device="cuda")
        big[:, :w * cn] = torch.from_numpy(frame.reshape(h, w * cn)).cuda()
        return big[:, :w * cn].unflatten(1, (w, cn))
    big = np.zeros((h, w * cn + pad), np.uint8)
    big[:, :w * cn] = frame.reshape(h, w * cn)
    return big[:, :w * cn].reshape(h, w, cn)


def _odd_base(frames):
    """The frames in one device buffer, unevenly spaced, every one but the first at an odd address."""
    import torch
    h, w, cn = frames[0].shape
    fb = h * w * cn
    big = torch.zeros(len(frames) * (fb + 8) + 8, dtype=torch.uint8, device="cuda")
    views, o = [], 0
    for f in frames:
        big[o:o + fb] = torch.from_numpy(f.reshape(-1)).cuda()
        views.append(big[o:o + fb].view(h, w, cn))
        o += fb + (1 if (o + fb) % 2 == 0 else 2)
    return views


# ---- 1. the fields against the restatement ------------------------------------------------------------------------------
# (h, w, channels, step, radius, warp, layout, epsilon): every value of every axis; radius < step / 2 (2 at 8, 6 at 16 and
# 32), a radius larger than the frame's half (12 at 33 x 17), sizes that are no multiple of the step, a frame of edge nodes.
# warp: aff / persp = small sub-pixel warps, far = one that leaves part of the grid uncovered.
ALIGN_CASES = [
    (77, 101, 3, 16, 6, "persp", "device", 0.01), (77, 101, 1, 8, 2, "aff", "host", 0.0), (77, 101, 4, 32, 12, "persp", "pad5", 0.01),
    (77, 101, 3, 8, 6, "far", "odd", 0.01), (77, 101, 1, 16, 12, "persp", "device", 0.0), (77, 101, 4, 16, 2, "aff", "host", 0.01),
    (80, 96, 3, 16, 6, "aff", "host", 0.01), (80, 96, 4, 8, 12, "persp", "device", 0.0), (80, 96, 1, 32, 6, "far", "pad5", 0.01),
    (80, 96, 3, 32, 2, "persp", "odd", 0.0), (80, 96, 1, 16, 12, "aff", "device", 0.01),
    (17, 33, 3, 8, 2, "persp", "device", 0.01), (17, 33, 1, 16, 12, "aff", "host", 0.01), (17, 33, 4, 32, 6, "persp", "odd", 0.0),
    (17, 33, 3, 16, 6, "far", "pad5", 0.01), (17, 33, 1, 8, 12, "persp", "host", 0.0),
]
_ALIGN_IDS = [f"{c[0]}x{c[1]}c{c[2]}-s{c[3]}-r{c[4]}-{c[5]}-{c[6]}-e{c[7]}" for c in ALIGN_CASES]


def align_stack(case):
    """(frames [3 of h x w x cn u8], forward warps, is_affine, MeshParameters): frame 0 shows a cosine scene, frame i the
    scene through its warp and a smooth displacement of about a pixel, with noise."""
    h, w, cn, step, radius, kind, _, eps = case
    rng = np.random.default_rng(zlib.crc32(("align" + str(case)).encode()))
    tex = _cosines(rng, 12, 0.1)
    affine = kind == "aff"
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames, warps = [], []
    for i in range(3):
        M = np.eye(3)
        u = np.zeros((2, h, w))
        if i:
            M[:2, :2] += rng.normal(0, 3e-3, (2, 2))
            M[:2, 2] = rng.uniform(-3, 3, 2)
            if not affine:
                M[2, :2] = rng.normal(0, 2e-5, 2)
            if kind == "far":
                M[0, 2] += 0.3 * w
            for c in range(2):
                th, ph = rng.uniform(0, 2 * np.pi, 2)
                u[c] = rng.uniform(0.5, 1.2) * np.cos(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / 110.0 + ph)
        # source pixel q shows the scene at M q + u
        W = M[2, 0] * x + M[2, 1] * y + M[2, 2]
        X, Y = (M[0, 0] * x + M[0, 1] * y + M[0, 2]) / W, (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / W
        v = 128.0 + 100.0 * tex(X + u[0], Y + u[1]) + rng.normal(0, 1.0, (h, w))
        if cn == 1:
            f = v[..., None]
        else:
            f = np.stack([0.9 * v + 10.0, v, 1.05 * v - 5.0] + ([rng.uniform(0, 255, (h, w))] if cn == 4 else []), axis=-1)
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        warps.append(M)
    return frames, warps, affine, MeshParameters(step=step, radius=radius, max_iters=8, epsilon=eps, max_shift=6.0, min_eig=1.0, fill=0)


def _laid_out(frames, layout):
    import torch
    if layout == "host":
        return frames
    if layout == "device":
        return torch.from_numpy(np.stack(frames)).cuda()
    if layout == "pad5":
        return [_padded(f, 5, True) for f in frames]
    return _odd_base(frames)


@pytest.mark.parametrize("case", ALIGN_CASES, ids=_ALIGN_IDS)
def test_fields_match_restatement(st, case):
    """|d - d_restated| <= 1e-5 px and equal status planes. The per-pixel values are the restatement's bits, so only the
    order of the f64 additions differs; that moves a cast of d by at most an f32 ulp (4.8e-7 for |d| < 8) and the iteration
    is a contraction: 1e-5 leaves about 20 ulps. Nodes with a decision within a relative 1e-9 of its threshold are left
    out, at most 1 % of a case's (the seeds here leave out none on the CPU)."""
    frames, warps, affine, p = align_stack(case)
    layout = case[6]
    fields, status = st.local_align(_laid_out(frames, layout), warps, p, is_affine=affine, return_status=True)
    assert st.timing()["align_ms"] > 0
    if layout == "pad5":                                    # the padded host rows too
        hf, hs = st.local_align([_padded(f, 5, False) for f in frames], warps, p, is_affine=affine, return_status=True)
        assert np.array_equal(hf, fields.cpu().numpy()) and np.array_equal(hs, status.cpu().numpy())
    fields = fields if isinstance(fields, np.ndarray) else fields.cpu().numpy()
    status = status if isinstance(status, np.ndarray) else status.cpu().numpy()
    gw, gh = grid_restate(case[1], case[0], p.step)
    assert fields.shape == (3, gh, gw, 2) and status.shape == (3, gh, gw) and mesh_grid(case[1], case[0], p.step) == (gw, gh)
    assert (fields[0] == 0).all() and (status[0] == 0).all()          # frame 0's planes are not written
    seen = set()
    for i in (1, 2):
        d, s, near = local_align_restate(frames[0], frames[i], warps[i], affine, p)
        assert near.mean() <= 0.01
        keep = ~near
        assert np.array_equal(status[i][keep], s[keep])
        err = np.abs(fields[i][keep] - d[keep]).max()
        print("frame", i, "max |d - d_restated|", err, "status values", np.unique(s))
        assert err <= 1e-5
        assert (fields[i][status[i] < 0] == 0).all()
        seen |= set(np.unique(s).tolist())
    assert any(v > 0 for v in seen)
    if case[5] == "far":
        assert -2 in seen
    if case[7] == 0.0:
        assert all(v == p.max_iters for v in seen if v > 0)


def test_excluded_frames_and_null_status(st):
    frames, warps, affine, p = align_stack(ALIGN_CASES[0])
    full = st.local_align(frames, warps, p, is_affine=affine)
    part = st.local_align(frames, warps, p, include=[1, 0, 1], is_affine=affine)
    assert np.array_equal(part[2], full[2]) and (part[1] == 0).all() and (full[1] != 0).any()
    assert np.array_equal(st.local_align(frames, warps, p, include=[0, 1, 1], is_affine=affine), full)   # frame 0 is the template regardless


# ---- 2. the fill, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ALIGN_CASES[3], ALIGN_CASES[8], ALIGN_CASES[14]], ids=[_ALIGN_IDS[3], _ALIGN_IDS[8], _ALIGN_IDS[14]])
def test_fill_matches_restatement(st, case):
    import torch
    frames, warps, affine, p = align_stack(case)
    raw, status = st.local_align(frames, warps, p, is_affine=affine, return_status=True)
    assert (status[1:] < 0).any() and (status[1:] > 0).any()
    dev = torch.from_numpy(np.stack(frames)).cuda()
    for passes in (1, 2, 5):
        p.fill = passes
        got, gs = st.local_align(frames, warps, p, is_affine=affine, return_status=True)
        dgot = st.local_align(dev, warps, p, is_affine=affine)          # without a status plane of the caller's
        assert np.array_equal(gs, status)                                # the status keeps the estimation's codes
        for i in (1, 2):
            ref = mesh_fill_restate(raw[i], status[i], passes)
            assert np.array_equal(got[i], ref) and np.array_equal(dgot[i].cpu().numpy(), ref)
            assert np.array_equal(got[i][status[i] > 0], raw[i][status[i] > 0])


# ---- 3. the mesh folds --------------------------------------------------------------------------------------------------
def _fold_inputs(seed, n, h, w, cn, dtype, affine, step):
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n):
        f = rng.random((h, w, cn)) * _SCALE[dtype]
        frames.append(np.rint(f).astype(dtype) if dtype != np.float32 else f.astype(np.float32))
    warps = []
    for _ in range(n):
        M = np.eye(3)
        M[:2, :2] += rng.normal(0, 4e-3, (2, 2))
        M[:2, 2] = rng.uniform(-4, 4, 2)
        if not affine:
            M[2, :2] = rng.normal(0, 2e-5, 2)
        warps.append(M)
    gw, gh = grid_restate(w, h, step)
    fields = rng.uniform(-3, 3, (n, gh, gw, 2)).astype(F)
    return frames, warps, fields


FOLD_CASES = [(np.uint8, 3, False, 16, (45, 70)), (np.uint8, 1, True, 8, (33, 65)), (np.uint8, 4, False, 32, (37, 70)),
              (np.uint16, 3, True, 16, (45, 70)), (np.uint16, 1, False, 32, (33, 65)), (np.uint16, 4, True, 8, (20, 70)),
              (np.float32, 3, False, 8, (45, 70)), (np.float32, 1, True, 16, (17, 33)), (np.float32, 4, False, 16, (33, 65))]
# the other motion model of each (depth, channels): with the nine above, every cell launch_mesh_fold's ladder has. 70 x 6: the
# 64-wide and the 4-row tile both have a ragged second tile
FOLD_CASES += [(c[0], c[1], not c[2], 8, (6, 70)) for c in FOLD_CASES]
_FOLD_IDS = [f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-s{c[3]}-{c[4][0]}x{c[4][1]}" for c in FOLD_CASES]


@pytest.mark.parametrize("case", FOLD_CASES, ids=_FOLD_IDS)
def test_mesh_stack_matches_restatement(st, case):
    import torch
    dtype, cn, affine, step, (h, w) = case
    n = 5
    frames, warps, fields = _fold_inputs(zlib.crc32(("fold" + str(case)).encode()), n, h, w, cn, dtype, affine, step)
    include = [1, 1, 0, 1, 1]
    idx = [i for i in range(n) if include[i]]
    alpha = _ALPHA[dtype]
    bv = (0.1, 0.2, 0.3, 0.4)
    zero = np.zeros_like(fields)
    for border in (BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101):
        kw = dict(is_affine=affine, border_mode=border, border_value=bv, alpha=alpha)
        got = st.mesh_stack(frames, warps, fields, step, include, **kw)
        ref = mesh_mean_restate([frames[i] for i in idx], [warps[i] for i in idx], affine, alpha,
                                [None if i == 0 else fields[i] for i in idx], step, border, bv)
        assert got.dtype == np.float32 and np.array_equal(got, ref), border
        # zero fields: the plain fold's bits (the engine's own samples, summed in fold order, x (float)(1 / N))
        acc = None
        for i in idx:
            s = np.asarray(st.warp_accumulate(frames[i], warps[i], acc=None, **kw))
            acc = s if acc is None else acc + s
        assert np.array_equal(st.mesh_stack(frames, warps, zero, step, include, **kw), acc * F(1.0 / len(idx))), border
    # the fields do push coordinates outside the frame, and they matter
    kw = dict(is_affine=affine, alpha=alpha)
    plain = st.mesh_stack(frames, warps, zero, step, include, **kw)
    moved = st.mesh_stack(frames, warps, fields, step, include, **kw)
    assert (plain != moved).mean() > 0.5
    dev = st.mesh_stack(torch.from_numpy(np.stack(frames)).cuda(), warps, torch.from_numpy(fields).cuda(), step, include, **kw)
    assert np.array_equal(dev.cpu().numpy(), moved)
    assert st.timing()["finalize_ms"] > 0


@pytest.mark.parametrize("case", FOLD_CASES, ids=_FOLD_IDS)
def test_mesh_local_weighted_stack_matches_restatement(st, case):
    import torch
    dtype, cn, affine, step, (h, w) = case
    n = 5
    seed = zlib.crc32(("lfold" + str(case)).encode())
    frames, warps, fields = _fold_inputs(seed, n, h, w, cn, dtype, affine, step)
    rng = np.random.default_rng(seed + 1)
    include = [1, 0, 1, 1, 1]
    idx = [i for i in range(n) if include[i]]
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0.5, 2.0, n).astype(F)
    maps = rng.integers(0, 5000, (n, h, w)).astype(F)
    alpha = _ALPHA[dtype]
    kw = dict(is_affine=affine, alpha=alpha)
    fl = [None if i == 0 else fields[i] for i in range(n)]
    samples = np.stack([mesh_fold_restate(frames[i], warps[i], affine, alpha, fl[i], step) for i in idx])
    kappa = np.stack([mesh_fold_restate(np.ones((h, w), F), warps[i], affine, 1.0, fl[i], step)[..., 0] for i in idx])
    omega = np.stack([mesh_fold_restate(maps[i], warps[i], affine, 1.0, fl[i], step)[..., 0] for i in idx])
    assert ((kappa > 0) & (kappa < 1)).mean() > 0.02
    for power, floor in ((2, 1.0), (1, 0.0), (4, 0.5)):
        out, den = st.mesh_local_weighted_stack(frames, warps, maps, fields, step, g, o, wt, include, floor=floor, power=power,
                                                return_coverage=True, **kw)
        ref, ref_den = local_weighted_restate(samples, kappa, omega, g[idx], o[idx], wt[idx], floor, power)
        assert np.array_equal(den, ref_den), (power, floor)
        assert np.array_equal(out, ref, equal_nan=True), (power, floor)
    # zero fields: stk_local_weighted_stack's bits
    a, ad = st.mesh_local_weighted_stack(frames, warps, maps, np.zeros_like(fields), step, g, o, wt, include, return_coverage=True, **kw)
    b, bd = st.local_weighted_stack(frames, warps, maps, g, o, wt, include, return_coverage=True, **kw)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(ad, bd)
    dout = st.mesh_local_weighted_stack(torch.from_numpy(np.stack(frames)).cuda(), warps, torch.from_numpy(maps).cuda(),
                                        torch.from_numpy(fields).cuda(), step, g, o, wt, include, **kw)
    assert np.array_equal(dout.cpu().numpy(), st.mesh_local_weighted_stack(frames, warps, maps, fields, step, g, o, wt, include, **kw),
                          equal_nan=True)


# ---- 4. the whole-stack forms equal their parts --------------------------------------------------------------------------
def _stats_equal(a, b):
    for x, y in zip(a, b):
        assert x["status"] == y["status"] and x["iterations"] == y["iterations"] and x["rho"] == y["rho"]
        assert x["n_matches"] == y["n_matches"] and np.array_equal(x["warp"], y["warp"])


@pytest.fixture(scope="module")
def small_stack():
    frames, _ = synth.make_stack(6, 128, 96)
    return frames.numpy()


MP = MeshParameters(step=16, radius=8, max_iters=6, epsilon=0.01, max_shift=4.0, min_eig=1.0, fill=2)


def test_ecc_match_local_aligned_equals_its_parts(st, small_stack):
    import torch
    host = small_stack
    dev = torch.from_numpy(host).cuda()
    lp = LocalParameters(3, 8, 3, 0.5)
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    warps = [s["warp"] for s in pstats]
    fields, status = st.local_align(dev, warps, MP, return_status=True)
    assert (status[1:] > 0).any()
    out, stats = st.ecc_match_local_aligned(dev, ECC, MP, return_stats=True)
    assert st.timing()["finalize_ms"] > 0
    _stats_equal(stats, pstats)
    ref = st.mesh_stack(dev, warps, fields, MP.step)
    assert np.array_equal(out.cpu().numpy(), ref.cpu().numpy()) and np.isfinite(out.cpu().numpy()).all()
    # with the local-sharpness weights
    lout, lstats = st.ecc_match_local_aligned(dev, ECC, MP, lp, return_stats=True)
    _stats_equal(lstats, pstats)
    maps = st.local_sharpness(dev, lp)
    lref = st.mesh_local_weighted_stack(dev, warps, maps, fields, MP.step, floor=lp.floor, power=lp.power)
    assert np.array_equal(lout.cpu().numpy(), lref.cpu().numpy())
    assert not np.array_equal(lout.cpu().numpy(), out.cpu().numpy())
    # host-fed: the same bits, outputs on the host
    assert np.array_equal(st.ecc_match_local_aligned(host, ECC, MP), out.cpu().numpy())
    assert np.array_equal(st.ecc_match_local_aligned(host, ECC, MP, lp), lout.cpu().numpy())
    # fields from the full-size frames under scale_down_width too
    sout, sstats = st.ecc_match_local_aligned(dev, ECC, MP, scale_down_width=96.0, return_stats=True)
    swarps = [s["warp"] for s in sstats]
    sref = st.mesh_stack(dev, swarps, st.local_align(dev, swarps, MP), MP.step)
    assert np.array_equal(sout.cpu().numpy(), sref.cpu().numpy())
    # a multi-device context runs the call on its first device: the single-device bits
    multi = Stacker(devices=[0, 0])
    try:
        mo = multi.ecc_match_local_aligned(dev, ECC, MP, lp)
    finally:
        multi.close()
    assert np.array_equal(mo.cpu().numpy(), lout.cpu().numpy())


def test_keypoint_match_local_aligned_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 160, 120)
    frames = frames.numpy()
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert pd >= 1 and pstats[2]["status"] != 0
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(pstats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(pstats)]
    fields = st.local_align(stack, warps, MP, include)
    for lp in (None, LocalParameters()):
        dropped, out, stats = st.keypoint_match_local_aligned(stack, KP, MP, lp, return_stats=True)
        assert st.timing()["finalize_ms"] > 0
        assert dropped == pd
        _stats_equal(stats, pstats)
        if lp is None:
            ref = st.mesh_stack(stack, warps, fields, MP.step, include)
        else:
            ref = st.mesh_local_weighted_stack(stack, warps, st.local_sharpness(stack, lp), fields, MP.step, include=include,
                                               floor=lp.floor, power=lp.power)
        assert np.array_equal(out, ref)


# ---- 5. ground truth ----------------------------------------------------------------------------------------------------
def test_quality_stack_through_the_engine(st):
    scene, frames, _ = quality_mesh_stack()
    ref, ref_mean, _, _ = quality_mesh_restated(frames)
    p = QM["mesh"]
    bgr = [np.repeat(f[..., None], 3, axis=2) for f in frames]
    I = [np.eye(3)] * len(bgr)
    fields = st.local_align(bgr, I, p)
    out = st.mesh_stack(bgr, I, fields, p.step)
    mean = st.mesh_stack(bgr, I, np.zeros_like(fields), p.step)
    r_engine, r_ref, r_mean = interior_rms(out[..., 0] * 255.0, scene), interior_rms(ref, scene), interior_rms(mean[..., 0] * 255.0, scene)
    print("quality stack: RMS engine", r_engine, "restatement", r_ref, "plain mean", r_mean)
    assert abs(r_engine - r_ref) <= 0.02 * r_ref
    assert r_engine <= 0.5 * r_mean
    assert np.array_equal(mean[..., 0] * 255.0, ref_mean.astype(F))


# ---- 6. layout and repeatability ----------------------------------------------------------------------------------------
def test_layout_repeatability_and_options(st, small_stack):
    import torch
    host = small_stack
    lp = LocalParameters()
    base = st.ecc_match_local_aligned(host, ECC, MP, lp)
    plain = st.ecc_match_local_aligned(host, ECC, MP)
    assert np.array_equal(st.ecc_match_local_aligned(host, ECC, MP, lp), base)
    assert np.array_equal(st.ecc_match_local_aligned(torch.from_numpy(host).cuda(), ECC, MP, lp).cpu().numpy(), base)
    assert np.array_equal(st.ecc_match_local_aligned([_padded(f, 5, False) for f in host], ECC, MP, lp), base)
    assert np.array_equal(st.ecc_match_local_aligned([_padded(f, 5, True) for f in host], ECC, MP).cpu().numpy(), plain)
    I = [np.eye(3)] * len(host)
    f0 = st.local_align(host, I, MP)
    for name, val, back in (("quantile_band_rows", 7, 0), ("ecc_slots", 4, 0), ("upload_batch", 2, 8)):
        st.set_option(name, val)
        try:
            other = st.ecc_match_local_aligned(host, ECC, MP, lp)
            of = st.local_align(host, I, MP)
        finally:
            st.set_option(name, back)
        assert np.array_equal(other, base), name
        assert np.array_equal(of, f0), name
    # host frames in batches of frame 0 and one more: a fresh context's frame workspace holds two frames
    fresh = Stacker(0)
    try:
        fresh.set_option("upload_batch", 2)
        assert np.array_equal(fresh.local_align(host, I, MP), f0)
    finally:
        fresh.close()


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected(st, small_stack):
    frames = small_stack[:3]
    I = [np.eye(3)] * 3
    gw, gh = mesh_grid(128, 96, 16)
    fields = np.zeros((3, gh, gw, 2), np.float32)
    maps = np.ones((3, 96, 128), np.float32)
    bad = [(dict(step=12), "step"), (dict(step=4), "step"), (dict(step=512), "step"), (dict(radius=1), "radius"),
           (dict(radius=33), "radius"), (dict(max_iters=0), "max_iters"), (dict(max_iters=33), "max_iters"),
           (dict(epsilon=-1.0), "epsilon"), (dict(epsilon=float("nan")), "epsilon"), (dict(epsilon=float("inf")), "epsilon"),
           (dict(max_shift=0.0), "max_shift"), (dict(max_shift=65.0), "max_shift"), (dict(max_shift=float("nan")), "max_shift"),
           (dict(min_eig=-1.0), "min_eig"), (dict(min_eig=float("inf")), "min_eig"), (dict(fill=-1), "fill"), (dict(fill=17), "fill")]
    for kw, field in bad:
        mp = MeshParameters(**kw)
        with pytest.raises(InvalidParams, match=field):
            st.local_align(frames, I, mp)
        with pytest.raises(InvalidParams, match=field):
            st.ecc_match_local_aligned(frames, ECC, mp)
        with pytest.raises(InvalidParams, match=field):
            st.keypoint_match_local_aligned(frames, KP, mp)
    for step in (12, 4, 512):
        with pytest.raises(InvalidParams, match="step"):
            st.mesh_stack(frames, I, fields, step)
        with pytest.raises(InvalidParams, match="step"):
            st.mesh_local_weighted_stack(frames, I, maps, fields, step)
    with pytest.raises(InvalidParams, match="radius"):
        st.ecc_match_local_aligned(frames, ECC, MP, LocalParameters(radius=0))
    with pytest.raises(InvalidParams, match="border_mode"):
        st.mesh_local_weighted_stack(frames, I, maps, fields, 16, border_mode=BORDER_REPLICATE)
    with pytest.raises(InvalidParams, match="border_mode"):
        st.keypoint_match_local_aligned(frames, KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9, BORDER_REPLICATE), MP, LocalParameters())
    with pytest.raises(InvalidParams, match="power"):
        st.mesh_local_weighted_stack(frames, I, maps, fields, 16, power=5)
    for dtype in (np.uint16, np.float32):
        deep = [f.astype(dtype) for f in frames]
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.local_align(deep, I, MP)
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.ecc_match_local_aligned(deep, ECC, MP)
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.keypoint_match_local_aligned(deep, KP, MP)
        st.mesh_stack(deep, I, fields, 16, alpha=_ALPHA[dtype])               # the folds alone take any depth
        st.mesh_local_weighted_stack(deep, I, maps, fields, 16, alpha=_ALPHA[dtype])
    calls = (lambda: st.mesh_stack(frames, I, fields, 16), lambda: st.mesh_local_weighted_stack(frames, I, maps, fields, 16),
             lambda: st.ecc_match_local_aligned(frames, ECC, MP), lambda: st.keypoint_match_local_aligned(frames, KP, MP, LocalParameters()))
    st.set_option("warp_subpixel_bits", 5)
    try:
        for call in calls:
            with pytest.raises(InvalidParams, match="warp_subpixel_bits"):
                call()
    finally:
        st.set_option("warp_subpixel_bits", 0)
    st.set_option("warp_interpolation", 2)
    try:
        for call in calls:
            with pytest.raises(NotImplementedYet, match="STK_INTER_CUBIC"):
                call()
        st.local_align(frames, I, MP)                                          # the estimation does not fold
    finally:
        st.set_option("warp_interpolation", 1)


def test_reserved_and_null_pointers_are_rejected(st, small_stack):
    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import HOST, _Marshalled
    m = _Marshalled(small_stack[:3])
    out = np.empty((96, 128, 3), np.float32)
    img = _ffi.ImageF32(out.ctypes.data, 128, 96, 3, HOST, 0)
    gw, gh = mesh_grid(128, 96, 16)
    fields = np.zeros((3, gh, gw, 2), np.float32)
    planes = np.ones((3, 96, 128), np.float32)
    fp = C.cast((C.c_void_p * 3)(*[fields.ctypes.data + i * fields[0].nbytes for i in range(3)]), C.c_void_p)
    hole = C.cast((C.c_void_p * 3)(fields.ctypes.data, None, fields.ctypes.data + 2 * fields[0].nbytes), C.c_void_p)
    first = C.cast((C.c_void_p * 3)(None, fields.ctypes.data + fields[0].nbytes, fields.ctypes.data + 2 * fields[0].nbytes), C.c_void_p)
    pp = C.cast((C.c_void_p * 3)(*[planes.ctypes.data + i * planes[0].nbytes for i in range(3)]), C.c_void_p)
    M = np.ascontiguousarray(np.stack([np.eye(3)] * 3).reshape(3, 9))
    Mp = C.c_void_p(M.ctypes.data)
    inc = np.array([1, 0, 1], np.int32)
    ep, kp, mp = ECC._c(), KP._c(), MP._c()
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    dropped = C.c_int32(0)
    bad = MP._c()
    bad.reserved = 1
    assert lib.stk_local_align(h, fr, Mp, None, 0, C.byref(bad), fp, None) == 2 and b"reserved" in lib.stk_last_error(h)
    assert lib.stk_ecc_match_local_aligned(h, fr, C.byref(ep), 0.0, C.byref(bad), None, C.byref(img), None) == 2
    assert b"reserved" in lib.stk_last_error(h)
    assert lib.stk_local_align(h, fr, Mp, None, 0, None, fp, None) == 2
    assert lib.stk_local_align(h, fr, None, None, 0, C.byref(mp), fp, None) == 2
    assert lib.stk_local_align(h, fr, Mp, None, 0, C.byref(mp), None, None) == 2
    assert lib.stk_local_align(h, fr, Mp, None, 0, C.byref(mp), hole, None) == 2
    assert lib.stk_local_align(h, fr, Mp, C.c_void_p(inc.ctypes.data), 0, C.byref(mp), hole, None) == 0     # excluded: may be NULL
    assert lib.stk_local_align(h, fr, Mp, None, 0, C.byref(mp), first, None) == 0                            # frame 0: may be NULL
    assert lib.stk_ecc_match_local_aligned(h, fr, C.byref(ep), 0.0, None, None, C.byref(img), None) == 2
    assert lib.stk_keypoint_match_local_aligned(h, fr, None, 0.0, C.byref(mp), None, C.byref(img), C.byref(dropped), None) == 2
    assert lib.stk_ecc_match_local_aligned(h, fr, C.byref(ep), 0.0, C.byref(mp), None, None, None) == 2
    assert lib.stk_mesh_stack(h, fr, None, None, 0, 0, None, 1.0 / 255, fp, 16, C.byref(img)) == 2
    assert lib.stk_mesh_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, 16, C.byref(img)) == 2
    assert lib.stk_mesh_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, hole, 16, C.byref(img)) == 2
    assert lib.stk_mesh_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, fp, 16, None) == 2
    assert lib.stk_mesh_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, first, 16, C.byref(img)) == 0
    assert lib.stk_mesh_local_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, pp, 1.0, 2, None, 16, C.byref(img), None) == 2
    assert lib.stk_mesh_local_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, None, 1.0, 2, fp, 16, C.byref(img), None) == 2
    assert lib.stk_mesh_local_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, pp, 1.0, 2, hole, 16, C.byref(img), None) == 2
    assert lib.stk_mesh_local_weighted_stack(h, fr, Mp, None, 0, 0, None, 1.0 / 255, None, pp, 1.0, 2, fp, 16, C.byref(img), None) == 0

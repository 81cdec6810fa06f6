"""Local normalisation on the GPU: stk_local_moments against math.fsum, the two folds through planes against the numpy
restatement (local_norm_restate.py) bit for bit, the whole-stack forms against their parts, the quality claim on the
device, and the refusals. As in test_gpu_weighted.py the fold's samples come from the engine's own single-frame warp and
kappa from the same warp of an all-ones frame under BORDER_CONSTANT 0, so what is restated is what this feature adds."""
import math
import zlib

import numpy as np
import pytest

from libstacker_rs_amd import (BORDER_CONSTANT, BORDER_REPLICATE, INTER_CUBIC, INTER_LINEAR, RANSAC, EccMatchParameters, InvalidParams,
                               KeyPointMatchParameters, LocalNormParameters, MotionType, NotImplementedYet, Stacker, local_norm_estimate, local_norm_grid,
                               synth)
from local_norm_restate import (LINEAR, cell_moments_restate, estimate_restate, grids, norm_mean_restate, norm_quantile_restate,
                                quality_rms)
from test_cpu_local_norm import quality_restated
from test_gpu_weighted import _ALPHA, engine_kappa, engine_samples, random_frames, shifted_warps

pytestmark = pytest.mark.gpu

F = np.float32
ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _padded(frames, device):
    """The frames as windows of a wider canvas (a padded row stride, a pixel to the right and a row below)."""
    import torch
    fr = np.stack(frames)
    n, h, w, c = fr.shape
    canvas = np.zeros((n, h + 2, w + 5, c), fr.dtype)
    canvas[:, 1:1 + h, 3:3 + w] = fr
    if device:
        canvas = torch.from_numpy(canvas).cuda()
    return canvas[:, 1:1 + h, 3:3 + w]


# ---- 1. cell moments -----------------------------------------------------------------------------------------------
# (h, w): width = step, step + 1 and neither; stat_step 3 does not divide the step; 64 leaves cells without a stepped pixel
MOMENT_CASES = [
    # dtype, cn, affine, border, sub, (h, w), step, stat_step
    (np.uint8, 3, False, BORDER_CONSTANT, 0, (45, 70), 8, 1),
    (np.uint8, 3, True, BORDER_CONSTANT, 0, (45, 70), 16, 3),
    (np.uint8, 1, False, BORDER_CONSTANT, 5, (45, 70), 32, 1),
    (np.uint8, 4, True, BORDER_CONSTANT, 0, (33, 64), 16, 64),
    (np.uint16, 1, True, BORDER_CONSTANT, 0, (33, 64), 64, 3),
    (np.uint16, 3, False, BORDER_REPLICATE, 0, (33, 64), 32, 1),
    (np.uint16, 4, False, BORDER_CONSTANT, 5, (40, 65), 8, 3),
    (np.float32, 1, False, BORDER_REPLICATE, 0, (40, 65), 64, 1),
    (np.float32, 3, True, BORDER_CONSTANT, 0, (40, 65), 16, 1),
    (np.float32, 4, False, BORDER_CONSTANT, 0, (40, 65), 64, 64),
]


@pytest.mark.parametrize("case", MOMENT_CASES, ids=[f"{np.dtype(c[0]).name}c{c[1]}-{'aff' if c[2] else 'persp'}-b{c[3]}-sp{c[4]}-{c[5][0]}x{c[5][1]}-s{c[6]}-t{c[7]}" for c in MOMENT_CASES])
def test_cell_moments_match_exact_sums(st, case):
    dtype, cn, affine, border, sub, (h, w), step, stat = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    n = 3
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine)                 # +-6 px: part of the rim is uncovered
    warps[0] = np.eye(3)
    if stat == 64:
        for M in warps[1:]:                               # pixel (0, 0), the one stepped pixel of cell (0, 0), stays covered
            M[:2, 2] = -np.abs(M[:2, 2]) - 1.0
    kw = dict(is_affine=affine, border_mode=border, border_value=(0, 0, 0, 0), alpha=_ALPHA[dtype])
    st.set_option("warp_subpixel_bits", sub)
    try:
        mom = st.local_moments(frames, warps, step, stat_step=stat, **kw)
        again = st.local_moments(frames, warps, step, stat_step=stat, **kw)
        dmom = st.local_moments(_padded(frames, True), warps, step, stat_step=stat, **kw)
        hmom = st.local_moments(_padded(frames, False), warps, step, stat_step=stat, **kw)
        st.set_option("warp_tune", 1)
        try:
            tuned = st.local_moments(frames, warps, step, stat_step=stat, **kw)
        finally:
            st.set_option("warp_tune", 0)
        whole = st.overlap_moments(frames, warps, stat_step=stat, **kw)
        samples = engine_samples(st, frames, warps, range(n), **kw)
        kappa = engine_kappa(st, (h, w), warps, range(n), affine)
    finally:
        st.set_option("warp_subpixel_bits", 0)
    gw, gh, cw, ch = grids(w, h, step)
    assert mom.shape == (n, ch, cw, cn, 6)
    for other in (again, dmom, hmom, tuned):
        assert np.array_equal(other, mom)                 # the same bits: every call, host or device, any row stride, any option
    exact, mag = cell_moments_restate(samples, kappa, step, stat)
    assert (mom[0] == 0).all()
    u = 2.0 ** -53
    cnt = exact[..., 0]
    assert np.array_equal(mom[..., 0], cnt)                                    # n exactly, every cell and channel
    err = np.abs(mom - exact)
    bound = cnt[..., None] * u * mag
    print("cell moments: worst error / bound", np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0)
    assert (err <= bound).all()
    assert (cnt[1:] > 0).any() and (kappa[1:] < 1).mean() > 0.03
    if stat == 64 and step < 64:
        assert (cnt[1:, :, 1:] == 0).all() and (cnt[1:, 1:] == 0).all()        # only cell (0, 0) holds a multiple of 64 here
    # the sum over the cells against the whole-overlap pass: n exactly, the sums within the same bound of the exact value
    tot = mom.reshape(n, ch * cw, cn, 6).sum(axis=1)
    tot_exact = np.array([[[math.fsum(exact[i, :, :, c, k].reshape(-1).tolist()) for k in range(6)] for c in range(cn)] for i in range(n)])
    tot_mag = mag.reshape(n, ch * cw, cn, 6).sum(axis=1)
    assert np.array_equal(tot[..., 0], whole[..., 0])
    tb = tot[..., :1] * u * tot_mag
    print("sum of cells: worst error / bound", np.max(np.abs(tot - tot_exact)[tb > 0] / tb[tb > 0]) if (tb > 0).any() else 0.0)
    assert (np.abs(tot - tot_exact) <= tb).all()
    assert (np.abs(whole - tot_exact) <= tb).all()


def test_cell_moments_leave_excluded_frames_zero(st):
    rng = np.random.default_rng(4)
    frames = random_frames(rng, 4, 45, 70, 3, np.uint8)
    warps = shifted_warps(rng, 4, False)
    mom = st.local_moments(frames, warps, 16, [1, 1, 0, 1], stat_step=2)
    assert (mom[0] == 0).all() and (mom[2] == 0).all() and (mom[1, ..., 0] > 0).any() and (mom[3, ..., 0] > 0).any()
    full = st.local_moments(frames, warps, 16, stat_step=2)
    assert np.array_equal(full[[1, 3]], mom[[1, 3]])


# ---- 2. the folds -------------------------------------------------------------------------------------------------
def _random_planes(rng, n, h, w, cn, step, none=()):
    gh, gw, _, _ = local_norm_grid(w, h, step)
    planes = []
    for i in range(n):
        P = np.concatenate([rng.uniform(0.5, 2.0, (gh, gw, cn)), rng.uniform(-0.1, 0.1, (gh, gw, cn))], axis=-1).astype(F)
        planes.append(None if i in none else P)
    return planes


@pytest.mark.parametrize("dtype,cn", [(np.uint8, 3), (np.float32, 1)], ids=["u8c3", "f32c1"])
def test_null_and_constant_planes_give_the_weighted_combines_bits(st, dtype, cn):
    """u8 BGR: the yardstick runs the fast kernel, the new states the generic one."""
    import torch
    rng = np.random.default_rng(cn)
    n, h, w, step = 6, 45, 131, 16
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, False)
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[2] = 0.0
    gh, gw, _, _ = local_norm_grid(w, h, step)
    const = [np.broadcast_to(np.concatenate([g[i], o[i]]), (gh, gw, 2 * cn)).copy() for i in range(n)]
    kw = dict(alpha=_ALPHA[dtype])
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    for cov in (True, False):
        ref, ref_den = st.weighted_stack(frames, warps, g, o, wt, coverage=cov, return_coverage=True, **kw)
        qref, qcnt = st.quantile_stack_weighted(frames, warps, 0.5, g, o, wt, coverage=cov, return_counts=True, **kw)
        for planes, rec in ((None, (g, o)), ([None] * n, (g, o)), (const, (None, None)), (const[:3] + [None] * 3, (g, o))):
            for fr in (frames, dframes):
                out, den = st.local_norm_stack(fr, warps, planes, step, rec[0], rec[1], wt, coverage=cov, return_den=True, **kw)
                assert np.array_equal(_np(out), ref) and np.array_equal(_np(den), ref_den)
                q, c = st.quantile_stack_local_norm(fr, warps, planes, step, 0.5, rec[0], rec[1], wt, coverage=cov, return_counts=True, **kw)
                assert np.array_equal(_np(q), qref) and np.array_equal(_np(c), qcnt)
        if cov:
            assert (ref_den < ref_den.max()).any()            # the rim is there: coverage matters


FOLD_CASES = [
    # n, dtype, cn, affine, coverage, border, (h, w), step, planes that are None
    (1, np.uint8, 1, False, 1, BORDER_CONSTANT, (45, 70), 16, ()),
    (2, np.uint16, 3, True, 0, BORDER_REPLICATE, (33, 64), 8, ()),
    (3, np.float32, 4, False, 1, BORDER_CONSTANT, (40, 65), 64, ()),
    (4, np.uint8, 3, False, 1, BORDER_CONSTANT, (45, 131), 32, (0, 2)),
    (5, np.uint16, 4, True, 1, BORDER_CONSTANT, (45, 70), 16, (3,)),
    (5, np.float32, 3, False, 0, BORDER_CONSTANT, (33, 64), 32, (0,)),
    (4, np.uint8, 4, True, 0, BORDER_CONSTANT, (40, 65), 8, ()),
    (3, np.uint16, 1, False, 1, BORDER_CONSTANT, (40, 65), 16, (0,)),
    (5, np.float32, 1, True, 1, BORDER_CONSTANT, (45, 70), 8, ()),
]


@pytest.mark.parametrize("case", FOLD_CASES, ids=[f"n{c[0]}-{np.dtype(c[1]).name}c{c[2]}-{'aff' if c[3] else 'persp'}-cov{c[4]}-b{c[5]}-{c[6][0]}x{c[6][1]}-s{c[7]}" for c in FOLD_CASES])
def test_folds_through_random_planes_match_the_restatement(st, case):
    import torch
    n, dtype, cn, affine, cov, border, (h, w), step, none = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine)
    planes = _random_planes(rng, n, h, w, cn, step, none)
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    if n >= 4:
        wt[1] = 0.0
    kw = dict(is_affine=affine, border_mode=border, border_value=(0, 0, 0, 0), alpha=_ALPHA[dtype])
    samples = engine_samples(st, frames, warps, range(n), **kw)
    kappa = engine_kappa(st, (h, w), warps, range(n), affine)
    ref, ref_den = norm_mean_restate(samples, kappa if cov else np.ones_like(kappa), planes, step, g, o, wt)
    part = kappa == F(1) if cov else np.ones(kappa.shape, bool)
    dframes = torch.from_numpy(np.stack(frames)).cuda()
    for fr in (frames, dframes, _padded(frames, True)):
        out, den = st.local_norm_stack(fr, warps, planes, step, g, o, wt, coverage=bool(cov), return_den=True, **kw)
        assert np.array_equal(_np(den), ref_den)
        assert np.array_equal(_np(out), ref, equal_nan=True)
    assert np.array_equal(st.local_norm_stack(frames, warps, planes, step, g, o, wt, coverage=bool(cov), **kw), ref, equal_nan=True)
    for q in (0.5, 0.3):
        qref, qn = norm_quantile_restate(samples, part, planes, step, q, g, o, wt)
        for fr in (frames, dframes):
            qo, qc = st.quantile_stack_local_norm(fr, warps, planes, step, q, g, o, wt, coverage=bool(cov), return_counts=True, **kw)
            assert np.array_equal(_np(qc), qn)
            assert np.array_equal(_np(qo), qref, equal_nan=True)
    if cov:
        assert (kappa < 1).mean() >= 0.03
    # the planes matter: the restatement with the records instead is something else
    if len(none) < n:
        assert not np.array_equal(norm_mean_restate(samples, kappa if cov else np.ones_like(kappa), [None] * n, step, g, o, wt)[0], ref)


def test_banded_quantile_addresses_the_grid_by_the_pixels_own_row(st):
    """quantile_band_rows = 7 on h = 45: bands start at rows that are no multiple of the step; a state that took the band's
    row for the grid's would interpolate the wrong nodes from the second band on."""
    rng = np.random.default_rng(7)
    n, h, w, cn, step = 5, 45, 70, 3, 8
    frames = random_frames(rng, n, h, w, cn, np.uint8)
    warps = shifted_warps(rng, n, False)
    planes = _random_planes(rng, n, h, w, cn, step)
    # planes that vary down the rows, so that a wrong row shows
    for P in planes:
        P[..., :cn] *= np.linspace(0.6, 1.6, P.shape[0], dtype=F)[:, None, None]
    whole, wc = st.quantile_stack_local_norm(frames, warps, planes, step, 0.5, return_counts=True)
    st.set_option("quantile_band_rows", 7)
    try:
        banded, bc = st.quantile_stack_local_norm(frames, warps, planes, step, 0.5, return_counts=True)
    finally:
        st.set_option("quantile_band_rows", 0)
    assert np.array_equal(banded, whole) and np.array_equal(bc, wc)
    samples = engine_samples(st, frames, warps, range(n))
    kappa = engine_kappa(st, (h, w), warps, range(n), False)
    qref, qn = norm_quantile_restate(samples, kappa == F(1), planes, step, 0.5)
    assert np.array_equal(banded, qref) and np.array_equal(bc, qn)


@pytest.mark.parametrize("option,value,back", [("warp_interpolation", INTER_CUBIC, INTER_LINEAR), ("warp_subpixel_bits", 5, 0)])
def test_cubic_and_classic_folds_match_the_restatement(st, option, value, back):
    rng = np.random.default_rng(value)
    n, h, w, cn, step = 4, 45, 70, 3, 16
    frames = random_frames(rng, n, h, w, cn, np.uint8)
    warps = shifted_warps(rng, n, False)
    planes = _random_planes(rng, n, h, w, cn, step, (2,))
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    # kappa is the linear fold's under the cubic fold too (the exact-coordinate one); under the classic path it is that path's
    if option == "warp_subpixel_bits":
        st.set_option(option, value)
    try:
        kappa = engine_kappa(st, (h, w), warps, range(n), False)
        st.set_option(option, value)
        samples = engine_samples(st, frames, warps, range(n))
        out, den = st.local_norm_stack(frames, warps, planes, step, g, o, return_den=True)
        qo, qc = st.quantile_stack_local_norm(frames, warps, planes, step, 0.5, g, o, return_counts=True)
    finally:
        st.set_option(option, back)
    plain = engine_samples(st, frames, warps, range(n))
    assert not np.array_equal(plain, samples)                       # the option is in force
    ref, ref_den = norm_mean_restate(samples, kappa, planes, step, g, o)
    assert np.array_equal(den, ref_den) and np.array_equal(out, ref)
    qref, qn = norm_quantile_restate(samples, kappa == F(1), planes, step, 0.5, g, o)
    assert np.array_equal(qc, qn) and np.array_equal(qo, qref)


# The cubic folds at every depth and channel count (kernels_local_norm.hip launches the generic cubic kernel for FoldNorm and
# FoldStoreNorm itself, through the one (depth, cn) ladder): 70 x 6 destinations, a ragged second 64-wide and 4-row tile;
# 5 frames; step 8, a 10 x 2 grid. Affine and perspective tables alternate down the list.
CUBIC_FORMATS = [(dt, cn) for dt in (np.uint8, np.uint16, np.float32) for cn in (1, 3, 4)]


@pytest.mark.parametrize("dtype,cn", CUBIC_FORMATS, ids=[f"{np.dtype(dt).name}c{cn}" for dt, cn in CUBIC_FORMATS])
def test_cubic_folds_match_the_restatement_at_every_depth_and_channel_count(st, dtype, cn):
    idx = CUBIC_FORMATS.index((dtype, cn))
    rng = np.random.default_rng(900 + idx)
    n, h, w, step = 5, 6, 70, 8
    affine = bool(idx % 2)
    frames = random_frames(rng, n, h, w, cn, dtype)
    warps = shifted_warps(rng, n, affine, reach=1.5)
    planes = _random_planes(rng, n, h, w, cn, step, (2,))
    g = rng.uniform(0.5, 2.0, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[3] = 0.0
    kw = dict(is_affine=affine, alpha=_ALPHA[dtype])
    # kappa is the linear fold's under the cubic fold too (the exact-coordinate one)
    kappa = engine_kappa(st, (h, w), warps, range(n), affine)
    plain = engine_samples(st, frames, warps, range(n), **kw)
    st.set_option("warp_interpolation", INTER_CUBIC)
    try:
        samples = engine_samples(st, frames, warps, range(n), **kw)
        out, den = st.local_norm_stack(frames, warps, planes, step, g, o, wt, return_den=True, **kw)
        qo, qc = st.quantile_stack_local_norm(frames, warps, planes, step, 0.5, g, o, wt, return_counts=True, **kw)
    finally:
        st.set_option("warp_interpolation", INTER_LINEAR)
    assert not np.array_equal(plain, samples)                       # the option is in force
    assert (kappa < 1).mean() >= 0.03 and (kappa == F(1)).mean() >= 0.3
    ref, ref_den = norm_mean_restate(samples, kappa, planes, step, g, o, wt)
    assert np.array_equal(den, ref_den)
    assert np.array_equal(out, ref, equal_nan=True)
    qref, qn = norm_quantile_restate(samples, kappa == F(1), planes, step, 0.5, g, o, wt)
    assert np.array_equal(qc, qn)
    assert np.array_equal(qo, qref, equal_nan=True)
    # the planes matter: the restatement with the records instead is something else
    assert not np.array_equal(norm_mean_restate(samples, kappa, [None] * n, step, g, o, wt)[0], ref)


# ---- 3. whole-stack forms --------------------------------------------------------------------------------------------
def _graded_stack():
    """A 320 x 240, N = 6 synth stack whose moving frames carry their own gain and a linear gradient."""
    frames, _ = synth.make_stack(6, 320, 240)
    fr = frames.numpy().astype(np.float64)
    rng = np.random.default_rng(6)
    y, x = np.mgrid[0:240, 0:320].astype(np.float64)
    for i in range(1, 6):
        gx, gy = rng.uniform(-12, 12, 2)
        fr[i] = rng.uniform(0.85, 1.1) * fr[i] + (gx * (x / 320 - 0.5) + gy * (y / 240 - 0.5))[..., None]
    return np.clip(np.rint(fr), 0, 255).astype(np.uint8)


def _same_stats(stats, pstats):
    for a, b in zip(stats, pstats):
        assert a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["rho"] == b["rho"]
        assert a["n_matches"] == b["n_matches"] and np.array_equal(a["warp"], b["warp"])


def _check_parts(st, stack, stats, include, np_, weights, mean_res, med_res, kw):
    """The whole-stack results against the parts on the stats' warps: moments, estimator, fold."""
    out, den, planes, applied = mean_res
    qout, qcnt, qplanes, qapplied = med_res
    n, h, w, cn = len(stack), stack[0].shape[0], stack[0].shape[1], stack[0].shape[2]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(stats)]
    mom = st.local_moments(stack, warps, np_.step, include, stat_step=np_.stat_step or 4, **kw)
    want = [None] * n
    for i in range(1, n):
        if not include[i]:
            assert planes[i] is None and applied[i]["weight"] == 0 and (applied[i]["gain"] == 1).all()
            continue
        P, glob = local_norm_estimate(w, h, cn, mom[i], np_, return_global=True)
        want[i] = P
        for pl, ap in ((planes, applied), (qplanes, qapplied)):
            assert np.array_equal(pl[i], P)
            assert np.array_equal(ap[i]["gain"], glob["gain"]) and np.array_equal(ap[i]["offset"], glob["offset"])
            assert ap[i]["flags"] == glob["flags"] and ap[i]["weight"] == F(weights[i])
        assert np.ptp(P[..., 0]) > 0                            # a field, not a constant
    assert planes[0] is None and (applied[0]["gain"] == 1).all() and applied[0]["weight"] == F(weights[0])
    ref, ref_den = st.local_norm_stack(stack, warps, want, np_.step, weights=weights, include=include, coverage=bool(np_.coverage),
                                       return_den=True, **kw)
    assert np.array_equal(_np(out), _np(ref)) and np.array_equal(_np(den), _np(ref_den))
    qref, qrc = st.quantile_stack_local_norm(stack, warps, want, np_.step, 0.5, weights=weights, include=include,
                                             coverage=bool(np_.coverage), return_counts=True, **kw)
    assert np.array_equal(_np(qout), _np(qref)) and np.array_equal(_np(qcnt), _np(qrc))


def test_ecc_forms_equal_their_parts(st):
    import torch
    host = _graded_stack()
    dev = torch.from_numpy(host).cuda()
    weights = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0]
    np_ = LocalNormParameters(step=32, stat_step=2, normalize=LINEAR, coverage=True, min_count=16, fill=4)
    plain, pstats = st.ecc_match(dev, ECC, return_stats=True)
    out, den, planes, applied, stats = st.ecc_match_local_normalized(dev, ECC, np_, None, weights, return_stats=True, return_den=True,
                                                                     return_norm=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    qout, qcnt, qplanes, qapplied, qstats = st.ecc_match_local_normalized(dev, ECC, np_, 0.5, weights, return_stats=True, return_counts=True,
                                                                          return_norm=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    _same_stats(stats, pstats)
    _same_stats(qstats, pstats)
    _check_parts(st, list(host), stats, [1] * 6, np_, weights, (out, den, planes, applied), (qout, qcnt, qplanes, qapplied),
                 dict(is_affine=False, border_mode=BORDER_CONSTANT, alpha=1.0 / 255.0))
    assert int(_np(qcnt).max()) == 5                            # frame 3 has weight 0
    # host-fed: the same bits, outputs on the host
    hout, hden = st.ecc_match_local_normalized(host, ECC, np_, None, weights, return_den=True)
    assert np.array_equal(hout, _np(out)) and np.array_equal(hden, _np(den))
    hq, hqc = st.ecc_match_local_normalized(host, ECC, np_, 0.5, weights, return_counts=True)
    assert np.array_equal(hq, _np(qout)) and np.array_equal(hqc, _np(qcnt))
    # the plain call is what it was
    plain2, pstats2 = st.ecc_match(dev, ECC, return_stats=True)
    assert np.array_equal(_np(plain2), _np(plain))
    _same_stats(pstats2, pstats)
    # a two-"device" context runs on its first device
    multi = Stacker(devices=[0, 0])
    try:
        mo = multi.ecc_match_local_normalized(dev, ECC, np_, None, weights)
    finally:
        multi.close()
    assert np.array_equal(_np(mo), _np(out))


def test_keypoint_forms_equal_their_parts(st):
    host = _graded_stack()
    stack = list(host)
    weights = [1.0, 2.0, 3.0, 0.5, 1.0, 1.5]
    np_ = LocalNormParameters(step=64, stat_step=0, normalize=LINEAR, coverage=True, min_count=0, fill=2)
    pd, plain, pstats = st.keypoint_match(stack, KP, return_stats=True)
    d, out, den, planes, applied, stats = st.keypoint_match_local_normalized(stack, KP, np_, None, weights, return_stats=True,
                                                                             return_den=True, return_norm=True, return_applied=True)
    assert st.timing()["finalize_ms"] > 0
    qd, qout, qcnt, qplanes, qapplied, qstats = st.keypoint_match_local_normalized(stack, KP, np_, 0.5, weights, return_stats=True,
                                                                                   return_counts=True, return_norm=True,
                                                                                   return_applied=True)
    assert d == qd == pd
    _same_stats(stats, pstats)
    _same_stats(qstats, pstats)
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(stats)]
    print("keypoint: dropped", d, "kept", sum(include))
    assert sum(include) == 6 - d and sum(include) >= 2
    _check_parts(st, stack, stats, include, np_, weights, (out, den, planes, applied), (qout, qcnt, qplanes, qapplied),
                 dict(is_affine=False, border_mode=BORDER_CONSTANT, alpha=1.0 / 255.0))
    pd2, plain2, pstats2 = st.keypoint_match(stack, KP, return_stats=True)
    assert pd2 == pd and np.array_equal(plain2, plain)
    _same_stats(pstats2, pstats)


# ---- 4. quality on the device ---------------------------------------------------------------------------------------
def test_device_quality_is_the_restatements(st):
    """The device's RMS error against the scene on quality_stack(1) (step 16, stat_step 2, LINEAR, min_count 16, fill 4,
    coverage 1) lies within 1 % of the restatement's, for the median and for the mean."""
    lmed, _, lmean, _, rplanes, rmed_img, rmean_img, frames, warps, truth = quality_restated(1)
    stack = [f[..., None] for f in frames]
    np_ = LocalNormParameters(step=16, stat_step=2, normalize=LINEAR, coverage=True, min_count=16, fill=4)
    mom = st.local_moments(stack, list(warps), 16, stat_step=2)
    h, w = frames[0].shape
    planes = [None] + [local_norm_estimate(w, h, 1, mom[i], np_) for i in range(1, len(stack))]
    mean = st.local_norm_stack(stack, list(warps), planes, 16)
    med = st.quantile_stack_local_norm(stack, list(warps), planes, 16, 0.5)
    dmed, dmean = quality_rms(med, truth), quality_rms(mean, truth)
    print(f"quality_stack(1): median device {dmed:.4f} restatement {lmed:.4f}; mean device {dmean:.4f} restatement {lmean:.4f}")
    assert abs(dmed - lmed) <= 0.01 * lmed
    assert abs(dmean - lmean) <= 0.01 * lmean


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(st):
    rng = np.random.default_rng(9)
    frames = random_frames(rng, 3, 45, 70, 3, np.uint8)
    warps = shifted_warps(rng, 3, False)
    planes = _random_planes(rng, 3, 45, 70, 3, 16)
    for step in (0, 4, 12, 512):
        with pytest.raises(InvalidParams, match="step"):
            st.local_moments(frames, warps, step)
    for stat in (0, 65, -1):
        with pytest.raises(InvalidParams, match="stat_step"):
            st.local_moments(frames, warps, 16, stat_step=stat)
    with pytest.raises(InvalidParams, match="frame 0"):
        st.local_moments(frames, warps, 16, [0, 1, 1])
    with pytest.raises(InvalidParams, match="step"):
        st.local_norm_stack(frames, warps, None, 12)
    with pytest.raises(InvalidParams, match="step"):
        st.quantile_stack_local_norm(frames, warps, None, 24, 0.5)
    # coverage = 1 under a non-zero border value, or another border mode: the mean refuses, as stk_weighted_stack does
    with pytest.raises(InvalidParams, match="coverage"):
        st.local_norm_stack(frames, warps, planes, 16, coverage=True, border_value=(0.5, 0, 0, 0))
    with pytest.raises(InvalidParams, match="coverage"):
        st.local_norm_stack(frames, warps, planes, 16, coverage=True, border_mode=BORDER_REPLICATE)
    st.local_norm_stack(frames, warps, planes, 16, coverage=False, border_value=(0.5, 0, 0, 0))
    with pytest.raises(InvalidParams):
        st.local_norm_stack(frames, warps, planes, 16, weights=[0, 0, 0])
    with pytest.raises(InvalidParams):
        st.local_norm_stack(frames, warps, planes, 16, include=[0, 0, 0])
    with pytest.raises(InvalidParams, match="planes"):
        st.local_norm_stack(frames, warps, planes, 32)            # planes of another grid
    small, _ = synth.make_stack(3, 128, 96)
    bad = [dict(step=12), dict(step=4), dict(stat_step=65), dict(stat_step=-1), dict(normalize=4), dict(normalize=-1), dict(min_count=-1),
           dict(fill=17), dict(fill=-1)]
    for kw in bad:
        p = LocalNormParameters(**{**dict(step=16), **kw})
        for call in (lambda: st.ecc_match_local_normalized(small, ECC, p), lambda: st.keypoint_match_local_normalized(small, KP, p, 0.5)):
            with pytest.raises(InvalidParams):
                call()
    # den with a quantile, counts without one
    p = LocalNormParameters(step=16)
    with pytest.raises(InvalidParams, match="den"):
        st.ecc_match_local_normalized(small, ECC, p, 0.5, return_den=True)
    with pytest.raises(InvalidParams, match="counts"):
        st.ecc_match_local_normalized(small, ECC, p, None, return_counts=True)
    with pytest.raises(InvalidParams, match="den"):
        st.keypoint_match_local_normalized(small, KP, p, 0.5, return_den=True)
    with pytest.raises(InvalidParams, match="counts"):
        st.keypoint_match_local_normalized(small, KP, p, None, return_counts=True)
    # coverage 1 under the keypoint parameters' non-zero border value
    kp = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9, BORDER_CONSTANT, (0.5, 0, 0, 0))
    with pytest.raises(InvalidParams, match="coverage"):
        st.keypoint_match_local_normalized(small, kp, p)


def test_reserved_fields_and_too_many_frames_are_refused(st):
    import ctypes as C

    from libstacker_rs_amd import _ffi
    from libstacker_rs_amd.api import _Marshalled
    small, _ = synth.make_stack(3, 128, 96)
    m = _Marshalled(small.numpy())
    out = np.zeros((96, 128, 3), F)
    img = _ffi.ImageF32(C.c_void_p(out.ctypes.data), 128, 96, 3, 0, 0)
    p = LocalNormParameters(step=16)._c()
    ecc = ECC._c()
    for k in (0, 1):
        p.reserved[k] = 1
        assert st._lib.stk_ecc_match_local_normalized(st._h, C.byref(m.c_frames), C.byref(ecc), 0.0, C.byref(p), None, None, C.byref(img),
                                                      None, None, None, None, None) == 2
        p.reserved[k] = 0
    assert st._lib.stk_ecc_match_local_normalized(st._h, C.byref(m.c_frames), C.byref(ecc), 0.0, None, None, None, C.byref(img),
                                                  None, None, None, None, None) == 2
    # N > 4096 for the quantile: refused before anything is allocated or read
    n = 4097
    tiny = np.zeros((n, 8, 8, 1), np.uint8)
    warps = [np.eye(3)] * n
    with pytest.raises(NotImplementedYet, match="4096"):
        st.quantile_stack_local_norm(tiny, warps, None, 8, 0.5)
    with pytest.raises(NotImplementedYet, match="4096"):
        st.ecc_match_local_normalized(np.zeros((n, 8, 8, 3), np.uint8), ECC, LocalNormParameters(step=8), 0.5)

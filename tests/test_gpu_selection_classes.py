"""The three selection kernels at every launch class: quantile_select_kernel (stk_quantile_stack),
quantile_select_masked_kernel (stk_quantile_stack_weighted) and both routes of robust_select_kernel (stk_robust_clip_stack,
stk_robust_clip_stack_weighted) against the f32 restatements of their definitions, bit for bit, at both ends of every
class's range of sample counts and at a ragged count in it, on tiny frames (5 x 13: 65 pixels, no multiple of any
workgroup's share, so the lanes beyond the band's last column are live in every launch).
The inputs come from selection_classes.py, and test_cpu_selection_classes.py shows on the CPU that they are what these
tests need: order statistics planted on either side of every kind of slot boundary, adversarial values that reach the
kernel bit for bit, and translation tables under which every pixel has its own set of participating frames. The plain
tests use f32 frames, identity warps and alpha = 1: the sample is the frame's value (asserted once, against the engine's
own single-frame warp), so their references are computed from the numpy frames alone."""
import functools

import numpy as np
import pytest

import selection_classes as sc
from libstacker_rs_amd import NotImplementedYet, RobustClipParameters, Stacker
from selection_classes import F, H, W
from test_cpu_quantile import quantile_restate
from test_cpu_robust import robust_quantile_restate
from test_cpu_robust_clip import robust_clip_restate, robust_clip_restate_weighted
from test_gpu_weighted import engine_kappa, engine_samples

pytestmark = pytest.mark.gpu

CASES = [(n, 1) for n in sc.N_LIST] + [(61, 3)]
MASKED_CASES = [(n, 1) for n in sc.MASKED_N] + [(61, 3)]
IDS = lambda cases: [f"n{n}-c{cn}" for n, cn in cases]
ROBUST = (RobustClipParameters(3.0, 3.0, 0.5 / 255.0, 2), RobustClipParameters(2.0, 3.5, 0.0, 3))
MASKED_Q = (0.5, 0.3, 1.0, 0.0)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _dev(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames)).cuda()


def _eye(n):
    return [np.eye(3)] * n


def _equal(got, ref):
    return np.array_equal(_np(got), ref, equal_nan=True)


plain_stack = functools.lru_cache(maxsize=2)(sc.plain_stack)


# ---- 1. class coverage as a stated condition -----------------------------------------------------------------------------
def test_every_kernel_is_swept_over_all_eleven_classes():
    """If the dispatch in kernels_quantile.hip or kernels_robust_clip.hip changes, selection_classes.launch_class has to
    follow (test_cpu_selection_classes.py compares it with the launchers' text) and this fails: revisit the lists."""
    assert sc.check_class_coverage([n for n, _ in CASES]) == sorted(sc.CLASSES)                       # plain quantile, plain robust route
    assert sc.check_class_coverage([n for n, _ in MASKED_CASES], both_ends_up_to=512) == sorted(sc.CLASSES)    # masked quantile, masked robust route
    assert sorted(sc.launch_class(n) for n in sc.ADVERSARIAL_N) == sorted(sc.CLASSES)


# ---- 2. the sample is the frame's value: once ---------------------------------------------------------------------------------
def test_the_sample_of_an_identity_warp_is_the_frames_value(st):
    # (the single-frame warp is the mean fold of one frame, 0 + sample: it returns a -0.0 sample as +0.0, nothing else differs)
    n = 9
    frames, _ = sc.plain_stack(n)
    got = engine_samples(st, list(frames), _eye(n), range(n), alpha=1.0)
    assert sc.same_bits(got, frames) and sc.same_bits(got, sc.shifted_samples(frames)[0])
    n = 7
    frames, _ = sc.adversarial_stack(n)
    model, _ = sc.shifted_samples(frames, classic=True, border=sc.ADVERSARIAL_BORDER)
    st.set_option("warp_subpixel_bits", 5)
    try:
        got = engine_samples(st, list(frames), _eye(n), range(n), alpha=1.0, border_value=(sc.ADVERSARIAL_BORDER,) * 4)
    finally:
        st.set_option("warp_subpixel_bits", 0)
    assert sc.same_bits(got, F(0) + model)               # the infinities and the NaNs included
    for y, x in sc.LATTICE:
        assert sc.same_bits(got[:, y, x], F(0) + frames[:, y, x])


# ---- 3. the plain quantile: samples the test controls -------------------------------------------------------------------------
def _formula(lo, hi, g):
    if g == 0:
        return lo
    d = hi - lo
    return hi - d * (F(1) - g) if g >= F(0.5) else lo + d * g


@pytest.mark.parametrize("n,cn", CASES, ids=IDS(CASES))
def test_plain_quantile_at_every_class(st, n, cn):
    frames, planted = plain_stack(n, cn)
    cols = frames.reshape(n, -1)
    warps = _eye(n)
    dev = _dev(frames)
    orders = {name: _dev(frames[o]) for name, o in sc.frame_orders(n).items()}
    for qi, q in enumerate(sc.QUANTILES):
        ref = quantile_restate(frames, q)
        # the planted order statistics, straight from the frames they were put in
        j, g = sc.rank_of(n, q)
        for k, pq, pj, a, b in planted:
            if pq == qi:
                assert pj == j and ref.reshape(-1)[k] == _formula(cols[a, k], cols[b, k] if j + 1 < n else cols[a, k], g)
        outs = {}
        for rows in (0, 1):                              # one row per band: m = 13 columns per launch
            st.set_option("quantile_band_rows", rows)
            try:
                outs[rows] = _np(st.quantile_stack(dev, warps, q, alpha=1.0))
            finally:
                st.set_option("quantile_band_rows", 0)
            assert np.array_equal(outs[rows], ref), (q, rows)
        for name, d in orders.items():                   # any order of the frames: the same bits
            got = _np(st.quantile_stack(d, warps, q, alpha=1.0))
            assert sc.same_bits(got, outs[0]) and np.array_equal(got, ref), (q, name)


@pytest.mark.parametrize("n,cn", CASES, ids=IDS(CASES))
def test_plain_robust_route_at_every_class(st, n, cn):
    frames, _ = plain_stack(n, cn)
    dev = _dev(frames)
    rejected = False
    for p in ROBUST:
        ref, ref_k = robust_clip_restate(frames, p.kappa_low, p.kappa_high, p.sigma_floor, p.iterations)
        out, cnt = st.robust_clip_stack(dev, _eye(n), p, alpha=1.0, return_counts=True)
        assert np.array_equal(_np(cnt), ref_k) and _equal(out, ref), p
        rejected |= bool((ref_k < n).any())
    assert rejected or n < 5


# ---- 4. adversarial values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.ADVERSARIAL_N)
def test_adversarial_values(st, n):
    frames, where = sc.adversarial_stack(n)
    samples, _ = sc.shifted_samples(frames, classic=True, border=sc.ADVERSARIAL_BORDER)
    dev = _dev(frames)
    warps = _eye(n)
    kw = dict(alpha=1.0, border_value=(sc.ADVERSARIAL_BORDER,) * 4)
    ones, unit, zero = np.ones((n, H, W), bool), np.ones((n, 1), F), np.zeros((n, 1), F)
    at = lambda img, name: _np(img)[where[name] + (0,)]
    st.set_option("warp_subpixel_bits", 5)               # the 4-weight path: an infinite sample stays infinite
    try:
        for q in sc.QUANTILES:
            ref = quantile_restate(samples, q)
            out = st.quantile_stack(dev, warps, q, **kw)
            assert _equal(out, ref), q
            # the masked kernel on the same keys, every entry present (u = s * 1 + 0)
            mref, mcnt = robust_quantile_restate(samples, ones, unit, zero, np.ones(n, F), q)
            mout, cnt = st.quantile_stack_weighted(dev, warps, q, coverage=False, return_counts=True, **kw)
            assert (mcnt == n).all() and np.array_equal(_np(cnt), mcnt) and _equal(mout, mref), q
            for img in (out, mout):
                assert np.isnan(at(img, "nan-last")) and np.isnan(at(img, "nan-first"))
                assert at(img, "equal") == F(0.3)
                if q == 0.5 and n >= 4:
                    assert np.isfinite(at(img, "+inf")) and np.isfinite(at(img, "-inf"))
                if q in (0.5, float(F(0.73))):
                    j, g = sc.rank_of(n, q)
                    lo, hi = F(0.25), F(0.75)
                    assert at(img, f"two:{round(q, 2)}:j+1") == _formula(lo, hi if j + 1 < n else lo, g)
                    assert at(img, f"two:{round(q, 2)}:j") == hi
    finally:
        st.set_option("warp_subpixel_bits", 0)


# ---- 5. the participation forms: every pixel its own N_p ----------------------------------------------------------------------
@pytest.mark.parametrize("n,cn", MASKED_CASES, ids=IDS(MASKED_CASES))
def test_masked_quantile_and_masked_robust_route_at_every_class(st, n, cn):
    s = sc.masked_stack(n, cn)
    frames, warps, wt, g, o = s["frames"], s["warps"], s["weights"], s["gain"], s["offset"]
    # samples and participation as the other participation tests take them: from the engine's own single-frame warp, the
    # coverage of a translation once per translation. They are the model's, which the conditions were checked on
    samples = engine_samples(st, list(frames), warps, range(n), alpha=1.0)
    kappa_of = {}
    for (tx, ty), M in zip(map(tuple, s["shifts"]), warps):
        if (tx, ty) not in kappa_of:
            kappa_of[tx, ty] = engine_kappa(st, (H, W), [M], [0], False)[0]
    full = np.stack([kappa_of[tuple(t)] for t in s["shifts"]]) == F(1.0)
    part = full & (wt > 0)[:, None, None]
    assert np.array_equal(part, s["part"]) and sc.same_bits(samples, F(0) + s["samples"])
    clean = ~(np.isnan(samples).any(axis=-1) & part).any(axis=0)
    n_p = sc.check_participation(n, part, wt, clean)
    dev = _dev(frames)
    kw = dict(coverage=True, alpha=1.0)
    for q in MASKED_Q:
        ref, rn = robust_quantile_restate(samples, full, g, o, wt, q)
        assert np.array_equal(rn, n_p)
        for rows in (0, 1):
            st.set_option("quantile_band_rows", rows)
            try:
                out, cnt = st.quantile_stack_weighted(dev, warps, q, g, o, wt, return_counts=True, **kw)
            finally:
                st.set_option("quantile_band_rows", 0)
            assert np.array_equal(_np(cnt), rn) and _equal(out, ref), (q, rows)
        for i, y, x in s["nans"]:                        # a genuine NaN of any payload is a sample: counted, and the output NaN
            assert part[i, y, x] and np.isnan(_np(out)[y, x, 0]) and _np(cnt)[y, x] == n_p[y, x] > 0
        assert (ref[n_p == 0] == 0).all() and not np.isnan(ref[clean]).any()
    rejected = False
    for p in ROBUST:
        ref, ref_k, ref_sw = robust_clip_restate_weighted(samples, full, g, o, wt, p.kappa_low, p.kappa_high, p.sigma_floor, p.iterations)
        out, cnt, kept = st.robust_clip_stack_weighted(dev, warps, p, g, o, wt, return_counts=True, return_kept_weight=True, **kw)
        assert np.array_equal(_np(cnt), ref_k) and np.array_equal(_np(kept), ref_sw) and _equal(out, ref), p
        rejected |= bool((ref_k < n_p[..., None]).any())
        none = n_p == 0
        assert (ref[none] == 0).all() and (ref_k[none] == 0).all() and (ref_sw[none] == 0).all()
        for i, y, x in s["nans"]:
            assert np.isnan(_np(out)[y, x, 0])
    assert rejected or n < 8


# ---- 6. host and device frames: once per kernel -------------------------------------------------------------------------------
def test_host_frames_give_the_device_frames_bits(st):
    n = 61
    frames, _ = sc.plain_stack(n)
    q, p = float(F(0.73)), ROBUST[0]
    assert sc.same_bits(st.quantile_stack(list(frames), _eye(n), q, alpha=1.0), _np(st.quantile_stack(_dev(frames), _eye(n), q, alpha=1.0)))
    h, d = (st.robust_clip_stack(f, _eye(n), p, alpha=1.0, return_counts=True) for f in (list(frames), _dev(frames)))
    assert sc.same_bits(h[0], _np(d[0])) and np.array_equal(h[1], _np(d[1]))
    s = sc.masked_stack(n)
    args = (s["gain"], s["offset"], s["weights"])
    h, d = (st.quantile_stack_weighted(f, s["warps"], 0.3, *args, coverage=True, alpha=1.0, return_counts=True)
            for f in (list(s["frames"]), _dev(s["frames"])))
    assert sc.same_bits(h[0], _np(d[0])) and np.array_equal(h[1], _np(d[1])) and np.isnan(h[0]).any()
    h, d = (st.robust_clip_stack_weighted(f, s["warps"], p, *args, coverage=True, alpha=1.0, return_counts=True, return_kept_weight=True)
            for f in (list(s["frames"]), _dev(s["frames"])))
    assert sc.same_bits(h[0], _np(d[0])) and np.array_equal(h[1], _np(d[1])) and np.array_equal(h[2], _np(d[2]))


# ---- 7. one sample too many ---------------------------------------------------------------------------------------------------
def test_4097_samples_are_refused_by_all_four_stack_calls(st):
    n = sc.MAX_SAMPLES + 1
    frames = np.zeros((n, 2, 4, 1), F)
    for call in (st.quantile_stack, st.quantile_stack_weighted, st.robust_clip_stack, st.robust_clip_stack_weighted):
        with pytest.raises(NotImplementedYet, match="4096"):
            call(frames, _eye(n))
    # and 4096 are not
    assert (st.quantile_stack(frames[:-1], _eye(n - 1), alpha=1.0) == 0).all()

"""The two clip combines through local-normalisation planes, CPU side: the numpy restatements (local_norm_clip_restate.py)
that the GPU tests (test_gpu_local_norm_clip.py) compare the engine against bit for bit, checked here against the weighted
restatements they are built on, a planted case with an exact answer and the quality claim; and the ABI's mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libstacker_rs_amd as ls
from libstacker_rs_amd import _ffi
from local_norm_clip_restate import norm_clip_restate, norm_robust_clip_restate, planted_stack
from local_norm_restate import (LINEAR, cell_moments_restate, global_records, grids, integer_shift_samples, quality_rms, quality_stack)
from test_cpu_local_norm import quality_restated
from test_cpu_robust import robust_clip_restate
from test_cpu_robust_clip import robust_clip_restate_weighted

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["stk_clip_stack_local_norm", "stk_robust_clip_stack_local_norm", "stk_ecc_match_local_normalized_clipped",
       "stk_keypoint_match_local_normalized_clipped"]
FLOOR = 0.5 / 255.0


# ---- 1. constant planes ---------------------------------------------------------------------------------------------
def test_constant_planes_give_the_weighted_restatements_bits():
    rng = np.random.default_rng(1)
    n, h, w, cn, step = 6, 20, 37, 3, 16
    s = rng.uniform(0, 1, (n, h, w, cn)).astype(F)
    s[3, 5:9] += F(0.4)                                       # something to reject
    part = rng.uniform(0, 1, (n, h, w)) > 0.15
    g = rng.uniform(0.8, 1.25, (n, cn)).astype(F)
    o = rng.uniform(-0.05, 0.05, (n, cn)).astype(F)
    wt = rng.uniform(0.1, 2.0, n).astype(F)
    wt[4] = 0
    gw, gh, _, _ = grids(w, h, step)
    const = [np.broadcast_to(np.concatenate([g[i], o[i]]), (gh, gw, 2 * cn)).copy() for i in range(n)]
    ref = robust_clip_restate(s, part, g, o, wt, 1.5, 2.0, 2)
    rref = robust_clip_restate_weighted(s, part, g, o, wt, 2.0, 2.5, FLOOR, 2)
    for planes, rec in (([None] * n, (g, o)), (None, (g, o)), (const, (None, None)), (const[:3] + [None] * 3, (g, o))):
        got = norm_clip_restate(s, part, planes, step, 1.5, 2.0, 2, rec[0], rec[1], wt)
        rgot = norm_robust_clip_restate(s, part, planes, step, 2.0, 2.5, FLOOR, 2, rec[0], rec[1], wt)
        for a, b in zip(got + rgot, ref + rref):
            assert np.array_equal(a, b, equal_nan=True)
    assert (ref[1] < n - 1).any() and (rref[1] < n - 1).any()            # the clips reject something here


# ---- 2. the planted exact case --------------------------------------------------------------------------------------
def test_planted_ramps_are_undone_exactly_through_the_planes_only():
    frames, planes, scene, mask = planted_stack()
    n = len(frames)
    part = np.ones(frames.shape[:3], bool)
    want = np.where(mask, n - 1, n)[..., None].astype(np.int32)
    assert mask.sum() == 270
    for name, local, unit in (
            ("median/MAD", norm_robust_clip_restate(frames, part, planes, 16, 3, 3, 0.25, 1),
             norm_robust_clip_restate(frames, part, None, 16, 3, 3, 0.25, 1)),
            ("sigma", norm_clip_restate(frames, part, planes, 16, 2, 2, 2), norm_clip_restate(frames, part, None, 16, 2, 2, 2))):
        out, counts, kept = local
        assert np.array_equal(out, scene), name
        assert np.array_equal(counts, want), name
        assert np.array_equal(kept, counts.astype(F)), name
        same = float((unit[0] == scene).mean())
        print(f"{name}: unit records equal the scene on {100 * same:.2f} % of the pixels, max error {np.abs(unit[0] - scene).max():.2f}")
        assert same < 0.01, name


# ---- 3. quality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_clips_through_the_planes_beat_the_global_records(seed):
    """Local / global RMS error against the scene (step 16, stat_step 2, LINEAR, min_count 16, fill 4, coverage 1), on the
    restatements alone: at most 0.55 for the median / MAD clip (kappa 3, floor 0.5 / 255, 2 iterations) and for the sigma
    clip (kappa 2, 2 iterations); the worst measured is 0.46."""
    planes = quality_restated(seed)[4]
    frames, warps, truth = quality_stack(seed)
    s, k = integer_shift_samples(frames, warps)
    n = len(frames)
    cells, _ = cell_moments_restate(s, k, 16, 2)
    g, o = global_records(cells, LINEAR)
    part, ones = k == 1, np.ones(n, F)
    lmad = quality_rms(norm_robust_clip_restate(s, part, planes, 16, 3, 3, FLOOR, 2)[0], truth)
    gmad = quality_rms(robust_clip_restate_weighted(s, part, g, o, ones, 3, 3, FLOOR, 2)[0], truth)
    lsig = quality_rms(norm_clip_restate(s, part, planes, 16, 2, 2, 2)[0], truth)
    gsig = quality_rms(robust_clip_restate(s, part, g, o, ones, 2, 2, 2)[0], truth)
    print(f"seed {seed}: median/MAD clip local {lmad:.3f} / global {gmad:.3f} = {lmad / gmad:.3f}; "
          f"sigma clip local {lsig:.3f} / global {gsig:.3f} = {lsig / gsig:.3f}")
    assert lmad / gmad <= 0.55
    assert lsig / gsig <= 0.55


# ---- 4. the ABI's mirrors ---------------------------------------------------------------------------------------------
def test_ctypes_table_matches_the_header_for_the_new_names():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "stacker.h")).read(), flags=re.S)
    lib = _ffi.load()
    typed = {"stk_local_norm_params": _ffi.LocalNormParams, "stk_frame_weight": _ffi.FrameWeight, "stk_clip_params": _ffi.ClipParams,
             "stk_robust_clip_params": _ffi.RobustClipParams, "stk_frames": _ffi.Frames, "stk_image_f32": _ffi.ImageF32,
             "stk_frame_stats": _ffi.FrameStats, "stk_ecc_params": _ffi.EccParams, "stk_keypoint_params": _ffi.KeypointParams}
    for name in NEW:
        m = re.search(r"stk_status\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _ffi.SIGNATURES[name]
        assert res is _ffi.c_status and len(args) == len(params), name
        for p, a in zip(params, args):
            if "*" not in p:
                assert a is {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}[p.split()[0]], (name, p)
                continue
            struct = [t for t in typed if re.search(r"\b%s\b" % t, p)]
            if struct:
                assert a is C.POINTER(typed[struct[0]]), (name, p)
            else:
                assert a in (C.c_void_p, C.POINTER(C.c_int32)), (name, p)
        assert getattr(lib, name) is not None
    for m in ("clip_stack_local_norm", "robust_clip_stack_local_norm", "ecc_match_local_normalized_clipped",
              "keypoint_match_local_normalized_clipped"):
        assert callable(getattr(ls.Stacker, m))


def test_wrappers_refuse_both_or_neither_clip():
    """clip= is one SigmaClipParameters or one RobustClipParameters; the refusal comes before the engine is touched."""
    st = object.__new__(ls.Stacker)                           # no context: the check needs none
    ecc = ls.EccMatchParameters(ls.MotionType.Homography, 50, 1e-3, 5)
    kp = ls.KeyPointMatchParameters(ls.RANSAC, 5.0, 0.80, 0.9)
    frames = np.zeros((3, 16, 16, 3), np.uint8)
    for clip in (None, (ls.SigmaClipParameters(), ls.RobustClipParameters()), 0.5):
        with pytest.raises(ls.InvalidParams, match="clip"):
            st.ecc_match_local_normalized_clipped(frames, ecc, ls.LocalNormParameters(step=8), clip)
        with pytest.raises(ls.InvalidParams, match="clip"):
            st.keypoint_match_local_normalized_clipped(frames, kp, ls.LocalNormParameters(step=8), clip)
    assert ls.Stacker._clip_choice(ls.SigmaClipParameters())[1] is None
    assert ls.Stacker._clip_choice(ls.RobustClipParameters())[0] is None

"""Coarse-to-fine local alignment on the GPU: stk_grey_pyramid, stk_local_align_pyramid and the two whole-stack forms against
the numpy restatement (mesh_pyramid_restate.py), against stk_local_align at one level and against their own parts. The
cases and the tolerance are the ones the CPU perturbation check qualifies (test_cpu_mesh_pyramid.py)."""
import ctypes as C

import numpy as np
import pytest

import mesh_pyramid_restate as mp
from interp_restate import F
from libstacker_rs_amd import (RANSAC, EccMatchParameters, InvalidParams, KeyPointMatchParameters, LocalParameters, MeshParameters,
                               MotionType, NotImplementedYet, Stacker, mesh_grid, synth)
from test_cpu_local import grey_restate
from test_cpu_mesh import interior_rms
from test_cpu_mesh_pyramid import QP, _flat_square_pair, quality_pyramid_stack
from test_gpu_mesh import ALIGN_CASES, _laid_out, _padded, _stats_equal, align_stack

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
MP3 = MeshParameters(step=16, radius=8, max_iters=6, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=2)


@pytest.fixture(scope="module")
def st():
    s = Stacker(0)
    yield s
    s.close()


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


# ---- 1. the pyramid kernel, exact ---------------------------------------------------------------------------------------
# widths at the 64-pixel tile's edges and at the ends of a four-pixel group; heights likewise
@pytest.mark.parametrize("cn", [1, 3, 4])
@pytest.mark.parametrize("size", [(64, 64), (65, 70), (127, 33), (130, 129), (66, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_grey_pyramid_is_exact(st, cn, size):
    import torch
    w, h = size
    levels = 4 if min(w, h) >> 3 >= 1 else 3
    rng = np.random.default_rng(w * 1000 + h * 10 + cn)
    frame = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    frame[: h // 3] = rng.choice(np.array([0, 255], np.uint8), (h // 3, w, cn))        # the rounding at the ends of the range
    want = mp.box_pyramid_restate(grey_restate(frame), levels)
    # host, device (dword-aligned rows when w cn is a multiple of 4), rows padded by 5 and by 4 bytes, an odd base address
    odd = torch.zeros(frame.size + 1, dtype=torch.uint8, device="cuda")
    odd[1:] = torch.from_numpy(frame.reshape(-1)).cuda()
    for what, f in (("host", frame), ("device", torch.from_numpy(frame).cuda()), ("pad5", _padded(frame, 5, True)),
                    ("pad4-host", _padded(frame, 4, False)), ("pad4", _padded(frame, 4 + (-w * cn) % 4, True)),
                    ("odd", odd[1:].view(h, w, cn))):
        got = st.grey_pyramid(f, levels)
        assert len(got) == levels - 1
        for l in range(1, levels):
            g = _np(got[l - 1])
            assert g.dtype == np.uint8 and g.shape == want[l].shape == (h >> l, w >> l), (what, l)
            assert np.array_equal(g, want[l]), (what, l, int(np.abs(g.astype(int) - want[l]).max()))
    assert np.array_equal(_np(st.grey_pyramid(frame, 2)[0]), want[1])


# ---- 2. one level is stk_local_align, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("case", [ALIGN_CASES[0], ALIGN_CASES[3], ALIGN_CASES[5], ALIGN_CASES[8], ALIGN_CASES[12]],
                         ids=lambda c: f"{c[0]}x{c[1]}c{c[2]}-s{c[3]}-r{c[4]}-{c[5]}-{c[6]}")
def test_one_level_is_local_align(st, case):
    frames, warps, affine, p = align_stack(case)
    for fill in (0, 2):
        p.fill = fill
        for layout in (case[6], "host"):
            f = _laid_out(frames, layout)
            a, sa = st.local_align(f, warps, p, is_affine=affine, return_status=True)
            b, sb = st.local_align_pyramid(f, warps, p, 1, is_affine=affine, return_status=True)
            assert np.array_equal(_np(a), _np(b)) and np.array_equal(_np(sa), _np(sb)), (fill, layout)
            assert (_np(sb)[1:] > 0).any()
    assert st.timing()["align_ms"] > 0


def test_one_level_on_the_pyramid_cases(st):
    for name in sorted(mp.GPU_CASES):
        frames, warps, affine, p, _ = mp.gpu_case(name)
        a, sa = st.local_align(list(frames), warps, p, is_affine=affine, return_status=True)
        b, sb = st.local_align_pyramid(list(frames), warps, p, 1, is_affine=affine, return_status=True)
        assert np.array_equal(a, b) and np.array_equal(sa, sb), name


# ---- 3. the fields against the restatement ------------------------------------------------------------------------------
def _check_fields(name, fields, status, res, levels, frames_with_field):
    tol = mp.gpu_tolerance(levels)
    for i in frames_with_field:
        err = np.abs(fields[i].astype(np.float64) - res[i][0]["d"]).max()
        print(name, "frame", i, "max |d - d_restated|", err, "tolerance", tol, "level-0 codes", np.unique(res[i][0]["status"]))
        if status is not None:
            assert np.array_equal(status[i], res[i][0]["status"]), (name, i)
        assert err <= tol, (name, i, err)


@pytest.mark.parametrize("layout", ["device", "host", "pad5", "odd"])
@pytest.mark.parametrize("name", sorted(mp.GPU_CASES))
def test_fields_match_restatement(st, name, layout):
    """Level-0 statuses equal; |d - d_restated| <= 1e-5 (2^levels - 1) px (mesh_pyramid_restate.gpu_tolerance)."""
    frames, warps, affine, p, levels, res = mp.gpu_case_restated(name)
    n = len(frames)
    fields, status = st.local_align_pyramid(_laid_out(list(frames), layout), warps, p, levels, is_affine=affine, return_status=True)
    fields, status = _np(fields), _np(status)
    gw, gh = mesh_grid(frames.shape[2], frames.shape[1], p.step)
    assert fields.shape == (n, gh, gw, 2) and (fields[0] == 0).all() and (status[0] == 0).all()
    _check_fields(name, fields, status, res, levels, range(1, n))
    if layout == "pad5":                                    # the padded host rows too: the device's bits
        hf, hs = st.local_align_pyramid([_padded(f, 5, False) for f in frames], warps, p, levels, is_affine=affine, return_status=True)
        assert np.array_equal(hf, fields) and np.array_equal(hs, status)
    t = st.timing()
    assert t["align_ms"] > 0 and t["prep_ms"] > 0


def test_excluded_frame_and_null_status(st):
    import torch
    name = "bgr-homography-3"
    frames, warps, affine, p, levels, res = mp.gpu_case_restated(name)
    dev = torch.from_numpy(frames).cuda()
    full = _np(st.local_align_pyramid(dev, warps, p, levels, is_affine=affine))               # no status planes at all
    _check_fields(name, full, None, res, levels, range(1, len(frames)))
    part, ps = st.local_align_pyramid(dev, warps, p, levels, include=[1, 0, 1, 1], is_affine=affine, return_status=True)
    part, ps = _np(part), _np(ps)
    assert (part[1] == 0).all() and (ps[1] == 0).all() and np.array_equal(part[2:], full[2:])
    hpart = st.local_align_pyramid(list(frames), warps, p, levels, include=[0, 0, 1, 1], is_affine=affine)   # frame 0 is the template regardless
    assert np.array_equal(hpart, part)
    # single NULL status entries, through the C interface
    from libstacker_rs_amd.api import _Marshalled
    m = _Marshalled(list(frames))
    gw, gh = mesh_grid(frames.shape[2], frames.shape[1], p.step)
    f = np.zeros((len(frames), gh, gw, 2), F)
    s = np.zeros((len(frames), gh, gw), np.int32)
    fp = (C.c_void_p * len(frames))(*[f.ctypes.data + i * f[0].nbytes for i in range(len(frames))])
    sp = (C.c_void_p * len(frames))(None, s.ctypes.data + s[0].nbytes, None, s.ctypes.data + 3 * s[0].nbytes)
    M = np.ascontiguousarray(np.asarray(warps, np.float64).reshape(len(frames), 9))
    c = p._c()
    assert st._lib.stk_local_align_pyramid(st._h, C.byref(m.c_frames), C.c_void_p(M.ctypes.data), None, int(affine), C.byref(c), levels,
                                           C.cast(fp, C.c_void_p), C.cast(sp, C.c_void_p)) == 0
    assert np.array_equal(f, full) and (s[2] == 0).all() and np.array_equal(s[3], res[3][0]["status"])


def test_empty_top_level_patch_and_nodes_beyond_the_edge(st):
    """101 x 77 at step 16: the last column of nodes sits at x = 112, beyond the image, and at level 1 of two its patch
    [50, 62] misses 1 <= x <= 48 too: -1 at both levels, d = 0 and m = 0 until the fill reaches it."""
    name = "grey-affine-2-odd"
    frames, warps, affine, p, levels, res = mp.gpu_case_restated(name)
    fields, status = st.local_align_pyramid(list(frames), warps, p, levels, is_affine=affine, return_status=True)
    for i in range(1, len(frames)):
        assert (res[i][1]["status"][:, -1] == -1).all() and (res[i][0]["status"][:, -1] == -1).all()
        assert not res[i][1]["m_est"][:, -1].any() and res[i][0]["m"][:, -1].all()
        assert (status[i][:, -1] == -1).all() and (np.abs(fields[i][:, -1]) > 1.0).any()
        assert (res[i][0]["status"][-1, :-1] != -1).all()            # the last row, y = 80: two patch rows inside
    _check_fields(name, fields, status, res, levels, range(1, len(frames)))


def test_a_failed_node_keeps_its_seed(st):
    f0, fi, p = _flat_square_pair()
    res = mp.pyramid_align_restate(f0, fi, np.eye(3), False, p, 3)
    assert not any(lv["near"].any() for lv in res)
    fields, status = st.local_align_pyramid([f0[..., None], fi[..., None]], [np.eye(3)] * 2, p, 3, return_status=True)
    assert status[1][3, 4] == -3 and np.array_equal(status[1], res[0]["status"])
    err = np.abs(fields[1].astype(np.float64) - res[0]["d"]).max()
    print("flat square: max |d - d_restated|", err, "node", fields[1][3, 4], "restated", res[0]["d"][3, 4])
    assert err <= mp.gpu_tolerance(3)
    assert np.abs(fields[1][3, 4] - np.array([4.0, -4.0], F)).max() < 0.5


# ---- 4. the whole-stack forms equal their parts --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_stack():
    frames, _ = synth.make_stack(5, 128, 96)
    return frames.numpy()


def test_ecc_match_local_aligned_pyramid_equals_its_parts(st, small_stack):
    import torch
    host = small_stack
    dev = torch.from_numpy(host).cuda()
    lp = LocalParameters(3, 8, 3, 0.5)
    _, pstats = st.ecc_match(dev, ECC, return_stats=True)
    warps = [s["warp"] for s in pstats]
    for levels in (2, 3):
        fields, status = st.local_align_pyramid(dev, warps, MP3, levels, return_status=True)
        assert (_np(status)[1:] > 0).any()
        out, stats = st.ecc_match_local_aligned_pyramid(dev, ECC, MP3, levels, return_stats=True)
        assert st.timing()["finalize_ms"] > 0
        _stats_equal(stats, pstats)
        assert np.array_equal(_np(out), _np(st.mesh_stack(dev, warps, fields, MP3.step))) and np.isfinite(_np(out)).all()
    lout = st.ecc_match_local_aligned_pyramid(dev, ECC, MP3, 3, lp)
    lref = st.mesh_local_weighted_stack(dev, warps, st.local_sharpness(dev, lp), fields, MP3.step, floor=lp.floor, power=lp.power)
    assert np.array_equal(_np(lout), _np(lref)) and not np.array_equal(_np(lout), _np(out))
    # host-fed: the same bits; one level: the single-level form's
    assert np.array_equal(st.ecc_match_local_aligned_pyramid(host, ECC, MP3, 3), _np(out))
    assert np.array_equal(st.ecc_match_local_aligned_pyramid(host, ECC, MP3, 3, lp), _np(lout))
    assert np.array_equal(_np(st.ecc_match_local_aligned_pyramid(dev, ECC, MP3, 1)), _np(st.ecc_match_local_aligned(dev, ECC, MP3)))


def test_keypoint_match_local_aligned_pyramid_with_a_dropped_frame(st):
    frames, _ = synth.make_stack(4, 160, 120)
    frames = frames.numpy()
    bad = np.full_like(frames[0], 128)                  # featureless: dropped
    stack = [frames[0], frames[1], bad, frames[2], frames[3]]
    pd, _, pstats = st.keypoint_match(stack, KP, return_stats=True)
    assert pd >= 1 and pstats[2]["status"] != 0
    include = [1 if (i == 0 or s["status"] == 0) else 0 for i, s in enumerate(pstats)]
    warps = [s["warp"] if include[i] else np.eye(3) for i, s in enumerate(pstats)]
    fields = st.local_align_pyramid(stack, warps, MP3, 3, include)
    for lp in (None, LocalParameters()):
        dropped, out, stats = st.keypoint_match_local_aligned_pyramid(stack, KP, MP3, 3, lp, return_stats=True)
        assert dropped == pd and st.timing()["finalize_ms"] > 0
        _stats_equal(stats, pstats)
        if lp is None:
            ref = st.mesh_stack(stack, warps, fields, MP3.step, include)
        else:
            ref = st.mesh_local_weighted_stack(stack, warps, st.local_sharpness(stack, lp), fields, MP3.step, include=include,
                                               floor=lp.floor, power=lp.power)
        assert np.array_equal(out, ref)


# ---- 5. repeatability and batches ---------------------------------------------------------------------------------------
def test_two_calls_and_host_batches_give_the_same_bits(st):
    import torch
    frames, warps, affine, p, levels, _ = mp.gpu_case_restated("bgr-homography-3")
    dev = torch.from_numpy(frames).cuda()
    a, sa = st.local_align_pyramid(dev, warps, p, levels, is_affine=affine, return_status=True)
    b, sb = st.local_align_pyramid(dev, warps, p, levels, is_affine=affine, return_status=True)
    assert np.array_equal(_np(a), _np(b)) and np.array_equal(_np(sa), _np(sb))
    # host frames in batches of frame 0 and one more: a fresh context's frame workspace holds two frames, and frame 0's
    # pyramid is built with the first batch only
    fresh = Stacker(0)
    try:
        fresh.set_option("upload_batch", 2)
        h, sh = fresh.local_align_pyramid(list(frames), warps, p, levels, is_affine=affine, return_status=True)
    finally:
        fresh.close()
    assert np.array_equal(h, _np(a)) and np.array_equal(sh, _np(sa))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(st, small_stack):
    frames = small_stack[:3]                            # 128 x 96
    I = [np.eye(3)] * 3
    calls = (lambda p, lv, f=frames: st.local_align_pyramid(f, I, p, lv),
             lambda p, lv, f=frames: st.ecc_match_local_aligned_pyramid(f, ECC, p, lv),
             lambda p, lv, f=frames: st.keypoint_match_local_aligned_pyramid(f, KP, p, lv))
    # (step, levels): what the restated arithmetic refuses at 128 x 96, and the word the message names
    word = {"levels": "levels", "step": "step", "size": "width"}
    for step, levels in ((16, 0), (16, 5), (16, -1), (8, 3), (16, 4), (8, 2), (16, 3), (32, 4), (32, 3)):
        why = mp.pyramid_refusal_restate(128, 96, step, levels)
        for call in calls:
            if why is None:
                call(MeshParameters(step=step, radius=4), levels)
            else:
                with pytest.raises(InvalidParams, match=word[why]):
                    call(MeshParameters(step=step, radius=4), levels)
    assert mp.pyramid_refusal_restate(128, 96, 32, 4) == "size" and mp.pyramid_refusal_restate(128, 96, 8, 3) == "step"
    small = [f[:31, :40] for f in frames]               # min(w, h) >> 1 = 15
    with pytest.raises(InvalidParams, match="width"):
        st.local_align_pyramid([np.ascontiguousarray(f) for f in small], I, MeshParameters(step=16, radius=4), 2)
    st.local_align_pyramid([np.ascontiguousarray(f) for f in small], I, MeshParameters(step=16, radius=4), 1)
    # everything stk_local_align refuses
    for kw, field in ((dict(step=12), "step"), (dict(radius=1), "radius"), (dict(max_iters=0), "max_iters"), (dict(epsilon=-1.0), "epsilon"),
                      (dict(max_shift=65.0), "max_shift"), (dict(min_eig=-1.0), "min_eig"), (dict(fill=17), "fill")):
        for call in calls:
            with pytest.raises(InvalidParams, match=field):
                call(MeshParameters(**kw), 2)
    for dtype in (np.uint16, np.float32):
        deep = [f.astype(dtype) for f in frames]
        for call in calls:
            with pytest.raises(NotImplementedYet, match="8-bit"):
                call(MP3, 2, deep)
        with pytest.raises(NotImplementedYet, match="8-bit"):
            st.grey_pyramid(deep[0], 2)
    for lv in (1, 5):
        with pytest.raises(InvalidParams, match="levels"):
            st.grey_pyramid(frames[0], lv)
    with pytest.raises(InvalidParams, match="width"):
        st.grey_pyramid(np.zeros((3, 40, 3), np.uint8), 3)
    # reserved and null pointers, through the C interface
    from libstacker_rs_amd.api import _Marshalled
    m = _Marshalled(frames)
    gw, gh = mesh_grid(128, 96, 16)
    fields = np.zeros((3, gh, gw, 2), F)
    fp = C.cast((C.c_void_p * 3)(*[fields.ctypes.data + i * fields[0].nbytes for i in range(3)]), C.c_void_p)
    hole = C.cast((C.c_void_p * 3)(fields.ctypes.data, None, fields.ctypes.data + 2 * fields[0].nbytes), C.c_void_p)
    M = np.ascontiguousarray(np.stack(I).reshape(3, 9))
    Mp, c, bad = C.c_void_p(M.ctypes.data), MP3._c(), MP3._c()
    bad.reserved = 1
    lib, h, fr = st._lib, st._h, C.byref(m.c_frames)
    assert lib.stk_local_align_pyramid(h, fr, Mp, None, 0, C.byref(bad), 2, fp, None) == 2 and b"reserved" in lib.stk_last_error(h)
    assert lib.stk_local_align_pyramid(h, fr, Mp, None, 0, None, 2, fp, None) == 2
    assert lib.stk_local_align_pyramid(h, fr, None, None, 0, C.byref(c), 2, fp, None) == 2
    assert lib.stk_local_align_pyramid(h, fr, Mp, None, 0, C.byref(c), 2, None, None) == 2
    assert lib.stk_local_align_pyramid(h, fr, Mp, None, 0, C.byref(c), 2, hole, None) == 2
    assert lib.stk_local_align_pyramid(h, fr, Mp, None, 0, C.byref(c), 2, fp, None) == 0
    assert lib.stk_grey_pyramid(h, fr, 2, None) == 2                       # three frames, and no planes


# ---- 7. ground truth ----------------------------------------------------------------------------------------------------
def test_quality_stack_through_the_engine(st):
    """The CPU test's three bounds on the engine's own fields and folds; the figures are printed."""
    scene, frames, truth = quality_pyramid_stack()
    p = QP["mesh"]
    bgr = [np.repeat(f[..., None], 3, axis=2) for f in frames]
    I = [np.eye(3)] * len(bgr)
    rms, errs = {}, {}
    for levels in (1, 2, 3):
        fields = st.local_align_pyramid(bgr, I, p, levels)
        out = st.mesh_stack(bgr, I, fields, p.step)
        rms[levels] = interior_rms(out[..., 0] * 255.0, scene, QP["margin"])
        e = []
        for i in range(1, len(frames)):
            nodes = -truth[i][::p.step, ::p.step]
            gh, gw = nodes.shape[:2]
            e.append(float(np.sqrt(((fields[i][:gh, :gw] - nodes)[1:-1, 1:-1] ** 2).sum(axis=-1).mean())))
        errs[levels] = e
    mean = st.mesh_stack(bgr, I, np.zeros_like(fields), p.step)
    r_mean = interior_rms(mean[..., 0] * 255.0, scene, QP["margin"])
    for levels in (1, 2, 3):
        print("quality stack through the engine, levels", levels, ": RMS mesh / plain mean", rms[levels] / r_mean,
              "field error worst / mean frame", max(errs[levels]), float(np.mean(errs[levels])))
    print("RMS(levels 3) / RMS(levels 1) =", rms[3] / rms[1])
    assert rms[3] <= 0.5 * rms[1]
    assert max(errs[3]) < 1.5
    assert np.mean(errs[1]) > 2.0

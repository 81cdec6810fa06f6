"""Coarse-to-fine local alignment, CPU side: the restatements of mesh_pyramid_restate.py against closed forms and
constructions (the box pyramid, the level matrices, an integer translation beyond one level's reach, the keep-the-seed rule,
the validity through a level that fails, the refusals), the quality stack that shows what the levels buy, and the
perturbation check that qualifies the cases and the tolerance of the GPU tests (test_gpu_mesh_pyramid.py)."""
import ctypes

import numpy as np
import pytest

import mesh_pyramid_restate as mp
from interp_restate import F, invert
from libstacker_rs_amd import MeshParameters, _ffi, mesh_pyramid_shapes
from test_cpu_mesh import grid_restate, interior_rms, local_align_restate, mesh_fill_restate, mesh_mean_restate


def _scene_u8(h, w, seed, shift=(0, 0), fmin=0.004, fmax=0.12):
    tex = mp.log_cosines(np.random.default_rng(seed), 24, fmin, fmax)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(128.0 + 100.0 * tex(x - shift[0], y - shift[1])), 0, 255).astype(np.uint8)


# ---- levels = 1 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
def test_one_level_is_local_align_plus_fill(affine):
    h, w = 61, 83
    f0, fi = _scene_u8(h, w, 1), _scene_u8(h, w, 1, shift=(1.5, -1.0))
    f0[20:40, 30:50] = 90                            # a flat square: holes for the fill
    M = np.array([[1.0, 0.01, -0.4], [-0.01, 1.0, 0.3], [0, 0, 1.0]])
    if not affine:
        M[2, :2] = (1e-5, -2e-5)
    p = MeshParameters(step=16, radius=6, max_iters=8, epsilon=0.01, max_shift=4.0, min_eig=1.0, fill=2)
    d, s, _ = local_align_restate(f0, fi, M, affine, p)
    out = mp.pyramid_align_restate(f0, fi, M, affine, p, 1)
    assert (s < 0).any() and (s > 0).any()
    assert np.array_equal(out[0]["status"], s) and np.array_equal(out[0]["d_est"], d)
    assert np.array_equal(out[0]["d"], mesh_fill_restate(d, s, p.fill))
    assert np.array_equal(out[0]["m_est"], s > 0)


# ---- the box pyramid ---------------------------------------------------------------------------------------------------
def test_box_pyramid_known_answers():
    # the +2 rounding: sums 0 .. 5 over one 2 x 2 block give 0 0 1 1 1 1, 1020 gives 255
    for total, want in ((0, 0), (1, 0), (2, 1), (3, 1), (5, 1), (6, 2), (1020, 255), (1017, 254), (1018, 255)):
        q, r = divmod(total, 4)
        blk = np.full(4, q) + (np.arange(4) < r)
        assert blk.sum() == total
        assert mp.box_pyramid_restate(blk.reshape(2, 2), 2)[1][0, 0] == want == (total + 2) >> 2
    # odd sizes: the last column and row are dropped at every halving
    g = np.arange(7 * 11).reshape(7, 11) % 251
    pyr = mp.box_pyramid_restate(g, 3)
    assert [a.shape for a in pyr] == [(7, 11), (3, 5), (1, 2)] == mesh_pyramid_shapes(11, 7, 3)
    assert pyr[1][2, 4] == (g[4, 8] + g[4, 9] + g[5, 8] + g[5, 9] + 2) >> 2
    assert pyr[2][0, 1] == (pyr[1][0, 2] + pyr[1][0, 3] + pyr[1][1, 2] + pyr[1][1, 3] + 2) >> 2
    # a constant stays, level by level; values stay in 0 .. 255
    assert all((a == 200).all() for a in mp.box_pyramid_restate(np.full((16, 16), 200), 4))
    rnd = np.random.default_rng(0).integers(0, 256, (33, 47))
    assert all(0 <= a.min() and a.max() <= 255 for a in mp.box_pyramid_restate(rnd, 4))
    with pytest.raises(Exception):
        mesh_pyramid_shapes(10, 10, 5)


# ---- the level matrices ------------------------------------------------------------------------------------------------
def test_level_matrices():
    # the double inverse is interp_restate.invert's before the cast
    H = np.array([[1.01, 0.02, -3.3], [-0.015, 0.99, 4.1], [2e-5, -1e-5, 1.0]])
    A = np.array([[0.99, 0.05, 2.5], [-0.05, 0.99, -1.25], [0, 0, 1.0]])
    for M, affine in ((H, False), (A, True), (A, False)):
        assert np.array_equal(np.asarray(mp.invert64(M, affine)).astype(F).astype(np.float64), invert(M, affine))
        assert np.array_equal(mp.level_matrix_restate(M, affine, 0), invert(M, affine))
    # a pure translation t becomes t / 2^l
    T = np.eye(3)
    T[0, 2], T[1, 2] = 8.0, -4.0
    for affine in (False, True):
        for l in (1, 2, 3):
            L = np.asarray(mp.level_matrix64(mp.invert64(T, affine), l)).reshape(3, 3)
            assert np.array_equal(L, [[1, 0, -8.0 / 2 ** l], [0, 1, 4.0 / 2 ** l], [0, 0, 1]])
    T[0, 2], T[1, 2] = 3.3, -1.7
    L = np.asarray(mp.level_matrix64(mp.invert64(T, False), 2)).reshape(3, 3)
    assert abs(L[0, 2] + 3.3 / 4) < 1e-15 and abs(L[1, 2] - 1.7 / 4) < 1e-15
    # an affine last row stays (0, 0, 1); a point maps consistently through C_l
    for l in (1, 2, 3):
        s, c = 2.0 ** l, (2.0 ** l - 1) / 2
        assert mp.level_matrix64(mp.invert64(A, True), l)[6:] == [0.0, 0.0, 1.0]
        L = np.asarray(mp.level_matrix64(mp.invert64(H, False), l)).reshape(3, 3)
        inv = np.asarray(mp.invert64(H, False)).reshape(3, 3)
        for xl, yl in ((0.0, 0.0), (10.0, 7.0), (23.5, 3.25)):
            q = L @ [xl, yl, 1.0]
            full = inv @ [s * xl + c, s * yl + c, 1.0]
            assert abs(q[0] / q[2] - (full[0] / full[2] - c) / s) < 1e-11 and abs(q[1] / q[2] - (full[1] / full[2] - c) / s) < 1e-11


# ---- an integer translation beyond one level's reach -------------------------------------------------------------------
def test_integer_translation_needs_the_levels():
    """Frame i is frame 0 moved by (8, -4) under the identity: d = (8, -4) at every node whose patches stay inside."""
    h, w = 96, 128
    f0, fi = _scene_u8(h, w, 8), _scene_u8(h, w, 8, shift=(8, -4))
    p = MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=16.0, min_eig=1.0, fill=2)
    inner = (slice(2, -2), slice(2, -2))
    want = np.array([8.0, -4.0], F)
    out3 = mp.pyramid_align_restate(f0, fi, np.eye(3), False, p, 3)
    err3 = np.sqrt(((out3[0]["d"][inner] - want) ** 2).sum(axis=-1))
    out1 = mp.pyramid_align_restate(f0, fi, np.eye(3), False, p, 1)
    err1 = np.sqrt(((out1[0]["d"][inner] - want) ** 2).sum(axis=-1))
    print("integer shift (8, -4): three levels max error", err3.max(), "one level mean error", err1.mean())
    assert (out3[0]["status"][inner] > 0).all()
    assert err3.max() < 0.05
    assert err1.mean() > 2.0


# ---- keep the seed -----------------------------------------------------------------------------------------------------
def _flat_square_pair():
    """A scene moved by (4, -4) with a flat 44 x 44 square around node (3, 4) of a step-16 grid (centre (64, 48)) in both
    frames: wider than the level-0 patch and than the level-1 patch with its gradient halo (2 (8 + 1) + 1 = 19 level pixels =
    38), narrower than the level-2 patch (17 level pixels = 68)."""
    h, w = 96, 128
    f0, fi = _scene_u8(h, w, 9), _scene_u8(h, w, 9, shift=(4, -4))
    f0[48 - 22:48 + 22, 64 - 22:64 + 22] = 77
    fi[48 - 22 - 4:48 + 22 - 4, 64 - 22 + 4:64 + 22 + 4] = 77
    return f0, fi, MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=16.0, min_eig=1.0, fill=2)


def test_a_failed_node_keeps_its_seed():
    f0, fi, p = _flat_square_pair()
    out = mp.pyramid_align_restate(f0, fi, np.eye(3), False, p, 3)
    j, k = 3, 4
    assert out[0]["status"][j, k] == -3 and out[1]["status"][j, k] == -3 and out[2]["status"][j, k] > 0
    assert out[2]["m"][j, k] and out[1]["m"][j, k] and out[0]["m_est"][j, k] and out[0]["m"][j, k]
    d2 = out[2]["d_est"][j, k]
    assert np.array_equal(out[0]["d"][j, k], F(4) * d2) and np.array_equal(out[1]["d"][j, k], F(2) * d2)
    assert np.abs(F(4) * d2 - np.array([4.0, -4.0], F)).max() < 0.5
    # not a filled value: the fill from the level-0 neighbours gives other bits
    filled = mesh_fill_restate(np.where((out[0]["status"] > 0)[..., None], out[0]["d_est"], F(0)), out[0]["status"], p.fill)
    assert not np.array_equal(filled[j, k], out[0]["d"][j, k])


def test_validity_passes_through_a_level_that_fails():
    # by construction: a flat template fails everywhere with -3; d and m are the seeds'
    rng = np.random.default_rng(2)
    g0, gi = np.full((24, 32), 50), rng.integers(0, 256, (24, 32))
    p = MeshParameters(step=16, radius=4, max_iters=4, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=2)
    gw, gh = grid_restate(64, 48, 16)
    seed, m_seed = rng.uniform(-2, 2, (gh, gw, 2)).astype(F), rng.random((gh, gw)) < 0.5
    d, s, m, _ = mp.level_estimate_restate(g0, gi, invert(np.eye(3), False), False, p, 1, gw, gh, seed, m_seed)
    assert (s == -3).all() and np.array_equal(d, seed) and np.array_equal(m, m_seed)
    # through the pyramid: every 2 x 2 box holds A + e, A - e / A - e, A + e with its own e, so level 1 is the constant A and
    # the top level of two measures nothing, while level 0 has texture: it starts as a single level does
    rng = np.random.default_rng(3)
    e = np.kron(rng.integers(-60, 61, (32, 48)), np.ones((2, 2), np.int64))
    y, x = np.mgrid[0:64, 0:96]
    f0 = (120 + np.where((x + y) % 2 == 0, e, -e)).astype(np.uint8)
    assert (mp.box_pyramid_restate(f0.astype(np.int64), 2)[1] == 120).all()
    fi = np.roll(f0, 2, axis=1)
    p = MeshParameters(step=16, radius=6, max_iters=4, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=1)
    out2, out1 = mp.pyramid_align_restate(f0, fi, np.eye(3), False, p, 2), mp.pyramid_align_restate(f0, fi, np.eye(3), False, p, 1)
    assert (out1[0]["status"] > 0).any()
    assert (out2[1]["status"] < 0).all() and not out2[1]["m"].any() and (out2[1]["d"] == 0).all()
    assert np.array_equal(out2[0]["status"], out1[0]["status"]) and np.array_equal(out2[0]["d"], out1[0]["d"])
    assert np.array_equal(out2[0]["m"], out1[0]["m"])
    # the fill carries m: a hole next to a valid node is valid after one pass, and only then
    d = np.zeros((1, 4, 2), F)
    d[0, 0] = (3, 1)
    o, m = mp.carried_fill_restate(d, np.array([[True, False, False, False]]), 1)
    assert m.tolist() == [[True, True, False, False]] and (o[0, 1] == (3, 1)).all() and (o[0, 2:] == 0).all()
    o, m = mp.carried_fill_restate(d, np.array([[True, False, False, False]]), 0)
    assert m.tolist() == [[True, False, False, False]] and np.array_equal(o, d)


# ---- the refusals ------------------------------------------------------------------------------------------------------
def test_refusal_arithmetic():
    r = mp.pyramid_refusal_restate
    assert r(96, 80, 16, 0) == "levels" and r(96, 80, 16, 5) == "levels" and r(96, 80, 16, 1) is None
    # step >> (levels - 1) >= 4: step 8 carries two levels, step 16 three, step 32 four
    assert r(512, 512, 8, 2) is None and r(512, 512, 8, 3) == "step"
    assert r(512, 512, 16, 3) is None and r(512, 512, 16, 4) == "step" and r(512, 512, 32, 4) is None
    # min(w, h) >> (levels - 1) >= 16
    assert r(64, 200, 16, 3) is None and r(63, 200, 16, 3) == "size" and r(200, 63, 16, 3) == "size"
    assert r(128, 128, 32, 4) is None and r(127, 128, 32, 4) == "size" and r(31, 31, 8, 1) is None and r(31, 32, 8, 2) == "size"
    # the order: levels, then step, then size
    assert r(10, 10, 8, 9) == "levels" and r(10, 10, 8, 3) == "step"


def test_symbols_and_signatures():
    lib = _ffi.load()
    for name in ("stk_grey_pyramid", "stk_local_align_pyramid", "stk_ecc_match_local_aligned_pyramid",
                 "stk_keypoint_match_local_aligned_pyramid"):
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert _ffi.SIGNATURES["stk_local_align_pyramid"][1][6] is ctypes.c_int32
    assert _ffi.SIGNATURES["stk_ecc_match_local_aligned_pyramid"][1][5] is ctypes.c_int32
    from libstacker_rs_amd import Stacker
    for name in ("grey_pyramid", "local_align_pyramid", "ecc_match_local_aligned_pyramid", "keypoint_match_local_aligned_pyramid"):
        assert callable(getattr(Stacker, name))


# ---- the quality stack: a scene with low frequencies seen through fields beyond one level's reach ---------------------
QP = dict(h=200, w=264, n=8, seed=5, n_cos=24, fmin=0.004, fmax=0.12, amp=(4.0, 7.0), wavelength=(260.0, 340.0), noise=2.0, margin=16,
          mesh=MeshParameters(step=16, radius=8, max_iters=10, epsilon=0.01, max_shift=16.0, min_eig=1.0, fill=2))


def quality_pyramid_stack(amp=None):
    """(scene H x W f64 in grey levels, frames n x H x W u8, true fields n x H x W x 2): test_cpu_mesh.quality_mesh_stack's
    construction with a log-uniform spectrum (a coarse level needs frequencies below 0.03 cycles/px to hold on to) and fields
    of 4 .. 7 px."""
    rng = np.random.default_rng(QP["seed"])
    h, w, n = QP["h"], QP["w"], QP["n"]
    tex = mp.log_cosines(rng, QP["n_cos"], QP["fmin"], QP["fmax"])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def scene(xx, yy):
        return 128.0 + 90.0 * tex(xx, yy)
    frames, truth = [], []
    for i in range(n):
        u = mp.smooth_field(rng, x, y, amp or QP["amp"], QP["wavelength"]) if i else np.zeros((h, w, 2))
        f = scene(x + u[..., 0], y + u[..., 1]) + rng.normal(0.0, QP["noise"], (h, w))
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
        truth.append(u)
    return scene(x, y), np.stack(frames), np.stack(truth)


def quality_figures(scene, frames, truth, fields):
    """(RMS of the mesh mean / RMS of the plain mean, field error at the inner nodes in px RMS per frame)."""
    p = QP["mesh"]
    I3 = [np.eye(3)] * len(frames)
    mesh = mesh_mean_restate(frames, I3, False, 1.0 / 255.0, fields, p.step)[..., 0] * 255.0
    mean = mesh_mean_restate(frames, I3, False, 1.0 / 255.0, [None] * len(frames), p.step)[..., 0] * 255.0
    errs = []
    for i in range(1, len(frames)):
        nodes = -truth[i][::p.step, ::p.step]
        gh, gw = nodes.shape[:2]
        errs.append(float(np.sqrt(((np.asarray(fields[i])[:gh, :gw] - nodes)[1:-1, 1:-1] ** 2).sum(axis=-1).mean())))
    return interior_rms(mesh, scene, QP["margin"]) / interior_rms(mean, scene, QP["margin"]), errs


def test_quality_stack_three_levels_halve_the_error():
    """The issue's bounds: RMS(levels 3) <= 0.5 RMS(levels 1), worst-frame field error < 1.5 px at three levels, mean-frame
    field error > 2 px at one level. Its f64 prototype measured 0.30, 0.83 px and 4.0 px; the f32 restatement's figures are
    printed here and recorded in DESIGN."""
    scene, frames, truth = quality_pyramid_stack()
    p, fig = QP["mesh"], {}
    for levels in (1, 2, 3):
        fields = [None] + [mp.pyramid_align_restate(frames[0], f, np.eye(3), False, p, levels)[0]["d"] for f in frames[1:]]
        fig[levels] = quality_figures(scene, frames, truth, fields)
        print("quality stack, levels", levels, ": RMS mesh / plain mean", round(fig[levels][0], 4), "field error worst / mean frame",
              round(max(fig[levels][1]), 3), round(float(np.mean(fig[levels][1])), 3))
    print("RMS(levels 3) / RMS(levels 1) =", fig[3][0] / fig[1][0])
    assert fig[3][0] <= 0.5 * fig[1][0]
    assert max(fig[3][1]) < 1.5
    assert np.mean(fig[1][1]) > 2.0


# ---- the perturbation check: what the GPU tests' tolerance assumes -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(mp.GPU_CASES))
def test_gpu_cases_survive_a_seed_perturbation(name):
    """gpu_tolerance assumes that a level does not expand the error of its seeds. For every case the GPU tests run, every seed
    of level l is moved by +- seed_bound(levels, l) per axis: every status at every level must stay, an estimated node must
    move by less than the bound, and a node that keeps its seed or is filled by at most the bound (plus the f32 rounding of
    the sum, 2^-20 px below 8 px). No decision of the unperturbed run may lie within 1e-9 of its threshold."""
    frames, warps, affine, p, levels, res = mp.gpu_case_restated(name)
    for i in range(1, len(frames)):
        base = res[i]
        assert not any(lv["near"].any() for lv in base), (name, i)
        assert (base[0]["status"] > 0).sum() >= base[0]["status"].size // 2, (name, i)
        planted = np.abs(base[0]["d"]).max()
        assert 3.0 < planted < 9.0, (name, i, planted)
        for l in range(levels - 1):
            b = mp.seed_bound(levels, l)
            for sx, sy in ((b, b), (-b, -b), (b, -b), (-b, b)):
                got = mp.pyramid_align_restate(frames[0], frames[i], warps[i], affine, p, levels, seed_shift={l: (sx, sy)})
                for q in range(levels):
                    assert np.array_equal(got[q]["status"], base[q]["status"]), (name, i, l, q)
                for q in range(l + 1):
                    move = np.abs(got[q]["d"].astype(np.float64) - base[q]["d"]).max(axis=-1)
                    est = base[q]["status"] > 0
                    scale = 2.0 ** (l - q)
                    assert (move[est] < b * scale).all(), (name, i, l, q, move[est].max(), b * scale)
                    assert (move[~est] <= b * scale + 2.0 ** -20).all(), (name, i, l, q, move[~est].max(), b * scale)

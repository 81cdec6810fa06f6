"""Local normalisation, CPU side: the numpy restatement (local_norm_restate.py) checked against planted answers and the
arithmetic it borrows; the shipped estimator and fill (stk_local_norm_estimate is plain host code) held to the restatement
bit for bit; the quality claim of the feature on the restatement alone; and the ctypes mirrors against the header."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import libstacker_rs_amd as ls
from libstacker_rs_amd import _ffi
from local_norm_restate import (LINEAR, NONE, OFFSET, GAIN, cell_moments_restate, estimate_restate, fill_restate, fma32, global_records,
                                grids, integer_shift_samples, norm_mean_restate, norm_quantile_restate, plane_at_pixels, quality_rms,
                                quality_stack)
from test_cpu_mesh import mesh_fill_restate
from test_cpu_robust import robust_quantile_restate
from test_cpu_weighted import weighted_restate

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_local_moments", "stk_local_norm_estimate", "stk_local_norm_stack", "stk_quantile_stack_local_norm",
       "stk_ecc_match_local_normalized", "stk_keypoint_match_local_normalized")


# ---- restatement self-checks -------------------------------------------------------------------------------------------
def test_fma_helper_is_the_fused_operation():
    # 2^-24 * 2^-24 + 1 is 1 after either rounding; (1 + 2^-23)(1 - 2^-23) - 1 = -2^-46 survives only fused
    a, b = F(1 + 2.0 ** -23), F(1 - 2.0 ** -23)
    assert fma32(a, b, F(-1)) == F(-2.0 ** -46)
    assert F(a * b) + F(-1) == 0
    # a case the f64 detour rounds twice: 1 + 2^-24 (an f32 tie) + a term below f64's last place
    x = fma32(F(2.0 ** -30), F(2.0 ** -30), F(1))
    assert x == F(1)
    rng = np.random.default_rng(0)
    p, q, r = (rng.normal(size=1000).astype(F) for _ in range(3))
    from fractions import Fraction
    for i in range(200):
        exact = Fraction(float(p[i])) * Fraction(float(q[i])) + Fraction(float(r[i]))
        got = Fraction(float(fma32(p[i], q[i], r[i])))
        ulp = Fraction(float(np.spacing(F(abs(float(got))))))
        assert abs(got - exact) <= ulp / 2


def test_planted_cell_gains_and_offsets_are_recovered():
    rng = np.random.default_rng(1)
    h, w, step = 64, 96, 32
    gw, gh, cw, ch = grids(w, h, step)
    base = rng.uniform(0.2, 0.8, (h, w, 1)).astype(np.float64)
    # X = (Y - o) / g per cell with dyadic g, o: every value and every product is exact, so LINEAR returns (g, o) exactly
    base = np.round(base * 256) / 256
    gs = np.array([[0.5, 1.0, 2.0], [2.0, 0.5, 1.0]])
    os_ = np.array([[0.125, -0.25, 0.0], [0.0, 0.125, -0.125]])
    X = np.empty_like(base)
    for J in range(ch):
        for K in range(cw):
            sl = (slice(J * step, (J + 1) * step), slice(K * step, (K + 1) * step))
            X[sl] = (base[sl] - os_[J, K]) / gs[J, K]
    samples = np.stack([base, X]).astype(F)
    assert (samples.astype(np.float64) == np.stack([base, X])).all()
    cells, _ = cell_moments_restate(samples, np.ones((2, h, w), F), step, 2)
    assert (cells[1, :, :, 0, 0] == (step // 2) ** 2).all() and (cells[0] == 0).all()
    g, o, fb = ls_estimate(cells[1])
    assert not fb.any()
    assert np.allclose(g[..., 0], gs, rtol=1e-6) and np.allclose(o[..., 0], os_, atol=1e-6)
    # the node planes: the corner nodes see one cell each and return its pair
    plane, valid, _ = estimate_restate(cells[1], w, h, step, LINEAR, 16, 0)
    assert (valid == 1).all()
    for (j, k), (J, K) in {(0, 0): (0, 0), (0, gw - 1): (0, cw - 1), (gh - 1, 0): (ch - 1, 0), (gh - 1, gw - 1): (ch - 1, cw - 1)}.items():
        assert np.isclose(plane[j, k, 0], gs[J, K], rtol=1e-6) and np.isclose(plane[j, k, 1], os_[J, K], atol=1e-6)


def ls_estimate(cells):
    from test_cpu_weighted import estimate
    return estimate(cells, LINEAR)


def test_fill_is_the_mesh_fills_arithmetic():
    rng = np.random.default_rng(2)
    gh, gw = 6, 7
    g = rng.uniform(0.5, 2, (gh, gw)).astype(F)
    o = rng.uniform(-0.2, 0.2, (gh, gw)).astype(F)
    valid = np.zeros((gh, gw), bool)
    valid[0, 0] = valid[2, 3] = valid[2, 4] = valid[5, 6] = True          # a hand-made mask: holes 1, 2 and 3 nodes from a valid one
    for passes in (0, 1, 2, 5):
        fg, fo, fm = fill_restate(g, o, valid, passes)
        ref = mesh_fill_restate(np.stack([g, o], axis=-1), valid.astype(np.int32), passes)
        # mesh_fill_restate leaves holes untouched; both agree wherever the fill has arrived, bit for bit
        assert np.array_equal(fg[fm], ref[..., 0][fm]) and np.array_equal(fo[fm], ref[..., 1][fm])
        assert np.array_equal(fg[valid], g[valid]) and np.array_equal(fo[valid], o[valid])
        assert (fm.sum() > valid.sum()) == (passes > 0)
    assert fill_restate(g, o, valid, 16)[2].all()
    # one hole beside one valid node: the neighbour's pair
    one = np.zeros((1, 2), bool)
    one[0, 0] = True
    fg, fo, fm = fill_restate(np.array([[1.5, 9]], F), np.array([[0.25, 9]], F), one, 1)
    assert fm.all() and fg[0, 1] == F(1.5) and fo[0, 1] == F(0.25)


def test_constant_planes_give_the_weighted_restatements_bits():
    rng = np.random.default_rng(3)
    n, h, w, cn, step = 5, 21, 37, 3, 16
    gw, gh, _, _ = grids(w, h, step)
    s = rng.random((n, h, w, cn)).astype(F)
    kappa = np.where(rng.random((n, h, w)) < 0.2, rng.random((n, h, w)), 1.0).astype(F)
    g = rng.uniform(0.5, 2, (n, cn)).astype(F)
    o = rng.uniform(-0.1, 0.1, (n, cn)).astype(F)
    wt = rng.uniform(0, 2, n).astype(F)
    planes = [np.broadcast_to(np.concatenate([g[i], o[i]]), (gh, gw, 2 * cn)).copy() for i in range(n)]
    ref, ref_den = weighted_restate(s, kappa, g, o, wt)
    for pl in (planes, [None] * n, [planes[0], None, planes[2], None, planes[4]]):
        out, den = norm_mean_restate(s, kappa, pl, step, g, o, wt)
        assert np.array_equal(out, ref) and np.array_equal(den, ref_den)
    part = kappa == 1
    qref, cref = robust_quantile_restate(s, part, g, o, wt, 0.5)
    qout, cout = norm_quantile_restate(s, part, planes, step, 0.5, wt=wt)
    assert np.array_equal(qout, qref) and np.array_equal(cout, cref)
    # and a plane that varies changes the result, pixel by pixel as the chain says
    P = rng.uniform(0.5, 2, (gh, gw, 2 * cn)).astype(F)
    G, O = plane_at_pixels(P, w, h, step)
    assert np.array_equal(G[0, 0], P[0, 0, :cn]) and np.array_equal(O[16, 32], P[1, 2, cn:])
    mid = fma32(F(0.5), P[0, 1, 0] - P[0, 0, 0], P[0, 0, 0])
    assert G[0, 8, 0] == mid


# ---- the shipped estimator and fill against the restatement ---------------------------------------------------------
def _random_cells(rng, ch, cw, cn, empty=0.2, constant_channel=None, big_gain=False):
    cells = np.zeros((ch, cw, cn, 6))
    for J in range(ch):
        for K in range(cw):
            if rng.random() < empty:
                continue
            n = int(rng.integers(1, 400))
            for c in range(cn):
                Y = rng.uniform(0.1, 0.9, n).astype(F).astype(np.float64)
                g, o = rng.uniform(0.6, 1.6), rng.uniform(-0.05, 0.05)
                if big_gain and (J + K) % 3 == 0:
                    g = rng.choice([0.1, 6.0])
                X = ((Y - o) / g + rng.normal(0, 0.01, n)).astype(F).astype(np.float64)
                if constant_channel == c:
                    X = np.full(n, 1.0)
                    Y = np.full(n, 1.0)
                cells[J, K, c] = [n, X.sum(), Y.sum(), (X * X).sum(), (Y * Y).sum(), (X * Y).sum()]
    return cells


@pytest.mark.parametrize("case", [
    dict(w=70, h=45, cn=3, step=16, normalize=LINEAR, min_count=16, fill=4),
    dict(w=70, h=45, cn=4, step=8, normalize=LINEAR, min_count=0, fill=16, constant_channel=3),       # BGRA alpha: vx = 0
    dict(w=64, h=33, cn=1, step=32, normalize=LINEAR, min_count=1, fill=0),
    dict(w=65, h=40, cn=3, step=64, normalize=GAIN, min_count=16, fill=2),
    dict(w=129, h=97, cn=3, step=16, normalize=LINEAR, min_count=16, fill=3, big_gain=True),          # gains beyond 4
    dict(w=129, h=97, cn=1, step=16, normalize=OFFSET, min_count=50, fill=1, empty=0.6),
    dict(w=90, h=60, cn=3, step=16, normalize=NONE, min_count=16, fill=2, empty=0.5),
    dict(w=90, h=60, cn=3, step=16, normalize=LINEAR, min_count=16, fill=16, empty=1.0),              # no valid node at all
    dict(w=90, h=60, cn=1, step=16, normalize=LINEAR, min_count=100000, fill=4),                      # none valid, global holds
], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_shipped_estimator_equals_the_restatement(case):
    rng = np.random.default_rng(zlib.crc32(str(sorted(case.items())).encode()))
    w, h, cn, step = case["w"], case["h"], case["cn"], case["step"]
    gw, gh, cw, ch = grids(w, h, step)
    cells = _random_cells(rng, ch, cw, cn, case.get("empty", 0.2), case.get("constant_channel"), case.get("big_gain", False))
    p = ls.LocalNormParameters(step=step, normalize=case["normalize"], min_count=case["min_count"], fill=case["fill"])
    plane, glob, valid = ls.local_norm_estimate(w, h, cn, cells, p, return_global=True, return_valid=True)
    mc = case["min_count"] or 16
    rplane, rvalid, (gg, go, gfb) = estimate_restate(cells, w, h, step, case["normalize"], mc, case["fill"])
    assert plane.shape == (gh, gw, 2 * cn) and plane.dtype == F
    assert np.array_equal(valid, rvalid)
    assert np.array_equal(plane, rplane)
    assert np.array_equal(glob["gain"], gg) and np.array_equal(glob["offset"], go)
    assert glob["flags"] == sum(int(b) << c for c, b in enumerate(gfb)) and glob["weight"] == 1.0
    if case.get("empty") == 1.0:
        assert (valid == 0).all() and glob["flags"] == (1 << cn) - 1 and (plane[..., :cn] == 1).all() and (plane[..., cn:] == 0).all()
    if case["min_count"] == 100000:
        assert (valid == 0).all() and glob["flags"] == 0 and (plane[..., 0] == gg[0]).all() and gg[0] != 1
    if case.get("constant_channel") is not None:
        c = case["constant_channel"]
        assert ((valid >> c) & 1 == 0).all() and (plane[..., c] == 1).all() and (plane[..., cn + c] == 0).all() and glob["flags"] == 1 << c
    if case.get("big_gain"):
        # a gain outside [0.25, 4] is an invalid node although its formula is fine
        assert ((valid & 1) == 0).any() and (valid & 1).any()


def test_estimator_refuses_bad_arguments():
    cells = np.zeros((3, 5, 1, 6))
    lib = _ffi.load()
    plane = np.zeros((4, 6, 2), F)
    for kw in (dict(step=12), dict(step=4), dict(step=512), dict(stat_step=65), dict(stat_step=-1), dict(normalize=4),
               dict(min_count=-1), dict(fill=17), dict(fill=-1)):
        with pytest.raises(ls.InvalidParams):
            ls.local_norm_estimate(70, 45, 1, cells, ls.LocalNormParameters(**{**dict(step=16), **kw}))
    p = ls.LocalNormParameters(step=16)._c()
    p.reserved[1] = 1
    assert lib.stk_local_norm_estimate(70, 45, 1, C.byref(p), C.c_void_p(cells.ctypes.data), C.c_void_p(plane.ctypes.data), None, None) == 2          # STK_INVALID_PARAMS
    p.reserved[1] = 0
    assert lib.stk_local_norm_estimate(70, 45, 2, C.byref(p), C.c_void_p(cells.ctypes.data), C.c_void_p(plane.ctypes.data), None, None) == 2          # STK_INVALID_PARAMS
    assert lib.stk_local_norm_estimate(70, 45, 1, C.byref(p), None, C.c_void_p(plane.ctypes.data), None, None) == 2          # STK_INVALID_PARAMS
    assert lib.stk_local_norm_estimate(70, 45, 1, None, C.c_void_p(cells.ctypes.data), C.c_void_p(plane.ctypes.data), None, None) == 2          # STK_INVALID_PARAMS
    assert lib.stk_local_norm_estimate(70, 45, 1, C.byref(p), C.c_void_p(cells.ctypes.data), C.c_void_p(plane.ctypes.data), None, None) == 0


# ---- quality -------------------------------------------------------------------------------------------------------
_QUALITY = {}


def quality_restated(seed):
    """(rms local median, rms global median, rms local mean, rms global mean, planes, samples, kappa, truth), computed once."""
    if seed not in _QUALITY:
        frames, warps, truth = quality_stack(seed)
        s, k = integer_shift_samples(frames, warps)
        n, h, w = k.shape
        cells, _ = cell_moments_restate(s, k, 16, 2)
        planes = [None] + [estimate_restate(cells[i], w, h, 16, LINEAR, 16, 4)[0] for i in range(1, n)]
        g, o = global_records(cells, LINEAR)
        part = k == 1
        lmed = norm_quantile_restate(s, part, planes, 16, 0.5)[0]
        gmed = robust_quantile_restate(s, part, g, o, np.ones(n, F), 0.5)[0]
        lmean = norm_mean_restate(s, k, planes, 16)[0]
        gmean = weighted_restate(s, k, g, o, np.ones(n, F))[0]
        _QUALITY[seed] = tuple(quality_rms(x, truth) for x in (lmed, gmed, lmean, gmean)) + (planes, lmed, lmean, frames, warps, truth)
    return _QUALITY[seed]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_local_normalisation_beats_the_global_one(seed):
    """Local / global RMS error against the scene at step 16, stat_step 2, LINEAR, min_count 16, fill 4, coverage 1, on the
    restatement alone: at most 0.55 for the median and for the mean (the f64 prototype's worst is 0.457)."""
    lmed, gmed, lmean, gmean = quality_restated(seed)[:4]
    print(f"seed {seed}: median local {lmed:.3f} / global {gmed:.3f} = {lmed / gmed:.3f}; mean local {lmean:.3f} / global {gmean:.3f} = {lmean / gmean:.3f}")
    assert lmed / gmed <= 0.55
    assert lmean / gmean <= 0.55


# ---- the ABI's mirrors ---------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "stacker.h")).read(), flags=re.S)


def test_ctypes_table_matches_the_header():
    hdr = _header()
    sig = _ffi.SIGNATURES
    lib = _ffi.load()
    for name in NEW:
        m = re.search(r"stk_status\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = sig[name]
        assert res is _ffi.c_status and len(args) == len(params), name
        for p, a in zip(params, args):
            # scalars by value and the typed struct pointers must agree; every other pointer is a void pointer
            if "*" not in p:
                want = {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}[p.split()[0]]
                assert a is want, (name, p)
            elif "stk_local_norm_params" in p:
                assert a is C.POINTER(_ffi.LocalNormParams), (name, p)
            elif "stk_frame_weight" in p:
                assert a is C.POINTER(_ffi.FrameWeight), (name, p)
            elif "stk_quantile_params" in p:
                assert a is C.POINTER(_ffi.QuantileParams), (name, p)
        assert getattr(lib, name) is not None
    for m in ("local_moments", "local_norm_stack", "quantile_stack_local_norm", "ecc_match_local_normalized",
              "keypoint_match_local_normalized"):
        assert callable(getattr(ls.Stacker, m))


def test_struct_layout_matches_the_header():
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*stk_local_norm_params\s*;", _header(), re.S).group(1)
    fields = [re.match(r"int32_t\s+(\w+)(\[(\d+)\])?$", d.strip()) for d in body.split(";") if d.strip()]
    assert all(fields)
    assert [f.group(1) for f in fields] == [f[0] for f in _ffi.LocalNormParams._fields_]
    assert C.sizeof(_ffi.LocalNormParams) == 4 * sum(int(f.group(3) or 1) for f in fields) == 32
    d = ls.LocalNormParameters()._c()
    assert (d.step, d.stat_step, d.normalize, d.coverage, d.min_count, d.fill, list(d.reserved)) == (64, 0, 3, 1, 0, 4, [0, 0])

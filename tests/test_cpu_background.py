"""CPU tests of the background model (include/stacker.h, stk_background_params): the struct layouts, the symbols and the Rust
table against the header; stk_background_estimate against the numpy restatement (tests/background_restate.py) bit for bit;
the planar case, exact by derivation; the quality of the definition on the restatement, before any GPU run; every refusal
of the host function; what the wrappers hand to the C ABI; the kernel map's file for the new kernels; the sanitizer harness."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import background_restate as br
import libstacker_rs_amd as ls
from libstacker_rs_amd import BG_CELL_DTYPE, BG_MEAN, BG_MEDIAN, BG_MODE, BackgroundParameters, InvalidParams, _ffi
from test_cpu_api_calls import CTX, new_stacker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("stk_background_cells", "stk_background_estimate", "stk_background_apply", "stk_background_flatten")
STRUCTS = (("stk_bg_cell", _ffi.BgCell, 48), ("stk_background_params", _ffi.BackgroundParams, 72))
PLANAR = [(150, 100, 32), (70, 70, 16), (257, 130, 64), (200, 140, 32)]
# The quality bar: 1.5 x the worst of the ten values measured on this restatement: 0.0406 for MEAN and 0.0412
# for MODE, both with recentre 1. The ten values, sizes 256 x 192 then 250 x 180, seeds 0 .. 4:
#   MEAN 0.0336 0.0302 0.0354 0.0388 0.0349 0.0386 0.0325 0.0383 0.0371 0.0406
#   MODE 0.0332 0.0307 0.0314 0.0312 0.0314 0.0335 0.0317 0.0351 0.0377 0.0412
QUALITY_BAR = {BG_MEAN: 1.5 * 0.0406, BG_MODE: 1.5 * 0.0412}
QUALITY_SIZES = ((256, 192), (250, 180))


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


def quality_params(estimator, recentre):
    return BackgroundParameters(step=32, clip_iters=3, kappa=3.0, min_count=64, max_reject=0.5, fill=4, filter=False, estimator=estimator,
                                recentre=recentre)


def planar_frame(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (1000 + 3 * x + 2 * y).astype(np.uint16)


def planar_params(step, target=(500.0,) * 4):
    return BackgroundParameters(step=step, clip_iters=0, estimator=BG_MEAN, recentre=True, filter=False, fill=4, min_count=64, target=target)


# ---- layouts, symbols, the Rust table -------------------------------------------------------------------------------
def test_struct_layouts_symbols_and_table_against_the_header(tmp_path):
    lines = []
    for cname, cls, _ in STRUCTS:
        lines.append('  printf("%%zu", sizeof(%s));\n' % cname)
        lines += ['  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_]
        lines.append('  printf("\\n");\n')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\nint main(void) {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["cc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    rows = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (cname, cls, size), row in zip(STRUCTS, rows):
        got = [int(v) for v in row.split()]
        assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], cname
        assert got[0] == size, cname
    assert BG_CELL_DTYPE.itemsize == 48
    assert [(n, BG_CELL_DTYPE.fields[n][1]) for n in BG_CELL_DTYPE.names] == [(f, getattr(_ffi.BgCell, f).offset) for f, _ in _ffi.BgCell._fields_]
    lib = _ffi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stacker.h")).read(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    rs = open(os.path.join(ROOT, "rust", "src", "amd_ffi.rs")).read()
    for name in NEW:
        assert name in _ffi.SIGNATURES and hasattr(lib, name) and re.search(r" T %s\b" % name, nm)
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        res, sig = _ffi.SIGNATURES[name]
        assert res is _ffi.c_status and len(args.split(",")) == len(sig), name
        assert "pub fn %s(" % name in rs
    for cname, _, _ in STRUCTS:
        assert "pub struct %s" % cname in rs
    assert re.search(r"STK_BG_MEDIAN\s*=\s*0,\s*STK_BG_MEAN\s*=\s*1,\s*STK_BG_MODE\s*=\s*2", hdr) and (BG_MEDIAN, BG_MEAN, BG_MODE) == (0, 1, 2)
    for name in ("BackgroundParameters", "background_estimate", "BG_CELL_DTYPE", "BG_MEDIAN", "BG_MEAN", "BG_MODE"):
        assert name in ls.__all__ and hasattr(ls, name)
    for method in ("background_cells", "background_apply", "background_flatten", "flatten_image"):
        assert callable(getattr(ls.Stacker, method))
    c = BackgroundParameters()._c(16)
    assert (c.step, c.clip_iters, c.kappa, c.f32_scale, c.estimator, c.min_count, c.max_reject, c.recentre, c.filter, c.fill, list(c.target),
            c.out_depth, list(c.reserved)) == (64, 3, 3.0, 1.0, 2, 0, 0.5, 1, 1, 4, [0.0] * 4, 16, [0, 0, 0])


# ---- 1. the estimator against the restatement -----------------------------------------------------------------------
def _random_cells(rng, gh, gw, cc, dead_channel=None):
    """records as the device writes them, around a sloped level; a tenth of them invalid in one of three ways"""
    cells = np.zeros((gh, gw, cc), BG_CELL_DTYPE)
    for j, k, c in itertools.product(range(gh), range(gw), range(cc)):
        n = int(rng.integers(200, 1090))
        kept = int(rng.integers(n * 6 // 10, n + 1))
        S = np.sort(rng.normal(2000 + 40 * k + 25 * j + 300 * c, 40, kept).round().clip(0, 65535).astype(np.int64))
        r = cells[j, k, c]
        r["n"], r["kept"], r["med"] = n, kept, S[(kept + 1) // 2 - 1]
        r["mad"] = np.sort(np.abs(S - r["med"]))[(kept + 1) // 2 - 1]
        r["lo"], r["hi"], r["sum"], r["sum2"] = S[0], S[-1], S.sum(), (S * S).sum()
        kind = rng.random()
        if kind < 0.04 or c == dead_channel:
            cells[j, k, c] = np.zeros((), BG_CELL_DTYPE)                    # an empty window
        elif kind < 0.08:
            r["kept"] = 30                                                  # below min_count
        elif kind < 0.12:
            r["n"] = 3 * kept                                               # too much rejected
    return cells


@pytest.mark.parametrize("estimator", [BG_MEDIAN, BG_MEAN, BG_MODE])
def test_estimate_equals_the_restatement(estimator):
    rng = np.random.default_rng(11 + estimator)
    seen_flags = set()
    for (w, h, step), channels, depth in zip([(150, 100, 32), (200, 140, 16), (257, 130, 64), (70, 70, 16), (300, 260, 128), (33, 17, 16)],
                                             (3, 1, 4, 3, 3, 1), (16, 8, 32, 32, 16, 16)):
        gw, gh = br.grid(w, h, step)
        cc = min(channels, 3)
        for recentre, filt, fill, dead in itertools.product((False, True), (False, True), (0, 4), (None, 1)):
            if dead is not None and cc < 2:
                continue
            p = BackgroundParameters(step=step, estimator=estimator, recentre=recentre, filter=filt, fill=fill, f32_scale=16.0,
                                     max_reject=0.45, min_count=0 if fill else 50)
            cells = _random_cells(rng, gh, gw, cc, dead)
            want = br.estimate_restate(cells, w, h, depth, p)
            got = ls.background_estimate(w, h, channels, depth, cells, p, return_rms=True, return_valid=True, return_flags=True)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (w, h, step, recentre, filt, fill, dead)
            assert got[2].tobytes() == want[2].tobytes() and got[3] == want[3] == (0 if dead is None else 2)
            if gw * gh >= 20:                                               # valid and invalid nodes both occur
                assert 0 < (want[2] == (1 << cc) - 1 - (0 if dead is None else 2)).mean() < 1
            seen_flags.add(got[3])
            if depth == 32:                                                 # sample units: the keys' level over f32_scale
                assert 100 < float(np.median(got[0])) < 250
            assert ls.background_estimate(w, h, channels, depth, cells, p).tobytes() == want[0].tobytes()
    assert seen_flags == {0, 2}


def test_estimate_by_hand():
    """17 x 17 at step 16: a 2 x 2 grid, windows [0, 8] and [8, 16] on both axes: p = 4 and 12, q = 0 and 16."""
    def rec(level, kept=81, mad=0):
        r = np.zeros((), BG_CELL_DTYPE)
        r["n"], r["kept"], r["med"], r["mad"], r["sum"], r["sum2"] = 81, kept, level, mad, kept * level, kept * level * level
        return r
    cells = np.zeros((2, 2, 1), BG_CELL_DTYPE)
    cells[0, 0, 0], cells[0, 1, 0], cells[1, 0, 0], cells[1, 1, 0] = rec(100), rec(180), rec(140), rec(220)
    p = BackgroundParameters(step=16, estimator=BG_MEDIAN, recentre=False, filter=False, fill=0)
    lev, rms, valid, flags = ls.background_estimate(17, 17, 1, 16, cells, p, return_rms=True, return_valid=True, return_flags=True)
    assert lev[..., 0].tolist() == [[100, 180], [140, 220]] and not rms.any() and valid.tolist() == [[1, 1], [1, 1]] and flags == 0
    # recentre: the slope between the centres is 80 / 8 per px in x and 40 / 8 in y; the nodes sit 4 px outside the centres
    p.recentre = True
    lev = ls.background_estimate(17, 17, 1, 16, cells, p)
    assert lev[..., 0].tolist() == [[100 - 40 - 20, 180 + 40 - 20], [140 - 40 + 20, 220 + 40 + 20]]
    # an invalid node keeps out of its neighbours' recentring: (0, 0) stays 100 in x, (1, 0) becomes 100 in x, so the y pass
    # (on the x pass's output) sees no slope in column 0; (1, 1) moves in x alone. The invalid node takes the lower median
    # of the valid levels 100, 100, 260.
    cells[0, 1, 0] = rec(180, kept=10)
    lev, valid = ls.background_estimate(17, 17, 1, 16, cells, p, return_valid=True)
    assert valid.tolist() == [[1, 0], [1, 1]] and lev[..., 0].tolist() == [[100, 100], [100, 260]]
    # MODE: mean 104 against med 100 with mad 10: |4| <= 0.3 x 14.826, level 2.5 x 100 - 1.5 x 104 = 94; mad 5: the median
    r = rec(100, mad=10)
    r["sum"] = 81 * 104
    cells[...] = r
    p = BackgroundParameters(step=16, estimator=BG_MODE, recentre=False, filter=False, fill=0)
    assert set(ls.background_estimate(17, 17, 1, 16, cells, p).ravel().tolist()) == {94.0}
    cells["mad"] = 5
    assert set(ls.background_estimate(17, 17, 1, 16, cells, p).ravel().tolist()) == {100.0}


# ---- 2. planar exactness --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,step", PLANAR)
def test_a_plane_is_modelled_exactly(w, h, step):
    """K = 1000 + 3x + 2y, MEAN without clipping: a window's mean is the plane at its centre p (the window is symmetric
    about p), recentring moves it to q along the plane's own slope, the edge extrapolation continues the slope to a last
    node beyond the frame, and the bilinear interpolation of a plane's node values is the plane: every step is exact in
    f64 / f32 for these integers, so the level equals K at every pixel and the flattened frame equals the target."""
    K = planar_frame(w, h)
    p = planar_params(step)
    gw, gh = br.grid(w, h, step)
    cells = br.cells_restate(K, p)
    assert (cells["n"][-1] == 0).all() or (cells["n"][:, -1] == 0).all()     # empty windows in the last row or column
    level, valid = ls.background_estimate(w, h, 1, 16, cells, p, return_valid=True)
    assert not valid[-1].all() or not valid[:, -1].all()
    jj, kk = np.mgrid[0:gh, 0:gw]
    assert (level[..., 0] == 1000 + 3 * kk * step + 2 * jj * step).all()
    B = br.level_at_pixels(level, w, h, step)[..., 0]
    assert (B == K).all()
    assert (br.apply_restate(K, level, step, p.target, 16) == 500).all()
    assert br.estimate_restate(cells, w, h, 16, p)[0].tobytes() == level.tobytes()


# ---- 3. quality, on the restatement ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quality():
    """{(estimator, recentre): the ten level errors}, sizes 256 x 192 and 250 x 180, seeds 0 .. 4"""
    out = {}
    for w, h in QUALITY_SIZES:
        for seed in range(5):
            f, bg = br.scene(w, h, seed)
            cells = br.cells_restate(f, quality_params(BG_MEAN, True))      # the records do not depend on estimator or recentre
            for est, rc in itertools.product((BG_MEAN, BG_MODE), (True, False)):
                lev = br.estimate_restate(cells, w, h, 16, quality_params(est, rc))[0]
                out.setdefault((est, rc), []).append(br.level_error(br.level_at_pixels(lev, w, h, 32)[..., 0], bg))
    return out


def test_level_error_on_gradient_scenes_is_under_the_bar(quality):
    bg = br.sky(256, 192)
    assert abs(float(np.sqrt(np.mean((bg - bg.mean()) ** 2))) - 115.8) < 0.1
    for est in (BG_MEAN, BG_MODE):
        print("estimator", est, "recentre 1:", np.round(quality[(est, True)], 4), "recentre 0:", np.round(quality[(est, False)], 4))
        assert max(quality[(est, True)]) <= QUALITY_BAR[est] and QUALITY_BAR[est] < 0.0625
        assert max(quality[(est, True)]) < 0.06                              # the issue's ceiling for the restatement itself


def test_recentring_beats_no_recentring_on_every_seed(quality):
    for est in (BG_MEAN, BG_MODE):
        assert all(a < b for a, b in zip(quality[(est, True)], quality[(est, False)]))


# ---- 4. refusals ----------------------------------------------------------------------------------------------------
BAD = [dict(step=8), dict(step=256), dict(step=48), dict(clip_iters=-1), dict(clip_iters=6), dict(kappa=0.0), dict(kappa=-1.0),
       dict(kappa=float("nan")), dict(kappa=float("inf")), dict(estimator=-1), dict(estimator=3), dict(min_count=-1), dict(max_reject=-0.1),
       dict(max_reject=1.5), dict(max_reject=float("nan")), dict(recentre=2), dict(filter=2), dict(filter=-1), dict(fill=-1), dict(fill=17),
       dict(target=(0.0, float("nan"), 0.0, 0.0)), dict(target=(0.0, 0.0, 0.0, float("inf")))]
BAD_F32 = [dict(f32_scale=0.0), dict(f32_scale=-1.0), dict(f32_scale=float("nan")), dict(f32_scale=float("inf"))]


def test_host_function_refusals():
    w, h = 70, 70
    cells = br.cells_restate(planar_frame(w, h), planar_params(16))
    assert ls.background_estimate(w, h, 1, 16, cells, planar_params(16)).shape == (6, 6, 1)
    for kw in BAD:
        with pytest.raises(InvalidParams):
            ls.background_estimate(w, h, 1, 16, cells, BackgroundParameters(**dict(dict(step=16), **kw)))
    for kw in BAD_F32:
        ls.background_estimate(w, h, 1, 16, cells, BackgroundParameters(step=16, **kw))          # read for f32 frames only
        with pytest.raises(InvalidParams):
            ls.background_estimate(w, h, 1, 32, cells, BackgroundParameters(step=16, **kw))
    for k in range(3):
        class Reserved(BackgroundParameters):
            def _c(self, depth=0):
                c = super()._c(depth)
                c.reserved[k] = 1
                return c
        with pytest.raises(InvalidParams):
            ls.background_estimate(w, h, 1, 16, cells, Reserved(step=16))
    with pytest.raises(InvalidParams):
        ls.background_estimate(w, h, 1, 16, cells[:5], planar_params(16))                      # a record table of the wrong size
    lib = _ffi.load()
    p = planar_params(16)._c(16)
    rec = np.ascontiguousarray(cells.reshape(-1))
    cp, lev = rec.ctypes.data_as(C.POINTER(_ffi.BgCell)), np.zeros(36, np.float32)
    good = (w, h, 1, 16, C.byref(p), cp, C.c_void_p(lev.ctypes.data), None, None, None)
    assert lib.stk_background_estimate(*good) == 0
    for i, v in ((0, 0), (1, -1), (2, 2), (2, 5), (3, 12), (3, 64), (4, None), (5, None), (6, None)):
        args = list(good)
        args[i] = v
        assert lib.stk_background_estimate(*args) == 2, i


# ---- 5. what the wrappers hand to the C ABI -------------------------------------------------------------------------
def _spy_frames(st, name, seen, w, h, cn, depth):
    """the stk_frames behind the void pointer, read at call time"""
    real = getattr(st._lib, name)

    def spy(*a):
        f = a[1]._obj
        seen["frames"] = (f.n, f.width, f.height, f.channels, f.depth, f.location, f.row_stride_bytes)
        seen["data"] = [bytes(C.string_at(f.data[k], w * h * cn * (depth // 8))) for k in range(f.n)]
        return real(*a)
    setattr(st._lib, name, spy)


@pytest.mark.parametrize("dt", [np.uint8, np.uint16, np.float32])
def test_what_the_wrappers_hand_to_the_c_abi(dt):
    rng = np.random.default_rng(3)
    n, h, w, cn = 3, 40, 50, 3
    depth = 8 * np.dtype(dt).itemsize
    frames = rng.integers(0, 200, (n, h, w, cn)).astype(dt)
    gw, gh = br.grid(w, h, 16)
    p = BackgroundParameters(step=16, clip_iters=2, kappa=2.5, f32_scale=8.0, estimator=BG_MEAN, min_count=9, max_reject=0.25, recentre=False,
                             filter=False, fill=7, target=(1.0, 2.0, 3.0, 4.0))
    mask = (rng.random((h, w)) < 0.1).astype(np.uint8)

    # background_cells
    st, seen = new_stacker(), {}
    _spy_frames(st, "stk_background_cells", seen, w, h, cn, depth)
    st._lib.reads = {3: h * w}
    cells = st.background_cells(frames, p, mask)
    name, snap = st._lib.last()
    assert name == "stk_background_cells" and snap[0] == CTX and snap[2] == _bytes_of(p._c(depth)) and snap[3][1] == mask.tobytes() and snap[4] == 0
    assert seen["frames"] == (n, w, h, cn, depth, 0, 0) and seen["data"] == [frames[i].tobytes() for i in range(n)]
    assert cells.shape == (n, gh, gw, 3) and cells.dtype == BG_CELL_DTYPE and snap[5] == _bytes_of(_ffi.BgCell())
    st.background_cells(frames)
    snap = st._lib.last()[1]
    assert snap[2] == _bytes_of(BackgroundParameters()._c(depth)) and snap[3] is None and snap[4] == 0
    with pytest.raises(InvalidParams):
        st.background_cells(frames, p, mask[:-1])
    with pytest.raises(ls.NotEnoughFiles):
        st.background_cells([])

    # background_apply
    planes = [rng.random((gh, gw, 3)).astype(np.float32), None, rng.random((gh, gw, 3)).astype(np.float32)]
    for out_depth in (None, 32):
        st, seen = new_stacker(), {}
        _spy_frames(st, "stk_background_apply", seen, w, h, cn, depth)
        st._lib.reads = {2: ("tbl", n, gh * gw * 3 * 4), 4: 16, 6: ("tbl", n, 0)}
        out = st.background_apply(frames, planes, 16, (1.0, 2.0, 3.0, 4.0), out_depth)
        name, snap = st._lib.last()
        od = depth if out_depth is None else 32
        assert name == "stk_background_apply" and snap[0] == CTX and snap[3] == 16 and snap[5] == od and snap[7] == 0
        assert snap[2][2] == [planes[0].tobytes(), None, planes[2].tobytes()] and snap[4][1] == np.array([1, 2, 3, 4], np.float32).tobytes()
        assert out.shape == (n, h, w, cn) and out.dtype == (np.float32 if od == 32 else dt)
        assert snap[6][1] == [out.ctypes.data + i * out[0].nbytes for i in range(n)]
        assert seen["frames"] == (n, w, h, cn, depth, 0, 0)
    st = new_stacker()
    st.background_apply(frames, None, 64)
    snap = st._lib.last()[1]
    assert snap[2] is None and snap[3] == 64
    mine = np.zeros((n, h, w + 3, cn), dt)[:, :, :w]                          # the caller's row-strided outputs
    st._lib.reads = {6: ("tbl", n, 0)}
    assert st.background_apply(frames, planes, 16, out=list(mine)) is not None
    snap = st._lib.last()[1]
    assert snap[7] == (w + 3) * cn * (depth // 8) and snap[6][1] == [mine[i].ctypes.data for i in range(n)]
    for bad in (planes[:2], [planes[0][:-1], None, None]):
        with pytest.raises(InvalidParams):
            st.background_apply(frames, bad, 16)

    # background_flatten, every combination of the return flags
    for flags in itertools.product((False, True), repeat=3):
        st, seen = new_stacker(), {}
        _spy_frames(st, "stk_background_flatten", seen, w, h, cn, depth)
        st._lib.reads = {3: h * w, 5: ("tbl", n, 0), 7: ("tbl", n, 0), 8: ("tbl", n, 0)}
        res = st.background_flatten(frames, p, mask, return_planes=flags[0], return_rms=flags[1], return_cells=flags[2])
        name, snap = st._lib.last()
        assert name == "stk_background_flatten" and snap[0] == CTX and snap[2] == _bytes_of(p._c(depth)) and snap[3][1] == mask.tobytes()
        assert snap[4] == 0 and snap[6] == 0 and seen["frames"] == (n, w, h, cn, depth, 0, 0)
        res = res if isinstance(res, tuple) else (res,)
        assert len(res) == 1 + sum(flags) and res[0].shape == (n, h, w, cn) and res[0].dtype == dt
        assert snap[5][1] == [res[0].ctypes.data + i * res[0][0].nbytes for i in range(n)]
        rest = list(res[1:])
        for k, idx in ((0, 7), (1, 8)):
            if flags[k]:
                a = rest.pop(0)
                assert a.shape == (n, gh, gw, 3) and a.dtype == np.float32 and snap[idx][1] == [a.ctypes.data + i * a[0].nbytes for i in range(n)]
            else:
                assert snap[idx] is None
        if flags[2]:
            assert rest.pop(0).dtype == BG_CELL_DTYPE and snap[9] is not None
        else:
            assert snap[9] is None
        assert rest == []
    st = new_stacker()
    st.background_flatten(frames, BackgroundParameters(out_depth=32))
    assert st._lib.last()[1][2] == _bytes_of(BackgroundParameters()._c(32))

    # flatten_image: a one-frame f32 stack
    if dt == np.float32:
        st, seen = new_stacker(), {}
        _spy_frames(st, "stk_background_flatten", seen, w, h, cn, 32)
        img, plane = st.flatten_image(frames[0], p, return_plane=True)
        assert seen["frames"] == (1, w, h, cn, 32, 0, 0) and seen["data"] == [frames[0].tobytes()]
        assert img.shape == (h, w, cn) and img.dtype == np.float32 and plane.shape == (gh, gw, 3)
        assert st.flatten_image(frames[0, ..., 0]).shape == (h, w, 1)
    else:
        with pytest.raises(InvalidParams):
            new_stacker().flatten_image(frames[0])


# ---- 6. the kernel map's supplement ---------------------------------------------------------------------------------
def test_the_new_kernels_have_their_rows_in_a_file_of_their_own_beside_the_kernel_map(tmp_path):
    """tests/kernel_map_background.tsv: one row per instantiation (nine of the cells kernel; fifteen of the apply kernel: five
    depth pairs x three channel counts), each naming the GPU test file, and nothing else; tests/kernel_map.tsv has none of
    them. tools/kernel_coverage.py reads the file as a part of the main map (its PARTS), so tests/test_cpu_kernel_map.py
    holds these rows against the tree like every other, and `map` writes a kernel back into the file that lists it."""
    from test_cpu_kernel_map import kc
    extra = os.path.join(ROOT, "tests", "kernel_map_background.tsv")
    assert kc.parts() == [extra] and extra not in kc.supplements()
    rows = kc.read_rows(extra)
    assert all(r[0] == "kernels_background" and r[3] == ["test_gpu_background.py"] for r in rows)
    types = ("unsigned char", "unsigned short", "float")
    cells = {re.search(r"<(.*?)>", r[2]).group(1) for r in rows if "background_cells_kernel<" in r[2]}
    apply_ = {re.search(r"<(.*?)>", r[2]).group(1) for r in rows if "background_apply_kernel<" in r[2]}
    assert cells == {"%s, %d" % (t, c) for t in types for c in (1, 3, 4)}
    pairs = [(t, t) for t in types] + [("unsigned char", "float"), ("unsigned short", "float")]
    assert apply_ == {"%s, %s, %d" % (a, b, c) for a, b in pairs for c in (1, 3, 4)}
    assert len(rows) == 24
    main = kc.read_rows(kc.MAP)
    assert not {r[1] for r in rows} & {r[1] for r in main} and not any(r[0] == "kernels_background" for r in main)
    assert kc.read_file(kc.MAP) == main + rows and kc.read_file(extra) == rows
    whole = kc.read_map()
    assert len(whole) == len(main) + 24 + sum(len(kc.read_rows(f)) for f in kc.supplements()) and {r[1] for r in rows} <= {r[1] for r in whole}
    # write_map on copies of every file: every row returns to its file, byte for byte
    files = [kc.MAP] + kc.parts() + kc.supplements()
    copies = [str(tmp_path / os.path.basename(f)) for f in files]
    for src, dst in zip(files, copies):
        open(dst, "w").write(open(src).read())
    kernels, seen = {}, {}
    for unit, mangled, _, tests in kc.read_map(copies[0]):
        kernels.setdefault(unit, []).append(mangled)
        seen[mangled] = set(tests)
    kc.write_map({u: sorted(v) for u, v in kernels.items()}, seen, copies[0])
    assert all(open(src).read() == open(dst).read() for src, dst in zip(files, copies))


# ---- 7. the sanitizer harness ---------------------------------------------------------------------------------------
def test_estimator_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "background_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "background_harness.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=500)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout[-1500:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

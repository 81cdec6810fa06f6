"""numpy restatement of the loader of the column-walking ECC pass (kernels_ecc_col.hip): which global and LDS bytes every
LDS-DMA transfer and every tap read of a strip touches, and in which order, without a single pixel value.

Restated: ecc_plan's strides, plane layout and reserves (stacker.cpp), launch_ecc_iter's unit partition and the kernel's
walk from a wave's units to strips, the classification of a strip from its four corners (fast / xb / ringable), the ring
route step by step (fill, wait, sample, locate, tap reads, the run-time check, up to two frame-0 rows and one template
row per step, the four-way slot rotation, `last`), the gather routes' and the first-iteration route's addresses, and
ecc_run's scratch launch for a start at the identity.

Arithmetic: f32 wherever the kernel uses f32. fma(a, b, c) is the f64 product plus addend rounded once to f32 (mode
"fma") or two f32 roundings (mode "muladd", for the ambiguity test only). v_rcp_f32 is the correctly rounded reciprocal
(mode "rn"), or one ulp above / below it ("up" / "down"); all three give exactly 1 for W = 1.

Outstanding transfers are a FIFO that completes in order: a transfer is its sequence number, and a wait that leaves k in
flight guarantees that every sequence number below (issued - k) has completed. That the hardware completes LDS-DMA in
order is NOT shown here: it is taken from the ISA guide.

The constants (REF_PAD, LROW, LWP, LK, LT, the lookahead default, the two reserve expressions, the thresholds of the
corner test) are read from the sources: an edit of either side fails the tests until the other follows."""
import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

F = np.float32
CSRC = Path(__file__).resolve().parent.parent / "libstacker_rs_amd" / "csrc"
NONE = -(1 << 40)              # "no row" in a slot


def _one(name, pattern, conv=int):
    """The single match of `pattern` in csrc/`name`; anything else is an error."""
    found = re.findall(pattern, (CSRC / name).read_text())
    assert len(found) == 1, "%s: %d matches of %r (the restatement reads this constant from the source)" % (name, len(found), pattern)
    return conv(found[0]) if not isinstance(found[0], tuple) else tuple(conv(v) for v in found[0])


@functools.lru_cache(maxsize=None)
def constants():
    col = "kernels_ecc_col.hip"
    c = SimpleNamespace()
    c.REF_PAD = _one("common.h", r"constexpr int REF_PAD = (\d+);")
    c.REF_PLANES = _one("stacker.cpp", r"constexpr int REF_PLANES = (\d+);")
    c.LROW = _one(col, r"constexpr int LROW = (\d+);")
    c.LWP = _one(col, r"constexpr int LWP = (\d+);")
    c.LK = _one(col, r"constexpr int LK = (\d+);")
    c.LT = _one(col, r"constexpr int LT = (\d+);")
    c.LOOKAHEAD = _one("context.h", r"int opt_ecc_ring_lookahead = (\d+);")
    c.RELAXED = _one(col, r"#define STK_COL_RELAXED (\d)")
    # the two reserve expressions of ecc_plan
    c.REF_TAIL = _one("stacker.cpp", r"ctx->ref\.reserve\(pl\.ref_plane_floats \* REF_PLANES \* sizeof\(float\) \+ (\d+)\)")
    c.TEMPL_TAIL_ROWS, c.TEMPL_TAIL = _one(
        "stacker.cpp", r"ctx->templates\.reserve\(pl\.templ_plane_stride \* sizeof\(float\) \* std::max\(n_templates, 1\) \+ "
                       r"(\d+) \* \(size_t\)pl\.templ_row_stride \* sizeof\(float\) \+ (\d+)\)")
    # derived exactly as the kernel derives them
    _one(col, r"(constexpr int LTOFF = \(LK \+ 1\) \* LROW;)", str)
    _one(col, r"(constexpr int LWAVE = LTOFF \+ LT \* 256;)", str)
    c.LTOFF = (c.LK + 1) * c.LROW
    c.LWAVE = c.LTOFF + c.LT * 256
    # the corner test
    c.W_MIN, c.INSET = _one(col, r"fast = fast & \(W >= ([\d.]+)f\) & \(px >= ([\d.]+)f\) & \(px <= c\.mxw - [\d.]+f\)", float)
    assert _one(col, r"& \(py >= ([\d.]+)f\) & \(py <= c\.mxh - [\d.]+f\);", float) == c.INSET
    assert _one(col, r"\(px <= c\.mxw - ([\d.]+)f\)", float) == c.INSET and _one(col, r"\(py <= c\.mxh - ([\d.]+)f\)", float) == c.INSET
    _one(col, r"(\(\(int\)__builtin_floorf\(sxmin\) - 2\) & ~3\))", str)
    _one(col, r"(\(\(int\)__builtin_floorf\(sxmax\) \+ 3 - xb <= LWP - 1\))", str)
    c.SPREAD = _one(col, r"\(__builtin_fabsf\(cpy\[1\] - cpy\[0\]\) <= ([\d.]+)f\) & \(__builtin_fabsf\(cpy\[3\] - cpy\[2\]\) <= [\d.]+f\);", float)
    assert _one(col, r"\(__builtin_fabsf\(cpy\[3\] - cpy\[2\]\) <= ([\d.]+)f\);", float) == c.SPREAD
    got = _one(col, r"ringable = ringable & \(y1 - y0 >= (\d+)\) & \(d0 >= ([\d.]+)f \* n\) & \(d0 <= ([\d.]+)f \* n\) & "
                    r"\(d1 >= ([\d.]+)f \* n\) & \(d1 <= ([\d.]+)f \* n\);", float)
    c.MIN_ROWS, c.RATE_LO, c.RATE_HI = int(got[0]), got[1], got[2]
    assert (got[3], got[4]) == (c.RATE_LO, c.RATE_HI)
    # the run-time check, the fetch rule and the two waits, as the model states them below
    _one(col, r"(violated \|= \(safe - \(ihi \+ 2\)\) \| \(ilo - 1 \+ LK - 1 - loaded\);)", str)
    assert (CSRC / col).read_text().count("if (loaded < ihi + la) dma_row();") == 2
    _one(col, r"(loaded = min\(i0, i1\) - 2;)", str)
    _one(col, r"(const int want = max\(i0, i1\) \+ la;)", str)
    _one(col, r"(wait_keep\(std::integral_constant<bool, STK_COL_RELAXED != 0>\{\}, prev_issued\);)", str)
    _one(col, r"(wait_keep\(std::false_type\{\}, prev_issued\);)", str)
    _one(col, r'("n"\(0\), "n"\(4 \+ X\), "n"\(3 \+ X\), "n"\(2 \+ X\), "n"\(1 \+ X\))', str)
    return c


# ---- arithmetic ---------------------------------------------------------------------------------------------------------
def fma(a, b, c, mode="fma"):
    a, b, c = np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)
    if mode == "fma":
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    assert mode == "muladd"
    return (a * b).astype(F) + c


def rcp(w, mode="rn"):
    w = np.asarray(w, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (F(1) / w).astype(F)
    if mode == "rn":
        return r
    assert mode in ("up", "down")
    moved = np.nextafter(r, F(np.inf) if mode == "up" else F(-np.inf), dtype=F)
    return np.where(w == F(1), r, moved).astype(F)


def warp9(warp, motion="homography"):
    """The nine f32 constants of the slot: rows 0 and 1 of the caller's start, (0, 0, 1) below a 2 x 3 motion."""
    m = np.eye(3, dtype=F)
    wv = np.asarray(warp, F)
    m[:wv.shape[0], :] = wv
    if motion != "homography":
        m[2] = (0, 0, 1)
    return m.reshape(9)


def source_coords(m, fx, fy, arith=("fma", "rn")):
    """(sx, sy, W) of the pixels (fx, fy): colX = fma(m0, x, m2), X = fma(m1, y, colX), ..., sx = X * rcp(W).
    (The corners are evaluated as fma(m1, y, fma(m0, x, m2)): the same two operations.)"""
    fm, rm = arith
    fx, fy = np.asarray(fx, F), np.asarray(fy, F)
    X = fma(m[1], fy, fma(m[0], fx, m[2], fm), fm)
    Y = fma(m[4], fy, fma(m[3], fx, m[5], fm), fm)
    W = fma(m[7], fy, fma(m[6], fx, m[8], fm), fm)
    r = rcp(W, rm)
    with np.errstate(invalid="ignore", over="ignore"):
        return (X * r).astype(F), (Y * r).astype(F), W


def floor_int(v):
    """v_cvt_flr_i32_f32 on a finite coordinate."""
    return np.floor(v).astype(np.int64)


# ---- ecc_plan -------------------------------------------------------------------------------------------------------------
def plan(w, h, n_templates=1, ecc_blocks=0, ecc_slots=0):
    c = constants()
    p = SimpleNamespace(w=w, h=h, n_templates=n_templates)
    p.templ_row_stride = (w + 3) & ~3
    p.templ_plane_stride = p.templ_row_stride * h
    p.ref_stride = (w + 2 * c.REF_PAD + 3) & ~3
    p.ref_plane_floats = p.ref_stride * (h + 2 * c.REF_PAD)
    slots = ecc_slots
    if slots <= 0:
        nt = max(n_templates, 1)
        if w * h <= 1920 * 1088:
            rounds = (nt + 63) // 64
            slots = (nt + rounds - 1) // rounds
        elif nt <= 128:
            slots = nt
        else:
            rounds = max(3, (nt + 95) // 96)
            slots = (nt + rounds - 1) // rounds
    p.n_slots = max(1, min(slots, max(n_templates, 1)))
    units = (h + 3) // 4
    strip_rows = ((w + 63) // 64) * h
    nb = ecc_blocks // p.n_slots if ecc_blocks > 0 else max(min(64, units), min(288, strip_rows // (4 * 112)))
    nb = max(8, min(units, nb))
    p.nb = max(8, (nb // 8) * 8)
    # the planes, in floats from the start of `ref`: I, gx, gy, (gx, gy), (I, gx, gy); each pointer is pixel (0, 0)
    corner = c.REF_PAD * p.ref_stride + c.REF_PAD
    rpf = p.ref_plane_floats
    p.corner = corner
    p.planes = {"I": (0, 1), "gx": (rpf, 1), "gy": (2 * rpf, 1), "gxy": (3 * rpf, 2), "igg": (5 * rpf, 3)}     # (first float, floats per pixel)
    p.base = {k: first + per * corner for k, (first, per) in p.planes.items()}
    assert 5 + 3 == c.REF_PLANES
    p.ref_bytes = rpf * c.REF_PLANES * 4 + c.REF_TAIL
    p.templ_bytes = p.templ_plane_stride * 4 * max(n_templates, 1) + c.TEMPL_TAIL_ROWS * p.templ_row_stride * 4 + c.TEMPL_TAIL
    # launch_ecc_iter
    total = ((w + 63) >> 6) * h
    p.units_q, p.units_r = total // (p.nb * 4), total % (p.nb * 4)
    return p


def strips(p):
    """Every wave's walk over its run of units: arrays wave, col, y0, y1 (one entry per strip, in launch order)."""
    out = []
    for g in range(p.nb * 4):
        u = g * p.units_q + min(g, p.units_r)
        uend = u + p.units_q + (1 if g < p.units_r else 0)
        while u < uend:
            col = u // p.h
            y0 = u - col * p.h
            y1 = min(p.h, y0 + (uend - u))
            u += y1 - y0
            out.append((g, col, y0, y1))
    a = np.asarray(out, np.int64).reshape(-1, 4)
    return SimpleNamespace(wave=a[:, 0], col=a[:, 1], y0=a[:, 2], y1=a[:, 3], n=len(a))


# ---- the corner test ------------------------------------------------------------------------------------------------------
def classify(p, s, m, ring=1, arith=("fma", "rn")):
    """fast, xb, ringable per strip, and why a fast strip is not ringable (bit 1 window, 2 lane spread, 4 rate, 8 short)."""
    c = constants()
    mxw, mxh = F(p.w - 1), F(p.h - 1)
    fast = s.col * 64 + 63 < p.w
    cx = [(s.col * 64).astype(F), (s.col * 64 + 63).astype(F)]
    cy = [s.y0.astype(F), (s.y1 - 1).astype(F)]
    cpx, cpy = [], []
    for k in range(4):
        px, py, W = source_coords(m, cx[k & 1], cy[k >> 1], arith)
        cpx.append(px)
        cpy.append(py)
        with np.errstate(invalid="ignore"):
            fast = fast & (W >= F(c.W_MIN)) & (px >= F(c.INSET)) & (px <= mxw - F(c.INSET)) & (py >= F(c.INSET)) & (py <= mxh - F(c.INSET))
    with np.errstate(invalid="ignore"):
        sxmin = np.where(fast, np.minimum(np.minimum(cpx[0], cpx[1]), np.minimum(cpx[2], cpx[3])), F(0))
        sxmax = np.where(fast, np.maximum(np.maximum(cpx[0], cpx[1]), np.maximum(cpx[2], cpx[3])), F(0))
        xb = (np.floor(sxmin).astype(np.int64) - 2) & ~np.int64(3)
        window = np.floor(sxmax).astype(np.int64) + 3 - xb <= c.LWP - 1
        spread = (np.abs(cpy[1] - cpy[0]) <= F(c.SPREAD)) & (np.abs(cpy[3] - cpy[2]) <= F(c.SPREAD))
        n = (s.y1 - 1 - s.y0).astype(F)
        d0, d1 = cpy[2] - cpy[0], cpy[3] - cpy[1]
        lo, hi = F(c.RATE_LO) * n, F(c.RATE_HI) * n
        rate = (d0 >= lo) & (d0 <= hi) & (d1 >= lo) & (d1 <= hi)
    long_enough = s.y1 - s.y0 >= c.MIN_ROWS
    ringable = fast & (ring != 0) & window & spread & long_enough & rate
    why = np.where(fast, (~window) * 1 + (~spread) * 2 + (~rate) * 4 + (~long_enough) * 8, 0)
    width = np.where(fast, np.floor(sxmax).astype(np.int64) + 3 - xb, 0)
    return SimpleNamespace(fast=fast, xb=xb, ringable=ringable, why=why, cpx=cpx, cpy=cpy, window=width)


@functools.lru_cache(maxsize=8)
def _image_coords_cached(w, h, mkey, arith):
    m = np.frombuffer(mkey, F)
    ncol = (w + 63) // 64
    xc = np.minimum(np.arange(ncol * 64), w - 1).astype(F)            # the lane clamp
    sx, sy, W = source_coords(m, xc[None, :], np.arange(h, dtype=F)[:, None], arith)
    return sx, sy


def image_coords(p, m, arith=("fma", "rn")):
    """(sx, sy) of every lane of every row, f32, [h, 64 * columns] (lanes past the frame repeat its last pixel)."""
    return _image_coords_cached(p.w, p.h, np.asarray(m, F).tobytes(), arith)


# ---- the ring route -------------------------------------------------------------------------------------------------------
def keep_in_flight(prev, extra):
    """wait_keep: the vmcnt its four branches leave."""
    return np.where(prev < 2, 1, np.where(prev == 2, 2, np.where(prev == 3, 3, 4))) + extra


def simulate_ring(p, s, cl, m, lookahead, arith=("fma", "rn"), frame=0, relaxed=None, relaxed_last=0):
    """Every ringable strip through run_ring, all strips at once (a strip is a row of the state arrays; the 64 lanes are the
    second axis). Returns per-strip results and the extremes of what was touched."""
    c = constants()
    relaxed = c.RELAXED if relaxed is None else relaxed
    LK, LT, LROW = c.LK, c.LT, c.LROW
    idx = np.flatnonzero(cl.ringable)
    S = len(idx)
    col, y0, y1, xb = s.col[idx], s.y0[idx], s.y1[idx], cl.xb[idx]
    sx_all, sy_all = image_coords(p, m, arith)
    lanes = np.arange(64)
    ar = np.arange(S)

    def row_coords(y):
        xs = col[:, None] * 64 + lanes[None, :]
        return floor_int(sx_all[y[:, None], xs]), floor_int(sy_all[y[:, None], xs])

    slot_row = np.full((S, LK + 1), NONE, np.int64)
    slot_seq = np.zeros((S, LK + 1), np.int64)
    t_row = np.full((S, LT), NONE, np.int64)
    t_seq = np.zeros((S, LT), np.int64)
    nissued = np.zeros(S, np.int64)           # sequence number of the next transfer
    completed = np.zeros(S, np.int64)         # every sequence number below this has landed
    issued = np.zeros(S, np.int64)
    loaded = np.zeros(S, np.int64)
    dst = np.zeros(S, np.int64)               # the running slot of the next frame-0 row (the kernel's `dst`, in slots)
    r = SimpleNamespace(index=idx, n=S)
    r.row_min = np.full(S, 1 << 40, np.int64)
    r.row_max = np.full(S, NONE, np.int64)
    r.trow_max = np.full(S, NONE, np.int64)
    r.slot_is_row_and_7 = np.ones(S, bool)
    r.lds_inside = np.ones(S, bool)
    r.n_row_transfers = np.zeros(S, np.int64)

    def dma_row(mask):
        k = np.flatnonzero(mask)
        row = loaded[k] + 1
        sl = dst[k]
        r.slot_is_row_and_7[k] &= sl == (row & (LK - 1))
        r.lds_inside[k] &= (sl * LROW >= 0) & (sl * LROW + LROW <= c.LWAVE)
        slot_row[k, sl] = row
        slot_seq[k, sl] = nissued[k]
        nissued[k] += 1
        issued[k] += 1
        z = k[sl == 0]                          # slot 0 ... and behind the last slot
        slot_row[z, LK] = loaded[z] + 1
        slot_seq[z, LK] = nissued[z]
        nissued[z] += 1
        issued[z] += 1
        r.lds_inside[z] &= LK * LROW + LROW <= c.LTOFF
        r.row_min[k] = np.minimum(r.row_min[k], row)
        r.row_max[k] = np.maximum(r.row_max[k], row)
        r.n_row_transfers[k] += 1
        dst[k] = np.where(sl + 1 == LK, 0, sl + 1)
        loaded[k] += 1

    next_trow = y0.copy()

    def dma_templ(mask, slot):
        k = np.flatnonzero(mask)
        t_row[k, slot] = next_trow[k]
        t_seq[k, slot] = nissued[k]
        nissued[k] += 1
        issued[k] += 1
        r.lds_inside[k] &= c.LTOFF + slot * 256 + 256 <= c.LWAVE
        r.trow_max[k] = np.maximum(r.trow_max[k], next_trow[k])
        next_trow[k] += 1

    def taps_unsafe(ix, iy):
        """Per strip: some lane's 2 x 2 taps are not the landed rows iy and iy + 1, or leave their slot."""
        sl = iy & (LK - 1)
        up = (np.take_along_axis(slot_row, sl, 1) == iy) & (np.take_along_axis(slot_seq, sl, 1) < completed[:, None])
        dn = (np.take_along_axis(slot_row, sl + 1, 1) == iy + 1) & (np.take_along_axis(slot_seq, sl + 1, 1) < completed[:, None])
        off = 12 * (ix - xb[:, None])
        inside = (off >= 0) & (off + 24 <= LROW) & (sl + 1 <= LK)
        return ~(up & dn & inside).all(axis=1), ~inside.all(axis=1)

    def sample_unsafe(slot, row):
        return ~((t_row[ar, slot] == row) & (t_seq[ar, slot] < completed))

    everyone = np.ones(S, bool)
    # fill
    ix, iy = row_coords(y0)
    i0, i1 = iy[:, 0], iy[:, 63]
    loaded[:] = np.minimum(i0, i1) - 2
    dst[:] = (loaded + 1) & (LK - 1)
    want = np.maximum(i0, i1) + lookahead
    while (loaded < want).any():
        dma_row(loaded < want)
    for k in range(3):
        dma_templ(everyone, k)
    completed[:] = nissued                     # s_waitcnt vmcnt(0)
    r.fill_transfers = nissued.copy()
    bad, outside = taps_unsafe(ix, iy)
    r.unflagged = bad.copy()                   # an unsafe read with `violated` still clear
    r.tap_outside_slot = outside.copy()
    ilo, ihi = np.minimum(i0, i1), np.maximum(i0, i1)
    r.guard_rows = ((iy >= ilo[:, None] - 1) & (iy <= ihi[:, None] + 1)).all(axis=1)
    r.guard_cols = ((ix >= xb[:, None]) & (ix + 1 <= xb[:, None] + c.LWP - 1)).all(axis=1)

    prev_issued = np.ones(S, np.int64)
    safe = loaded.copy()
    before_prev = loaded.copy()
    violated = np.zeros(S, bool)
    r.first_violation = np.full(S, -1, np.int64)
    r.max_in_flight = np.zeros(S, np.int64)
    n_steps = y1 - y0 - 1
    for j in range(int(n_steps.max()) if S else 0):
        act = j < n_steps
        # wait
        k = keep_in_flight(prev_issued, 1 if relaxed else 0)
        completed = np.where(act, np.maximum(completed, nissued - k), completed)
        r.max_in_flight = np.maximum(r.max_in_flight, np.where(act, nissued - completed, 0))
        safe = np.where(act, before_prev, safe)
        bad_t = sample_unsafe(j & 3, y0 + j)
        # locate and read the taps of the next row
        y = np.minimum(y0 + j + 1, y1 - 1)
        ix, iy = row_coords(y)
        i0, i1 = iy[:, 0], iy[:, 63]
        ilo, ihi = np.minimum(i0, i1), np.maximum(i0, i1)
        bad, outside = taps_unsafe(ix, iy)
        v = ((safe - (ihi + 2)) < 0) | ((ilo - 1 + LK - 1 - loaded) < 0)
        r.first_violation = np.where(act & v & ~violated, j, r.first_violation)
        violated |= act & v
        r.unflagged |= act & (bad | bad_t) & ~violated
        r.tap_outside_slot |= act & outside
        r.guard_rows &= ~act | ((iy >= ilo[:, None] - 1) & (iy <= ihi[:, None] + 1)).all(axis=1)
        r.guard_cols &= ~act | ((ix >= xb[:, None]) & (ix + 1 <= xb[:, None] + c.LWP - 1)).all(axis=1)
        before_prev = np.where(act, loaded, before_prev)
        issued = np.where(act, 0, issued)
        dma_row(act & (loaded < ihi + lookahead))
        dma_row(act & (loaded < ihi + lookahead))
        dma_templ(act, (j + 3) & 3)
        prev_issued = np.where(act, issued, prev_issued)
    # last: only the previous step's transfers may be in flight
    k = keep_in_flight(prev_issued, relaxed_last)
    r.last_keep = k
    r.last_prev_issued = prev_issued.copy()
    completed = np.maximum(completed, nissued - k)
    r.unflagged |= sample_unsafe(n_steps & 3, y1 - 1) & ~violated
    r.violated = violated
    r.xb, r.col, r.y0, r.y1 = xb, col, y0, y1
    # global byte ranges: frame-0 rows in `ref` (LROW bytes from column xb of the interleaved plane), template rows (256 bytes)
    r.ref_lo = 4 * (p.base["igg"] + 3 * (r.row_min * p.ref_stride + xb))
    r.ref_hi = 4 * (p.base["igg"] + 3 * (r.row_max * p.ref_stride + xb)) + LROW
    r.templ_hi = 4 * (frame * p.templ_plane_stride + r.trow_max * p.templ_row_stride + col * 64) + 256
    r.templ_lo = 4 * (frame * p.templ_plane_stride + y0 * p.templ_row_stride + col * 64)
    return r


def ring_slack(p, r):
    """Least slack of each reserve over the strips of one simulation (None without ring strips): rows and columns of the
    zero border left untouched, bytes of the tail behind the planes and rows / bytes of the tail behind the templates.
    Negative = outside."""
    c = constants()
    if r.n == 0:
        return None
    first, per = p.planes["igg"]
    plane_end = 4 * (first + per * p.ref_plane_floats)
    return dict(
        border_rows_top=int((r.row_min + c.REF_PAD).min()),
        border_rows_bottom=int((p.h + c.REF_PAD - 1 - r.row_max).min()),
        border_cols_left=int((r.xb + c.REF_PAD).min()),
        # a slot is LROW bytes = 85 1/3 pixels: its last byte against the end of the padded row
        border_cols_right=int(np.floor((p.ref_stride - c.REF_PAD - (r.xb + c.LROW / 12.0))).min()),
        plane_start_bytes=int((r.ref_lo - 4 * first).min()),
        ref_tail_bytes=int((p.ref_bytes - r.ref_hi).min()),
        ref_tail_used=int(max(0, (r.ref_hi - plane_end).max())),
        templ_tail_rows=int((p.h - 1 + c.TEMPL_TAIL_ROWS - r.trow_max).min()),
        templ_tail_bytes=int((p.templ_bytes - r.templ_hi).min()),
        templ_start_bytes=int(r.templ_lo.min()),
    )


# ---- the gather routes and the first-iteration route ----------------------------------------------------------------------
def gather_ranges(p, s, cl, m, arith=("fma", "rn")):
    """Byte ranges of the gather loop's loads, every strip by the route it would take without the ring: least distance of
    any load from the ends of its plane (I: 8 bytes at bo and bo1; gxy: 16 bytes at 2 bo and 2 bo1), for the masked and the
    unmasked route, and of the template sample from the ends of the template."""
    sx_all, sy_all = image_coords(p, m, arith)
    fast_px = np.zeros(sx_all.shape, bool)
    for k in range(s.n):
        fast_px[s.y0[k]:s.y1[k], s.col[k] * 64:s.col[k] * 64 + 64] = cl.fast[k]
    rs, corner, rpf = p.ref_stride, p.corner, p.ref_plane_floats
    out = {}
    with np.errstate(invalid="ignore"):
        flx, fly = np.floor(sx_all), np.floor(sy_all)
    for route, sel in (("masked", ~fast_px), ("unmasked", fast_px)):
        if not sel.any():
            out[route] = None
            continue
        fx, fy = flx[sel], fly[sel]
        if route == "masked":           # v_med3_f32(fl, -2, size): NaN -> -2
            fx = np.where(np.isnan(fx), F(-2), np.clip(fx, F(-2), F(p.w)))
            fy = np.where(np.isnan(fy), F(-2), np.clip(fy, F(-2), F(p.h)))
        assert np.isfinite(fx).all() and np.isfinite(fy).all(), "the unmasked route met a non-finite coordinate"
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        assert (np.abs(iy) < 1 << 23).all() and rs < 1 << 23                         # __mul24
        bo = (iy * rs + ix + corner) << 2
        bo1 = bo + (rs << 2)
        assert (bo >= 0).all() and (2 * bo1 + 16 < 1 << 32).all()                     # 32-bit unsigned offsets
        out[route] = dict(
            I_lo=int(bo.min()), I_hi=int(4 * rpf - (bo1.max() + 8)),
            gxy_lo=int(2 * bo.min()), gxy_hi=int(8 * rpf - (2 * bo1.max() + 16)),
            ix=(int(ix.min()), int(ix.max())), iy=(int(iy.min()), int(iy.max())))
    # template sample: row min(y, y1 - 1) (the repeat past the strip end), pixel min(x, tw - 1), 4 bytes
    yc = np.minimum(np.maximum(s.y1 + 1, s.y1), s.y1 - 1)                            # issue(y + 2) of the last row
    xc = np.minimum(s.col * 64 + 63, p.w - 1)
    hi = 4 * (yc * p.templ_row_stride + xc) + 4
    out["templ"] = dict(lo=0, hi=int((p.templ_plane_stride * 4 - hi).min()))
    return out


def first_iter_ranges(p, s, rows_per_batch=8):
    """The loads of ecc_first_iter_body, batch by batch: (rows touched, least distance from the end of the template plane
    and of the igg plane). A lane reads 4 bytes of T and 12 bytes of the interleaved plane at pixel min(x, tw - 1)."""
    R = rows_per_batch
    worst_t, worst_g, rows = 1 << 60, 1 << 60, 0
    first, per = p.planes["igg"]
    for k in range(s.n):
        y0, y1 = int(s.y0[k]), int(s.y1[k])
        touched = []
        y = y0
        n_full = (y1 - y0) // R
        if n_full > 0:
            touched.append((y, y + R))
            gi = 0
            while gi + 2 <= n_full:
                touched.append((y + R, y + 2 * R))
                if gi + 2 < n_full:
                    touched.append((y + 2 * R, y + 3 * R))
                y += 2 * R
                gi += 2
            if gi < n_full:
                y += R
        touched.append((y, y1))
        top = max(b for _, b in touched) - 1
        assert min(a for a, _ in touched) >= y0 and top <= y1 - 1, (k, touched)
        rows += y1 - y0
        xc = min(int(s.col[k]) * 64 + 63, p.w - 1)
        worst_t = min(worst_t, p.templ_plane_stride * 4 - (4 * (top * p.templ_row_stride + xc) + 4))
        worst_g = min(worst_g, 4 * per * p.ref_plane_floats - (4 * (p.base["igg"] - first + 3 * (top * p.ref_stride + xc)) + 12))
    return dict(rows=rows, templ_hi=worst_t, igg_hi=worst_g)


# ---- ecc_run ----------------------------------------------------------------------------------------------------------
def is_identity(m):
    return np.array_equal(np.asarray(m, F).view(np.uint32), np.eye(3, dtype=F).reshape(9).view(np.uint32))


def launches(m, motion="homography", first_iter=1, depth=8):
    """The effective column-pass launches of a one-iteration call from the start m: [(warp, route)]. A start at the identity
    (homography, 8- or 16-bit images, option ecc_first_iter) first runs the general route at the identity on a scratch slot,
    then the frame itself takes the first-iteration route, which has no ring."""
    m = np.asarray(m, F)
    if first_iter and motion == "homography" and depth != 32 and is_identity(m):
        return [(np.eye(3, dtype=F).reshape(9), "general"), (m, "first_iter")]
    return [(m, "general")]


def expected_counters(w, h, start, motion="homography", lookahead=None, ecc_blocks=0, first_iter=1, ring=1, arith=("fma", "rn")):
    """(ecc_ring_fallbacks, ecc_first_iter_slots, ring strips) of stk_find_transform_ecc with max_count = 1."""
    c = constants()
    la = c.LOOKAHEAD if lookahead is None else lookahead
    p = plan(w, h, 1, ecc_blocks)
    s = strips(p)
    fallbacks = first_slots = ring_strips = 0
    for m, route in launches(warp9(start, motion), motion, first_iter):
        if route == "first_iter":
            first_slots += 1
            continue
        cl = classify(p, s, m, ring, arith)
        r = simulate_ring(p, s, cl, m, la, arith)
        fallbacks += int(r.violated.sum())
        ring_strips += r.n
    return fallbacks, first_slots, ring_strips


def end_lane_rows(p, s, cl, m, arith):
    """Row indices of lanes 0 and 63 at every row of every ringable strip (what the loader's scalars are made of)."""
    sx_all, sy_all = image_coords(p, m, arith)
    out = []
    for k in np.flatnonzero(cl.ringable):
        xs = s.col[k] * 64
        out.append(floor_int(sy_all[s.y0[k]:s.y1[k], [xs, xs + 63]]))
    return out


# ---- warp classes of the CPU sweep (template pixel -> frame-0 pixel) -------------------------------------------------------
def _affine(a=1.0, b=0.0, tx=0.0, c=0.0, d=1.0, ty=0.0):
    return np.array([[a, b, tx], [c, d, ty], [0, 0, 1.0]])


def window_warp(target):
    """A column scale under which the strips of column 1 (x = 64 .. 127) have floor(sxmax) + 3 - xb == target: their
    source columns run from 64.5 (xb = 60) to target + 57.5."""
    a = (target - 7) / 63.0
    return _affine(a=a, tx=64.5 - 64 * a, ty=0.3)


def rate_warp(p, rate):
    """Source row rising by `rate` per template row, centred (rows past the frame make their strips leave the fast class)."""
    return _affine(d=rate, ty=(p.h - 1) * (1 - rate) / 2 + 0.25, tx=0.4)


def warp_classes(p, heavy=True):
    """name -> 3 x 3 start for the geometry of plan p. `heavy` = False: the representative subset used at the BASELINE sizes."""
    from libstacker_rs_amd import synth
    w, h = p.w, p.h
    out = {"identity": np.eye(3), "shift30": _affine(tx=30.3, ty=29.6)}
    for r in (0.6, 1.4):
        out["rate%.2f" % r] = rate_warp(p, r)
    out["spread+0.9"] = _affine(c=0.899 / 63, ty=0.5, tx=0.5)
    out["gen12"] = synth.random_homography(np.random.Generator(np.random.PCG64(synth.SEED + 2)), w, h, 12.0)
    # perspective whose local row rate leaves what the corners of a strip show: the rate is d / W^2 with W falling along y
    # (-a: strips that pass the corner test and fail the run-time check at the production lookahead)
    for name, a, d, q in (("local-rate-a", 0.8, 0.90, 0.50), ("local-rate-b", 0.8, 0.90, 0.20), ("local-rate-c", 1.0, 0.75, -0.30)):
        out[name] = np.array([[a, 0, 0.4], [0, d, 0.3], [0, -q / h, 1.0]])
    out["border-tl"] = _affine(tx=0.06, ty=0.06)
    out["border-br"] = _affine(tx=-0.06, ty=-0.06)
    if not heavy:
        return out
    out["subpixel"] = _affine(tx=0.37, ty=0.61)
    out["shift-30"] = _affine(tx=-30.3, ty=-29.6)
    for r in (0.7, 1.0, 1.3, 0.59, 1.41):
        out["rate%.2f" % r] = rate_warp(p, r)
    for t in (84, 85, 86):
        out["window%d" % t] = window_warp(t)
    out["spread-0.9"] = _affine(c=-0.899 / 63, ty=h * 0.02 + 1.5, tx=0.5)
    out["spread+0.91"] = _affine(c=0.91 / 63, ty=0.5, tx=0.5)
    for k, st in enumerate((1.0, 4.0)):
        out["gen%d" % st] = synth.random_homography(np.random.Generator(np.random.PCG64(synth.SEED + 3 + k)), w, h, st)
    out["local-rate-x"] = np.array([[1, 0, 0.4], [0.004, 1.25, 0.3], [-0.1 / w, -0.15 / h, 1.0]])
    out["border-2.5"] = _affine(tx=2.5, ty=-2.5)
    return out


# ---- the GPU case table (test_gpu_ecc_ring.py; its conditions are asserted on the CPU by test_cpu_ecc_ring.py) ----------------
A, B = (200, 449), (97, 191)          # (h, w) of SHAPES in test_cpu_ecc_iteration.py: the smallest with strips of 8 rows or more
# name, (h, w), motion, ecc_blocks (0 = from the plan), start, what the case is there for
GPU_TABLE = [
    ("identity", A, "homography", 8, np.eye(3), "first-iteration route: the scratch launch's strips are the ones counted"),
    ("shift30", A, "homography", 8, _affine(tx=30.3, ty=29.6), "plain"),
    ("subpixel-plan-nb", A, "homography", 0, _affine(tx=0.37, ty=0.61), "nb from the plan: strips of 8 and 9 rows"),
    ("rate0.7", A, "homography", 8, _affine(d=0.7, ty=30.25, tx=0.4), "fall-backs stop at lookahead 4"),
    ("rate1.3", A, "homography", 8, _affine(d=1.3, ty=-29.75, tx=0.4), "fall-backs stop only at lookahead 5"),
    ("rotation", B, "homography", 8, _affine(c=0.5 / 63, b=-0.5 / 63, tx=1.3, ty=0.4), "lanes half a row apart"),
    ("affine-shear", A, "affine", 8, _affine(a=1.05, b=0.02, tx=-8.6, c=0.004, d=0.9, ty=9.3), "the affine kernel"),
    ("translation", B, "translation", 8, _affine(tx=2.3, ty=1.7), "the translation kernel"),
    ("persp-local-rate", A, "homography", 8, np.array([[0.86, 0, 0.4], [0, 0.85, 3.0], [0, -0.14 / 200, 1.0]]),
     "the row rate 0.85 / W^2 crosses 1 down the frame: at lookahead 4 the lower strips fall back, the upper ones do not"),
    ("persp-gentle", B, "homography", 8, np.array([[1.01, 0.002, 0.7], [-0.003, 0.98, 1.9], [2e-5, -3e-5, 1.0]]), "perspective, every strip in the ring"),
    ("zero-window", A, "homography", 8, _affine(a=1.4, tx=-80.2, ty=0.3), "no ring strip: window too wide"),
    ("zero-spread", A, "homography", 8, _affine(c=1.2 / 63, tx=0.5, ty=0.5), "no ring strip: lane spread"),
    ("zero-rate", A, "homography", 8, _affine(d=1.6, ty=-59.75, tx=0.4), "no ring strip: rate"),
    ("zero-border", B, "homography", 8, _affine(tx=130.3, ty=0.2), "no ring strip: every strip touches the right border"),
]
ZERO_REASON = {"zero-window": 1, "zero-spread": 2, "zero-rate": 4}


def table_case(name):
    return next(c for c in GPU_TABLE if c[0] == name)


def case_start(case):
    """The start as the caller passes it: 3 x 3 f32 for the homography, 2 x 3 otherwise."""
    m = np.asarray(case[4], np.float64).astype(F)
    return m if case[2] == "homography" else m[:2]


def case_model(case, lookahead, first_iter=1, arith=("fma", "rn")):
    name, (h, w), motion, blocks, start, _ = case
    return expected_counters(w, h, case_start(case), motion, lookahead, blocks, first_iter, 1, arith)


def sample_template(inp, m):
    """The template that the start m aligns exactly: inp sampled bilinearly (f64, zero outside) at m's coordinates, u8."""
    h, w = inp.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    m = np.asarray(m, np.float64)
    W = m[2, 0] * x + m[2, 1] * y + m[2, 2]
    X, Y = (m[0, 0] * x + m[0, 1] * y + m[0, 2]) / W, (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / W
    ix, iy = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    ax, ay = X - ix, Y - iy
    src = np.pad(inp.astype(np.float64), 1)

    def at(xx, yy):
        return src[np.clip(yy + 1, 0, h + 1), np.clip(xx + 1, 0, w + 1)]
    v = (at(ix, iy) * (1 - ax) + at(ix + 1, iy) * ax) * (1 - ay) + (at(ix, iy + 1) * (1 - ax) + at(ix + 1, iy + 1) * ax) * ay
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)

"""The LDS-ring loader of the column-walking ECC pass against its restatement (ecc_ring_restate.py), on the CPU: every
global range a transfer or a tap load touches lies inside what ecc_plan reserves, every LDS range inside the wave's ring,
every tap and template sample is read after its transfer has landed and before anything overwrites it — or the kernel's
own run-time check has fired by then — and the case table of test_gpu_ecc_ring.py meets the conditions that make its
counter comparison mean something. No GPU, no pixel values: addresses and order only."""
import numpy as np
import pytest

import ecc_ring_restate as R
from test_cpu_ecc_iteration import SHAPES

C = R.constants()
LOOKAHEADS = (1, 2, 3, 4, 5)
# (h, w), heavy: the BASELINE sizes take the representative classes, everything else every class
GEOMETRIES = [((2160, 3840), False), ((1080, 1920), False)] + [(hw, True) for hw, _ in SHAPES] + \
             [((64, 193), True), ((64, 194), True), ((64, 195), True),            # widths 1, 2, 3 (mod 4)
              ((8, 2049), True), ((9, 2049), True), ((15, 1025), True), ((16, 1025), True)]   # a strip of 8 rows is a whole column / just fits
SLACK = {}            # reserve -> (least slack, where)
RING_STRIPS = {}      # geometry -> ring strips simulated


def _note_slack(where, sl):
    for k, v in sl.items():
        if k == "ref_tail_used":                     # (not a slack: the most of the tail any transfer used)
            k, v = "ref_tail_unused", C.REF_TAIL - v
        if k not in SLACK or v < SLACK[k][0]:
            SLACK[k] = (v, where)


def test_constants_come_from_the_sources():
    assert C.LTOFF == (C.LK + 1) * C.LROW and C.LWAVE == C.LTOFF + C.LT * 256
    assert C.LK & (C.LK - 1) == 0 and 1 <= C.LOOKAHEAD <= 5
    assert 12 * (C.LWP - 1) + 12 <= C.LROW < 12 * (C.LWP + 1), "LWP is the number of whole pixels in a slot"
    assert C.REF_PAD >= 2 and C.REF_PAD % 4 == 0
    with pytest.raises(AssertionError):
        R._one("common.h", r"constexpr int NO_SUCH_CONSTANT = (\d+);")


@pytest.mark.parametrize("hw", [g for g, _ in GEOMETRIES], ids=lambda g: "%dx%d" % g)
def test_plan_and_partition(hw):
    h, w = hw
    for blocks in (0, 8):
        p = R.plan(w, h, 1, blocks)
        assert p.nb % 8 == 0 and p.nb >= 8 and (blocks == 0 or p.nb == 8)
        assert p.templ_row_stride % 4 == 0 and 0 <= p.templ_row_stride - w < 4
        assert p.ref_stride % 4 == 0 and 0 <= p.ref_stride - (w + 2 * C.REF_PAD) < 4
        assert p.ref_plane_floats == p.ref_stride * (h + 2 * C.REF_PAD)
        # the five planes tile the buffer in order, the tail behind them
        end = 0
        for name in ("I", "gx", "gy", "gxy", "igg"):
            first, per = p.planes[name]
            assert first == end and p.base[name] == first + per * (C.REF_PAD * p.ref_stride + C.REF_PAD)
            end = first + per * p.ref_plane_floats
        assert p.ref_bytes == 4 * end + C.REF_TAIL
        assert p.templ_bytes == 4 * p.templ_row_stride * (h + C.TEMPL_TAIL_ROWS) + C.TEMPL_TAIL
        s = R.strips(p)
        ncol = (w + 63) // 64
        assert p.units_q * p.nb * 4 + p.units_r == ncol * h and 0 <= p.units_r < p.nb * 4
        # the strips are the (column, row) units in column-major order, each exactly once; a wave's run is contiguous
        u = s.col * h + s.y0
        assert (s.y1 > s.y0).all() and (s.y1 <= h).all() and (s.col < ncol).all()
        assert u[0] == 0 and (u[1:] == (u + s.y1 - s.y0)[:-1]).all() and (u + s.y1 - s.y0)[-1] == ncol * h
        assert (np.diff(s.wave) >= 0).all() and s.wave.max() < 4 * p.nb
        per_wave = np.bincount(s.wave, weights=s.y1 - s.y0, minlength=4 * p.nb)
        assert set(per_wave) <= {p.units_q, p.units_q + 1} and (per_wave == p.units_q + 1).sum() == p.units_r
    if hw == (2160, 3840):
        assert R.plan(w, h, 63).nb == 288 and R.plan(w, h, 255).n_slots == 85 and R.plan(w, h, 63, 8).nb == 8
    if hw == (1080, 1920):
        assert R.plan(w, h, 64).nb == 72 and R.plan(w, h, 64).n_slots == 64


def _affine_start(m):
    return tuple(np.asarray(m, np.float64)[2]) == (0.0, 0.0, 1.0)


@pytest.mark.parametrize("hw,heavy", GEOMETRIES, ids=lambda g: "%dx%d" % g if isinstance(g, tuple) else "")
def test_ring_ranges_and_order(hw, heavy):
    """Assertions a to d of the loader, every warp class, nb from the plan and ecc_blocks = 8, lookahead 1 .. 5."""
    h, w = hw
    n_ring, possible = 0, False
    for blocks in (0, 8):
        p = R.plan(w, h, 1, blocks)
        s = R.strips(p)
        possible |= bool(((s.y1 - s.y0 >= C.MIN_ROWS) & (s.col * 64 + 63 < w)).any())
        for name, start in R.warp_classes(p, heavy).items():
            m = R.warp9(start)
            cl = R.classify(p, s, m)
            assert not (cl.ringable & ~cl.fast).any()
            for la in LOOKAHEADS:
                where = "%dx%d nb %d %s lookahead %d" % (h, w, p.nb, name, la)
                r = R.simulate_ring(p, s, cl, m, la)
                if r.n == 0:
                    continue
                n_ring += r.n if la == C.LOOKAHEAD else 0
                # a. global ranges
                sl = R.ring_slack(p, r)
                _note_slack(where, sl)
                for key in ("border_rows_top", "border_rows_bottom", "border_cols_left", "plane_start_bytes", "ref_tail_bytes",
                            "templ_tail_rows", "templ_tail_bytes", "templ_start_bytes"):
                    assert sl[key] >= 0, (where, key, sl)
                assert sl["ref_tail_used"] <= C.REF_TAIL, (where, sl)
                # b. LDS ranges
                assert r.lds_inside.all() and r.slot_is_row_and_7.all() and not r.tap_outside_slot.any(), where
                assert (r.max_in_flight <= 4 + C.RELAXED).all(), where
                # c. landed and not overwritten, or the run-time check has fired by then
                assert not r.unflagged.any(), (where, np.flatnonzero(r.unflagged)[:4], r.col[r.unflagged][:4], r.y0[r.unflagged][:4])
                # the guard of one row / one pixel that the kernel's comment claims
                assert r.guard_rows.all() and r.guard_cols.all(), (where, np.flatnonzero(~(r.guard_rows & r.guard_cols))[:4])
                # the strict wait of `last`: only the previous step's transfers may be in flight
                assert (r.last_keep == np.maximum(1, np.minimum(r.last_prev_issued, 4))).all(), where
                # at lookahead 1 the check fires on every ring strip, at its first step
                if la == 1:
                    assert r.violated.all() and (r.first_violation == 0).all(), where
                # d. an admissible affine warp never falls back at the production lookahead
                if la == C.LOOKAHEAD and _affine_start(start):
                    assert not r.violated.any(), (where, int(r.violated.sum()))
    RING_STRIPS[hw] = n_ring
    if possible:                                         # (a whole column in at least 8 rows of one wave)
        assert n_ring > 0, "no class put a strip of %dx%d into the ring: the geometry checks nothing" % hw


def test_classes_reach_what_they_are_named_for():
    p = R.plan(449, 200, 1, 8)
    s = R.strips(p)
    cls = R.warp_classes(p)
    why = {n: R.classify(p, s, R.warp9(m)) for n, m in cls.items()}
    col1 = s.col == 1
    for t in (84, 85, 86):                               # the window of LWP - 1, LWP and LWP + 1 pixels, on the strips of column 1
        cl = why["window%d" % t]
        assert t - 85 == t - C.LWP and cl.fast[col1].sum() >= 2 and (cl.window[col1 & cl.fast] == t).all()
        assert cl.ringable[col1 & cl.fast].all() == (t <= C.LWP - 1) and cl.ringable[col1 & cl.fast].any() == (t <= C.LWP - 1)
    assert why["rate0.59"].ringable.sum() == 0 and why["rate1.41"].ringable.sum() == 0 and why["spread+0.91"].ringable.sum() == 0
    for n in ("rate0.70", "rate1.00", "rate1.30", "spread+0.9", "spread-0.9", "gen1", "gen4", "border-tl", "border-br"):
        assert why[n].ringable.sum() >= 8, n
    # the perspective classes: strips that pass the corner test and still fail the run-time check at the production lookahead
    # or below it, beside strips that pass both
    mixed = 0
    for n in ("local-rate-a", "local-rate-b", "local-rate-c", "local-rate-x"):
        for la in LOOKAHEADS:
            r = R.simulate_ring(p, s, why[n], R.warp9(cls[n]), la)
            mixed += bool(r.n and r.violated.any() and not r.violated.all())
    assert mixed > 0
    r = R.simulate_ring(p, s, why["local-rate-a"], R.warp9(cls["local-rate-a"]), C.LOOKAHEAD)
    assert r.violated.any() and not r.violated.all() and not r.unflagged.any()     # what the run-time check exists for
    # the border classes reach the zero border: rows above / below the image, columns left of it
    r = R.simulate_ring(p, s, why["border-tl"], R.warp9(cls["border-tl"]), C.LOOKAHEAD)
    assert r.row_min.min() < 0 and r.xb.min() < 0
    r = R.simulate_ring(p, s, why["border-br"], R.warp9(cls["border-br"]), C.LOOKAHEAD)
    assert r.row_max.max() >= p.h and r.trow_max.max() >= p.h


@pytest.mark.parametrize("hw,heavy", GEOMETRIES, ids=lambda g: "%dx%d" % g if isinstance(g, tuple) else "")
def test_gather_and_first_iteration_addresses(hw, heavy):
    """The routes without the ring: the masked gather (clamped into [-2, iw] x [-2, ih]: two pixels of the border), the
    unmasked gather (no clamp: the corner test must keep it inside the image), the template sample and the
    first-iteration route's batched loads."""
    h, w = hw
    for blocks in (0, 8):
        p = R.plan(w, h, 1, blocks)
        s = R.strips(p)
        f = R.first_iter_ranges(p, s)
        assert f["rows"] == ((w + 63) // 64) * h and f["templ_hi"] >= 0 and f["igg_hi"] >= 0
        if blocks == 0 and not heavy:
            continue                                   # (the gather addresses do not depend on the partition's size class)
        for name, start in R.warp_classes(p, heavy).items():
            m = R.warp9(start)
            cl = R.classify(p, s, m)
            g = R.gather_ranges(p, s, cl, m)
            where = "%dx%d nb %d %s" % (h, w, p.nb, name)
            assert g["templ"]["hi"] >= 0
            for route in ("masked", "unmasked"):
                if g[route] is None:
                    continue
                assert min(g[route][k] for k in ("I_lo", "I_hi", "gxy_lo", "gxy_hi")) >= 0, (where, route, g[route])
                _note_slack(where, {"gather_" + route + "_bytes": min(g[route][k] for k in ("I_lo", "I_hi", "gxy_lo", "gxy_hi"))})
            if g["masked"]:
                assert g["masked"]["ix"][0] >= -2 and g["masked"]["ix"][1] <= w and g["masked"]["iy"][0] >= -2 and g["masked"]["iy"][1] <= h
            if g["unmasked"]:                          # 2 x 2 taps inside the image itself
                assert g["unmasked"]["ix"][0] >= 0 and g["unmasked"]["ix"][1] <= w - 2, (where, g["unmasked"])
                assert g["unmasked"]["iy"][0] >= 0 and g["unmasked"]["iy"][1] <= h - 2, (where, g["unmasked"])


def test_scratch_launch_of_an_identity_start_is_counted():
    h, w = R.A
    eye = np.eye(3, dtype=np.float32)
    for la in LOOKAHEADS:
        with_route = R.expected_counters(w, h, eye, "homography", la, 8, first_iter=1)
        without = R.expected_counters(w, h, eye, "homography", la, 8, first_iter=0)
        assert with_route[1] == 1 and without[1] == 0 and with_route[0] == without[0] and with_route[2] == without[2] > 0
    assert len(R.launches(R.warp9(eye[:2], "affine"), "affine")) == 1
    off = eye.copy()
    off[0, 2] = np.float32(1e-30)
    assert len(R.launches(R.warp9(off))) == 1 and len(R.launches(R.warp9(eye), depth=32)) == 1
    neg = eye.copy()
    neg[0, 1] = np.float32(-0.0)                        # the comparison is bitwise
    assert len(R.launches(R.warp9(neg))) == 1


# ---- e. the GPU table is not vacuous ----------------------------------------------------------------------------------------
ARITH = [(f, r) for f in ("fma", "muladd") for r in ("rn", "up", "down")]


def _table_counts(case):
    return [R.case_model(case, la) for la in LOOKAHEADS]


def test_gpu_table_conditions():
    names = [c[0] for c in R.GPU_TABLE]
    assert len(names) == len(set(names)) and 12 <= len(names) <= 16
    assert {c[1] for c in R.GPU_TABLE} == {R.A, R.B} and {R.A, R.B} <= {hw for hw, _ in SHAPES}
    assert sum(c[3] == 0 for c in R.GPU_TABLE) == 1 and all(c[3] in (0, 8) for c in R.GPU_TABLE)
    assert {c[2] for c in R.GPU_TABLE} == {"homography", "affine", "translation"}
    assert sum(c[2] == "affine" for c in R.GPU_TABLE) == 1 and sum(c[2] == "translation" for c in R.GPU_TABLE) == 1
    persp = [c for c in R.GPU_TABLE if tuple(np.asarray(c[4], np.float64)[2]) != (0.0, 0.0, 1.0)]
    assert 1 <= len(persp) <= 4
    counts = {c[0]: _table_counts(c) for c in R.GPU_TABLE}
    stops_at = {}
    for case in R.GPU_TABLE:
        name = case[0]
        fb = [k[0] for k in counts[name]]
        ring = counts[name][0][2]
        assert all(k[2] == ring for k in counts[name])
        if name.startswith("zero-"):
            assert ring == 0 and fb == [0] * 5, name
            continue
        assert ring >= 8, (name, ring)
        assert fb[0] == ring and fb[-1] == 0 and all(a >= b for a, b in zip(fb, fb[1:])), (name, fb)
        stops_at[name] = 1 + max(k for k in range(5) if fb[k] > 0) + 1
    assert 4 in stops_at.values() and 5 in stops_at.values()
    assert any(0 < k[0] < k[2] for c in persp for k in counts[c[0]]), "no perspective case with a partial fall-back"
    assert counts["identity"][0][1] == 1 and all(counts[n][0][1] == 0 for n in names if n != "identity")
    # the four empty cases are empty for the reason they name, and for that reason alone
    for case in R.GPU_TABLE:
        name, (h, w), motion, blocks = case[:4]
        if not name.startswith("zero-"):
            continue
        p = R.plan(w, h, 1, blocks)
        s = R.strips(p)
        cl = R.classify(p, s, R.warp9(R.case_start(case), motion))
        long_fast = cl.fast & (s.y1 - s.y0 >= C.MIN_ROWS)
        if name == "zero-border":
            assert not cl.fast.any() and ((s.y1 - s.y0 >= C.MIN_ROWS) & (s.col * 64 + 63 < w)).sum() >= 8
        else:
            assert long_fast.sum() >= 8 and (cl.why[long_fast] == R.ZERO_REASON[name]).all(), (name, np.bincount(cl.why[long_fast]))


@pytest.mark.parametrize("name", [c[0] for c in R.GPU_TABLE])
def test_gpu_table_case_is_unambiguous(name):
    """v_rcp_f32 is accurate to one ulp, not bit-specified, and the model's fma rounds twice: every classification, every
    row index of lanes 0 and 63 and every count must be the same under all six readings."""
    case = R.table_case(name)
    _, (h, w), motion, blocks = case[:4]
    p = R.plan(w, h, 1, blocks)
    s = R.strips(p)
    ref = None
    for m, route in R.launches(R.warp9(R.case_start(case), motion), motion):
        if route != "general":
            continue
        for arith in ARITH:
            cl = R.classify(p, s, m, 1, arith)
            rows = R.end_lane_rows(p, s, cl, m, arith)
            got = (cl.fast.copy(), cl.ringable.copy(), np.where(cl.ringable, cl.xb, 0), rows,
                   [R.expected_counters(w, h, R.case_start(case), motion, la, blocks, 1, 1, arith) for la in LOOKAHEADS])
            if ref is None:
                ref = got
                continue
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), (name, arith)
            assert len(got[3]) == len(ref[3]) and all(np.array_equal(a, b) for a, b in zip(got[3], ref[3])), (name, arith)
            assert got[4] == ref[4], (name, arith)


def test_gpu_table_iterations_are_well_posed():
    """One iteration from each start on the images the GPU test uses ends without an error on the CPU oracle."""
    import oracle
    from test_cpu_ecc_iteration import scene
    omotion = {"homography": oracle.MOTION_HOMOGRAPHY, "affine": oracle.MOTION_AFFINE, "translation": oracle.MOTION_TRANSLATION}
    for case in R.GPU_TABLE:
        name, (h, w), motion = case[:3]
        inp = scene(h, w)
        templ = R.sample_template(inp, case[4])
        rc, Wo, rho, its = oracle.find_transform_ecc(templ, inp, R.case_start(case), omotion[motion], 1, None, 5)
        assert rc == 0 and its == 1 and rho > 0.5, (name, rc, its, rho)


def test_print_the_slack_table():
    """Least slack of every reserve over everything the sweeps above simulated (run with -s to see it; DESIGN.md keeps a copy)."""
    if not SLACK:                                        # (run on its own: the smallest geometry with ring strips)
        test_ring_ranges_and_order(R.A, True)
    print("\nreserve / least slack / where")
    for k in sorted(SLACK):
        print("  %-24s %10d   %s" % (k, SLACK[k][0], SLACK[k][1]))
    print("  border rows reached: top %d, bottom %d of %d; columns left %d of %d; bytes of the %d-byte tail used: %d; template rows past the end: %d of %d"
          % (C.REF_PAD - SLACK["border_rows_top"][0], C.REF_PAD - SLACK["border_rows_bottom"][0], C.REF_PAD,
             C.REF_PAD - SLACK["border_cols_left"][0], C.REF_PAD, C.REF_TAIL, C.REF_TAIL - SLACK["ref_tail_unused"][0],
             C.TEMPL_TAIL_ROWS - SLACK["templ_tail_rows"][0], C.TEMPL_TAIL_ROWS))
    print("  ring strips simulated at the production lookahead:", {"%dx%d" % k: v for k, v in RING_STRIPS.items()})

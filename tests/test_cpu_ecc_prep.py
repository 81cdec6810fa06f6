"""The ECC preparation suite without a GPU: is the case table of ecc_prep_restate.py worth running, and do the restatements
the GPU tests (test_gpu_ecc_prep.py) compare against say what they should?"""
import numpy as np
import pytest

import oracle
import ecc_prep_restate as R


def test_every_route_is_reached():
    assert {c.route for c in R.CASES} == set(R.ROUTES)
    entries = {(c.entry, c.kind) for c in R.CASES}
    assert {("ecc", "u8c3"), ("hybrid", "u16c3"), ("ecc", "f32c3"), ("ecc", "u8c4"), ("fte", "u8c1"), ("fte", "f32c1")} <= entries
    assert any(c.scale_down_width and c.kind == "u8c3" for c in R.CASES) and any(c.scale_down_width and c.kind == "f32c3" for c in R.CASES)
    assert any(c.layout != "tight" and c.expect == "fallback" for c in R.CASES)
    assert any(c.layout != "tight" and c.expect == "streamed" for c in R.CASES)
    assert {c.upload_batch for c in R.CASES if c.route == "host_fed" and c.n == 6} == {1, 2, 3, 5}
    assert any(c.route == "host_fed" and c.n == 6 and c.expect == "mixed" for c in R.CASES)


def test_the_table_holds_the_sizes_the_kernel_constants_call_for():
    streamed = [c for c in R.CASES if c.route == "stream"]
    widths = {c.w for c in streamed if c.h == 40}
    heights = {c.h for c in streamed if c.w == 252}
    # a last writer lane, a feeder lane or a workgroup boundary on the image edge: one width just below, at and above
    # every multiple of a wave's 248 px and of a workgroup's 992 px that the table reaches
    for unit in (R.WAVE_PX, R.GROUP_PX):
        for m in range(unit, max(widths) + 1, unit):
            assert {m - 4, m, m + 4} <= widths, (unit, m)
    assert {8, 12} <= widths                                 # the narrowest the kernel takes, and one quad more
    assert {R.GS_SEG - 1, R.GS_SEG, R.GS_SEG + 1, 2 * R.GS_SEG - 1, 2 * R.GS_SEG, 2 * R.GS_SEG + 1} <= heights
    assert min(heights) >= 8                                 # (below: the tiled kernel's own reflect loop, test_gpu_stages.py)
    # each size with every kernel size the streaming kernel is instantiated for, in both depths
    for w, h in {(c.w, c.h) for c in streamed}:
        got = {(c.gauss, c.kind) for c in streamed if (c.w, c.h) == (w, h)}
        assert got == {(g, k) for g in R.GAUSS for k in ("u8c3", "u16c3")}, (w, h)
    for c in R.CASES:                                        # tests stay quick
        assert c.n <= 19 and c.w <= 1000 and c.h <= 65


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_route_model_gives_the_intended_count(case):
    count = R.case_route_count(case)
    if case.expect == "streamed":
        assert count == case.n - 1 > 0
    elif case.expect == "fallback":
        assert count == 0
    else:
        assert case.expect == "mixed" and 0 < count < case.n - 1


def test_route_model_cuts():
    m = R.route_model
    # host-fed: frame 0 alone, then batches; a batch of one frame goes frame by frame
    assert R.runs_of("host", 6, 2, 5, 1, False) == [(1, 2), (3, 2), (5, 1)]
    assert [m(252, 33, 8, 3, 756, "host", 6, upload_batch=b) for b in (1, 2, 3, 5, 8)] == [0, 4, 5, 5, 5]
    # device-resident: runs of 16 only beyond 2 x slots moving frames and with the overlap on
    assert R.runs_of("device", 19, 8, 1, 1, False) == [(1, 16), (17, 2)]
    assert R.runs_of("device", 19, 8, 9, 1, False) == [(1, 18)]
    assert R.runs_of("device", 19, 8, 1, 0, False) == [(1, 18)]
    assert R.runs_of("device", 18, 8, 1, 1, False) == [(1, 16), (17, 1)]
    assert m(252, 33, 8, 3, 756, "device", 18, slots=1) == 16            # the last run is one frame: tiled
    assert R.effective_slots(18, 252, 33) == 18 and R.effective_slots(18, 252, 33, 1) == 1 and R.effective_slots(100, 252, 33) == 50
    # every gate of launch_grey_blur_batch / prepare_templates on its own
    ok = dict(w=252, h=33, depth=8, channels=3, row_stride=756, location="device", n=4)
    assert m(**ok) == 3
    for change in (dict(w=250, row_stride=750), dict(w=4, row_stride=12), dict(depth=32, row_stride=3024), dict(channels=4, row_stride=1008),
                   dict(row_stride=757), dict(gauss=9), dict(prep_stream=0), dict(scaled=True), dict(n=2), dict(base_mod4=3),
                   dict(frame_step=756 * 33 + 2), dict(even=False)):
        assert m(**{**ok, **change}) == 0, change
    assert m(**{**ok, "depth": 16, "row_stride": 1512}) == 3 and m(**{**ok, "w": 8, "row_stride": 24}) == 3


def test_gradients_are_the_float64_differences_rounded_once():
    rng = np.random.default_rng(3)
    for shape in ((33, 41), (5, 2), (2, 7), (1, 6), (6, 1)):
        I = (rng.standard_normal(shape) * 300).astype(np.float32)
        gx, gy = R.gradients(I)
        assert gx.dtype == np.float32 and gy.dtype == np.float32
        D = I.astype(np.float64)
        h, w = shape
        xs, ys = np.arange(w), np.arange(h)
        def r101(p, n):
            return np.array([0 if n == 1 else (-q if q < 0 else 2 * n - 2 - q if q >= n else q) for q in p])
        ex = (-0.5 * D[:, r101(xs - 1, w)] + 0.5 * D[:, r101(xs + 1, w)]).astype(np.float32)
        ey = (-0.5 * D[r101(ys - 1, h), :] + 0.5 * D[r101(ys + 1, h), :]).astype(np.float32)
        assert np.array_equal(gx, ex) and np.array_equal(gy, ey), shape
    I = rng.standard_normal((4, 2)).astype(np.float32)       # two pixels wide: both neighbours are the other pixel
    assert np.array_equal(R.gradients(I)[0], np.zeros((4, 2), np.float32))
    ox, oy = oracle.gradients(I)
    assert np.array_equal(R.gradients(I)[0], ox) and np.array_equal(R.gradients(I)[1], oy)


def test_expected_planes_are_what_the_stage_tests_pin():
    frames = R.case_frames("u8c3", 252, 33, 4)
    exp = R.expected_planes(list(frames), 5)
    assert exp["templates"].shape == (3, 33, 252) and exp["I"].shape == (33, 252)
    for i in range(4):
        pinned = oracle.gaussian_blur_f32(oracle.grey(frames[i]), 5)       # test_gpu_stages.py: test_fused_grey_blur_bit_exact
        assert np.array_equal(exp["I"] if i == 0 else exp["templates"][i - 1], pinned)
    assert len({exp["templates"][i].tobytes() for i in range(3)} | {exp["I"].tobytes()}) == 4    # a misplaced template shows
    # BGRA: the grey of the BGR part; one plane: itself; scaled: INTER_AREA between grey and blur
    bgra = R.case_frames("u8c4", 252, 33, 4)
    assert np.array_equal(R.grey_of(bgra[1]), oracle.grey(np.ascontiguousarray(bgra[1][..., :3])))
    g = R.case_frames("u8c1", 252, 33, 2)
    assert np.array_equal(R.expected_planes(list(g), 5)["I"], oracle.gaussian_blur_f32(g[0], 5))
    big = R.case_frames("u8c3", 500, 65, 4)
    ew, eh = oracle.scaled_size(500, 65, 252.0)
    sc = R.expected_planes(list(big), 5, 252.0)
    assert sc["I"].shape == (eh, ew)
    assert np.array_equal(sc["templates"][0], oracle.gaussian_blur_f32(oracle.resize_area_u8(oracle.grey(big[1]), ew, eh), 5))
    # 16-bit: blur of float(grey16), as test_fused_grey_blur_u16_bit_exact pins it
    f16 = R.case_frames("u16c3", 252, 33, 4)
    assert f16.dtype == np.uint16 and int(f16.max()) > 255
    assert np.array_equal(R.expected_planes(list(f16), 5)["I"], oracle.gaussian_blur_f32(oracle.grey(f16[0]).astype(np.float32), 5))


def test_tolerances_follow_the_number_formats():
    assert R.tolerance("u8c3", 7) == (0.0, 0.0) and R.tolerance("u16c3", 5) == (0.0, 0.0) and R.tolerance("u8c4", 3) == (0.0, 0.0)
    assert R.tolerance("u16c3", 7) == (2e-6, 0.0)
    assert R.tolerance("f32c3", 5) == (2e-6, 1e-6) and R.tolerance("f32c1", 5) == (2e-6, 1e-6)
    # the exactness argument, on the worst case: every partial sum of the two passes fits 24 bits
    taps = {3: (0.5, 0.25), 5: (0.375, 0.25, 0.0625), 7: (0.28125, 0.21875, 0.109375, 0.03125)}
    tap_bits = {3: 2, 5: 4, 7: 6}                            # the taps are multiples of 2^-2 / 2^-4 / 2^-6 and sum to 1
    for gauss, t in taps.items():
        scaled = [v * 2 ** tap_bits[gauss] for v in t]
        assert all(s == int(s) for s in scaled) and any(int(s) % 2 for s in scaled)
        assert t[0] + 2 * sum(t[1:]) == 1.0
    for gauss, bits, exact in ((7, 8, True), (5, 8, True), (3, 8, True), (5, 16, True), (3, 16, True), (7, 16, False)):
        assert (bits + 2 * tap_bits[gauss] <= 24) == exact, (gauss, bits)      # integers below 2^bits through two passes
        assert (R.tolerance("u%dc3" % bits, gauss) == (0.0, 0.0)) == exact

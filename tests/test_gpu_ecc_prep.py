"""The planes ECC preparation hands to the iteration kernels, read back after the real entry points (Stacker.ecc_prepared,
the test hook stk_ecc_prepared) and compared, plane by plane, with the oracle's restatement (ecc_prep_restate.py).

Every case runs ecc_match, hybrid_match or find_transform_ecc with one iteration and no epsilon, then checks
  * the route: stk_get_counter "prep_stream_frames" is what route_model reads out of stacker.cpp for the case;
  * templates and I against the oracle, bit for bit wherever every partial sum is representable (tolerance());
  * that the planes do not depend on the route: bit-identical to the same stack, device-resident, prep_stream = 0;
  * gx, gy = the central differences of the returned I, the interleaved copies, and a border that is exactly zero.
A frame whose ECC fails (a sliver that does not correlate) is still a case: the planes are there and are checked."""
import numpy as np
import pytest

import ecc_prep_restate as R
from libstacker_rs_amd import EccMatchParameters, InvalidParams, KeyPointMatchParameters, MotionType, OpenCvError, RANSAC, Stacker

pytestmark = pytest.mark.gpu

KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)


def _params(gauss):
    return EccMatchParameters(MotionType.Homography, 1, None, gauss)


def _run(stacker, entry, frames, gauss, scale_down_width=None):
    """The entry point of a case; only the engine's own ECC failure is let through (the planes exist by then)."""
    try:
        if entry == "ecc":
            stacker.ecc_match(frames, _params(gauss), scale_down_width=scale_down_width)
        elif entry == "hybrid":
            stacker.hybrid_match(frames, KP, _params(gauss))
        else:
            stacker.find_transform_ecc(frames[1], frames[0], np.eye(3), _params(gauss))
    except OpenCvError as e:
        assert str(e).startswith("findTransformECC:"), e
    return stacker.ecc_prepared(), stacker.timing()["prep_stream_frames"]


def _device_frames(case):
    """The case's frames as the call gets them: a contiguous device tensor, host arrays, or a window of a device canvas."""
    import torch
    content = R.case_frames(case.kind, case.w, case.h, case.n)
    if case.entry == "fte":
        return content
    if case.location == "host":
        return list(content)
    if case.layout == "tight":
        return torch.from_numpy(content.copy()).cuda()
    hc, wc, y0, x0 = case.layout
    rng = np.random.default_rng(hc * 1000 + wc)
    canvas = rng.integers(0, np.iinfo(content.dtype).max + 1, (case.n, hc, wc, content.shape[3]), dtype=content.dtype)
    canvas[:, y0:y0 + case.h, x0:x0 + case.w] = content
    canvas = torch.from_numpy(canvas).cuda()
    frames = canvas[:, y0:y0 + case.h, x0:x0 + case.w]
    depth, cn, rs, step, base = R.case_layout(case)          # the layout the model was asked about is the one handed over
    assert not frames.is_contiguous() and frames.stride(1) * frames.element_size() == rs and frames.stride(0) * frames.element_size() == step
    assert frames.data_ptr() % 4 == base
    return frames


_BASELINES = {}


def _baseline(stacker, case):
    """The same stack prepared device-resident (a contiguous tensor) by the per-frame kernels: prep_stream = 0. One per
    (stack, kernel size, entry point), shared by the cases that differ in route only, and never written."""
    key = (case.entry, case.kind, case.w, case.h, case.n, case.gauss, case.scale_down_width)
    if key not in _BASELINES:
        import torch
        content = R.case_frames(case.kind, case.w, case.h, case.n)
        if case.entry == "fte":
            # no stack form of this call: the stage entry point launches the same kernel on the same plane
            planes = {"templates": stacker.gaussian_blur_f32(content[1], case.gauss)[None], "I": stacker.gaussian_blur_f32(content[0], case.gauss)}
        else:
            stacker.set_option("prep_stream", 0)
            try:
                got, count = _run(stacker, case.entry, torch.from_numpy(content.copy()).cuda(), case.gauss, case.scale_down_width)
            finally:
                stacker.set_option("prep_stream", 1)
            assert count == 0
            pad = got["pad"]
            planes = {"templates": got["templates"], "I": got["I"][pad:-pad, pad:-pad]}
        for v in planes.values():
            v.setflags(write=False)
        _BASELINES[key] = planes
    return _BASELINES[key]


def _check_reference_planes(got, h, w, label=""):
    """gx, gy, the interleaved copies and the zero border, all from the planes themselves; returns the interior of I."""
    pad = got["pad"]
    assert pad > 0
    for name, k in (("I", 1), ("gx", 1), ("gy", 1), ("gxy", 2), ("igg", 3)):
        assert got[name].shape == ((h + 2 * pad, w + 2 * pad) if k == 1 else (h + 2 * pad, w + 2 * pad, k)), (label, name)
    inner = (slice(pad, pad + h), slice(pad, pad + w))
    I = got["I"][inner]
    gx, gy = R.gradients(I)
    assert np.array_equal(got["gx"][inner], gx), (label, "gx")
    assert np.array_equal(got["gy"][inner], gy), (label, "gy")
    assert np.array_equal(got["gxy"][inner][..., 0], gx) and np.array_equal(got["gxy"][inner][..., 1], gy), (label, "gxy")
    igg = got["igg"][inner]
    assert np.array_equal(igg[..., 0], I) and np.array_equal(igg[..., 1], gx) and np.array_equal(igg[..., 2], gy), (label, "igg")
    for name in ("I", "gx", "gy", "gxy", "igg"):
        border = got[name].copy()
        border[inner] = 0
        # (bit patterns: -0.0 and NaN are not a zero border either)
        assert not border.view(np.uint32).any(), (label, name, "border", int(np.count_nonzero(border.view(np.uint32))))
    return I


def _check_against_oracle(got_planes, kind, gauss, label):
    rtol, atol = R.tolerance(kind, gauss)
    worst = 0.0
    for name, got, want in got_planes:
        assert got.shape == want.shape and got.dtype == np.float32, (label, name, got.shape, want.shape)
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        if d.max() > 0:
            worst = max(worst, float((d / np.maximum(np.abs(want.astype(np.float64)), 1e-30)).max()))
        if rtol == 0.0 and atol == 0.0:
            assert np.array_equal(got, want), (label, name, "max |d|", float(d.max()), "pixels", int(np.count_nonzero(d)))
        else:
            np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg="%s %s" % (label, name))
    if worst > 0:
        print("%s: engine and oracle differ, largest relative difference %.3e (rtol %g atol %g)" % (label, worst, rtol, atol))


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_prepared_planes(stacker, case):
    frames = _device_frames(case)
    options = {"upload_batch": (case.upload_batch, R.UPLOAD_BATCH_DEFAULT), "ecc_slots": (case.ecc_slots, 0), "prep_overlap": (case.prep_overlap, 1)}
    try:
        for name, (value, _) in options.items():
            if value is not None:
                stacker.set_option(name, value)
        got, count = _run(stacker, case.entry, frames, case.gauss, case.scale_down_width)
    finally:
        for name, (value, default) in options.items():
            if value is not None:
                stacker.set_option(name, default)
    # route: a case that means to test the streaming kernel does not pass on the fall-back, nor the other way round
    assert count == R.case_route_count(case), (count, R.case_route_count(case))
    want = R.case_expected(case.kind, case.w, case.h, case.n, case.gauss, case.scale_down_width)
    eh, ew = want["I"].shape
    n_templates = 1 if case.entry == "fte" else case.n - 1
    assert got["templates"].shape == (n_templates, eh, ew)
    I = _check_reference_planes(got, eh, ew, case.name)
    # route invariance first (bit for bit in every case): a difference here is the route's, whatever the oracle says
    base = _baseline(stacker, case)
    assert np.array_equal(I, base["I"]), (case.name, "I differs from the per-frame route")
    for i in range(n_templates):
        if not np.array_equal(got["templates"][i], base["templates"][i]):
            where = [j for j in range(n_templates) if np.array_equal(got["templates"][i], base["templates"][j])]
            bad = np.argwhere(got["templates"][i] != base["templates"][i])
            raise AssertionError("%s: template %d differs from the per-frame route at %d pixels, first (y, x) = %s, last = %s; equals template %s"
                                 % (case.name, i, len(bad), tuple(bad[0]), tuple(bad[-1]), where or "none"))
    planes = [("I", I, want["I"])] + [("template %d" % i, got["templates"][i], want["templates"][i]) for i in range(n_templates)]
    _check_against_oracle(planes, case.kind, case.gauss, case.name)


def test_hook_needs_a_preparation():
    fresh = Stacker(0)
    try:
        with pytest.raises(InvalidParams):
            fresh.ecc_prepared()
        assert fresh.timing()["prep_stream_frames"] == 0
    finally:
        fresh.close()


def test_border_cache_across_geometries():
    """The zero border of the five frame-0 planes is written once per (buffer, width, height): ref_planes_kernel only writes
    the interior. One context, a sequence of geometries in which the second's border lies where the first's interior was,
    the first returns after it (its border then lies in the second's interior), a row is added, the same geometry comes
    again through find_transform_ecc (a cache hit: nothing is cleared) and a larger frame makes the buffer grow."""
    import torch
    ctx = Stacker(0)
    ref_bytes = lambda w, h, pad: ((w + 2 * pad + 3) & ~3) * (h + 2 * pad) * 8 * 4 + 4096       # ecc_plan's ctx->ref.reserve
    steps = [("ecc", 256, 40), ("ecc", 128, 80), ("ecc", 256, 40), ("ecc", 256, 41), ("fte", 256, 41), ("ecc", 1000, 40)]
    try:
        cap, pad, grew = 0, None, []
        for k, (entry, w, h) in enumerate(steps):
            kind = "u8c3" if entry == "ecc" else "u8c1"
            n = 4 if entry == "ecc" else 2
            content = R.case_frames(kind, w, h, n)
            got, count = _run(ctx, entry, torch.from_numpy(content.copy()).cuda() if entry == "ecc" else content, 5)
            assert count == (n - 1 if entry == "ecc" else 0)
            label = "step %d: %s %dx%d" % (k, entry, w, h)
            I = _check_reference_planes(got, h, w, label)
            want = R.case_expected(kind, w, h, n, 5, None)
            assert np.array_equal(I, want["I"]), label
            assert np.array_equal(got["templates"], want["templates"]), label
            pad = got["pad"]
            need = ref_bytes(w, h, pad)                     # DevBuf::reserve: grows by an eighth, never shrinks
            grew.append(need > cap)
            if need > cap:
                cap = need + (need >> 3)
        assert grew == [True, False, False, False, False, True]               # a reallocation at the end, none in between
        # the second geometry's planes (176 floats a row) lie across the first's (304 a row): border over interior and back
        assert ((128 + 2 * pad + 3) & ~3) != ((256 + 2 * pad + 3) & ~3)
    finally:
        ctx.close()

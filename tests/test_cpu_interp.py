"""The restatement of the bicubic fold (interp_restate.py) on its own: exact weights, f32 against f64, and the quality
inequality the feature exists for."""
import numpy as np

import interp_restate as ir

F = np.float32


def test_weights_at_zero_are_minus_zero_one_zero_minus_zero():
    for dtype in (np.float32, np.float64):
        w = [np.asarray(v) for v in ir.weights(np.zeros(1), dtype)]
        assert [float(v[0]) for v in w] == [0.0, 1.0, 0.0, 0.0]
        assert np.signbit(w[0][0]) and np.signbit(w[3][0]) and not np.signbit(w[2][0])


def test_weights_at_one_half_are_exact():
    for dtype in (np.float32, np.float64):
        w = ir.weights(np.full(1, 0.5), dtype)
        assert [float(np.asarray(v)[0]) * 32 for v in w] == [-3.0, 19.0, 19.0, -3.0]


def test_weights_sum_to_one_and_stay_below_1_375_in_magnitude():
    t = np.linspace(0, 1, 4097)[:-1]
    w = np.stack(ir.weights(t, np.float64))
    assert np.abs(w.sum(axis=0) - 1).max() <= 4 * 2.0 ** -52
    assert np.abs(w).sum(axis=0).max() <= 1.375


def test_f32_path_stays_within_2_pow_minus_19_of_f64():
    """<= 27 roundings of size 2^-24 * 1.375^2 * V per sample: 2^-19 V with room (observed: about 6 * 2^-24 V)."""
    rng = np.random.default_rng(1)
    n = 200_000
    worst = 0.0
    for top, alpha in ((255, 1.0 / 255.0), (65535, 1.0 / 65535.0), (255, 1.0), (None, 1.0)):
        taps = rng.random((n, 4, 4)).astype(F) if top is None else rng.integers(0, top + 1, (n, 4, 4)).astype(F)
        tx, ty = rng.random(n).astype(F), rng.random(n).astype(F)
        a = F(alpha)
        s32 = ir.sample(taps, tx, ty, a, np.float32)
        s64 = ir.sample(taps, tx.astype(np.float64), ty.astype(np.float64), a, np.float64)
        V = np.abs(taps.astype(np.float64)).max(axis=(1, 2)) * float(a)
        assert s32.dtype == np.float32
        err = np.abs(s32.astype(np.float64) - s64) / V
        worst = max(worst, err.max())
        assert err.max() <= 2.0 ** -19
    print("f32 vs f64 restatement: worst", worst / 2.0 ** -24, "x 2^-24 V")


def restated_quality(seed):
    """(rms linear, rms cubic) of the stacked mean against the analytic scene, f64 samples, grey levels."""
    frames, warps, scene = ir.quality_stack(seed)
    n, h, w, _ = frames.shape
    m = np.zeros((h, w), bool)
    m[5:h - 5, 5:w - 5] = True
    lin = np.zeros((h, w))
    cub = np.zeros((h, w))
    for k in range(n):
        inv = ir.invert(warps[k], False)
        X, Y = ir.coords64(inv, h, w, False)
        inside, ix, iy, tx, ty = ir.footprint(X, Y, h, w)
        assert inside[m].all()
        lin[m] += ir.bilinear64(frames[k][..., 0], X[m], Y[m])
        cub[m] += ir.sample(ir.gather(frames[k], ix[m], iy[m])[:, 0], tx[m], ty[m], F(1.0), np.float64)
    rms = lambda img: float(np.sqrt(np.mean((img[m] / n - scene[m]) ** 2)))
    return rms(lin), rms(cub)


def test_cubic_samples_stack_closer_to_the_scene_than_linear_ones():
    rl, rc = restated_quality(7)
    print("restated quality: linear", rl, "cubic", rc, "ratio", rc / rl)
    assert rc / rl < 0.25


def test_python_constants_are_opencvs():
    from libstacker_rs_amd import api
    assert (api.INTER_LINEAR, api.INTER_CUBIC) == (1, 2)

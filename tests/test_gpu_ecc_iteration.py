"""One ECC iteration on the GPU against the float64 restatement (test_cpu_ecc_iteration.ecc_iteration_restate) where the
column-walking pixel pass changes its route: templates half outside frame 0 (the masked body), rotated ones (no LDS ring, a
ragged rim), frames whose last 64-pixel column is partial, one lane wide or the only one, thin frames, and a frame with fewer
row units than waves. stk_find_transform_ecc with max_count = 1, no epsilon and a caller's start IS that iteration: the
result is a direct function of the pass's sums (Hessian, both projections, correlation, error projection).

The bar comes from the reference side alone: the engine may be as far from float64 as 3 x the floor plus one ulp of the
f32 the result is stored in. The floor is the largest of three distances from the same float64 answer, all computed on the
CPU: the oracle's, the f32-per-column accumulation model's, and the f32 solve's — the float64 sums cast to f32 with every
entry moved one ulp (16 seeded draws) and solved as OpenCV solves them, by f32 LU. The third is there for a derived
reason: the oracle's own distance is one draw of that solve's round-off, and on thin or half-covered
homography cases one draw is up to 10 x below what the last bit of the sums is worth (8 x 65, `id`: the oracle 1.8e-5 px,
the draws 9.4e-5 median, 2.2e-4 max; the engine, all four routes, 8.6e-5 .. 9.0e-5)."""
import numpy as np
import pytest

import oracle
from libstacker_rs_amd import EccMatchParameters, MotionType, synth
from test_cpu_ecc_iteration import CASES, SHAPES, get_case

pytestmark = pytest.mark.gpu

MOTION = {"translation": MotionType.Translation, "euclidean": MotionType.Euclidean, "affine": MotionType.Affine,
          "homography": MotionType.Homography}
# the margin this project gave a kernel-vs-floor ratio before it had measurements: operation order, v_rcp_f32 in the
# coordinates, the factorisation of the sums into per-lane moments of Y
FLOOR_FACTOR = 3.0
RHO_BAR = 1e-5
DEFAULTS = {"ecc_blocks": 0, "ecc_ring": 1, "ecc_variant": 3}
ROUTES = [("default", {}),
          ("blocks8", {"ecc_blocks": 8}),                          # long strips: the LDS ring is eligible
          ("blocks8-gather", {"ecc_blocks": 8, "ecc_ring": 0}),    # the same strips through the gather loop
          ("variant0", {"ecc_variant": 0})]                        # the direct kernel, on its own against float64


def run_route(stacker, c, options, max_count=1):
    """(warp 3x3 f32, rho, iterations, ring fall-backs) of the engine's iteration(s) on case c under the given options."""
    p = EccMatchParameters(MOTION[c.motion], max_count, None, c.gauss)
    try:
        for k, v in options.items():
            stacker.set_option(k, v)
        W, rho, its = stacker.find_transform_ecc(c.templ, c.inp, c.start_arg, p)
        fallbacks = stacker.timing()["ecc_ring_fallbacks"]
    finally:
        for k in options:
            stacker.set_option(k, DEFAULTS[k])
    return W, rho, its, fallbacks


def check_against_float64(stacker, c, failures, worst):
    floor = c.floor
    bar = FLOOR_FACTOR * floor + c.ulp
    got = {}
    for name, options in ROUTES:
        W, rho, its, fallbacks = run_route(stacker, c, options)
        got[name] = (W, rho)
        e_gpu, drho = c.error(W), abs(rho - c.rho64)
        print("%-36s %-15s e_gpu %.2e px = %.2f x floor (%.2e; bar %.2e)  |drho| %.1e  coverage %.2f"
              % (c.id, name, e_gpu, e_gpu / floor, floor, bar, drho, c.coverage))
        w = worst.setdefault(name, [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e_gpu / floor), max(w[1], e_gpu / bar), max(w[2], drho)
        if its != 1:
            failures.append((c.id, name, "iterations", its))
        if not e_gpu <= bar:
            failures.append((c.id, name, "e_gpu %.3e > bar %.3e (floor %.3e)" % (e_gpu, bar, floor)))
        if not drho <= RHO_BAR:
            failures.append((c.id, name, "|drho| %.3e" % drho))
        if name == "blocks8" and (c.h, c.w) == (200, 449) and c.truth in ("id", "shift") and fallbacks != 0:
            failures.append((c.id, name, "ring fall-backs", fallbacks))
    # ring and gather read the same taps and run the same arithmetic: not one bit apart
    if not (np.array_equal(got["blocks8"][0], got["blocks8-gather"][0]) and got["blocks8"][1] == got["blocks8-gather"][1]):
        failures.append((c.id, "ring vs gather differ", got["blocks8"], got["blocks8-gather"]))


def report(worst):
    for name, (ratio, of_bar, drho) in worst.items():
        print("worst %-15s e_gpu / floor %.2f   e_gpu / bar %.2f   |drho| %.1e" % (name, ratio, of_bar, drho))


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=["%dx%d" % s for s, _ in SHAPES])
def test_one_iteration_matches_float64(stacker, shape):
    failures, worst = [], {}
    for case in CASES:
        if case[:2] == shape:
            check_against_float64(stacker, get_case(case), failures, worst)
    report(worst)
    assert not failures, failures


@pytest.mark.parametrize("gauss,depth", [(3, 8), (7, 8), (5, 32)], ids=["gauss3", "gauss7", "f32"])
def test_one_iteration_other_preparations(stacker, gauss, depth):
    """Other blur sizes and a float32 template / input pair, at half coverage and under perspective, with a partial last
    column. (The f32 blur is allclose-level against the oracle's, not bit-exact: e_oracle carries that.)"""
    failures, worst = [], {}
    for truth in ("shift", "persp"):
        check_against_float64(stacker, get_case((97, 191, truth, "homography"), gauss, depth), failures, worst)
    report(worst)
    assert not failures, failures


@pytest.mark.parametrize("shape", [(97, 191), (200, 449)], ids=["97x191", "200x449"])
def test_three_fixed_iterations_match_the_oracle(stacker, shape):
    """test_fixed_iteration_count_no_eps's bars (three iterations, then <= 0.01 px from the oracle), at half coverage,
    under rotation and perspective, with a partial last column."""
    h, w = shape
    failures = []
    for truth in ("shift", "rot", "persp"):
        for motion in ("homography", "affine"):
            c = get_case((h, w, truth, motion))
            rc, Wo, rho_o, its_o = oracle.find_transform_ecc(c.templ, c.inp, c.start_arg, c.omotion, 3, None, c.gauss)
            assert rc == 0 and its_o == 3, c.id
            for name, options in ROUTES:
                W, rho, its, _ = run_route(stacker, c, options, max_count=3)
                assert motion == "homography" or np.array_equal(W[2], [0, 0, 1])
                e = synth.corner_error(W, Wo, w, h)
                print("%-36s %-15s 3 iterations: %.2e px from the oracle, |drho| %.1e" % (c.id, name, e, abs(rho - rho_o)))
                if its != 3 or not e <= 0.01:
                    failures.append((c.id, name, its, e))
    assert not failures, failures

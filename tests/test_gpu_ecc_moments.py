"""The homography moment sums on a TALL frame. The column pass multiplies the three Jacobian terms by the row number Y before
it forms the Hessian moments and the projections (every sum one fma of two of the six values j, j * Y), so at row 2160 a
factor is up to 2160 times the Jacobian — and the iteration cases of test_gpu_ecc_iteration.py stop at 200 rows. The frame
here is 2161 rows (a 4K frame's height plus one, odd) by 70 columns: one full column strip and a six-lane one, strips of
several hundred rows by default and of ~270 with ecc_blocks = 8.

 * one iteration against the float64 restatement by test_gpu_ecc_iteration.check_against_float64: four routes, the bar
   3 x floor + one ulp computed from the CPU side alone, ring and gather bit-equal;
 * the same frame with the affine model, whose accumulation is the plain one: its bars, and the column pass against the
   direct kernel (ecc_variant 0) the way test_gpu_ecc.py compares them;
 * a 4-frame 70 x 2161 stack through ecc_match: the first-iteration route and the general route give the same bits, and
   so do one slot with refills and three slots."""
import numpy as np
import pytest

import test_gpu_ecc_first_iter as first_iter
from libstacker_rs_amd import synth
from test_cpu_ecc_iteration import get_case
from test_cpu_ecc_moments import TALL_AFFINE, TALL_CASES, TRUTHS
from test_gpu_ecc_iteration import check_against_float64, report, run_route

pytestmark = pytest.mark.gpu

W, H, N = 70, 2161, 4


@pytest.mark.parametrize("case", TALL_CASES, ids=TRUTHS)
def test_tall_frame_matches_float64(stacker, case):
    failures, worst = [], {}
    check_against_float64(stacker, get_case(case), failures, worst)
    report(worst)
    assert not failures, failures


@pytest.mark.parametrize("case", TALL_AFFINE, ids=TRUTHS)
def test_tall_frame_affine(stacker, case):
    """The other motions' accumulation did not change: the same bars, and the column pass within 0.02 px of the direct
    kernel with the same iteration count (test_direct_variant_agrees_with_production's figures)."""
    c = get_case(case)
    failures, worst = [], {}
    check_against_float64(stacker, c, failures, worst)
    report(worst)
    assert not failures, failures
    # three iterations only where the step is well posed by test_cases_are_admissible's conditions (CPU side alone): an
    # affine map cannot follow `persp` over 2161 rows (w falls to 0.57), its first step moves a corner by 1600 px at
    # rho = 0.25, and what follows such a step amplifies the last bit of any two summation orders
    for max_count in ((1, 3) if c.move <= 8.0 and c.rho64 >= 0.75 else (1,)):
        W3, rho3, its3, _ = run_route(stacker, c, {}, max_count)
        W0, rho0, its0, _ = run_route(stacker, c, {"ecc_variant": 0}, max_count)
        e = synth.corner_error(W3, W0, c.w, c.h)
        print("%-34s %d iteration(s): column pass %.2e px from the direct kernel, |drho| %.1e" % (c.id, max_count, e, abs(rho3 - rho0)))
        assert its3 == its0 == max_count, (c.id, its3, its0)
        assert np.array_equal(W3[2], [0, 0, 1]) and np.array_equal(W0[2], [0, 0, 1])
        assert e <= 0.02, (c.id, max_count, e)


@pytest.fixture(scope="module")
def tall_stack():
    return first_iter.stack(N, W, H).cuda()


@pytest.fixture(scope="module")
def tall_reference(stacker, tall_stack):
    """The stack by the general route alone, computed once."""
    res, count = first_iter.run(stacker, tall_stack, first_iter.PRODUCTION, {"ecc_first_iter": 0})
    assert not isinstance(res[0], type), res
    assert count == 0
    return res


def test_first_iteration_route_on_a_tall_frame(stacker, tall_stack, tall_reference):
    on, c_on = first_iter.run(stacker, tall_stack, first_iter.PRODUCTION, {})
    print("iterations", on[1], "rho", on[2])
    first_iter.assert_same(on, tall_reference, "first iteration route, %d x %d" % (W, H))
    assert c_on == N - 1, c_on


def test_shard_invariance_on_a_tall_frame(stacker, tall_stack, tall_reference):
    one, _ = first_iter.run(stacker, tall_stack, first_iter.PRODUCTION, {"ecc_slots": 1})
    three, _ = first_iter.run(stacker, tall_stack, first_iter.PRODUCTION, {"ecc_slots": 3})
    first_iter.assert_same(one, three, "ecc_slots 1 against 3")
    first_iter.assert_same(one, tall_reference, "ecc_slots 1 against the general route")

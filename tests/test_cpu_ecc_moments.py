"""The tall cases of test_gpu_ecc_moments.py, on the CPU alone. The homography pass multiplies the Jacobian terms by the row
number before it forms the moment sums, so the frames that can show a fault of that are tall ones (the iteration cases of
test_cpu_ecc_iteration.py stop at 200 rows): 2161 rows — a 4K frame's height plus one, odd — by 70 columns, one full column
strip and six lanes. Here: the cases are admissible by the conditions test_cases_are_admissible applies, and the model of
f32 accumulation down a whole column, which sets the GPU test's floor together with the oracle and the f32 solve, still
lands where float64 does at that height."""
import pytest

from test_cpu_ecc_iteration import get_case

TALL = (2161, 70)
TRUTHS = ("id", "shift", "persp")
TALL_CASES = [TALL + (truth, "homography") for truth in TRUTHS]
TALL_AFFINE = [TALL + (truth, "affine") for truth in TRUTHS]


@pytest.mark.parametrize("case", TALL_CASES, ids=TRUTHS)
def test_tall_cases_are_admissible(case):
    c = get_case(case)
    print("%-34s coverage %.3f rho %.4f move %.3f px floor %.2e px" % (c.id, c.coverage, c.rho64, c.move, c.floor))
    assert c.move <= 8.0, c.id
    assert c.coverage >= 0.25, c.id
    assert c.rho64 >= 0.75, c.id


@pytest.mark.parametrize("case", TALL_CASES, ids=TRUTHS)
def test_f32_columns_reach_float64_on_a_tall_frame(case):
    """The bars of test_precision_models_account_for_the_oracle: each model within 2e-3 px of float64, and the oracle's own
    distance accounted for by three times the larger model plus one ulp of the frame size."""
    c = get_case(case)
    print("%-34s oracle %.2e px  f32-columns %.2e px  f32-solve %.2e px" % (c.id, c.e_oracle, c.e_f32col, c.e_f32solve))
    assert c.e_f32col <= 2e-3 and c.e_f32solve <= 2e-3, (c.id, c.e_f32col, c.e_f32solve)
    assert c.e_oracle <= 3.0 * max(c.e_f32col, c.e_f32solve) + c.ulp, (c.id, c.e_oracle, c.e_f32col, c.e_f32solve)

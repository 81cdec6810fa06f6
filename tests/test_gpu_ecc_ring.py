"""The LDS ring of the column-walking ECC pass on the device, against the counts its restatement predicts.

stk_find_transform_ecc with max_count = 1, no epsilon and a caller's start runs exactly one pass on one slot, so
`ecc_ring_fallbacks` and `ecc_first_iter_slots` describe that pass. Under the debug option ecc_ring_lookahead = 1 every
ring strip fails the run-time check at its first step (safe = max(i0, i1) + 1 < ihi + 2): the counter is then the number
of strips that took the ring, and the model (ecc_ring_restate.py) says how many that must be; at 2 .. 5 it says which
strips still fall back. The table's cases and the conditions that make them worth running (enough ring strips, one empty
case per reason, fall-backs that stop at lookahead 4 and at 5, a partial fall-back, no case that hangs on the last bit of
v_rcp_f32) are asserted on the model alone by test_cpu_ecc_ring.py. Whatever route a strip takes, the warp and rho must
be the bits of the gather route."""
import numpy as np
import pytest

import ecc_ring_restate as R
from libstacker_rs_amd import EccMatchParameters, MotionType
from test_cpu_ecc_iteration import scene

pytestmark = pytest.mark.gpu

MOTION = {"homography": MotionType.Homography, "affine": MotionType.Affine, "translation": MotionType.Translation}
DEFAULTS = {"ecc_blocks": 0, "ecc_ring": 1, "ecc_ring_lookahead": R.constants().LOOKAHEAD, "ecc_first_iter": 1}


def _run(stacker, templ, inp, start, params, opts):
    try:
        for k, v in opts.items():
            stacker.set_option(k, v)
        W, rho, its = stacker.find_transform_ecc(templ, inp, start.copy(), params)
        t = stacker.timing()
    finally:
        for k, v in DEFAULTS.items():
            stacker.set_option(k, v)
    return W, rho, its, int(t["ecc_ring_fallbacks"]), int(t["ecc_first_iter_slots"])


@pytest.mark.parametrize("name", [c[0] for c in R.GPU_TABLE])
def test_ring_counters_match_the_model(stacker, name):
    case = R.table_case(name)
    _, (h, w), motion, blocks, start64, _ = case
    inp = scene(h, w)
    templ = R.sample_template(inp, start64)
    start = R.case_start(case)
    params = EccMatchParameters(MOTION[motion], 1, None, 5)
    Wg, rho_g, its_g, fb_g, _ = _run(stacker, templ, inp, start, params, {"ecc_blocks": blocks, "ecc_ring": 0})
    assert its_g == 1 and fb_g == 0
    lines = []
    for first_iter in ((1, 0) if name == "identity" else (1,)):
        for la in (1, 2, 3, 4, 5):
            want_fb, want_first, ring_strips = R.case_model(case, la, first_iter)
            W, rho, its, fb, first = _run(stacker, templ, inp, start, params,
                                          {"ecc_blocks": blocks, "ecc_ring_lookahead": la, "ecc_first_iter": first_iter})
            lines.append("%s first_iter %d lookahead %d: ring strips %d, fall-backs %d (model %d), first-iteration slots %d (model %d)"
                         % (name, first_iter, la, ring_strips, fb, want_fb, first, want_first))
            print(lines[-1])
            assert fb == want_fb, lines
            assert first == want_first, lines
            assert its == 1
            assert np.array_equal(W, Wg) and rho == rho_g, (name, la, first_iter)

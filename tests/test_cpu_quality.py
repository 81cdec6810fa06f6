"""stk_rank_frames (include/stacker.h): the example's sort / skip / reverse (examples/main.rs:53, 64) as host code, checked
without a GPU against its three-line Python restatement."""
import ctypes as C
import math

import numpy as np
import pytest

from libstacker_rs_amd import InvalidParams, NotEnoughFiles, SelectParameters, _ffi, rank_frames
from libstacker_rs_amd.api import QUALITY_WEIGHT_NONE, QUALITY_WEIGHT_SCORE, SHARPNESS_GLVN, SHARPNESS_LAPM, SHARPNESS_TENG


def _scores(column, metric=SHARPNESS_TENG):
    """n x 4 scores with `column` in the ranked metric and unrelated values in the other three."""
    n = len(column)
    sc = np.random.default_rng(n).random((n, 4)) * 100
    sc[:, metric] = column
    return sc


def _restated(column, drop=0):
    """main.rs:53 (stable ascending sort), :64 skip(drop) and rev()."""
    n = len(column)
    return sorted(range(n), key=lambda i: column[i])[drop:][::-1]


def _check_permutation(order, n):
    assert sorted(int(i) for i in order) == list(range(n))


DISTINCT = [7.5, 1.25, 9.0, 3.5, 0.5, 8.0, 2.0]
TIES = [2.0, 5.0, 2.0, 5.0, 1.0, 2.0, 5.0, 9.0]


@pytest.mark.parametrize("metric", [SHARPNESS_LAPM, SHARPNESS_TENG, SHARPNESS_GLVN])
def test_distinct_scores_sort_skip_reverse(metric):
    order, kept, w = rank_frames(_scores(DISTINCT, metric), SelectParameters(metric=metric))
    assert kept == len(DISTINCT)
    assert list(order) == _restated(DISTINCT)
    assert order[0] == 2 and order[-1] == 4
    assert np.array_equal(w, np.ones(len(DISTINCT), np.float32))


def test_ties_come_out_in_descending_frame_index():
    order, kept, _ = rank_frames(_scores(TIES))
    assert list(order) == _restated(TIES) == [7, 6, 3, 1, 5, 2, 0, 4]
    assert kept == len(TIES)


def test_a_nan_score_is_equal_to_every_other():
    # everything left of the NaN is below everything right of it: no stable sort has a reason to move a frame across it
    col = [2.0, 1.0, float("nan"), 4.0, 3.0]
    order, kept, _ = rank_frames(_scores(col))
    assert list(order) == _restated(col) == [3, 4, 2, 0, 1]
    _check_permutation(order, 5)
    # where the comparison leaves the order open the header defines it: the NaN frame keeps its place and no frame moves
    # across it (a straight insertion sort, Rust's sort_by on short slices)
    col = [3.0, 1.0, float("nan"), 2.0, 0.5]
    order, kept, _ = rank_frames(_scores(col), SelectParameters(drop_worst=1))
    assert list(order) == [3, 4, 2, 0, 1]                     # sorted on each side of the NaN: 1 0 | 2 | 4 3, then reversed
    assert kept == 4


@pytest.mark.parametrize("column", [DISTINCT, TIES])
@pytest.mark.parametrize("drop", [0, 1, "n-1"])
def test_drop_worst(column, drop):
    n = len(column)
    d = n - 1 if drop == "n-1" else drop
    order, kept, _ = rank_frames(_scores(column), SelectParameters(drop_worst=d))
    assert kept == n - d
    assert list(order[:kept]) == _restated(column, d)
    _check_permutation(order, n)
    assert list(order) == _restated(column)                   # the dropped frames follow, best first


@pytest.mark.parametrize("n,fraction", [(7, 1.0), (7, 0.5), (8, 0.5), (10, 0.25), (10, 0.31), (3, 0.01)])
def test_keep_fraction(n, fraction):
    col = list(np.random.default_rng(n).permutation(n).astype(np.float64))
    order, kept, _ = rank_frames(_scores(col), SelectParameters(keep_fraction=fraction))
    assert kept == max(1, math.ceil(float(np.float32(fraction)) * n))
    assert kept == {(7, 1.0): 7, (7, 0.5): 4, (8, 0.5): 4, (10, 0.25): 3, (10, 0.31): 4, (3, 0.01): 1}[(n, fraction)]
    assert list(order[:kept]) == _restated(col)[:kept]
    _check_permutation(order, n)


def test_parameter_errors():
    sc = _scores(DISTINCT)
    with pytest.raises(InvalidParams):
        rank_frames(sc, SelectParameters(drop_worst=1, keep_fraction=0.5))
    with pytest.raises(InvalidParams):
        rank_frames(sc, SelectParameters(keep_fraction=1.5))
    with pytest.raises(InvalidParams):
        rank_frames(sc, SelectParameters(keep_fraction=float("nan")))
    with pytest.raises(InvalidParams):
        rank_frames(sc, SelectParameters(drop_worst=-1))
    with pytest.raises(InvalidParams):
        rank_frames(sc, SelectParameters(metric=4))
    with pytest.raises(InvalidParams):
        rank_frames(sc, SelectParameters(weight_mode=2))
    with pytest.raises(NotEnoughFiles):
        rank_frames(sc, SelectParameters(drop_worst=len(DISTINCT)))          # nothing kept
    with pytest.raises(NotEnoughFiles):
        rank_frames(np.zeros((0, 4)))
    order, kept, _ = rank_frames(sc)                                          # and the library still answers
    assert kept == len(DISTINCT)


def test_score_weights():
    col = np.array(DISTINCT)
    order, kept, w = rank_frames(_scores(col), SelectParameters(drop_worst=2, weight_mode=QUALITY_WEIGHT_SCORE))
    assert w.dtype == np.float32 and kept == 5
    best = col[order[0]]
    for i in range(kept):
        assert w[i] == np.float32(col[order[i]] / best)
    assert w[0] == 1.0 and np.array_equal(w[kept:], np.ones(2, np.float32))
    # an all-zero column: the best score is 0, every weight is 1
    order, kept, w = rank_frames(_scores([0.0] * 5), SelectParameters(weight_mode=QUALITY_WEIGHT_SCORE))
    assert np.array_equal(w, np.ones(5, np.float32)) and list(order) == [4, 3, 2, 1, 0]
    _, _, w = rank_frames(_scores(col), SelectParameters(weight_mode=QUALITY_WEIGHT_NONE))
    assert np.array_equal(w, np.ones(len(col), np.float32))


def test_weights_are_optional_in_the_c_call():
    lib = _ffi.load()
    sc = np.ascontiguousarray(_scores(DISTINCT))
    order = (C.c_int32 * len(DISTINCT))()
    kept = C.c_int32(0)
    sp = SelectParameters(drop_worst=1)._c()
    assert lib.stk_rank_frames(C.c_void_p(sc.ctypes.data), len(DISTINCT), C.byref(sp), order, C.byref(kept), None) == 0
    assert list(order)[:kept.value] == _restated(DISTINCT, 1)


def test_struct_sizes_match_the_header(tmp_path):
    """The ctypes mirrors against what a C compiler makes of include/stacker.h itself."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text(
        '#include <stddef.h>\n#include <stdio.h>\n#include "stacker.h"\n'
        "int main(void) {\n"
        '    printf("%d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(stk_select_params), (int)offsetof(stk_select_params, metric),\n'
        "           (int)offsetof(stk_select_params, ksize), (int)offsetof(stk_select_params, drop_worst),\n"
        "           (int)offsetof(stk_select_params, keep_fraction), (int)offsetof(stk_select_params, weight_mode),\n"
        "           (int)offsetof(stk_select_params, reserved), (int)sizeof(stk_timing), (int)offsetof(stk_timing, prep_ms),\n"
        "           (int)STK_QUALITY_WEIGHT_SCORE);\n"
        "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S, T = _ffi.SelectParams, _ffi.Timing
    assert got == [C.sizeof(S), S.metric.offset, S.ksize.offset, S.drop_worst.offset, S.keep_fraction.offset, S.weight_mode.offset,
                   S.reserved.offset, C.sizeof(T), T.prep_ms.offset, QUALITY_WEIGHT_SCORE]
    assert [name for name, _ in S._fields_] == ["metric", "ksize", "drop_worst", "keep_fraction", "weight_mode", "reserved"]

"""The inputs of test_gpu_selection_classes.py, CPU side (selection_classes.py): the dispatch function against the launchers'
text, the class coverage of the swept sample counts, the builders, and every condition the GPU tests put on their inputs,
shown to hold for the chosen inputs before any of them reaches a GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import selection_classes as sc
from selection_classes import F, H, W
from test_cpu_quantile import quantile_restate

CSRC = Path(__file__).resolve().parent.parent / "libstacker_rs_amd" / "csrc"


# ---- 1. the dispatch and the class coverage ---------------------------------------------------------------------------
def test_launch_class_is_the_launchers_dispatch():
    """select_plan (select_body.h) holds the four lines, once, and no other file under csrc/ holds them or computes a G or a
    group count of its own: the three launchers all go through it. launch_class restates them. A change of the dispatch
    fails here first: follow it in launch_class, then check_class_coverage says what N_LIST no longer hits."""
    lines = ["const int groups = (n + 3) / 4;",
             "while (ls < 6 && (groups + (1 << ls) - 1) >> ls > 8) ls++;",
             "const int per = (groups + (1 << ls) - 1) >> ls;",
             "const int G = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;"]
    files = sorted(p for p in CSRC.iterdir() if p.is_file())
    assert CSRC / "select_body.h" in files and CSRC / "kernels_quantile.hip" in files and CSRC / "kernels_robust_clip.hip" in files
    for path in files:
        text = path.read_text(errors="replace")
        once = 1 if path.name == "select_body.h" else 0
        for line in lines:
            assert text.count(line) == once, (path.name, line)
        if path.suffix in (".hip", ".h"):                # (stacker.cpp has an ECC variable named groups)
            assert len(re.findall(r"const int groups\b", text)) == once and len(re.findall(r"const int G\b", text)) == once, path.name
    for name in ("kernels_quantile.hip", "kernels_robust_clip.hip"):
        assert "select_plan(m, n)" in (CSRC / name).read_text()
    assert "constexpr int QUANTILE_MAX_SAMPLES = 4096;" in (CSRC / "common.h").read_text()
    assert sc.MAX_SAMPLES == 4096


def test_class_table():
    assert sc.class_ranges() == {(0, 1): (1, 4), (0, 2): (5, 8), (0, 4): (9, 16), (0, 8): (17, 32), (1, 8): (33, 64), (2, 8): (65, 128),
                                 (3, 8): (129, 256), (4, 8): (257, 512), (5, 8): (513, 1024), (6, 8): (1025, 2048),
                                 (6, 16): (2049, 4096)}
    assert sc.split_of(33) == (32, 1) and sc.split_of(4096) == (64, 63) and sc.split_of(32) == (32, 0) and sc.split_of(2048) == (32, 63)


def test_the_swept_sample_counts_hit_every_class():
    assert sc.check_class_coverage(sc.N_LIST) == sorted(sc.CLASSES)              # the plain quantile and the plain robust route
    assert sc.check_class_coverage(sc.MASKED_N, both_ends_up_to=512) == sorted(sc.CLASSES)     # the two participation forms
    assert sorted(sc.launch_class(n) for n in sc.ADVERSARIAL_N) == sorted(sc.CLASSES)
    assert all(n % 4 for n in sc.ADVERSARIAL_N)
    assert (sc.launch_class(1), 1 % 4) == ((0, 1), 1)
    with pytest.raises(AssertionError):
        sc.check_class_coverage([n for n in sc.N_LIST if n != 2049])
    with pytest.raises(AssertionError):
        sc.check_class_coverage([n for n in sc.N_LIST if n not in (126, 65)] + [68])          # no ragged n in (2, 8)
    assert all((H * W * cn // rows) % (256 >> ls) for ls in range(7) for cn in (1, 3) for rows in (1, H))   # col >= m lanes are live


def test_quantiles_and_ranks():
    q = sc.QUANTILES
    assert len(q) == 8 and q[0] == 0.0 and q[1] == 1.0 and q[6] < 1.0 and F(q[6]) == np.nextafter(F(1), F(0)) and 0 < q[7] < 2e-7
    assert all(F(v) == v for v in q)
    assert sc.rank_of(5, 0.5) == (2, F(0)) and sc.rank_of(4, 0.5) == (1, F(0.5)) and sc.rank_of(4096, 1.0) == (4095, F(0))
    j, g = sc.rank_of(4096, q[6])
    assert j == 4094 and 0.99 < g < 1
    j, g = sc.rank_of(4096, q[7])
    assert j == 0 and 0 < g < 1e-3


# ---- 2. the sample model ------------------------------------------------------------------------------------------------
def test_shifted_samples_at_the_identity_and_a_translation():
    rng = np.random.default_rng(1)
    fr = rng.normal(0, 1, (3, H, W, 2)).astype(F)
    for classic in (False, True):
        s, inside = sc.shifted_samples(fr, classic=classic)
        assert sc.same_bits(s, fr) and inside.all()
    s, inside = sc.shifted_samples(fr, [(2, 1), (0, 0), (12, 4)])
    assert sc.same_bits(s[0, :H - 1, :W - 2], fr[0, 1:, 2:]) and (s[0, H - 1:] == 0).all() and (s[0, :, W - 2:] == 0).all()
    assert inside[0, :H - 1, :W - 2].all() and inside[0].sum() == (H - 1) * (W - 2) and inside[2].sum() == 1
    # a NaN or an infinity makes NaN of the three pixels that hold it as a zero-weight tap; the 4-weight path keeps an infinity
    fr[1, 2, 4, 0] = np.inf
    for classic in (False, True):
        s, _ = sc.shifted_samples(fr, classic=classic)
        assert np.isnan(s[1, 1:3, 3:5, 0]).sum() == (3 if classic else 4) and np.isnan(s[1, ..., 0]).sum() == (3 if classic else 4)
        assert not np.isnan(s[1, ..., 1]).any()
    assert sc.shifted_samples(fr, classic=True)[0][1, 2, 4, 0] == np.inf


def test_same_bits_tells_the_zeros_apart():
    a = np.array([0.0, -0.0, np.nan, 1.0], F)
    assert sc.same_bits(a, a.copy()) and not sc.same_bits(a, np.array([0.0, 0.0, np.nan, 1.0], F))
    assert not sc.same_bits(a, np.array([0.0, -0.0, 2.0, 1.0], F))


# ---- 3. columns with planted order statistics -------------------------------------------------------------------------------
def test_placement_pairs():
    assert sc.placement_pairs(1) == []
    assert sc.placement_pairs(4) == [(0, 3), (3, 0)]
    assert sc.placement_pairs(9) == [(0, 8), (8, 0), (7, 8), (8, 7)]                               # G = 4: groups 0..3, 4..7, 8
    assert sc.placement_pairs(33) == [(0, 32), (32, 0), (31, 32), (32, 31), (27, 28), (28, 27)]
    assert sc.placement_pairs(2049) == [(0, 2048), (2048, 0), (2047, 2048), (2048, 2047), (64, 63), (2043, 2044), (2044, 2043)]
    for n in sc.N_LIST:
        per_split, _ = sc.split_of(n)
        pairs = sc.placement_pairs(n)
        assert all(0 <= a < n and 0 <= b < n and a != b for a, b in pairs)
        assert len(pairs) * len(sc.QUANTILES) <= H * W
        if n > 1:
            assert (0, n - 1) in pairs and (n - 1, 0) in pairs
        if n > per_split:                                # a pair across a lane-split boundary
            assert any(abs(a - b) == 1 and max(a, b) % per_split == 0 for a, b in pairs)
        if n > 4 and per_split > 4:                      # and one across a group boundary inside a split
            assert any(abs(a - b) == 1 and max(a, b) % 4 == 0 and max(a, b) % per_split for a, b in pairs)


@pytest.mark.parametrize("n", sc.N_LIST)
def test_plain_stack_plants_what_it_says(n):
    for cn in (1, 3) if n == 61 else (1,):
        frames, planted = sc.plain_stack(n, cn)
        assert frames.shape == (n, H, W, cn) and frames.dtype == F and np.isfinite(frames).all()
        cols = frames.reshape(n, -1)
        assert len(planted) == len(sc.placement_pairs(n)) * len(sc.QUANTILES)
        for k, qi, j, a, b in planted:
            c = cols[:, k]
            srt = np.sort(c)
            assert (np.diff(srt) > 0).all() and srt[0] < 0 < srt[-1]
            assert (j, ) == sc.rank_of(n, sc.QUANTILES[qi])[:1]
            assert c[a] == srt[j] and c[b] == srt[j + 1 if j + 1 < n else j - 1]
        # the sample of a finite frame under the identity is the frame's value: the reference needs the frames alone
        assert sc.same_bits(sc.shifted_samples(frames)[0], frames)
        orders = sc.frame_orders(n)
        assert sorted(orders) == ["random", "reversed", "rotated"]
        assert all(sorted(o.tolist()) == list(range(n)) for o in orders.values())
        assert n < 4 or len({tuple(o.tolist()) for o in orders.values()} | {tuple(range(n))}) == 4


# ---- 4. adversarial values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.ADVERSARIAL_N)
def test_adversarial_stack_reaches_the_kernel_as_built(n):
    frames, where = sc.adversarial_stack(n)
    samples, _ = sc.shifted_samples(frames, classic=True, border=sc.ADVERSARIAL_BORDER)
    fmax = np.finfo(F).max
    for y, x in sc.LATTICE:                              # bit for bit: the sign of a zero, the infinities, the NaNs
        assert sc.same_bits(samples[:, y, x, 0], frames[:, y, x, 0]), (y, x)
    col = {name: frames[:, y, x, 0] for name, (y, x) in where.items()}
    assert len(col) == 14
    z = col["zeros"]
    assert set(np.abs(z).tolist()) <= {0.0, float(F(1e-45)), float(F(1e-40))} and 0 < F(1e-45) < F(1e-40) < np.finfo(F).tiny
    if n >= 6:
        assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any() and (z > 0).any() and (z < 0).any()
        assert {fmax, -fmax, np.inf, -np.inf} <= set(col["huge"].tolist())
    one = F(1)
    for name, sign in (("ulp+", 1), ("ulp-", -1)):
        assert set((sign * col[name]).tolist()) == {float(np.nextafter(one, F(0))), 1.0, float(np.nextafter(one, F(2)))}
        assert min((col[name] == v).sum() for v in set(col[name].tolist())) >= n // 3
    assert len(set(col["equal"].tolist())) == 1
    for q in (0.5, 0.73):
        j, _ = sc.rank_of(n, q)
        a, b = np.sort(col[f"two:{q}:j+1"]), np.sort(col[f"two:{q}:j"])
        assert a[j] == F(0.25) and (j + 1 == n or a[j + 1] == F(0.75))
        assert b[j] == F(0.75) and (j == 0 or b[j - 1] == F(0.25))
    assert (np.diff(col["ramp"]) < 0).all()
    assert np.isnan(col["nan-last"][-1]) and np.isnan(col["nan-last"]).sum() == 1
    assert np.isnan(col["nan-first"][0]) and np.isnan(col["nan-first"]).sum() == 1
    assert (col["+inf"] == np.inf).sum() == 1 and (col["-inf"] == -np.inf).sum() == 1
    assert np.isfinite(np.delete(col["+inf"], np.argmax(col["+inf"]))).all()
    if n >= 4:                                           # the infinity lies beyond the median's two order statistics
        assert np.isfinite(quantile_restate(col["+inf"][:, None], 0.5)).all() and np.isfinite(quantile_restate(col["-inf"][:, None], 0.5)).all()
    for name in ("nan-last", "nan-first"):
        assert np.isnan(quantile_restate(col[name][:, None], 0.5)).all()


# ---- 5. participation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.MASKED_N)
def test_translation_table_gives_every_condition(n):
    for cn in (1, 3) if n == 61 else (1,):
        s = sc.masked_stack(n, cn)
        sh, wt, part = s["shifts"], s["weights"], s["part"]
        assert sh.shape == (n, 2) and (sh >= 0).all() and (sh[:, 0] < W).all() and (sh[:, 1] < H).all()
        assert (wt >= 0).all() and wt[0] == 1 and wt[-1] == 1 and ((wt == 0).any() or n < 8)
        assert all(np.array_equal(M, [[1, 0, -tx], [0, 1, -ty], [0, 0, 1]]) for M, (tx, ty) in zip(s["warps"], sh))
        # participation by hand: pixel (y, x) of the destination maps to (y + ty, x + tx) of the frame
        yy, xx = np.mgrid[0:H, 0:W]
        for i in range(0, n, max(1, n // 16)):
            assert np.array_equal(part[i], (yy + sh[i, 1] < H) & (xx + sh[i, 0] < W) & (wt[i] > 0))
        clean = ~(np.isnan(s["samples"]).any(axis=-1) & part).any(axis=0)
        n_p = sc.check_participation(n, part, wt, clean)
        assert n_p.max() == (wt > 0).sum() and n_p[:, W - 1].max() == 0
        # the genuine NaNs: five payloads in frames of at least three lane splits, each a participating sample
        per_split, _ = sc.split_of(n)
        assert len(s["nans"]) == (5 if n >= 33 else 0)
        if n >= 33:
            bits = [int(s["frames"][i].view(np.uint32)[y + sh[i, 1], x + sh[i, 0], 0]) for i, y, x in s["nans"]]
            assert bits == sc.NAN_BITS
            assert all(part[i, y, x] and np.isnan(s["samples"][i, y, x, 0]) for i, y, x in s["nans"])
            assert len({i // per_split for i, _, _ in s["nans"]}) >= (3 if n > 2 * per_split else 2)
            assert (~clean).any() and clean.sum() >= H * W // 2


def test_check_participation_refuses_interiors():
    n = 65
    part = np.ones((n, H, W), bool)
    with pytest.raises(AssertionError):
        sc.check_participation(n, part, np.ones(n, F))
    s = sc.masked_stack(n)
    with pytest.raises(AssertionError):                  # every sample of every pixel also in the first split
        sc.check_participation(n, s["part"] | (np.arange(n) == 1)[:, None, None], s["weights"])

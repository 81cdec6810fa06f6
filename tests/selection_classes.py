"""Inputs for the tests of the three selection kernels (quantile_select_kernel, quantile_select_masked_kernel,
robust_select_kernel) at every launch class: the launchers' dispatch as a function of the sample count, the sample counts
the tests sweep, and the builders of the stacks (columns with planted order statistics, adversarial values, translation
tables that give every pixel its own set of participating frames). Plain numpy, no engine: test_cpu_selection_classes.py
checks the builders and the conditions the GPU tests (test_gpu_selection_classes.py) rely on."""
import numpy as np

F = np.float32
H, W = 5, 13                                            # 65 pixels: no multiple of T = 256 >> ls for any ls <= 6

# ---- the dispatch ---------------------------------------------------------------------------------------------------
MAX_SAMPLES = 4096


def launch_class(n):
    """(ls, G) of select_plan (select_body.h), through which launch_quantile_select, launch_quantile_select_masked and
    launch_robust_select all go, for n samples: a pixel-channel's keys lie on S = 2^ls lanes of one wave, 4G keys per lane;
    frame i on split i // (4G)."""
    groups = (n + 3) // 4
    ls = 0
    while ls < 6 and (groups + (1 << ls) - 1) >> ls > 8:
        ls += 1
    per = (groups + (1 << ls) - 1) >> ls
    G = 1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8 if per <= 8 else 16
    return ls, G


CLASSES = [(0, 1), (0, 2), (0, 4), (0, 8), (1, 8), (2, 8), (3, 8), (4, 8), (5, 8), (6, 8), (6, 16)]

# Both ends of every class's range and one n in it that is no multiple of 4. If the dispatch in select_plan (select_body.h)
# changes, launch_class above has to follow it (test_cpu_selection_classes.py compares the text)
# and check_class_coverage then fails on this list: revisit it, the classes' edges have moved.
N_LIST = [1, 4, 5, 8, 9, 16, 17, 30, 32, 33, 61, 64, 65, 126, 128, 129, 250, 256,
          257, 507, 512, 513, 1021, 1024, 1025, 2047, 2048, 2049, 4095, 4096]
# the participation forms: above 512 samples the smallest n of a class and a ragged one
MASKED_N = [n for n in N_LIST if n not in (1024, 2048, 4096)]
# one ragged n per class for the adversarial values
ADVERSARIAL_N = [3, 7, 13, 30, 61, 126, 250, 507, 1021, 2047, 4095]


def class_ranges():
    """{class: (smallest n, largest n)} over n = 1 .. MAX_SAMPLES."""
    r = {}
    for n in range(1, MAX_SAMPLES + 1):
        c = launch_class(n)
        r[c] = (r[c][0], n) if c in r else (n, n)
    return r


def check_class_coverage(ns, both_ends_up_to=MAX_SAMPLES):
    """Asserts that `ns` hits all eleven classes, each at the smallest n of its range and at one n that is no multiple of 4,
    and, for the classes whose range ends at or below `both_ends_up_to`, at the largest n too. Returns the classes hit."""
    ranges = class_ranges()
    assert sorted(ranges) == sorted(CLASSES), sorted(ranges)
    hit = {}
    for n in ns:
        hit.setdefault(launch_class(n), []).append(n)
    assert sorted(hit) == sorted(CLASSES), sorted(hit)
    for c, (lo, hi) in ranges.items():
        assert lo in hit[c], (c, lo)
        assert hi in hit[c] or hi > both_ends_up_to, (c, hi)
        assert any(n % 4 for n in hit[c]), c
    return sorted(hit)


def split_of(n):
    """(frames per lane split, index of the split that holds frame n - 1)."""
    _, G = launch_class(n)
    return 4 * G, (n - 1) // (4 * G)


# ---- quantiles ------------------------------------------------------------------------------------------------------
QUANTILES = [float(F(v)) for v in (0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 0.73, np.nextafter(F(1), F(0)), 1e-7)]


def rank_of(n, q):
    """(j, g) of the definition: vi = (float)(n - 1) * q, j = floor(vi), g = vi - j, each operation in f32."""
    vi = F(n - 1) * F(q)
    jf = np.floor(vi)
    return int(jf), F(vi - jf)


# ---- the engine's sample of frame i at an integer translation -------------------------------------------------------------
def shifted_samples(frames, shifts=None, classic=False, border=0.0):
    """What the fold samples from `frames` (n x h x w x c, f32, alpha = 1) under BORDER_CONSTANT `border` where destination
    pixel (x, y) maps to (x + tx, y + ty) of frame i (`shifts`: n x (tx, ty) integers; None: the identity), which is the
    warp [[1, 0, -tx], [0, 1, -ty], [0, 0, 1]] of the frame onto the destination: the bilinear formula of
    warp_linear_sample.inc.h at fractions 0, in f32, operation by operation. The taps right of and below a pixel enter with
    weight 0: a finite tap leaves the value alone (up to the sign of a zero), a NaN or an infinite one makes the sample
    NaN. classic: the 4-weight path (warp_subpixel_bits != 0) instead of the lerp chain. Returns (samples, inside), inside
    (n x h x w) where the pixel maps into the frame: kappa == 1 there and 0 elsewhere."""
    fr = np.asarray(frames, F)
    n, h, w, c = fr.shape
    sh = np.zeros((n, 2), int) if shifts is None else np.asarray(shifts, int).reshape(n, 2)
    reach = int(np.abs(sh).max()) + 1
    pad = np.full((n, h + 2 * reach, w + 2 * reach, c), F(border), F)
    pad[:, reach:reach + h, reach:reach + w] = fr
    ins = np.zeros((n, h + 2 * reach, w + 2 * reach), bool)
    ins[:, reach:reach + h, reach:reach + w] = True
    out = np.empty_like(fr)
    inside = np.empty((n, h, w), bool)
    zero, one = F(0), F(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            x0, y0 = reach + sh[i, 0], reach + sh[i, 1]
            p00 = pad[i, y0:y0 + h, x0:x0 + w]
            p01 = pad[i, y0:y0 + h, x0 + 1:x0 + 1 + w]
            p10 = pad[i, y0 + 1:y0 + 1 + h, x0:x0 + w]
            p11 = pad[i, y0 + 1:y0 + 1 + h, x0 + 1:x0 + 1 + w]
            if classic:
                out[i] = ((p00 * one + p01 * zero) + p10 * zero) + p11 * zero
            else:
                t0 = zero * (p01 - p00) + p00               # fma(0, d, p): the product is exact, one rounding
                t1 = zero * (p11 - p10) + p10
                out[i] = zero * (t1 - t0) + t0
            inside[i] = ins[i, y0:y0 + h, x0:x0 + w]
    return out, inside


def same_bits(a, b):
    """a == b bit for bit, any NaN equal to any NaN (the sign of a zero counts)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- columns with planted order statistics --------------------------------------------------------------------------------
def placement_pairs(n):
    """Frame pairs (a, b) to hold s_(j) and s_(j+1): frame 0 and the tail slot n - 1, the two frames on either side of a
    lane-split boundary (the last one, both ways round, and the first one), and the two on either side of the last 4-frame
    group boundary that is no split boundary. Only what n has: none of it at n = 1."""
    per_split, _ = split_of(n)
    pairs = [(0, n - 1), (n - 1, 0)]
    bounds = list(range(per_split, n, per_split))
    if bounds:
        e = bounds[-1]
        pairs += [(e - 1, e), (e, e - 1)]
        if bounds[0] != e:
            pairs.append((bounds[0], bounds[0] - 1))
    groups = [e for e in range(4, n, 4) if e % per_split]
    if groups:
        e = groups[-1]
        pairs += [(e - 1, e), (e, e - 1)]
    return [(a, b) for a, b in pairs if a != b]


def placement_column(n, j, a, b, rng):
    """n distinct values on both sides of zero in random order, but s_(j) in frame a and s_(j+1) in frame b (s_(j-1) at
    j = n - 1)."""
    vals = ((np.arange(n) - 0.37 * n + rng.uniform(-0.3, 0.3, n)) * 0.01).astype(F)
    j1 = j + 1 if j + 1 < n else j - 1
    ranks = np.empty(n, int)
    ranks[a], ranks[b] = j, j1
    rest = np.array([f for f in range(n) if f not in (a, b)], int)
    ranks[rest] = rng.permutation([r for r in range(n) if r not in (j, j1)])
    return vals[ranks]


def random_column(n, rng, k):
    """Finite values of a random magnitude; every third column rounded so that it has ties (and no zero: the fold's sample
    of a zero does not keep its sign)."""
    c = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-3, 3)
    if k % 3 == 0:
        c = np.round(c, 1)
        c[c == 0] = 0.1
    return c.astype(F)


def plain_stack(n, cn=1):
    """(frames n x H x W x cn, planted): one column per quantile of QUANTILES and pair of placement_pairs with that
    quantile's s_(j) and s_(j+1) planted, random finite columns in the other pixel-channels. planted: (column, index into
    QUANTILES, j, a, b) each; column k is pixel-channel k of the frame in memory order."""
    rng = np.random.default_rng(1000 + 8 * n + cn)
    m = H * W * cn
    cols, planted = [], []
    for qi, q in enumerate(QUANTILES):
        j, _ = rank_of(n, q)
        for a, b in placement_pairs(n):
            planted.append((len(cols), qi, j, a, b))
            cols.append(placement_column(n, j, a, b, rng))
    assert len(cols) <= m
    while len(cols) < m:
        cols.append(random_column(n, rng, len(cols)))
    return np.stack(cols, axis=1).reshape(n, H, W, cn), planted


def frame_orders(n):
    """The frame orders of the metamorphic check: reversed, rotated by one, random."""
    rng = np.random.default_rng(n)
    orders = {"reversed": np.arange(n)[::-1].copy(), "rotated": np.roll(np.arange(n), 1), "random": rng.permutation(n)}
    while n >= 4 and any(np.array_equal(orders["random"], o) for o in (np.arange(n), orders["reversed"], orders["rotated"])):
        orders["random"] = rng.permutation(n)
    return orders


# ---- adversarial values -----------------------------------------------------------------------------------------------
ADVERSARIAL_BORDER = -0.0
LATTICE = [(y, x) for y in range(0, H, 2) for x in range(0, W, 2)]


def adversarial_columns(n, rng):
    """{name: column of n samples}."""
    fmax, inf, nan = np.finfo(F).max, F(np.inf), F(np.nan)

    def cyc(values):
        return rng.permutation(np.resize(np.asarray(values, F), n))

    def two(k):                                          # k samples of the lower value, n - k of the upper one
        return rng.permutation(np.where(np.arange(n) < k, F(0.25), F(0.75)).astype(F))

    def noise():
        return rng.normal(0, 1, n).astype(F)

    def with_value(col, at, v):
        col[at] = v
        return col

    one = F(1)
    P = {}
    P["zeros"] = cyc([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40])
    P["huge"] = cyc([fmax, -fmax, inf, -inf, 1.0, -2.0])
    P["ulp+"] = cyc([np.nextafter(one, F(0)), one, np.nextafter(one, F(2))])
    P["ulp-"] = cyc([-np.nextafter(one, F(0)), -one, -np.nextafter(one, F(2))])
    P["equal"] = np.full(n, 0.3, F)
    for q in (0.5, 0.73):
        j, _ = rank_of(n, q)
        P[f"two:{q}:j+1"] = two(j + 1)                   # s_(j) is the lower value, s_(j+1) the upper one
        P[f"two:{q}:j"] = two(j)                         # s_(j) is the upper value already
    P["ramp"] = ((n - np.arange(n)) * 0.125).astype(F)
    P["nan-last"] = with_value(noise(), n - 1, nan)
    P["nan-first"] = with_value(noise(), 0, nan)
    P["+inf"] = with_value(noise(), int(rng.integers(n)), inf)
    P["-inf"] = with_value(noise(), int(rng.integers(n)), -inf)
    return P


def adversarial_stack(n):
    """(frames n x H x W x 1, where): every pattern of adversarial_columns in a pixel of its own on the lattice of even rows
    and columns (`where`: name -> (y, x)), random finite columns on the rest of the lattice, -0.0 off it. Sampled by the
    4-weight path under BORDER_CONSTANT -0.0, a lattice pixel's three zero-weight taps are all -0.0, so its sample is the
    frame's value bit for bit, infinities, NaNs and the sign of a zero included (shifted_samples, classic)."""
    rng = np.random.default_rng(2000 + n)
    frames = np.full((n, H, W, 1), -0.0, F)
    cols = adversarial_columns(n, rng)
    assert len(cols) <= len(LATTICE)
    where = {}
    for k, (y, x) in enumerate(LATTICE):
        if k < len(cols):
            name = list(cols)[k]
            frames[:, y, x, 0] = cols[name]
            where[name] = (y, x)
        else:
            frames[:, y, x, 0] = random_column(n, rng, 1)
    return frames, where


# ---- participation: every pixel its own N_p ------------------------------------------------------------------------------
NAN_BITS = [0x7fc00000, 0xffffffff, 0x7fa00000, 0xffa00000, 0x7f800001]


def translation_table(n):
    """(shifts n x (tx, ty), weights n): integer translations that push the frames progressively out of view to the left and
    up, so that the pixels of the right and lower rim lose them one by one, and a few zero weights. The last frame moves by
    one pixel, frame 0 by two and every other frame by three or more: the last column is covered by nobody, the one before
    by frame n - 1 alone, the next by the two."""
    sh = np.zeros((n, 2), int)
    wt = np.ones(n, F)
    for i in range(n):
        sh[i] = (3 + i % 10, (i // 3) % H)
    sh[0] = (2, 0)
    sh[n - 1] = (1, 1 if n > 1 else 0)               # (the lowest row does without the last frame)
    if n >= 8:
        wt[[i for i in range(1, n - 1) if i % 7 == 3 and i % 32 not in (0, 31)]] = 0.0      # (none next to a split boundary)
    return sh, wt


def masked_stack(n, cn=1):
    """The stack of the participation tests: dict of frames (n x H x W x cn f32: one scene in destination coordinates, noise
    and ~3 % outliers, so that the clip has something to reject), shifts, warps, weights, gain and offset (n x cn), and the
    model's samples (n x H x W x cn) and participation flags (n x H x W, weight > 0 included). From 33 samples on the five
    NaN payloads of NAN_BITS sit in frames of different lane splits, each in a pixel of the lower left that its frame
    covers."""
    rng = np.random.default_rng(3000 + 8 * n + cn)
    sh, wt = translation_table(n)
    scene = rng.uniform(0.2, 0.8, (H, W, cn))
    frames = rng.uniform(0, 1, (n, H, W, cn)).astype(F)
    for i in range(n):
        d = np.clip(scene + rng.normal(0, 0.03, scene.shape), 0, 1)
        d[rng.random((H, W)) < 0.03] = rng.choice([0.0, 1.0])
        tx, ty = sh[i]
        frames[i, ty:, tx:] = d[:H - ty, :W - tx].astype(F)
    nans = []
    if n >= 33:
        per_split, last = split_of(n)
        # (not the top left corner, the one pixel every live frame covers, nor a pixel whose zero-weight taps it holds)
        free = [(y, x) for y in (4, 2) for x in (0, 3, 6)]
        free += [(y, x) for y in range(H - 1, -1, -1) for x in range(W) if (y, x) not in free and (y > 1 or x > 1)]
        for bits, i in zip(NAN_BITS, (0, n - 1, per_split - 1, per_split, n // 2)):
            while wt[i] == 0:
                i += 1
            tx, ty = sh[i]
            y, x = next((y, x) for y, x in free if y + ty < H and x + tx < W)
            free.remove((y, x))
            frames[i].view(np.uint32)[y + ty, x + tx, 0] = bits
            nans.append((i, y, x))
    samples, inside = shifted_samples(frames, sh)
    part = inside & (wt > 0)[:, None, None]
    warps = []
    for tx, ty in sh:
        M = np.eye(3)
        M[0, 2], M[1, 2] = -tx, -ty                      # frame -> destination: the fold samples through the inverse
        warps.append(M)
    gain = rng.uniform(0.9, 1.1, (n, cn)).astype(F)
    offset = rng.uniform(-0.02, 0.02, (n, cn)).astype(F)
    return dict(frames=frames, shifts=sh, warps=warps, weights=wt, gain=gain, offset=offset, samples=samples, part=part, nans=nans)


def check_participation(n, part, weights, clean=None):
    """The conditions the participation tests put on their inputs, from the flags alone (n x H x W). N_p takes the values 0,
    1, 2 (those the live count allows), a value in [3, live) where there is one, and the live count itself. With the keys
    on more than one lane split: some pixel that has samples has absent entries in two different splits, and some pixel's
    samples lie all in the last split. Each of them at a pixel of `clean` (H x W; default: any), the pixels without a NaN
    among their samples. Returns N_p."""
    live = int((np.asarray(weights) > 0).sum())
    n_p = part.sum(axis=0)
    clean = np.ones(n_p.shape, bool) if clean is None else clean
    for v in (0, 1, 2):
        assert v > live or ((n_p == v) & clean).any(), (n, v)
    assert live <= 3 or ((n_p >= 3) & (n_p < live) & clean).any(), n
    assert ((n_p == live) & clean).any(), n
    per_split, last = split_of(n)
    if last >= 1:
        split = np.arange(n) // per_split
        absent_splits = np.stack([(~part[split == s]).any(axis=0) for s in range(last + 1)]).sum(axis=0)
        assert ((absent_splits >= 2) & (n_p > 0) & clean).any(), n
        assert ((n_p > 0) & ~part[split != last].any(axis=0) & clean).any(), n
    return n_p

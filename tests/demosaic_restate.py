"""Colour-filter mosaics in numpy: a vectorised restatement of include/stacker.h, stk_mosaic, that the engine equals bit
for bit (tests/test_gpu_demosaic.py) and that a scalar loop written from the same text equals (tests/test_cpu_demosaic.py).
Integer mosaics run in int64 (every sum fits int32: see test_cpu_demosaic.py), f32 mosaics in float32 arrays, where numpy
rounds every operation on its own, in the order the header fixes."""
import numpy as np

F = np.float32
RGGB, GRBG, GBRG, BGGR = range(4)
BILINEAR, MHC, HA, SUPERPIXEL = range(4)
PATTERNS = (RGGB, GRBG, GBRG, BGGR)
METHODS = (BILINEAR, MHC, HA, SUPERPIXEL)
CELLS = {RGGB: (2, 1, 1, 0), GRBG: (1, 2, 0, 1), GBRG: (1, 0, 2, 1), BGGR: (0, 1, 1, 2)}     # channel (0 B, 1 G, 2 R) of the cell's samples
DTYPES = {8: np.uint8, 16: np.uint16, 32: F}
REACH = 3


def colour(pattern, x, y):
    """Channel (0 = B, 1 = G, 2 = R) of pixel (x, y); x, y scalars or arrays."""
    return np.asarray(CELLS[pattern])[(np.asarray(y) & 1) * 2 + (np.asarray(x) & 1)]


def colours(pattern, h, w):
    return colour(pattern, np.arange(w)[None, :], np.arange(h)[:, None])


def cfa_mask(w, h, pattern, channel):
    return (colours(pattern, h, w) == channel).astype(F)


def mosaic_of(bgr, pattern):
    """The mosaic a sensor of this pattern sees of an H x W x 3 B G R image."""
    h, w = bgr.shape[:2]
    return np.take_along_axis(bgr, colours(pattern, h, w)[..., None], 2)[..., 0]


def reflect(i, n):
    """BORDER_REFLECT_101, applied until the index is inside."""
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def finish(S, k, integer, out_depth):
    """Numerator S over 2^k as output samples."""
    if not integer:
        return S if k == 0 else S * F(1.0 / (1 << k))
    if out_depth == 32:
        return S.astype(F) * F(1.0 / (1 << k))
    hi = 255 if out_depth == 8 else 65535
    return np.clip((S + ((1 << k) >> 1)) >> k, 0, hi).astype(DTYPES[out_depth])


def g8_plane(P):
    """Hamilton-Adams green in eighths by the R / B formula at every position of the padded plane P that is at least 2 inside."""
    c = P[2:-2, 2:-2]
    W, E, N, S = P[2:-2, 1:-3], P[2:-2, 3:-1], P[1:-3, 2:-2], P[3:-1, 2:-2]
    two = P.dtype.type(2)
    tH = (two * c - P[2:-2, :-4]) - P[2:-2, 4:]
    tV = (two * c - P[:-4, 2:-2]) - P[4:, 2:-2]
    dH = np.abs(W - E) + np.abs(tH)
    dV = np.abs(N - S) + np.abs(tV)
    gH = two * (W + E) + tH
    gV = two * (N + S) + tV
    return np.where(dH < dV, two * gH, np.where(dV < dH, two * gV, gH + gV))


def demosaic_one(mosaic, pattern, method, out_depth=None):
    """One H x W mosaic as H x W x 3 (SUPERPIXEL: H/2 x W/2 x 3) B G R of out_depth (None: the mosaic's)."""
    mosaic = np.asarray(mosaic)
    h, w = mosaic.shape
    integer = mosaic.dtype != F
    depth = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16, np.dtype(F): 32}[mosaic.dtype]
    od = depth if out_depth is None else out_depth
    assert od in (depth, 32)
    A = np.int64 if integer else F
    T = A
    with np.errstate(invalid="ignore", over="ignore"):
        if method == SUPERPIXEL:
            assert w >= 2 and h >= 2
            m = mosaic[:h // 2 * 2, :w // 2 * 2].astype(A)
            cell = [m[0::2, 0::2], m[0::2, 1::2], m[1::2, 0::2], m[1::2, 1::2]]
            col = CELLS[pattern]
            greens = [cell[k] for k in range(4) if col[k] == 1]
            out = np.empty((h // 2, w // 2, 3), DTYPES[od])
            out[..., 0] = finish(cell[col.index(0)], 0, integer, od)
            out[..., 1] = finish(greens[0] + greens[1], 1, integer, od)
            out[..., 2] = finish(cell[col.index(2)], 0, integer, od)
            return out
        assert w >= 3 and h >= 3
        R = REACH
        P = np.pad(mosaic.astype(A), R, mode="reflect")            # numpy's "reflect" is BORDER_REFLECT_101, repeated as needed
        sh = lambda dy, dx: P[R + dy:R + dy + h, R + dx:R + dx + w]
        c = sh(0, 0)
        k = lambda v: T(v)
        h1, v1 = sh(0, -1) + sh(0, 1), sh(-1, 0) + sh(1, 0)
        d = (sh(-1, -1) + sh(-1, 1)) + (sh(1, -1) + sh(1, 1))
        if method == BILINEAR:
            green_rb, opp_rb, row_g, col_g = (v1 + h1, 2), (d, 2), (h1, 1), (v1, 1)
        elif method == MHC:
            h2, v2 = sh(0, -2) + sh(0, 2), sh(-2, 0) + sh(2, 0)
            x1, x2 = v1 + h1, v2 + h2
            green_rb = (k(8) * c + k(4) * x1 - k(2) * x2, 4)
            opp_rb = (k(12) * c + k(4) * d - k(3) * x2, 4)
            row_g = (k(10) * c + k(8) * h1 - k(2) * d - k(2) * h2 + v2, 4)
            col_g = (k(10) * c + k(8) * v1 - k(2) * d - k(2) * v2 + h2, 4)
        else:
            G8full = g8_plane(P)                                   # positions -1 .. h, -1 .. w: the formula on the reflected mosaic
            g8 = lambda dy, dx: G8full[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            d8 = lambda dy, dx: k(8) * sh(dy, dx) - g8(dy, dx)     # meaningful at R / B positions, read only there
            G8g = k(8) * c
            green_rb = (g8(0, 0), 3)
            opp_rb = ((k(4) * g8(0, 0) + (d8(-1, -1) + d8(-1, 1))) + (d8(1, -1) + d8(1, 1)), 5)
            row_g = ((k(2) * G8g + d8(0, -1)) + d8(0, 1), 4)
            col_g = ((k(2) * G8g + d8(-1, 0)) + d8(1, 0), 4)
        fin = lambda pair: finish(pair[0], pair[1], integer, od)
        own, green_rb, opp_rb, row_g, col_g = finish(c, 0, integer, od), fin(green_rb), fin(opp_rb), fin(row_g), fin(col_g)
    col = colours(pattern, h, w)
    red_rows = (np.arange(h)[:, None] & 1) == (pattern >> 1)       # rows that hold red sites
    out = np.empty((h, w, 3), DTYPES[od])
    is_g = col == 1
    out[..., 1] = np.where(is_g, own, green_rb)
    out[..., 2] = np.where(col == 2, own, np.where(col == 0, opp_rb, np.where(red_rows, row_g, col_g)))
    out[..., 0] = np.where(col == 0, own, np.where(col == 2, opp_rb, np.where(red_rows, col_g, row_g)))
    return out


def demosaic(mosaics, pattern, method, out_depth=None):
    return np.stack([demosaic_one(m, pattern, method, out_depth) for m in mosaics])


def same_bits(a, b):
    """Equal as bytes where finite; NaN exactly where the other has NaN (any payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != F:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))

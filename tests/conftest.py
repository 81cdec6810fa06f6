import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def assert_stack_close(out, ref, bulk=4e-6):
    """Stacked image vs the oracle's when the warps agree to round-off but are not bit-identical (H to ~1e-8 relative, ECC
    warps to 1-2 f32 ulp): the warp kernels work from the f32 inverse matrix, so one ulp of an entry moves the sample
    position by ~1e-4 px at x ~ 2000 and a high-contrast edge pixel by ~1e-5. Bar: the north-star tolerance everywhere
    (max |a - b| <= 1e-4 * max |b|), and f32 fold round-off (`bulk`, 1e-6 per folded frame) for 99.9 % of the samples."""
    d = np.abs(np.asarray(out, np.float64) - np.asarray(ref, np.float64))
    assert d.max() <= 1e-4 * np.abs(ref).max(), d.max()
    assert np.percentile(d, 99.9) <= bulk, np.percentile(d, 99.9)


def interior_mask(shape_hw, warps, margin=2):
    """Pixels at least `margin` px inside EVERY frame's warped border (SURVEY 8d's evaluation region)."""
    import oracle
    from scipy.ndimage import binary_erosion
    h, w = shape_hw
    ones = np.full((h, w, 1), 255, np.uint8)
    m = np.ones((h, w), bool)
    for W in warps:
        W = np.asarray(W, np.float64).reshape(-1)
        is_affine = W.size == 6
        cov = oracle.warp_frame(ones, W.reshape(2, 3) if is_affine else W.reshape(3, 3), is_affine=is_affine)[..., 0]
        m &= cov >= 1.0 - 1e-6
    return binary_erosion(m, structure=np.ones((2 * margin + 1, 2 * margin + 1), bool), border_value=0)


def ecc_stack_error(out, ref, frames, warps, alpha=1.0 / 255.0):
    """(max relative error of `out` vs the oracle's stack `ref` over the interior, the oracle's own 1-ulp floor).

    Relative error as SURVEY 8d defines it: |a - b| / max(|b|, 1e-3), MAX over pixels >= 2 px from every warped border.
    The floor: the same quantity between `ref` and the oracle's fold of the same frames with every entry of its own f32
    warps moved by one ulp (seeded signs) — what the last bit of findTransformECC's f32 result is worth in the image."""
    import oracle
    n = len(frames)
    h, w = ref.shape[:2]
    m = interior_mask((h, w), [warps[i] for i in range(1, n)])
    rel = (np.abs(out.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-3))[m]
    rng = np.random.default_rng(7)
    acc = oracle.warp_frame(frames[0], np.eye(3), alpha=alpha)
    for i in range(1, n):
        W = np.asarray(warps[i], np.float32)
        Wp = np.nextafter(W, np.where(rng.integers(0, 2, W.shape) > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        if W.shape[0] == 3:
            Wp[2, 2] = W[2, 2]
        acc = oracle.warp_frame(frames[i], Wp.astype(np.float64), is_affine=W.shape[0] == 2, alpha=alpha, acc=acc)
    pert = oracle.scale(acc, n)
    floor = (np.abs(pert.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-3))[m]
    return float(rel.max()), float(floor.max())


ECC_FLOOR_FACTOR = 1.3


def assert_ecc_stack_close(out, ref, frames, warps, alpha=1.0 / 255.0, label="", iters=None, iters_ref=None, bar=1e-4):
    """North-star bar for the end-to-end ECC stack: MAX relative error <= 1e-4 over the interior, or — on frames wide
    enough that one f32 ulp of the warp matrix moves a sample by more than that is worth (x ~ 2000: 1.2e-4 px) — <= 1.3 x
    the oracle's own 1-ulp floor (round 4; it was 3 x. Measured: 1.24 x the floor at 1080p, 2.1e-4 against 1.7e-4, and
    0.79 x at 4K, 4.8e-4 against 6.1e-4: 1.25 would leave the 1080p stack 1 % of room).
    `iters` / `iters_ref`, when given, must be EQUAL: the test stacks are seeded and the engine is deterministic, so a
    count that differs from the oracle's is a regression, not a tolerance (round 3 switched to a 0.05 bar then).
    Prints the error under both readings of "relative": per pixel, |a - b| / max(|b|, 1e-3) (the one asserted),
    and against the image's range, max |a - b| / max |b|. `bar`: 1e-4 (the north star) unless the caller states another."""
    err, floor = ecc_stack_error(out, ref, frames, warps, alpha)
    if iters is not None:
        assert [int(a) for a in iters] == [int(b) for b in iters_ref], ("iteration counts differ from the oracle's", list(iters), list(iters_ref))
    n = len(frames)
    m = interior_mask(ref.shape[:2], [warps[i] for i in range(1, n)])
    d = np.abs(np.asarray(out, np.float64) - ref)[m]
    range_rel = float(d.max() / np.abs(ref).max())
    print("%s ecc stack: max |a-b|/max(|b|,1e-3) %.3e (oracle 1-ulp floor %.3e = %.2f x), max |a-b|/max|b| %.3e"
          % (label, err, floor, err / max(floor, 1e-30), range_rel))
    assert err <= max(bar, ECC_FLOOR_FACTOR * floor), (err, floor)
    return err, floor


@pytest.fixture(scope="session")
def stacker():
    """One stk_ctx on cuda:0 for the whole GPU session (fails loudly without the HIP library)."""
    from libstacker_rs_amd import Stacker
    s = Stacker(0)
    yield s
    s.close()


@pytest.fixture(scope="session")
def small_stack():
    """4 x 320x240 synthetic BGR u8 frames + ground-truth homographies (seeded)."""
    from libstacker_rs_amd import synth
    frames, G = synth.make_stack(4, 320, 240)
    return frames.numpy(), G


def _write_png(path, img, palette=None, bits=None):
    """Minimal PNG writer (zlib + CRC), no gamma chunk: 8- or 16-bit grey (HxW), RGB (HxWx3, given as BGR) or RGBA (HxWx4);
    `palette` (Nx3 RGB, uint8): HxW indices as a colour-type-3 image; `bits` in (1, 2, 4): HxW grey values < 2**bits packed."""
    import struct
    import zlib
    a = np.asarray(img)
    h, w = a.shape[:2]
    extra = b""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    if palette is not None:
        depth, ctype = 8, 3
        rows = [np.ascontiguousarray(a[y].astype(np.uint8)).tobytes() for y in range(h)]
        extra = chunk(b"PLTE", np.ascontiguousarray(np.asarray(palette, np.uint8)).tobytes())
    elif bits in (1, 2, 4):
        depth, ctype = bits, 0
        per = 8 // bits
        rows = []
        for y in range(h):
            v = np.zeros(-(-w // per) * per, np.uint8)
            v[:w] = a[y]
            v = v.reshape(-1, per)
            rows.append(np.sum(v.astype(np.uint16) << (bits * (per - 1 - np.arange(per))), axis=1).astype(np.uint8).tobytes())
    else:
        assert a.dtype in (np.uint8, np.uint16)
        if a.ndim == 3 and a.shape[2] == 3:
            a = a[..., ::-1]                                 # BGR in memory -> RGB on disk
        depth = a.dtype.itemsize * 8
        ctype = {2: 0, 3: 2, 4: 6}[2 if a.ndim == 2 else a.shape[2]]
        rows = [np.ascontiguousarray(a[y]).astype(">u%d" % a.dtype.itemsize).tobytes() for y in range(h)]   # big-endian samples
    raw = b"".join(b"\x00" + r for r in rows)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) + extra +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


@pytest.fixture(scope="session")
def write_png():
    """Writer of small test PNGs (no Pillow in the main interpreter)."""
    return _write_png


def _write_tiff(path, img):
    """Minimal baseline TIFF writer: little-endian, uncompressed, one strip; 8/16-bit grey (HxW) or RGB (HxWx3 given as BGR)."""
    import struct
    a = np.asarray(img)
    assert a.dtype in (np.uint8, np.uint16)
    if a.ndim == 3:
        a = a[..., ::-1]
    h, w = a.shape[:2]
    spp = 1 if a.ndim == 2 else 3
    bps = a.dtype.itemsize * 8
    data = np.ascontiguousarray(a).astype("<u%d" % a.dtype.itemsize).tobytes()
    n_tags = 10
    ifd_ofs = 8
    bps_ofs = ifd_ofs + 2 + 12 * n_tags + 4
    data_ofs = bps_ofs + 8
    def tag(t, typ, count, value):
        return struct.pack("<HHII", t, typ, count, value)
    ifd = struct.pack("<H", n_tags)
    ifd += tag(256, 4, 1, w) + tag(257, 4, 1, h)
    ifd += tag(258, 3, spp, bps_ofs if spp == 3 else bps)
    ifd += tag(259, 3, 1, 1) + tag(262, 3, 1, 2 if spp == 3 else 1)
    ifd += tag(273, 4, 1, data_ofs) + tag(277, 3, 1, spp) + tag(278, 4, 1, h) + tag(279, 4, 1, len(data)) + tag(284, 3, 1, 1)
    ifd += struct.pack("<I", 0)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd_ofs) + ifd + struct.pack("<HHHH", bps, bps, bps, 0) + data)


def _write_tiff_tiled(path, img, tile=(16, 16)):
    """Tiled baseline TIFF (little-endian, uncompressed): 8/16-bit grey (HxW), RGB (HxWx3 given as BGR) or RGBA (HxWx4 given as BGRA)."""
    import struct
    a = np.asarray(img)
    if a.ndim == 3:
        a = a[..., [2, 1, 0] + ([3] if a.shape[2] == 4 else [])]
    h, w = a.shape[:2]
    spp = 1 if a.ndim == 2 else a.shape[2]
    bps = a.dtype.itemsize * 8
    tw, th = tile
    tiles = []
    for y0 in range(0, h, th):
        for x0 in range(0, w, tw):
            t = np.zeros((th, tw) + a.shape[2:], a.dtype)
            blk = a[y0:y0 + th, x0:x0 + tw]
            t[:blk.shape[0], :blk.shape[1]] = blk
            tiles.append(t.astype("<u%d" % a.dtype.itemsize).tobytes())
    nt = len(tiles)
    tags = []
    def tag(t, typ, count, value):
        tags.append(struct.pack("<HHII", t, typ, count, value))
    n_tags = 12 + (1 if spp == 4 else 0)
    ifd_ofs = 8
    extra_ofs = ifd_ofs + 2 + 12 * n_tags + 4
    bps_ofs = extra_ofs
    offs_ofs = bps_ofs + 8
    cnts_ofs = offs_ofs + 4 * nt
    data_ofs = cnts_ofs + 4 * nt
    tag(256, 4, 1, w); tag(257, 4, 1, h)
    tag(258, 3, spp, bps_ofs if spp > 2 else bps)
    tag(259, 3, 1, 1); tag(262, 3, 1, 2 if spp >= 3 else 1)
    tag(277, 3, 1, spp); tag(284, 3, 1, 1)
    tag(322, 4, 1, tw); tag(323, 4, 1, th)
    tag(324, 4, nt, offs_ofs if nt > 1 else data_ofs)
    tag(325, 4, nt, cnts_ofs if nt > 1 else len(tiles[0]))
    if spp == 4:
        tag(338, 3, 1, 2)                                  # EXTRASAMPLES: unassociated alpha
    tag(339, 3, 1, 1)                                      # SAMPLEFORMAT uint
    assert len(tags) == n_tags
    offs, o = [], data_ofs
    for t in tiles:
        offs.append(o); o += len(t)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd_ofs) + struct.pack("<H", n_tags) + b"".join(tags) + struct.pack("<I", 0))
        f.write(struct.pack("<HHHH", bps, bps, bps, bps))
        f.write(struct.pack("<%dI" % nt, *offs) + struct.pack("<%dI" % nt, *[len(t) for t in tiles]))
        f.write(b"".join(tiles))


def _write_bmp(path, img, palette=None, top_down=False):
    """Uncompressed BMP: HxWx3 (BGR, 24 bit), HxWx4 (BGRA, 32 bit) or HxW indices with an Nx3 BGR palette (8 bit)."""
    import struct
    a = np.asarray(img, np.uint8)
    h, w = a.shape[:2]
    bpp = 8 if a.ndim == 2 else a.shape[2] * 8
    row = ((w * bpp + 31) // 32) * 4
    rows = []
    for y in (range(h) if top_down else range(h - 1, -1, -1)):
        r = np.ascontiguousarray(a[y]).tobytes()
        rows.append(r + b"\0" * (row - len(r)))
    pal = b""
    if bpp == 8:
        pal = b"".join(bytes([int(c[0]), int(c[1]), int(c[2]), 0]) for c in np.asarray(palette, np.uint8))
    ofs = 14 + 40 + len(pal)
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", ofs + row * h, 0, 0, ofs))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, -h if top_down else h, 1, bpp, 0, row * h, 2835, 2835, len(pal) // 4, 0))
        f.write(pal + b"".join(rows))


_JPEG_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
_JPEG_CHROM = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
_ZIGZAG = sorted(range(64), key=lambda k: (k // 8 + k % 8, k // 8 if (k // 8 + k % 8) % 2 else -(k // 8)))


def _write_jpeg(path, img, quality=90, subsampling="420"):
    """Minimal baseline JPEG writer (JFIF, no restart markers): 8-bit grey (HxW) or colour (HxWx3 given as BGR) with
    chroma 4:4:4 or 4:2:0 (2 x 2 mean). The Annex K quantisation tables scaled by `quality` as libjpeg scales them;
    flat Huffman tables (every DC category a 4-bit code, every AC run/size symbol an 8-bit one): valid, if a little
    larger than the standard ones."""
    import struct
    a = np.asarray(img, np.uint8)
    h, w = a.shape[:2]
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    qt = [np.clip((np.array(t) * scale + 50) // 100, 1, 255) for t in (_JPEG_LUM, _JPEG_CHROM)]
    if a.ndim == 2:
        planes, samp, mcu = [a.astype(np.float64)], [1], 8
    else:
        b, g, r = (a[..., i].astype(np.float64) for i in range(3))
        planes = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128,
                  0.5 * r - 0.418688 * g - 0.081312 * b + 128]
        samp, mcu = ([2, 1, 1], 16) if subsampling == "420" else ([1, 1, 1], 8)
    H, W = -(-h // mcu) * mcu, -(-w // mcu) * mcu
    u = np.arange(8)
    C = np.sqrt(2 / 8) * np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16)
    C[0] /= np.sqrt(2)
    coefs = []                                               # per component: (blocks down, blocks across, 64) in zigzag order
    for c, p in enumerate(planes):
        p = np.pad(p, ((0, H - h), (0, W - w)), mode="edge")
        f = mcu // 8 // samp[c]
        if f > 1:
            p = p.reshape(H // f, f, W // f, f).mean(axis=(1, 3))
        blk = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3) - 128.0
        q = np.round(C @ blk @ C.T / qt[min(c, 1)].reshape(8, 8)).astype(np.int64)
        coefs.append(q.reshape(q.shape[0], q.shape[1], 64)[..., _ZIGZAG])
    ac_syms = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    ac_code = {s: i for i, s in enumerate(ac_syms)}
    vals, lens = [], []

    def put(v, n):
        if n:
            vals.append(v); lens.append(n)

    def amp(v):
        s = int(abs(v)).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    pred = [0] * len(planes)
    for my in range(H // mcu):
        for mx in range(W // mcu):
            for c, zz in enumerate(coefs):
                for dy in range(samp[c]):
                    for dx in range(samp[c]):
                        z = zz[my * samp[c] + dy, mx * samp[c] + dx].tolist()
                        s, v = amp(z[0] - pred[c])
                        pred[c] = z[0]
                        put(s, 4); put(v, s)
                        last = 0
                        for k in np.flatnonzero(z[1:]).tolist():
                            run = k - last
                            while run > 15:
                                put(ac_code[0xF0], 8); run -= 16
                            s, v = amp(z[k + 1])
                            put(ac_code[(run << 4) | s], 8); put(v, s)
                            last = k + 1
                        if last != 63:
                            put(ac_code[0x00], 8)
    vals, lens = np.array(vals, np.int64), np.array(lens, np.int64)
    idx = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    bits = (vals[idx] >> (lens[idx] - 1 - pos)) & 1
    data = np.packbits(np.concatenate([bits, np.ones(-len(bits) % 8, np.int64)]).astype(np.uint8))
    data = np.insert(data, np.flatnonzero(data == 0xFF) + 1, 0)   # byte stuffing

    def seg(marker, body):
        return struct.pack(">HH", marker, len(body) + 2) + body
    nq = 1 if len(planes) == 1 else 2
    out = b"\xff\xd8" + seg(0xFFE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xFFDB, b"".join(bytes([i]) + bytes(qt[i].astype(np.uint8)[_ZIGZAG].tolist()) for i in range(nq)))
    out += seg(0xFFC0, struct.pack(">BHHB", 8, h, w, len(planes)) +
               b"".join(bytes([c + 1, (samp[c] << 4) | samp[c], min(c, 1)]) for c in range(len(planes))))
    dc_counts, ac_counts = [0] * 16, [0] * 16
    dc_counts[3], ac_counts[7] = 12, len(ac_syms)
    out += seg(0xFFC4, bytes([0x00] + dc_counts + list(range(12))) + bytes([0x10] + ac_counts + ac_syms))
    out += seg(0xFFDA, bytes([len(planes)]) + b"".join(bytes([c + 1, 0x00]) for c in range(len(planes))) + bytes([0, 63, 0]))
    with open(path, "wb") as f:
        f.write(out + data.tobytes() + b"\xff\xd9")


@pytest.fixture(scope="session")
def write_jpeg():
    """Writer of test JPEGs (baseline, Huffman-coded; no encoder in the main interpreter)."""
    return _write_jpeg


@pytest.fixture(scope="session")
def write_tiff_tiled():
    return _write_tiff_tiled


@pytest.fixture(scope="session")
def write_bmp():
    return _write_bmp


@pytest.fixture(scope="session")
def write_tiff():
    """Writer of small test TIFFs (no Pillow in the main interpreter)."""
    return _write_tiff

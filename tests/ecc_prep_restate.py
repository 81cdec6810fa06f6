"""What ECC preparation must hand to the iteration kernels, restated from the oracle and numpy, and the table of cases the
CPU and GPU tests of that stage share (test_cpu_ecc_prep.py, test_gpu_ecc_prep.py). No GPU is needed for this file.

The stage (stacker.cpp: ecc_shard_impl, stk_find_transform_ecc; kernels_prep.hip):
  template i - 1 = GaussianBlur(float(grey(frame i)), g x g)            one f32 plane per moving frame
  I = the same of frame 0; gx, gy its central differences (REFLECT_101); interleaved (gx, gy) and (I, gx, gy) copies;
      the five planes carry a zero border of REF_PAD pixels that is written once per geometry
with, under scale_down_width, cv::resize(INTER_AREA) between grey and blur. Which KERNEL writes a template depends on the
frames' layout, on how the stack is cut into runs and on options: route_model restates that from the code, so that a case
which means to test the streaming kernel cannot pass on the per-frame fall-back (stk_get_counter "prep_stream_frames")."""
import functools
from collections import namedtuple

import numpy as np

import oracle

# kernels_prep.hip: output quads (4 px) per wave, waves per workgroup, output rows per segment, rows prefetched
GS_QW, GS_WAVES, GS_SEG, GS_PF = 62, 4, 32, 4
WAVE_PX, GROUP_PX = 4 * GS_QW, 4 * GS_QW * GS_WAVES          # 248, 992
PREP_RUN = 16                                                # ecc_shard_impl: frames per run of an overlapped preparation
UPLOAD_BATCH_DEFAULT = 8                                     # context.h: opt_upload_batch


# ---- expected planes ---------------------------------------------------------------------------------------------------
def _reflect101(p, n):
    p = np.asarray(p)
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p)
    return np.where(p >= n, 2 * n - 2 - p, p)


def gradients(I):
    """gx = -0.5 I[x - 1] + 0.5 I[x + 1], gy likewise down the columns, BORDER_REFLECT_101, in float32. Both products are
    exact (a power of two), so the sum rounds once whether or not a compiler fuses it: expected bit for bit."""
    I = np.asarray(I, np.float32)
    h, w = I.shape
    xs, ys = np.arange(w), np.arange(h)
    half = np.float32(0.5)
    gx = (-half * I[:, _reflect101(xs - 1, w)]) + (half * I[:, _reflect101(xs + 1, w)])
    gy = (-half * I[_reflect101(ys - 1, h), :]) + (half * I[_reflect101(ys + 1, h), :])
    return gx.astype(np.float32), gy.astype(np.float32)


def grey_of(frame):
    """cvtColor(BGR2GRAY) of a frame in its own depth; BGRA gives the grey of its BGR part; a single plane is itself."""
    f = np.asarray(frame)
    if f.ndim == 2:
        return f
    return oracle.grey(np.ascontiguousarray(f[..., :3]))


def expected_planes(frames, gauss, scale_down_width=None):
    """{"templates" [n - 1, h, w], "I", "gx", "gy" [h, w]} (no border) of a stack, from the oracle and numpy only."""
    planes = []
    for f in frames:
        g = grey_of(f)
        if scale_down_width:
            ew, eh = oracle.scaled_size(g.shape[1], g.shape[0], float(scale_down_width))
            g = oracle.resize_area_f32(g, ew, eh) if g.dtype == np.float32 else oracle.resize_area_u8(g, ew, eh)
        planes.append(oracle.gaussian_blur_f32(g.astype(np.float32), gauss))
    I = planes[0]
    gx, gy = gradients(I)
    templates = np.stack(planes[1:]) if len(planes) > 1 else np.empty((0,) + I.shape, np.float32)
    return {"templates": templates, "I": I, "gx": gx, "gy": gy}


# ---- which kernel writes a template ------------------------------------------------------------------------------------
def effective_slots(n_templates, w, h, ecc_slots=0):
    """ecc_plan: frames in flight. 0 = auto: frames up to 1080p go through at most 64 slots in equal rounds."""
    slots = ecc_slots
    if slots <= 0:
        nt = max(n_templates, 1)
        if w * h <= 1920 * 1088:
            rounds = (nt + 63) // 64
            slots = (nt + rounds - 1) // rounds
        elif nt <= 128:
            slots = nt
        else:
            rounds = max(3, (nt + 95) // 96)
            slots = (nt + rounds - 1) // rounds
    return max(1, min(slots, max(n_templates, 1)))


def runs_of(location, n, upload_batch, slots, prep_overlap, scaled):
    """[(first frame, count)] as ecc_shard_impl hands the moving frames 1 .. n - 1 to prepare_templates."""
    if n <= 1:
        return []
    if location == "host":                                   # upload.cpp: batch 0 is frame 0 alone, then batches of upload_batch
        b = max(1, upload_batch)
        return [(i, min(b, n - i)) for i in range(1, n, b)]
    if not scaled and prep_overlap and n - 1 > 2 * slots:    # device-resident, prepared under the iteration
        return [(i, min(PREP_RUN, n - i)) for i in range(1, n, PREP_RUN)]
    return [(1, n - 1)]


def run_streams(count, w, depth, channels, row_stride, frame_step, base_mod4, prep_stream, scaled, gauss):
    """prepare_templates + launch_grey_blur_batch: does a run of `count` evenly spaced frames take the streaming kernel?"""
    return bool(count >= 2 and prep_stream and not scaled and frame_step > 0 and channels == 3 and depth in (8, 16)
                and gauss in (3, 5, 7) and w % 4 == 0 and w >= 8 and row_stride % 4 == 0 and frame_step % 4 == 0 and base_mod4 == 0)


def route_model(w, h, depth, channels, row_stride, location, n, upload_batch=UPLOAD_BATCH_DEFAULT, slots=None, prep_stream=1,
                prep_overlap=1, scaled=False, gauss=5, frame_step=None, base_mod4=0, even=True):
    """Templates of a call that grey_blur_stream_kernel must write (the counter "prep_stream_frames"). row_stride and
    frame_step in bytes (frame_step None: rows * row_stride, a contiguous tensor or the engine's own upload buffer, which
    also starts on a 256-byte boundary); `slots`: None = effective_slots of the call with the option at 0."""
    if slots is None:
        slots = effective_slots(n - 1, w, h)
    if location == "host":                                   # frames land row_stride * h apart in the engine's buffer
        frame_step, base_mod4, even = row_stride * h, 0, True
    elif frame_step is None:
        frame_step = row_stride * h
    total = 0
    for _, count in runs_of(location, n, upload_batch, slots, prep_overlap, scaled):
        if even and run_streams(count, w, depth, channels, row_stride, frame_step, base_mod4, prep_stream, scaled, gauss):
            total += count
    return total


# ---- the case table ----------------------------------------------------------------------------------------------------
# entry: "ecc" (ecc_match), "hybrid" (hybrid_match, the only call that runs ECC on 16-bit frames), "fte" (find_transform_ecc
#        on two grey planes); kind: u8c3 | u16c3 | f32c3 | u8c4 | u8c1 | f32c1; location: "device" | "host";
# layout: "tight" or (Hc, Wc, y0, x0): a window of a device canvas whose planes are Hc x Wc pixels (test_gpu_strided.py);
# route: the route of ecc_shard_impl the case is there for; expect: "streamed" (count > 0), "fallback" (exactly 0) or
#        "mixed" (0 < count < n - 1)
Case = namedtuple("Case", "name entry kind w h n gauss location layout upload_batch ecc_slots prep_overlap scale_down_width route expect")

# all at height 40: the narrowest two, then every multiple of a wave's 248 px up to a workgroup's 992 with its neighbours
WIDTHS = (8, 12, 244, 248, 252, 256, 492, 496, 500, 740, 744, 748, 988, 992, 996, 1000)
HEIGHTS = (8, 31, 32, 33, 63, 64, 65)                                   # all at width 252
GAUSS = (3, 5, 7)
N_SWEEP = 4


def _case(name, entry, kind, w, h, n, gauss, route, expect, location="device", layout="tight", upload_batch=None, ecc_slots=None,
          prep_overlap=None, scale_down_width=None):
    return Case(name, entry, kind, w, h, n, gauss, location, layout, upload_batch, ecc_slots, prep_overlap, scale_down_width, route, expect)


def _build_cases():
    cases = []
    sizes = [(w, 40) for w in WIDTHS] + [(252, h) for h in HEIGHTS]
    for w, h in sizes:
        for gauss in GAUSS:
            cases.append(_case("stream-%dx%d-g%d-u8" % (w, h, gauss), "ecc", "u8c3", w, h, N_SWEEP, gauss, "stream", "streamed"))
            cases.append(_case("stream-%dx%d-g%d-u16" % (w, h, gauss), "hybrid", "u16c3", w, h, N_SWEEP, gauss, "stream", "streamed"))
    # fall-back routes
    for w in (250, 333):                                     # w % 4 != 0: the generic kernel; the template row stride is not w
        cases.append(_case("generic-%dx40-u8" % w, "ecc", "u8c3", w, 40, 4, 5, "generic", "fallback"))
    cases.append(_case("generic-252x33-f32", "ecc", "f32c3", 252, 33, 4, 5, "generic", "fallback"))
    cases.append(_case("generic-250x40-f32", "ecc", "f32c3", 250, 40, 3, 7, "generic", "fallback"))
    cases.append(_case("generic-252x33-bgra", "ecc", "u8c4", 252, 33, 4, 5, "generic", "fallback"))
    cases.append(_case("generic-333x40-bgra", "ecc", "u8c4", 333, 40, 3, 3, "generic", "fallback"))
    cases.append(_case("scaled-500x65-u8", "ecc", "u8c3", 500, 65, 4, 5, "scaled", "fallback", scale_down_width=252.0))
    cases.append(_case("scaled-500x65-u8-host", "ecc", "u8c3", 500, 65, 4, 5, "scaled", "fallback", location="host", scale_down_width=252.0))
    cases.append(_case("scaled-500x65-f32", "ecc", "f32c3", 500, 65, 3, 5, "scaled", "fallback", scale_down_width=333.0))
    cases.append(_case("fte-252x33-u8", "fte", "u8c1", 252, 33, 2, 5, "find_transform", "fallback"))
    cases.append(_case("fte-333x40-u8", "fte", "u8c1", 333, 40, 2, 7, "find_transform", "fallback"))
    cases.append(_case("fte-252x33-f32", "fte", "f32c1", 252, 33, 2, 5, "find_transform", "fallback"))
    # padded rows: a row stride of 263 * 3 = 789 bytes (no multiple of 4: frame by frame, the generic kernel) and one of
    # 260 * 3 = 780 bytes with the window 4 pixels in (dword-aligned rows and frames: the streaming kernel, rows padded)
    cases.append(_case("padded-odd-252x33-u8", "ecc", "u8c3", 252, 33, 4, 5, "padded", "fallback", layout=(37, 263, 2, 3)))
    cases.append(_case("padded-dword-252x33-u8", "ecc", "u8c3", 252, 33, 4, 5, "padded", "streamed", layout=(37, 260, 2, 4)))
    cases.append(_case("padded-dword-252x33-u16", "hybrid", "u16c3", 252, 33, 4, 7, "padded", "streamed", layout=(37, 258, 2, 4)))
    # batching: host-fed stacks, 5 moving frames cut by upload_batch (a batch of one frame takes the tiled kernel). By
    # upload.cpp's cut only batch size 2 mixes the kernels within the 6-frame stack (2 + 2 + 1); 1 gives five batches of
    # one, all tiled, 3 and 5 give 3 + 2 and 5, all streamed. Two more stacks end on a batch of one: 3 + 1 and 5 + 1.
    for ub, expect in ((1, "fallback"), (2, "mixed"), (3, "streamed"), (5, "streamed")):
        cases.append(_case("host-6x252x33-batch%d" % ub, "ecc", "u8c3", 252, 33, 6, 5, "host_fed", expect, location="host", upload_batch=ub))
    cases.append(_case("host-5x252x33-batch3", "ecc", "u8c3", 252, 33, 5, 7, "host_fed", "mixed", location="host", upload_batch=3))
    cases.append(_case("host-7x996x40-batch5", "ecc", "u8c3", 996, 40, 7, 3, "host_fed", "mixed", location="host", upload_batch=5))
    cases.append(_case("host-4x250x40", "ecc", "u8c3", 250, 40, 4, 5, "host_fed", "fallback", location="host"))
    # device-resident, more than 2 x slots moving frames: runs of 16 (here 16 + 2) on the prep stream under the iteration
    cases.append(_case("overlap-19x252x33", "ecc", "u8c3", 252, 33, 19, 5, "overlap", "streamed", ecc_slots=1))
    cases.append(_case("overlap-off-19x252x33", "ecc", "u8c3", 252, 33, 19, 5, "one_run", "streamed", ecc_slots=1, prep_overlap=0))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


CASES = _build_cases()
ROUTES = ("stream", "generic", "scaled", "find_transform", "padded", "host_fed", "overlap", "one_run")

_EL = {"u8": 1, "u16": 2, "f32": 4}


def case_layout(case):
    """(depth, channels, row stride in bytes, frame step in bytes, base address mod 4) of the frames as the engine gets them
    (device allocations and the engine's upload buffer start on at least a 256-byte boundary)."""
    depth_s, cn = case.kind.split("c")
    el, cn = _EL[depth_s], int(cn)
    if case.layout == "tight":
        rs = case.w * cn * el
        return 8 * el, cn, rs, rs * case.h, 0
    hc, wc, y0, x0 = case.layout
    rs = wc * cn * el
    return 8 * el, cn, rs, hc * rs, (y0 * rs + x0 * cn * el) % 4


def case_route_count(case):
    """route_model of a case of the table."""
    depth, cn, rs, step, base = case_layout(case)
    n_templates = 1 if case.entry == "fte" else case.n - 1
    ew, eh = (case.w, case.h) if not case.scale_down_width else oracle.scaled_size(case.w, case.h, float(case.scale_down_width))
    if case.entry == "fte":                                  # its own two launch_grey_blur calls: prepare_templates never runs
        return 0
    return route_model(case.w, case.h, depth, cn, rs, case.location, case.n,
                       upload_batch=UPLOAD_BATCH_DEFAULT if case.upload_batch is None else case.upload_batch,
                       slots=effective_slots(n_templates, ew, eh, case.ecc_slots or 0),
                       prep_stream=1, prep_overlap=1 if case.prep_overlap is None else case.prep_overlap,
                       scaled=bool(case.scale_down_width), gauss=case.gauss, frame_step=step, base_mod4=base)


# ---- images ------------------------------------------------------------------------------------------------------------
MASTER_N, MASTER_W, MASTER_H = 19, 1024, 80


@functools.lru_cache(None)
def _master(depth):
    """One textured synthetic stack per depth (synth.make_stack: a corner-rich scene, every moving frame resampled through its
    own homography with its own gain and noise, so no two frames agree); the cases take its top-left windows."""
    from libstacker_rs_amd import synth
    frames, _ = synth.make_stack(MASTER_N if depth == 8 else 4, MASTER_W, MASTER_H, depth=depth)
    a = frames.numpy()
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def case_frames(kind, w, h, n):
    """(n, h, w, C) — (n, h, w) for one channel — of `kind`, contiguous and read-only."""
    depth_s, cn = kind.split("c")
    rng = np.random.default_rng(1000 * w + h)
    if depth_s == "u16":
        s = _master(16)[:n, :h, :w]
    else:
        s = _master(8)[:n, :h, :w]
    assert s.shape[:3] == (n, h, w)
    if depth_s == "f32":                                     # real f32 content: fractions, values outside 0 .. 255
        s = s.astype(np.float32) * np.float32(1.03125) + rng.random(s.shape, dtype=np.float32) - np.float32(3.0)
    if cn == "4":
        s = np.concatenate([s, rng.integers(0, 256, s.shape[:3] + (1,), dtype=np.uint8)], axis=3)
    elif cn == "1":
        s = s[..., 1]
    s = np.ascontiguousarray(s)
    s.setflags(write=False)
    return s


@functools.lru_cache(None)
def case_expected(kind, w, h, n, gauss, scale_down_width):
    exp = expected_planes(list(case_frames(kind, w, h, n)), gauss, scale_down_width)
    for v in exp.values():
        v.setflags(write=False)
    return exp


def tolerance(kind, gauss):
    """(rtol, atol) of templates and I against the oracle; (0, 0) = bit for bit. 8-bit greys are integers below 2^8 and the
    taps of g = 3 / 5 / 7 are multiples of 2^-2 / 2^-4 / 2^-6: after the row and the column pass every partial sum is a
    multiple of 2^-12 below 2^8, at most 20 significant bits, exact in any order. 16-bit greys: 16 + 2 x 4 = 24 bits for
    g = 5, exact; g = 7 needs 28: positive weights that sum to 1 and about 20 roundings of 2^-24 each bound the relative
    error by 1.2e-6 (2e-6, no absolute term). f32 frames: the bar of test_fused_grey_blur_f32_input_and_large_kernel."""
    depth_s = kind.split("c")[0]
    if depth_s == "u8" or (depth_s == "u16" and gauss in (3, 5)):
        return 0.0, 0.0
    if depth_s == "u16":
        return 2e-6, 0.0
    return 2e-6, 1e-6

"""Stream ordering of device arguments: every kernel reads its inputs after they were written and writes
its outputs before they are reused — on a context bound to torch's stream by stream order alone, on an unbound one
through the wrapper's drains.

The instrument. Every device argument of a call starts out holding POISON: ordinary image content that differs from
the true content (the stack mirrored left-right in reverse frame order, another seeded field for f32 and int32 planes;
never NaN, never constant, never zero). The true content arrives late: a delay (torch.cuda._sleep, calibrated against a
pair of events) followed by buf.copy_(true) on the producer stream. An unrelated stream snapshots every buffer while
the delay runs — the snapshot must still be the poison, else the case FAILS with "the delay did not hold". Then the
call is made. A missing dependency makes the engine read the poison, or the late copy land on top of a result: a wrong
but finite answer through the normal code path, which the comparison — bit equality with the same call on the same
context on the true content, everything synchronised — sees. The delay is 3 x the reference run's duration, at least
20 ms, at most 500 ms.

Part 0 proves that the instrument sees a missing dependency (the producer on a stream the bound context knows nothing
of: the result is the poison's). Part A holds a bound context's gates through every route that leaves ctx->stream.
Part B holds an unbound context's wrapper: what the wrapper itself enqueues after _marshal's drain (fills, casts,
.contiguous() copies) sits behind a delay, and the engine must still see it finished. Part B is one-sided: a correct
wrapper cannot fail it. On the wrapper as it was before its drains were moved behind its own torch ops, all 15 Part B
cases failed on the MI355X."""
import contextlib
import time

import numpy as np
import pytest
import torch

from libstacker_rs_amd import (CalibrationParameters, DefectParameters, EccMatchParameters, KeyPointMatchParameters,
                               LocalParameters, MeshParameters, MotionType, RANSAC, Stacker, StarParameters, mesh_grid, synth)

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
ECC_AFFINE = EccMatchParameters(MotionType.Affine, 5000, 1e-5, 5)
ECC_HYBRID = EccMatchParameters(MotionType.Homography, 200, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
OPTION_DEFAULTS = {"ecc_slots": 0, "prep_overlap": 1, "ecc_groups": 0, "kp_lanes": 3}
MIN_DELAY_MS, MAX_DELAY_MS, DELAY_FACTOR = 20.0, 500.0, 3.0
W, H, N = 131, 97, 5                      # the caller-held-warps families: ragged against every tile
STEP = 16


# ---- the instrument --------------------------------------------------------------------------------------------------
def _sleep_ms(cycles):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(int(cycles))
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _runs_while_sleeping(sleeper, runner, cycles_per_ms):
    """Does work on `runner` complete while `sleeper` sleeps (two torch streams may share a hardware queue)?"""
    x = torch.zeros(16, device="cuda")
    ev = torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(sleeper):
        torch.cuda._sleep(int(20 * cycles_per_ms))
    with torch.cuda.stream(runner):
        x.add_(1)
        ev.record()
    t0 = time.perf_counter()
    ev.synchronize()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return dt < 0.010


class Rig:
    """The bound context, its stream S, a snapshot stream T and a foreign producer stream P that run beside each other."""


@pytest.fixture(scope="module")
def rig():
    assert hasattr(torch.cuda, "_sleep")
    r = Rig()
    _sleep_ms(1_000_000)                                     # warm-up
    first = max(_sleep_ms(1_000_000), 1e-3)
    cycles = int(1_000_000 * 20.0 / first)                   # aim at 20 ms and measure again
    r.cycles_per_ms = cycles / _sleep_ms(cycles)
    r.S = torch.cuda.Stream()
    with torch.cuda.stream(r.S):
        r.st = Stacker(0)
        r.st.use_torch_stream()
    pool = [torch.cuda.Stream() for _ in range(8)]
    r.T = next((c for c in pool if _runs_while_sleeping(r.S, c, r.cycles_per_ms)), None)
    assert r.T is not None, "no torch stream runs beside the bound one: the delay cannot be observed"
    r.P = next((c for c in pool if c is not r.T and _runs_while_sleeping(c, r.S, r.cycles_per_ms)
                and _runs_while_sleeping(c, r.T, r.cycles_per_ms)), None)
    assert r.P is not None, "no torch stream to produce on beside the bound one"
    r.free = Stacker(0)                                      # Part B's unbound context
    print("stream-order calibration: %.0f sleep cycles per ms" % r.cycles_per_ms)
    yield r
    r.st.close()
    r.free.close()


def _bits(x):
    """Host copy of a result: tensors and arrays as (dtype, shape, bytes), containers kept."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return ("f64", (), np.float64(x).tobytes())
    return x


def _clone_device(x):
    if isinstance(x, torch.Tensor):
        return x.clone() if x.is_cuda else x
    if isinstance(x, dict):
        return {k: _clone_device(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clone_device(v) for v in x]
    return x


def _poison(t, seed):
    """Content of t's kind that is not t's: integer images mirrored (and in reverse frame order), else a seeded field over t's range."""
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 + seed)
    if t.dtype in (torch.uint8, torch.uint16):
        dims = (0, 2) if t.dim() == 4 else (1,)
        p = t.view(torch.int16).flip(dims).view(torch.uint16) if t.dtype == torch.uint16 else t.flip(dims)
    elif t.dtype == torch.int32:
        p = torch.randint(0, int(t.max()) + 2, t.shape, generator=g, device="cuda", dtype=torch.int32)
    else:
        lo, hi = float(t.min()), float(t.max())
        p = (torch.rand(t.shape, generator=g, device="cuda") * ((hi - lo) or 1.0) + lo).to(t.dtype)
    p = p.contiguous()
    assert _bits(p) != _bits(t) and bool(torch.isfinite(p.float()).all())
    return p


class _SyncCounter:
    """Counts torch.cuda.Stream.synchronize and torch.cuda.synchronize across a block."""

    def __init__(self):
        self.n = 0

    @contextlib.contextmanager
    def counting(self):
        mp = pytest.MonkeyPatch()
        real_s, real_g = torch.cuda.Stream.synchronize, torch.cuda.synchronize

        def stream_sync(this):
            self.n += 1
            return real_s(this)

        def global_sync(*a, **k):
            self.n += 1
            return real_g(*a, **k)
        mp.setattr(torch.cuda.Stream, "synchronize", stream_sync)
        mp.setattr(torch.cuda, "synchronize", global_sync)
        try:
            yield self
        finally:
            mp.undo()


class Case:
    """args: name -> the TRUE content of every device argument; call(st, a): the wrapper call on buffers a[name]."""

    def __init__(self, args, call, options=None, after=None):
        self.args, self.call, self.options, self.after = args, call, options or {}, after


def _reference(st, stream, case, content=None):
    """The call on the true content (or `content`), everything synchronised: (result bits, duration in ms). A first,
    untimed call takes the allocations of a context's first visit to a route, so that neither the timed run nor the
    delayed call that follows contains them."""
    with torch.cuda.stream(stream):
        case.call(st, {k: v.clone() for k, v in (content or case.args).items()})
    a = {k: v.clone() for k, v in (content or case.args).items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):
        res = case.call(st, a)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return _bits(res), ms


def _delay_ms(ref_ms, label):
    assert ref_ms <= MAX_DELAY_MS, "%s: the call takes %.0f ms, longer than one sleep may be: split the case" % (label, ref_ms)
    d = min(max(DELAY_FACTOR * ref_ms, MIN_DELAY_MS), MAX_DELAY_MS)
    print("%s: reference run %.2f ms, delay D = %.1f ms" % (label, ref_ms, d))
    return d


def _delayed(rig, case, d_ms, producer, poison):
    """The delayed producer: (result bits, bits of the clones taken on the bound stream right behind the call, torch syncs)."""
    bufs = {k: v.clone() for k, v in poison.items()}
    torch.cuda.synchronize()
    with torch.cuda.stream(producer):
        torch.cuda._sleep(int(d_ms * rig.cycles_per_ms))
        for k in bufs:
            bufs[k].copy_(case.args[k])
    with torch.cuda.stream(rig.T):
        snaps = {k: v.clone() for k, v in bufs.items()}
    counter = _SyncCounter()
    with torch.cuda.stream(rig.S):
        with counter.counting():
            res = case.call(rig.st, bufs)
        late = _clone_device(res)
    torch.cuda.synchronize()
    for k in bufs:
        assert _bits(snaps[k]) == _bits(poison[k]), "the delay did not hold (%s was written before the snapshot)" % k
    return _bits(res), _bits(late), counter.n


def _run_bound(rig, case, label):
    st = rig.st
    try:
        for k, v in case.options.items():
            st.set_option(k, v)
        want, ms = _reference(st, rig.S, case)
        if case.after:
            case.after(st)
        poison = {k: _poison(v, i) for i, (k, v) in enumerate(case.args.items())}
        got, late, syncs = _delayed(rig, case, _delay_ms(ms, label), rig.S, poison)
        if case.after:
            case.after(st)
    finally:
        for k in case.options:
            st.set_option(k, OPTION_DEFAULTS[k])
    assert syncs == 0, "the wrapper of a bound context synchronised torch %d times" % syncs
    assert got == want, "the engine did not see the late arguments (or the late copy landed on a result)"
    assert late == want, "a consumer on the bound stream, right behind the call, saw another result"


# ---- content -----------------------------------------------------------------------------------------------------------
_cache = {}


def _stack(n, w=320, h=240, depth=8):
    key = ("stack", n, w, h, depth)
    if key not in _cache:
        _cache[key] = synth.make_stack(n, w, h, depth=depth, device="cuda")[0].contiguous()
    return _cache[key]


def _field(shape, lo, hi, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo).to(dtype)


def _warps(n):
    out = []
    for i in range(n):
        M = np.eye(3)
        M[0, 2], M[1, 2] = 0.7 * i, -0.4 * i
        out.append(M)
    return out


def _grid():
    gw, gh = mesh_grid(W, H, STEP)
    return gh, gw


def _maps():
    return _field((N, H, W), 0.0, 3.0, 21)


def _fields():
    gh, gw = _grid()
    return _field((N, gh, gw, 2), -1.5, 1.5, 22)


def _clean():
    return (_stack(N, W, H).float().mean(0) / 255.0).contiguous()


def _counts():
    g = torch.Generator(device="cuda")
    g.manual_seed(23)
    return torch.randint(3, N + 1, (H, W), generator=g, device="cuda", dtype=torch.int32)


def _norm_planes():
    rng = np.random.default_rng(24)
    gh, gw = _grid()
    return [None] + [np.concatenate([rng.uniform(0.5, 2.0, (gh, gw, 3)), rng.uniform(-0.1, 0.1, (gh, gw, 3))], -1).astype(np.float32)
                     for _ in range(N - 1)]


def _masters():
    bias = _field((H, W, 3), 8.0, 12.0, 31)
    dark = _field((H, W, 3), 1.0, 3.0, 32)
    flat = _field((H, W, 3), 90.0, 110.0, 33)
    g = torch.Generator(device="cuda")
    g.manual_seed(34)
    defects = (torch.rand((H, W), generator=g, device="cuda") < 0.01).to(torch.uint8) * 5
    return bias, dark, flat, defects


def _star_stack():
    if "stars" not in _cache:
        w, h, n = 240, 180, 4
        mots = [None] + [synth.star_motion(w, h, 3.0 * i, 1.5 * i, -1.0 * i) for i in range(1, n)]
        _cache["stars"] = torch.from_numpy(synth.make_star_stack(mots, w, h, 60, seed=9)[0]).cuda()
    return _cache["stars"]


# ---- Part 0: the detector detects --------------------------------------------------------------------------------------
def _control_cases():
    frames = _stack(4)
    M = np.array([[1.0, 0.01, 2.5], [-0.01, 1.0, -1.5], [0.0, 0.0, 1.0]])
    return {"warp_accumulate": Case({"frame": frames[1].contiguous()}, lambda st, a: st.warp_accumulate(a["frame"], M)),
            "stack_sharpness": Case({"frames": frames}, lambda st, a: st.stack_sharpness(a["frames"], 3))}


@pytest.mark.parametrize("name", ["warp_accumulate", "stack_sharpness"])
def test_part0_a_producer_the_context_does_not_know_is_seen(rig, name):
    """The producer runs on P, the context on S: the wrapper believes stream order holds, the engine reads the poison."""
    case = _control_cases()[name]
    poison = {k: _poison(v, i) for i, (k, v) in enumerate(case.args.items())}
    truth, _ = _reference(rig.st, rig.S, case)
    want, ms = _reference(rig.st, rig.S, case, poison)
    assert want != truth
    got, late, syncs = _delayed(rig, case, _delay_ms(ms, "part 0 " + name), rig.P, poison)
    rig.P.synchronize()
    assert syncs == 0
    assert got == want and late == want, "a missing dependency is invisible to the instrument"


# ---- Part A: bound context, delayed producer ---------------------------------------------------------------------------
def _prep_counter(n):
    def check(st):
        assert st.timing()["prep_stream_frames"] == n - 1
    return check


def _ecc_case(entry, n, options=None, scale=None, params=ECC, after=None):
    frames = _stack(n)
    if entry == "ecc_match":
        return Case({"frames": frames}, lambda st, a: st.ecc_match(a["frames"], params, scale, return_stats=True), options, after)
    args = {"frames": frames, "sum_out": _field((240, 320, 3), 0.0, 1.0, 41)}
    return Case(args, lambda st, a: (st.ecc_match_shard(a["frames"], params, True, a["sum_out"], scale), a["sum_out"]), options, after)


def _kp_case(entry, n, options=None, scale=None):
    frames = _stack(n)
    if entry == "keypoint_match":
        return Case({"frames": frames}, lambda st, a: st.keypoint_match(a["frames"], KP, scale, return_stats=True), options)
    args = {"frames": frames, "sum_out": _field((240, 320, 3), 0.0, 1.0, 42)}
    return Case(args, lambda st, a: (st.keypoint_match_shard(a["frames"], KP, True, a["sum_out"], scale), a["sum_out"]), options)


ECC_ROUTES = {
    # everything on ctx->stream
    "baseline": lambda e: _ecc_case(e, 4),
    # overlap_prep (stacker.cpp:676: device frames, not scaled, n - 1 = 11 > 2 x 4 slots): templates on prep_stream behind
    # gate_ev (stacker.cpp:370-371, 742-761)
    "overlap_prep": lambda e: _ecc_case(e, 12, {"ecc_slots": 4, "prep_overlap": 1}, after=_prep_counter(12)),
    # two slot groups (stacker.cpp:392-393: ecc_groups = 2 and n_slots = 8 >= 8; n - 1 = 11 <= 16, so no overlap_prep):
    # the second launch sequence on ecc_stream2 behind gate_ev2 (stacker.cpp:399-400), joined at 458-459
    "two_groups": lambda e: _ecc_case(e, 12, {"ecc_slots": 8, "ecc_groups": 2}),
    # grey -> INTER_AREA -> blur through the shared scratch
    "scaled": lambda e: _ecc_case(e, 4, scale=160),
    # the affine fold table
    "affine": lambda e: _ecc_case(e, 4, params=ECC_AFFINE),
}
KP_ROUTES = {
    "one_lane": lambda e: _kp_case(e, 4),
    # lanes (keypoint.cpp:586-587: kp_lanes = 2, device frames, n = 17 >= 16): lane 1 on a helper context whose stream
    # waits for gate_ev (keypoint.cpp:778-791); the lanes' tails on tail_stream (keypoint.cpp:648: n_lanes > 1)
    "two_lanes": lambda e: _kp_case(e, 17, {"kp_lanes": 2}),
    "two_lanes_scaled": lambda e: _kp_case(e, 17, {"kp_lanes": 2}, scale=200),       # the same through gfull
}


@pytest.mark.parametrize("entry", ["ecc_match", "ecc_match_shard"])
@pytest.mark.parametrize("route", list(ECC_ROUTES))
def test_bound_ecc(rig, entry, route):
    _run_bound(rig, ECC_ROUTES[route](entry), "%s %s" % (entry, route))


@pytest.mark.parametrize("entry", ["keypoint_match", "keypoint_match_shard"])
@pytest.mark.parametrize("route", list(KP_ROUTES))
def test_bound_keypoint(rig, entry, route):
    _run_bound(rig, KP_ROUTES[route](entry), "%s %s" % (entry, route))


def test_bound_hybrid_shard_16_bit(rig):
    # the lanes' grey16 -> grey8, then the seeded ECC queue
    args = {"frames": _stack(4, depth=16), "sum_out": _field((240, 320, 3), 0.0, 1.0, 43)}
    _run_bound(rig, Case(args, lambda st, a: (st.hybrid_match_shard(a["frames"], KP, ECC_HYBRID, True, a["sum_out"]), a["sum_out"])),
               "hybrid_match_shard")


def test_bound_warp_accumulate_into_a_late_accumulator(rig):
    M = np.array([[1.0, 0.01, 2.5], [-0.01, 1.0, -1.5], [0.0, 0.0, 1.0]])
    args = {"frame": _stack(4)[2].contiguous(), "acc": _field((240, 320, 3), 0.0, 2.0, 44)}      # acc.copy_(prev) behind the delay
    _run_bound(rig, Case(args, lambda st, a: st.warp_accumulate(a["frame"], M, acc=a["acc"])), "warp_accumulate acc")


@pytest.mark.parametrize("mode", ["in_place", "out"])
def test_bound_finalize_mean(rig, mode):
    args = {"sum": _field((240, 320, 3), 0.0, 7.0, 45)}
    if mode == "out":
        args["out"] = _field((240, 320, 3), 0.0, 1.0, 46)
    _run_bound(rig, Case(args, lambda st, a: (st.finalize_mean(a["sum"], 7, a.get("out")), a["sum"])), "finalize_mean " + mode)


def _family_cases():
    if "family" not in _cache:
        _cache["family"] = _build_family_cases()
    return _cache["family"]


def _build_family_cases():
    fr, wp = _stack(N, W, H), _warps(N)
    F, X = {"frames": fr}, lambda **kw: dict({"frames": fr}, **kw)
    norm = _norm_planes()
    bias, dark, flat, defects = _masters()
    mesh = MeshParameters(step=STEP)
    cal = lambda a: CalibrationParameters(bias=a["bias"], dark=a["dark"], flat=a["flat"], dark_scale=[1.0, 0.5, 2.0, 1.5, 1.0],
                                          flat_mean=[100.0] * 3, flat_min=1.0, defects=a["defects"])
    stars = {"frames": _star_stack()}
    return {
        "clip_stack": Case(F, lambda st, a: st.clip_stack(a["frames"], wp, return_counts=True)),
        "quantile_stack": Case(F, lambda st, a: st.quantile_stack(a["frames"], wp)),
        "weighted_stack": Case(F, lambda st, a: st.weighted_stack(a["frames"], wp, return_coverage=True)),
        "robust_clip_stack": Case(F, lambda st, a: st.robust_clip_stack(a["frames"], wp, return_counts=True)),
        "overlap_moments": Case(F, lambda st, a: st.overlap_moments(a["frames"], wp)),
        "local_norm_stack": Case(F, lambda st, a: st.local_norm_stack(a["frames"], wp, norm, STEP, return_den=True)),
        "clip_stack_local_norm": Case(F, lambda st, a: st.clip_stack_local_norm(a["frames"], wp, norm, STEP, return_counts=True)),
        "local_sharpness": Case(F, lambda st, a: st.local_sharpness(a["frames"], LocalParameters())),
        "local_moments": Case(F, lambda st, a: st.local_moments(a["frames"], wp, STEP)),
        "local_weighted_stack": Case(X(maps=_maps()), lambda st, a: st.local_weighted_stack(a["frames"], wp, a["maps"], return_coverage=True)),
        "local_align": Case(F, lambda st, a: st.local_align(a["frames"], wp, mesh, return_status=True)),
        "local_align_pyramid": Case(F, lambda st, a: st.local_align_pyramid(a["frames"], wp, mesh, 2, return_status=True)),
        "mesh_stack": Case(X(fields=_fields()), lambda st, a: st.mesh_stack(a["frames"], wp, a["fields"], STEP)),
        "mesh_local_weighted_stack": Case(X(maps=_maps(), fields=_fields()),
                                          lambda st, a: st.mesh_local_weighted_stack(a["frames"], wp, a["maps"], a["fields"], STEP)),
        "mesh_drizzle_stack": Case(X(fields=_fields()), lambda st, a: st.mesh_drizzle_stack(a["frames"], wp, a["fields"], STEP, return_den=True)),
        "drizzle_stack": Case(X(maps=_maps()), lambda st, a: st.drizzle_stack(a["frames"], wp, maps=a["maps"], return_den=True)),
        "reject_maps": Case(X(clean=_clean(), counts=_counts(), maps=_maps(), out=_field((N, H, W), 0.0, 1.0, 25)),
                            lambda st, a: st.reject_maps(a["frames"], wp, a["clean"], None, a["counts"], maps=a["maps"], out=a["out"],
                                                         return_counts=True)),
        "stack_sharpness": Case(F, lambda st, a: st.stack_sharpness(a["frames"], 3)),
        "star_detect": Case(stars, lambda st, a: st.star_detect(a["frames"], StarParameters(), return_peaks=True)),
        "star_align": Case(stars, lambda st, a: st.star_align(a["frames"], StarParameters())),
        "calibrate": Case(X(bias=bias, dark=dark, flat=flat, defects=defects), lambda st, a: st.calibrate(a["frames"], cal(a))),
        "defect_map": Case({"master": dark}, lambda st, a: st.defect_map(a["master"], DefectParameters(True, False, 0.5), return_counts=True)),
        "image_mean": Case({"image": flat}, lambda st, a: st.image_mean(a["image"])),
        "master_stack": Case(F, lambda st, a: st.master_stack(a["frames"], 0, return_counts=True)),
        "grey": Case({"frame": fr[1].contiguous()}, lambda st, a: st.grey(a["frame"])),
        "grey_pyramid": Case({"frame": fr[1].contiguous()}, lambda st, a: st.grey_pyramid(a["frame"], 4)),
        "grey_blur_f32": Case({"frame": fr[1].contiguous()}, lambda st, a: st.grey_blur_f32(a["frame"], 5)),
    }


FAMILY = ["clip_stack", "quantile_stack", "weighted_stack", "robust_clip_stack", "overlap_moments", "local_norm_stack",
          "clip_stack_local_norm", "local_sharpness", "local_moments", "local_weighted_stack", "local_align", "local_align_pyramid",
          "mesh_stack", "mesh_local_weighted_stack", "mesh_drizzle_stack", "drizzle_stack", "reject_maps", "stack_sharpness",
          "star_detect", "star_align", "calibrate", "defect_map", "image_mean", "master_stack", "grey", "grey_pyramid", "grey_blur_f32"]


@pytest.mark.parametrize("name", FAMILY)
def test_bound_caller_held_warps(rig, name):
    """n = 5 frames of 131 x 97 under identity-plus-shift warps held on the host; EVERY device argument arrives late."""
    _run_bound(rig, _family_cases()[name], name)


# ---- Part B: unbound context, work the wrapper enqueues after the drain ----------------------------------------------------
def _seed_allocator(like):
    """Blocks of the sizes the wrapper is about to allocate, left holding finite poison: a fresh torch.ones / torch.zeros
    block then most likely holds it until its fill runs."""
    held = []
    for i, (shape, dtype) in enumerate(like):
        held.append(_field(shape, 2.0, 9.0, 900 + i).to(dtype))
    torch.cuda.synchronize()
    del held


def _run_unbound(rig, call, like, label):
    """call(st) on the unbound context: once plain and synchronised, once with a delay on torch's current stream right
    behind every drain the wrapper makes (_marshal's, and each _tensor_ready: a drain that comes BEFORE the wrapper's own
    copy of an argument hides nothing that way), so that every torch op the wrapper issues from there on is late."""
    st = rig.free
    call(st)                                                 # (allocations of the first visit)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = call(st)
    torch.cuda.synchronize()
    d = _delay_ms((time.perf_counter() - t0) * 1e3, label)
    want = _bits(want)
    real_marshal, real_ready = st._marshal, st._tensor_ready

    def delay(devices):
        for dev in devices:
            with torch.cuda.device(dev):
                torch.cuda._sleep(int(d * rig.cycles_per_ms))

    def late_marshal(frames):
        m = real_marshal(frames)
        delay(m.devices)
        return m

    def late_ready(t):
        real_ready(t)
        delay([t.device])
    _seed_allocator(like)
    st._marshal, st._tensor_ready = late_marshal, late_ready
    try:
        got = call(st)
    finally:
        del st._marshal, st._tensor_ready
    torch.cuda.synchronize()
    got_bits = _bits(got)
    assert got_bits == want, "the engine ran ahead of torch work the wrapper itself had enqueued"
    return got


F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def test_unbound_reject_maps_fresh_planes(rig):
    fr, wp = _stack(N, W, H), _warps(N)
    clean, counts = _clean(), _counts()
    got = _run_unbound(rig, lambda st: st.reject_maps(fr, wp, clean, None, counts, include=[1, 1, 0, 1, 1], return_counts=True),
                       [((N, H, W), F32)], "unbound reject_maps")
    assert bool((got[0][2] == 1).all())                      # the excluded frame's plane: all ones, not what the block held


@pytest.mark.parametrize("levels", [None, 2])
def test_unbound_local_align_fresh_fields(rig, levels):
    fr, wp = _stack(N, W, H), _warps(N)
    gh, gw = _grid()
    mesh = MeshParameters(step=STEP)
    if levels is None:
        call = lambda st: st.local_align(fr, wp, mesh, include=[1, 1, 0, 1, 1], return_status=True)
    else:
        call = lambda st: st.local_align_pyramid(fr, wp, mesh, levels, include=[1, 1, 0, 1, 1], return_status=True)
    fields, status = _run_unbound(rig, call, [((N, gh, gw, 2), F32), ((N, gh, gw), I32)], "unbound local_align %s" % levels)
    assert not bool(fields[2].any()) and not bool(status[2].any())
    assert not bool(fields[0].any()) and not bool(status[0].any())


def test_unbound_grey_pyramid(rig):
    frame = _stack(4)[1].contiguous()
    _run_unbound(rig, lambda st: st.grey_pyramid(frame, 4), [((240 >> l, 320 >> l), U8) for l in (1, 2, 3)], "unbound grey_pyramid")


def _as(kind, t):
    """t as the wrapper does not take it as it is: float64, or a column-strided view of a wider tensor (same values)."""
    if kind == "float64":
        return t.double()
    if t.dim() == 2:
        big = t.repeat_interleave(2, dim=1)
        return big[:, ::2]
    idx = 1 if t.dim() == 3 and t.shape[-1] == 3 else 2       # an H x W x C image steps its pixels, a stack of planes its columns
    big = t.repeat_interleave(2, dim=idx)
    return big[(slice(None),) * idx + (slice(None, None, 2),)]


@pytest.mark.parametrize("kind", ["float64", "strided"])
@pytest.mark.parametrize("name", ["local_weighted_stack", "mesh_local_weighted_stack", "mesh_stack", "mesh_drizzle_stack", "reject_maps"])
def test_unbound_arguments_the_wrapper_converts(rig, name, kind):
    fr, wp = _stack(N, W, H), _warps(N)
    gh, gw = _grid()
    maps, fields = _as(kind, _maps()), _as(kind, _fields())
    assert not (kind == "strided" and (maps.is_contiguous() or fields.is_contiguous()))
    like_m, like_f = [((H, W), F32)] * N, [((gh, gw, 2), F32)] * N
    if name == "local_weighted_stack":
        call, like = (lambda st: st.local_weighted_stack(fr, wp, maps)), like_m
    elif name == "mesh_local_weighted_stack":
        call, like = (lambda st: st.mesh_local_weighted_stack(fr, wp, maps, fields, STEP)), like_m + like_f
    elif name == "mesh_stack":
        call, like = (lambda st: st.mesh_stack(fr, wp, fields, STEP)), like_f
    elif name == "mesh_drizzle_stack":
        call, like = (lambda st: st.mesh_drizzle_stack(fr, wp, fields, STEP)), like_f
    else:
        clean, counts = _as(kind, _clean()), _as(kind, _counts())
        call = lambda st: st.reject_maps(fr, wp, clean, None, counts, maps=maps, return_counts=True)
        like = [((H, W, 3), F32), ((H, W), I32), ((N, H, W), F32), ((N, H, W), F32)]
    _run_unbound(rig, call, like, "unbound %s %s" % (name, kind))


def test_unbound_image_argument_with_unpacked_pixels(rig):
    # a master whose pixel step is not packed: _image_stride_bytes refuses it and the wrapper falls back to .contiguous()
    fr = _stack(N, W, H)
    bias = _as("strided", _masters()[0])
    assert tuple(bias.shape) == (H, W, 3) and bias.stride(1) == 6
    _run_unbound(rig, lambda st: st.calibrate(fr, CalibrationParameters(bias=bias)), [((H, W, 3), F32)], "unbound calibrate bias view")

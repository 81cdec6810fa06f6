"""A call's outputs and stats are a function of its arguments and the context's options only: never of
what the same context did before.

A context lives as long as its shard and keeps grow-only workspaces, buffers that several features share, caches keyed
on geometry and regions that are read but must not matter. Every other GPU file runs on one session-wide context in one
fixed order, or on a fresh context whose memory the allocator very often hands out zero-filled: a missing memset, a
masked-out tap computed as 0 x garbage, a counter assumed to be zero or a stale cache would pass all of them.

The catalogue below names one small case per entry point and route; every case has a neighbour, the same entry point on
another geometry (wider, lower, more frames, bright content; NaN and inf planted in f32 inputs that take them). The
reference of a case is the case's result on a context made for it alone and closed afterwards: numerical correctness is
pinned by each family's own file, this one pins independence, so the comparison is == on bytes (NaN positions count)
and there is no tolerance anywhere.

  Part 0  the instrument: option debug_poison really destroys what ecc_prepared() reads back, reports its bytes, refuses
          a value that is no byte, and the catalogue reaches every workspace (stk_get_counter "workspaces_empty").
  Part A  on the session's context: poison with 0xFF (f32 NaN, int -1, u8 255), run, compare; again with 0x7F (a huge
          finite float that survives NaN filters, a large positive int).
  Part B  on the session's context, no poison: neighbour, case, neighbour, case; and the named sequences through the
          geometry caches and the shared buffers.
  Part C  three seeded shuffles of the whole catalogue with neighbours interleaved at random.
  Part D  a multi-device context [0, 0]: the three whole-stack calls after poison and after their neighbours.

Workspaces the catalogue cannot reach (LANE_UNREACHED below): the 22 workspaces of stk_ctx itself in every hidden keypoint
lane context. A lane runs ORB, the 2-NN match and findHomography on its own KeypointWorkspace and HgWorkspace and nothing
else; no public call makes it fold, iterate ECC or combine."""
import os

import numpy as np
import pytest
import torch

from libstacker_rs_amd import (LMEDS, RANSAC, CalibrationParameters, DefectParameters, DrizzleParameters, EccMatchParameters,
                               InvalidParams, KeyPointMatchParameters, LocalNormParameters, LocalParameters, MeshParameters,
                               MotionType, RobustClipParameters, SelectParameters, SigmaClipParameters, Stacker,
                               StarParameters, WeightParameters, mesh_grid, synth)

pytestmark = pytest.mark.gpu

ECC = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
ECC_AFFINE = EccMatchParameters(MotionType.Affine, 5000, 1e-5, 5)
ECC_HYBRID = EccMatchParameters(MotionType.Homography, 200, 1e-5, 5)
KP = KeyPointMatchParameters(RANSAC, 5.0, 0.80, 0.9)
KP_LMEDS = KeyPointMatchParameters(LMEDS, 5.0, 0.80, 0.9)
OPTION_DEFAULTS = {"ecc_slots": 0, "prep_overlap": 1, "ecc_groups": 0, "kp_lanes": 3, "orb_patch_blur": 1, "orb_resize_tables": 1,
                   "upload_batch": 8, "warp_interpolation": 1, "orb_device_cull": 1}
STEP = 16
# (w, h, n) of a case and of its neighbour: wider, lower, more frames
G_FAM = ((131, 97, 5), (163, 61, 7))          # caller-held warps: two 64-wide tiles, the second one ragged
G_ECC = ((320, 240, 4), (384, 200, 6))
G_ORB = ((640, 480, 4), (704, 400, 6))
G_STAR = ((240, 180, 4), (300, 140, 5))
LANE_UNREACHED = 22                           # per hidden lane context: the DevBufs of stk_ctx itself (module docstring)


# ---- results ------------------------------------------------------------------------------------------------------------
def _bits(x):
    """Host copy of a result: tensors and arrays as (dtype, shape, bytes), containers kept."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        if x.dtype == object:
            return [_bits(v) for v in x]
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return {k: _bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_bits(v) for v in x]
    if isinstance(x, (float, np.floating)):
        return ("f64", (), np.float64(x).tobytes())
    if isinstance(x, np.integer):
        return int(x)
    return x


def _where(a, b, path="result"):
    """The first place two _bits trees differ, for the failure message."""
    if type(a) is not type(b):
        return "%s: %s against %s" % (path, type(a).__name__, type(b).__name__)
    if isinstance(a, dict):
        for k in a:
            if a[k] != b.get(k):
                return _where(a[k], b.get(k), "%s[%r]" % (path, k))
    if isinstance(a, list):
        if len(a) != len(b):
            return "%s: %d against %d entries" % (path, len(a), len(b))
        for i, (u, v) in enumerate(zip(a, b)):
            if u != v:
                return _where(u, v, "%s[%d]" % (path, i))
    if isinstance(a, tuple) and len(a) == 3 and isinstance(a[2], bytes) and a[:2] == b[:2] and a[0] != "f64":
        u, v = np.frombuffer(a[2], a[0]).reshape(a[1]), np.frombuffer(b[2], b[0]).reshape(b[1])
        bad = np.argwhere(u.view(np.uint8).reshape(u.shape + (-1,)).astype(np.int16) != v.view(np.uint8).reshape(v.shape + (-1,)))
        at = tuple(int(t) for t in bad[0][:u.ndim])
        return "%s %s%s: %d elements differ, first at %s: %r against %r" % (path, a[0], a[1], len({tuple(t[:u.ndim]) for t in bad}), at, u[at], v[at])
    return "%s: %r against %r" % (path, a, b)


# ---- content (seeded, built once) ---------------------------------------------------------------------------------------
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _stack(n, w, h, depth=8, bright=False):
    """A synthetic stack on the device; bright: its upper half of the value range (a neighbour's content), still alignable."""
    def make():
        t = synth.make_stack(n, w, h, depth=depth, device="cuda")[0].contiguous()
        if bright and depth == 16:
            a = t.cpu().numpy().view(np.uint16)
            return torch.from_numpy((a // 2 + 32768).astype(np.uint16)).cuda().contiguous()
        return (t // 2 + 128).contiguous() if bright else t
    return _memo(("stack", n, w, h, depth, bright), make)


def _noise(n, w, h, seed):
    """Bright random frames: what a neighbour of a caller-held-warps case folds."""
    def make():
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.randint(128, 256, (n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)
    return _memo(("noise", n, w, h, seed), make)


def _field(shape, lo, hi, seed, dtype=torch.float32, nonfinite=False):
    def make():
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        t = (torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo).to(dtype)
        return _plant(t.contiguous()) if nonfinite else t.contiguous()
    return _memo(("field", tuple(shape), lo, hi, seed, str(dtype), nonfinite), make)


def _warps(n):
    out = []
    for i in range(n):
        M = np.eye(3)
        M[0, 2], M[1, 2] = 0.7 * i, -0.4 * i
        out.append(M)
    return out


def _grid(w, h):
    gw, gh = mesh_grid(w, h, STEP)
    return gh, gw


def _plant(a):
    """NaN and +-inf planted in a float32 array, in place (a neighbour's f32 inputs, where the call takes them)."""
    flat = a.reshape(-1)
    flat[7::97] = float("nan")
    flat[11::193] = float("inf")
    flat[13::389] = float("-inf")
    return a


def _norm_planes(w, h, n, seed, nonfinite=False):
    rng = np.random.default_rng(seed)
    gh, gw = _grid(w, h)
    planes = [np.concatenate([rng.uniform(0.5, 2.0, (gh, gw, 3)), rng.uniform(-0.1, 0.1, (gh, gw, 3))], -1).astype(np.float32)
              for _ in range(n - 1)]
    return [None] + [_plant(p) if nonfinite else p for p in planes]


def _star_stack(k):
    def make():
        w, h, n = G_STAR[k]
        mots = [None] + [synth.star_motion(w, h, 3.0 * i, 1.5 * i, -1.0 * i) for i in range(1, n)]
        fr = synth.make_star_stack(mots, w, h, 60, seed=9 + k)[0]
        if k:                                                  # the neighbour: the same kind of field under a bright sky
            fr = np.minimum(fr.astype(np.int32) + 100, 255).astype(np.uint8)
        return torch.from_numpy(fr).cuda()
    return _memo(("stars", k), make)


def _put(where, x):
    """x where the case's frames live: a device tensor as it is, or its host copy (a 4-d stack as a list of frames)."""
    if where == "dev" or x is None:
        return x
    if isinstance(x, list):
        return [_put(where, v) for v in x]
    if isinstance(x, torch.Tensor):
        a = x.cpu().numpy()
        return list(a) if a.ndim == 4 else a
    return x


def _grey(k, w, h):
    """An 8-bit grey image on the host (the stage-level calls take host images)."""
    return _memo(("grey", k, w, h), lambda: np.ascontiguousarray(_stack(2, w, h, bright=bool(k))[1].float().mean(-1).round().byte().cpu().numpy()))


def _points(n, seed, outliers=None):
    """Point pairs under a homography: a tenth of them (or the fraction `outliers`) outliers, the rest with a little noise."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 600, (n, 2))
    H = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
    p = np.concatenate([src, np.ones((n, 1))], 1) @ H.T
    dst = p[:, :2] / p[:, 2:] + rng.normal(0, 0.3, (n, 2))
    bad = rng.choice(n, n // 10 if outliers is None else int(outliers * n), replace=False)
    dst[bad] = rng.uniform(0, 600, (len(bad), 2))
    return src.astype(np.float32), dst.astype(np.float32)


def _point_batch(k, seed):
    """A batch for find_homography_batch whose members end in different rounds (10 %, 50 % and 70 % of outliers), with a
    member that never reaches the device (3 points) and one that needs no round (4 points) between them; the neighbour's
    batch is larger in every buffer."""
    plan = ([(3, 0.0), (129, 0.7), (40, 0.1), (4, 0.0), (65, 0.5), (300, 0.1), (64, 0.7)],
            [(500, 0.7), (5, 0.0), (200, 0.5), (700, 0.1), (3, 0.0), (100, 0.7), (90, 0.5), (33, 0.1), (260, 0.7)])[k]
    return [_points(n, seed + 10 * i, f) for i, (n, f) in enumerate(plan)]


# ---- the catalogue ------------------------------------------------------------------------------------------------------
class Case:
    """build(k) -> run(stacker): k = 0 the case itself, k = 1 its neighbour. options: set for the call, restored behind it."""

    def __init__(self, name, build, options=None):
        self.name, self.build, self.options = name, build, options or {}
        self._run = {}

    def _call(self, st, k):
        if k not in self._run:
            self._run[k] = self.build(k)
        try:
            for o, v in self.options.items():
                st.set_option(o, v)
            return self._run[k](st)
        finally:
            for o in self.options:
                st.set_option(o, OPTION_DEFAULTS[o])

    def run(self, st):
        return _bits(self._call(st, 0))

    def neighbour(self, st):
        """The neighbour's result does not matter, only what it leaves behind — but it must run: a neighbour that is refused
        (for its arguments, or because it does not align) would leave nothing behind and make the case's visit vacuous, so
        no refusal is caught here. The whole-stack neighbours are bright but alignable stacks for that reason."""
        self._call(st, 1)


CATALOGUE = []
BY_NAME = {}


def case(name, options=None):
    def register(build):
        c = Case(name, build, options)
        CATALOGUE.append(c)
        BY_NAME[name] = c
        return build
    return register


# ECC ---------------------------------------------------------------------------------------------------------------------
def _ecc_frames(k, n=None, where="dev"):
    w, h, n0 = G_ECC[k]
    return _put(where, _stack(n or n0, w, h, bright=bool(k)))


@case("ecc_match homography, host-fed")
def _(k):
    fr = _ecc_frames(k, where="host")
    return lambda st: st.ecc_match(fr, ECC, return_stats=True)


@case("ecc_match affine")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match(fr, ECC_AFFINE, return_stats=True)


@case("ecc_match scale_down_width")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match(fr, ECC, (160, 150)[k], return_stats=True)


@case("ecc_match resident, 12 frames, overlapped preparation", {"ecc_slots": 4, "prep_overlap": 1})
def _(k):
    w, h, _n = G_ECC[k]
    fr = _stack((12, 14)[k], w, h, bright=bool(k))
    return lambda st: st.ecc_match(fr, ECC, return_stats=True)


@case("find_transform_ecc")
def _(k):
    w, h, _n = G_ECC[k]
    fr = _stack(2, w, h, bright=bool(k)).float().mean(-1).round().byte().cpu().numpy()
    return lambda st: st.find_transform_ecc(fr[0], fr[1], np.eye(3, dtype=np.float32), ECC)


@case("hybrid_match 8 bit")
def _(k):
    w, h, n = G_ORB[k]
    fr = _stack(n, w, h, bright=bool(k))
    return lambda st: st.hybrid_match(fr, KP, ECC_HYBRID, return_stats=True)


@case("hybrid_match 16 bit")
def _(k):
    w, h, n = G_ORB[k]
    fr = _stack(n, w, h, depth=16, bright=bool(k))
    return lambda st: st.hybrid_match(fr, KP, ECC_HYBRID, return_stats=True)


# keypoint and homography -------------------------------------------------------------------------------------------------
def _orb_frames(k, n=None, where="dev"):
    w, h, n0 = G_ORB[k]
    return _put(where, _stack(n or n0, w, h, bright=bool(k)))


@case("keypoint_match host-fed")
def _(k):
    fr = _orb_frames(k, where="host")
    return lambda st: st.keypoint_match(fr, KP, return_stats=True)


@case("keypoint_match resident")
def _(k):
    fr = _orb_frames(k)
    return lambda st: st.keypoint_match(fr, KP, return_stats=True)


@case("keypoint_match resident, 16 frames, two lanes", {"kp_lanes": 2})
def _(k):
    fr = _orb_frames(k, (16, 18)[k])
    return lambda st: st.keypoint_match(fr, KP, return_stats=True)


@case("keypoint_match two lanes, scaled, LMEDS, whole-level blur", {"kp_lanes": 2, "orb_patch_blur": 0})
def _(k):
    fr = _orb_frames(k, (16, 18)[k])
    return lambda st: st.keypoint_match(fr, KP_LMEDS, (320, 300)[k], return_stats=True)


@case("keypoint_match scale_down_width")
def _(k):
    fr = _orb_frames(k)
    return lambda st: st.keypoint_match(fr, KP, (320, 300)[k], return_stats=True)


@case("keypoint_match_mixed")
def _(k):
    fr = _orb_frames(k, where="host")
    cut = (24, 40)[k]
    mixed = [fr[0]] + [np.ascontiguousarray(f[i * 4:f.shape[0] - cut, i * 4:f.shape[1] - cut + 8]) for i, f in enumerate(fr[1:], 1)]
    return lambda st: st.keypoint_match(mixed, KP, return_stats=True)


@case("keypoint_match with a featureless frame dropped")
def _(k):
    fr = _orb_frames(k, where="host")
    fr = list(fr[:2]) + [np.full_like(fr[0], 128)] + list(fr[2:])
    return lambda st: st.keypoint_match(fr, KP, return_stats=True)


@case("orb_detect_and_compute 517 x 301")
def _(k):
    g = _grey(k, *((517, 301), (600, 260))[k])
    return lambda st: st.orb_detect_and_compute(g)


@case("orb_detect_and_compute 129 x 200")
def _(k):
    g = _grey(k, *((129, 200), (100, 260))[k])
    return lambda st: st.orb_detect_and_compute(g)


@case("orb_detect_and_compute whole-level blur, host cull", {"orb_patch_blur": 0, "orb_device_cull": 0})
def _(k):
    g = _grey(k, *((517, 301), (600, 260))[k])
    return lambda st: st.orb_detect_and_compute(g)


@case("bf_knn2_hamming")
def _(k):
    rng = np.random.default_rng(50 + k)
    q = rng.integers(0, 256, ((300, 500)[k], 32), dtype=np.uint8)
    t = rng.integers(0, 256, ((257, 100)[k], 32), dtype=np.uint8)
    return lambda st: st.bf_knn2_hamming(q, t)


@case("find_homography RANSAC")
def _(k):
    s, d = _points((200, 350)[k], 60 + k)
    return lambda st: st.find_homography(s, d, RANSAC, 3.0)


@case("find_homography LMEDS")
def _(k):
    s, d = _points((200, 350)[k], 62 + k)
    return lambda st: st.find_homography(s, d, LMEDS, 3.0)


@case("find_homography_batch RANSAC")
def _(k):
    batch = _point_batch(k, 600 + k)
    return lambda st: st.find_homography_batch(batch, RANSAC, 3.0)


@case("find_homography_batch LMEDS")
def _(k):
    batch = _point_batch(k, 640 + k)
    return lambda st: st.find_homography_batch(batch, LMEDS, 3.0)


# star registration -------------------------------------------------------------------------------------------------------
for _where_ in ("dev", "host"):
    def _star_cases(where):
        @case("star_detect (%s)" % where)
        def _(k):
            fr = _put(where, _star_stack(k))
            return lambda st: st.star_detect(fr, StarParameters(), return_peaks=True)

        @case("star_align (%s)" % where)
        def _(k):
            fr = _put(where, _star_stack(k))
            return lambda st: st.star_align(fr, StarParameters())

        @case("star_match (%s)" % where)
        def _(k):
            fr = _put(where, _star_stack(k))
            return lambda st: st.star_match(fr, StarParameters(), return_stats=True)
    _star_cases(_where_)


# caller-held-warps combines, device-resident and host-fed -------------------------------------------------------------
def _family(where):
    def fam(k):
        """Frames, warps and side inputs of geometry k where `where` says."""
        w, h, n = G_FAM[k]
        fr = _stack(n, w, h) if k == 0 else _noise(n, w, h, 70)
        gh, gw = _grid(w, h)
        bad = bool(k)          # the neighbour's f32 inputs carry NaN and +-inf: every one of them is documented as unchecked or as
        # defined on non-finite values (include/stacker.h: weight maps, mesh fields, norm planes, the clean image, the masters)
        d = dict(w=w, h=h, n=n, fr=_put(where, fr), wp=_warps(n),
                 maps=_put(where, _field((n, h, w), 0.0, 3.0, 21 + k, nonfinite=bad)),
                 fields=_put(where, _field((n, gh, gw, 2), -1.5, 1.5, 22 + k, nonfinite=bad)),
                 norm=_norm_planes(w, h, n, 24 + k, nonfinite=bad),
                 clean=_put(where, _memo(("clean", k), lambda: (_plant if bad else (lambda t: t))((fr.float().mean(0) / 255.0).contiguous()))),
                 counts=_put(where, _memo(("counts", k), lambda: torch.randint(3, n + 1, (h, w), device="cuda", dtype=torch.int32,
                                                                                generator=torch.Generator(device="cuda").manual_seed(23 + k)))),
                 bias=_put(where, _field((h, w, 3), 8.0, 12.0, 31 + k, nonfinite=bad)),
                 dark=_put(where, _field((h, w, 3), 1.0, 3.0, 33 + k, nonfinite=bad)),
                 flat=_put(where, _field((h, w, 3), 90.0, 110.0, 35 + k, nonfinite=bad)),
                 defects=_put(where, _memo(("defects", k), lambda: ((_field((h, w), 0.0, 1.0, 37 + k) < 0.01).to(torch.uint8) * 5).contiguous())))
        return d

    def add(name, call, options=None):
        @case("%s (%s)" % (name, where), options)
        def _(k):
            a = fam(k)
            return lambda st: call(st, a)

    mesh = MeshParameters(step=STEP)
    add("clip_stack", lambda st, a: st.clip_stack(a["fr"], a["wp"], SigmaClipParameters(), return_counts=True))
    add("quantile_stack", lambda st, a: st.quantile_stack(a["fr"], a["wp"]))
    add("weighted_stack", lambda st, a: st.weighted_stack(a["fr"], a["wp"], return_coverage=True))
    add("overlap_moments", lambda st, a: st.overlap_moments(a["fr"], a["wp"]))
    add("robust_clip_stack", lambda st, a: st.robust_clip_stack(a["fr"], a["wp"], RobustClipParameters(), return_counts=True))
    add("clip_stack_weighted", lambda st, a: st.clip_stack_weighted(a["fr"], a["wp"], weights=np.linspace(0.5, 1.5, a["n"]),
                                                                     return_counts=True, return_kept_weight=True))
    add("quantile_stack_weighted", lambda st, a: st.quantile_stack_weighted(a["fr"], a["wp"], 0.3, weights=np.linspace(0.5, 1.5, a["n"]),
                                                                             return_counts=True))
    add("local_sharpness", lambda st, a: st.local_sharpness(a["fr"], LocalParameters()))
    add("local_weighted_stack", lambda st, a: st.local_weighted_stack(a["fr"], a["wp"], a["maps"], return_coverage=True))
    add("local_align", lambda st, a: st.local_align(a["fr"], a["wp"], mesh, return_status=True))
    add("local_align_pyramid", lambda st, a: st.local_align_pyramid(a["fr"], a["wp"], mesh, 2, return_status=True))
    add("mesh_stack", lambda st, a: st.mesh_stack(a["fr"], a["wp"], a["fields"], STEP))
    add("mesh_local_weighted_stack", lambda st, a: st.mesh_local_weighted_stack(a["fr"], a["wp"], a["maps"], a["fields"], STEP))
    add("drizzle_stack scale 2", lambda st, a: st.drizzle_stack(a["fr"], a["wp"], DrizzleParameters(scale=2.0), maps=a["maps"], return_den=True))
    add("mesh_drizzle_stack scale 2", lambda st, a: st.mesh_drizzle_stack(a["fr"], a["wp"], a["fields"], STEP, DrizzleParameters(scale=2.0),
                                                                           return_den=True))
    add("reject_maps", lambda st, a: st.reject_maps(a["fr"], a["wp"], a["clean"], None, a["counts"], maps=a["maps"], return_counts=True))
    add("local_moments then local_norm_stack", lambda st, a: (st.local_moments(a["fr"], a["wp"], STEP),
                                                              st.local_norm_stack(a["fr"], a["wp"], a["norm"], STEP, return_den=True)))
    add("clip_stack_local_norm", lambda st, a: st.clip_stack_local_norm(a["fr"], a["wp"], a["norm"], STEP, return_counts=True))
    add("robust_clip_stack_local_norm", lambda st, a: st.robust_clip_stack_local_norm(a["fr"], a["wp"], a["norm"], STEP, return_counts=True))
    add("quantile_stack_local_norm", lambda st, a: st.quantile_stack_local_norm(a["fr"], a["wp"], a["norm"], STEP, return_counts=True))
    add("calibrate, three masters and a map",
        lambda st, a: st.calibrate(a["fr"], CalibrationParameters(bias=a["bias"], dark=a["dark"], flat=a["flat"],
                                                                  dark_scale=list(np.linspace(0.5, 2.0, a["n"])), flat_mean=[100.0] * 3,
                                                                  flat_min=1.0, defects=a["defects"])))
    add("defect_map", lambda st, a: st.defect_map(a["dark"], DefectParameters(True, False, 0.5), return_counts=True))
    add("image_mean", lambda st, a: st.image_mean(a["flat"]))
    add("master_stack", lambda st, a: st.master_stack(a["fr"], 0, return_counts=True))
    add("stack_sharpness", lambda st, a: st.stack_sharpness(a["fr"], 3))
    add("grey_pyramid", lambda st, a: st.grey_pyramid(a["fr"][1], 4))
    add("warp_accumulate u8 BGR", lambda st, a: st.warp_accumulate(a["fr"][2], a["wp"][2] @ np.array([[1, 0.01, 0], [-0.01, 1, 0], [1e-5, 0, 1]])))
    add("warp_accumulate u8 BGR, cubic", lambda st, a: st.warp_accumulate(a["fr"][2], a["wp"][2]), {"warp_interpolation": 2})


for _where_ in ("dev", "host"):
    _family(_where_)


@case("warp_accumulate f32, 4 channels")
def _(k):
    w, h, _n = G_FAM[k]
    fr = _field((h, w, 4), 0.0, 255.0, 80 + k, nonfinite=bool(k))        # the neighbour: NaN and inf planted
    M = np.array([[1.0, 0.01, 2.5], [-0.01, 1.0, -1.5], [1e-5, 0.0, 1.0]])
    return lambda st: st.warp_accumulate(fr, M)


@case("single-image sharpness metrics")
def _(k):
    w, h, _n = G_FAM[k]
    g = _grey(k, w, h)
    return lambda st: (st.sharpness_modified_laplacian(g), st.sharpness_variance_of_laplacian(g), st.sharpness_tenengrad(g, 3),
                       st.sharpness_normalized_gray_level_variance(g))


@case("scale_image_grey")
def _(k):
    w, h, _n = G_FAM[k]
    g = _grey(k, w, h)
    return lambda st: st.scale_image_grey(g, (50.0, 40.0)[k])


# whole-stack forms, one per family -----------------------------------------------------------------------------------------
@case("ecc_match_clipped")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match_clipped(fr, ECC, SigmaClipParameters(), return_stats=True, return_counts=True)


@case("keypoint_match_quantile")
def _(k):
    fr = _orb_frames(k)
    return lambda st: st.keypoint_match_quantile(fr, KP, 0.5, return_stats=True)


@case("ecc_match_weighted")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match_weighted(fr, ECC, WeightParameters(normalize=3, stat_step=4), return_stats=True, return_coverage=True,
                                            return_applied=True)


@case("ecc_match_robust_clipped, host-fed")
def _(k):
    fr = _ecc_frames(k, where="host")
    return lambda st: st.ecc_match_robust_clipped(fr, ECC, RobustClipParameters(), return_stats=True, return_counts=True)


@case("ecc_match_local_aligned_pyramid")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match_local_aligned_pyramid(fr, ECC, MeshParameters(step=STEP), 2, return_stats=True)


@case("keypoint_match_drizzle_rejected")
def _(k):
    fr = _orb_frames(k)
    return lambda st: st.keypoint_match_drizzle_rejected(fr, KP, DrizzleParameters(scale=2.0), return_den=True, return_maps=True,
                                                         return_rejected=True, return_stats=True)


@case("ecc_match_local_normalized_clipped")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match_local_normalized_clipped(fr, ECC, LocalNormParameters(step=32), SigmaClipParameters(), return_stats=True, return_counts=True,
                                                            return_norm=True)


@case("ecc_match_ranked")
def _(k):
    fr = _ecc_frames(k)
    return lambda st: st.ecc_match_ranked(fr, ECC, SelectParameters(drop_worst=1), return_scores=True, return_stats=True)


# files ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _files_dir(tmp_path_factory):
    _cache["dir"] = tmp_path_factory.mktemp("history")
    yield
    _cache.clear()
    for c in CATALOGUE:
        c._run.clear()


@case("ecc_match_files")
def _(k):
    w, h, n = G_ECC[k]
    paths = []
    for i, f in enumerate(_ecc_frames(k, where="host")):
        p = os.path.join(str(_cache["dir"]), "f%d_%d.ppm" % (k, i))
        with open(p, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(f[..., ::-1]).tobytes())
        paths.append(p)
    return lambda st: st.ecc_match_files(paths, ECC)


NAMES = [c.name for c in CATALOGUE]
assert len(set(NAMES)) == len(NAMES)


# ---- the reference: the case on a context of its own ----------------------------------------------------------------------
_refs = {}


def _reference(name):
    if name not in _refs:
        torch.cuda.synchronize()
        st = Stacker(0)
        try:
            _refs[name] = BY_NAME[name].run(st)
        finally:
            st.close()
    return _refs[name]


def _same(got, name, what):
    want = _reference(name)
    assert got == want, "%s, %s: %s" % (name, what, _where(got, want))


def _poison(st, b):
    st.set_option("debug_poison", b)


# ---- Part 0: the instrument works ---------------------------------------------------------------------------------------------
def test_part0_poison_destroys_what_the_context_held(stacker):
    BY_NAME["ecc_match affine"].run(stacker)
    before = stacker.ecc_prepared()
    assert np.isfinite(before["templates"]).all() and np.isfinite(before["I"]).all()
    _poison(stacker, 0xFF)
    after = stacker.ecc_prepared()
    assert after["templates"].shape == before["templates"].shape            # ecc_prepared's geometry stays valid
    assert np.isnan(after["templates"]).all() and np.isnan(after["I"]).all()
    assert stacker.timing()["debug_poison_bytes"] > 0
    _poison(stacker, 0x7F)
    assert (stacker.ecc_prepared()["I"].view(np.uint32) == 0x7F7F7F7F).all()


@pytest.mark.parametrize("value", [-1, 256, 1 << 40])
def test_part0_poison_refuses_what_is_no_byte(stacker, value):
    BY_NAME["ecc_match affine"].run(stacker)
    before = _bits(stacker.ecc_prepared())
    filled = stacker.timing()["debug_poison_bytes"]
    with pytest.raises(InvalidParams):
        stacker.set_option("debug_poison", value)
    assert _bits(stacker.ecc_prepared()) == before and stacker.timing()["debug_poison_bytes"] == filled


def test_part0_the_catalogue_reaches_every_workspace():
    """On a context of its own, not the session's: how many lane contexts the session's owns depends on the files that ran
    before this one (resident stacks of 24 frames and more under the default of three lanes), and the lanes beyond the
    first are reached by none of this file's cases, so no number could be asserted there. Unreached here: LANE_UNREACHED
    per lane context, one lane context. The references are made first, so that this context is the second one alive."""
    for c in CATALOGUE:
        _reference(c.name)
    st = Stacker(0)
    try:
        n0 = st.timing()["workspaces_empty"]
        assert n0 == 22 + 16 + 8                                           # stk_ctx, KeypointWorkspace, HgWorkspace: all empty
        for c in CATALOGUE:
            assert c.run(st) == _refs[c.name], c.name
        assert st.timing()["workspaces_empty"] == LANE_UNREACHED * 1
    finally:
        st.close()


# ---- Part A: after a poison ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xFF, 0x7F])
@pytest.mark.parametrize("name", NAMES)
def test_partA_after_poison(stacker, name, byte):
    _reference(name)
    _poison(stacker, byte)
    _same(BY_NAME[name].run(stacker), name, "after debug_poison 0x%02X" % byte)


# ---- Part B: after the neighbour ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_partB_after_the_neighbour(stacker, name):
    c = BY_NAME[name]
    for visit in (1, 2):
        c.neighbour(stacker)
        _same(c.run(stacker), name, "visit %d behind its neighbour" % visit)


def _ecc_at(w, h, n, depth=8):
    fr = _stack(n, w, h, depth=depth)
    if depth == 16:
        return lambda st: _bits(st.hybrid_match(fr, KP, ECC_HYBRID, return_stats=True))
    return lambda st: _bits(st.ecc_match(fr, ECC, return_stats=True))


def _fresh(run):
    st = Stacker(0)
    try:
        return run(st)
    finally:
        st.close()


def test_partB_ecc_border_cache_across_geometries(stacker):
    """320 x 240, 256 x 200, 320 x 240 again: nothing in between touches ctx->ref, so the second visit of a geometry finds
    the reference planes' zero border through the cache or not at all."""
    big, small, larger = _ecc_at(320, 240, 4), _ecc_at(256, 200, 4), _ecc_at(384, 288, 4)
    want_big, want_small = _fresh(big), _fresh(small)
    assert big(stacker) == want_big
    assert small(stacker) == want_small
    assert big(stacker) == want_big
    assert small(stacker) == want_small
    # the cache HIT: the key (ctx->ref.p, w, h) is unchanged only when a geometry repeats back to back. Behind a larger call
    # (which leaves its planes behind the smaller geometry's extents) each geometry runs three times in a row: the first run
    # zeroes the border, the second and third find it through the cache
    for run, want in ((big, want_big), (small, want_small)):
        larger(stacker)
        for visit in (1, 2, 3):
            assert run(stacker) == want, "visit %d in a row behind the larger call" % visit


def test_partB_ecc_u8_then_hybrid_16_bit_of_the_same_size(stacker):
    u8, u16 = _ecc_at(320, 240, 4), _ecc_at(320, 240, 4, depth=16)
    want8, want16 = _fresh(u8), _fresh(u16)
    assert u8(stacker) == want8
    assert u16(stacker) == want16
    assert u8(stacker) == want8
    assert u16(stacker) == want16


@pytest.mark.parametrize("tables", [1, 0])
def test_partB_orb_resize_tables_across_geometries(stacker, tables):
    a, b = BY_NAME["orb_detect_and_compute 517 x 301"], BY_NAME["orb_detect_and_compute 129 x 200"]
    try:
        stacker.set_option("orb_resize_tables", tables)
        for c in (a, b, a, b):
            _same(c.run(stacker), c.name, "orb_resize_tables = %d, alternating geometries" % tables)
    finally:
        stacker.set_option("orb_resize_tables", 1)


@pytest.mark.parametrize("where", ["dev", "host"])
def test_partB_one_buffer_four_layouts(stacker, where):
    """drizzle_stack, star_detect, calibrate, local_norm_stack: ctx->local as a DrizzleLayout, a StarLayout, a CalLayout and a
    NormLayout in turn; then robust_clip_stack and quantile_stack through ctx->quantile."""
    for _ in (1, 2):
        for name in ("drizzle_stack scale 2", "star_detect", "calibrate, three masters and a map", "local_moments then local_norm_stack",
                     "robust_clip_stack", "quantile_stack"):
            name = "%s (%s)" % (name, where)
            _same(BY_NAME[name].run(stacker), name, "in the shared-buffer sequence")


def test_partB_host_fed_before_and_after_the_frame_workspace_grows():
    """A host-fed stack under upload_batch = 2 on a context whose frame workspace is empty (small batches), then a 16-frame
    call that grows it, then the first stack again (batches as large as the workspace allows)."""
    w, h, _n = G_ECC[0]
    five, sixteen = _put("host", _stack(5, w, h)), _put("host", _stack(16, w, h))
    calls = {"ecc": lambda st, fr: _bits(st.ecc_match(fr, ECC, return_stats=True)),
             "sharpness": lambda st, fr: _bits(st.stack_sharpness(fr, 3)),
             "local_sharpness": lambda st, fr: _bits(st.local_sharpness(fr, LocalParameters()))}
    for label, call in calls.items():
        want = _fresh(lambda st: call(st, five))
        st = Stacker(0)
        try:
            st.set_option("upload_batch", 2)
            assert call(st, five) == want, label + ": empty frame workspace, upload_batch = 2"
            call(st, sixteen)
            assert call(st, five) == want, label + ": behind the 16-frame call"
            st.set_option("debug_poison", 0xFF)
            assert call(st, five) == want, label + ": grown workspace, poisoned"
        finally:
            st.close()


# ---- Part C: shuffled ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [101, 202, 303])
def test_partC_shuffled_catalogue(stacker, seed):
    rng = np.random.default_rng(seed)
    order = [NAMES[i] for i in rng.permutation(len(NAMES))]
    trail = []
    for name in order:
        if rng.random() < 0.5:
            other = NAMES[int(rng.integers(len(NAMES)))]
            trail.append("~" + other)
            BY_NAME[other].neighbour(stacker)
        trail.append(name)
        got = BY_NAME[name].run(stacker)
        want = _reference(name)
        assert got == want, "seed %d, %s behind %s: %s" % (seed, name, trail[-6:-1], _where(got, want))


# ---- Part D: a multi-device context [0, 0] ------------------------------------------------------------------------------------
MULTI = ["ecc_match affine", "keypoint_match resident", "hybrid_match 8 bit"]


_multi_refs = {}


@pytest.fixture(scope="module")
def multi():
    """The shared [0, 0] context, made after the references (each on a fresh [0, 0] context, closed again): two alive at most."""
    for name in MULTI:
        fresh = Stacker(devices=[0, 0])
        try:
            _multi_refs[name] = BY_NAME[name].run(fresh)
        finally:
            fresh.close()
    m = Stacker(devices=[0, 0])
    yield m
    m.close()


@pytest.mark.parametrize("name", MULTI)
def test_partD_multi_device_context(multi, name):
    c, want = BY_NAME[name], _multi_refs[name]
    for byte in (0xFF, 0x7F):
        multi.set_option("debug_poison", byte)
        assert multi.timing()["debug_poison_bytes"] > 0
        got = c.run(multi)
        assert got == want, "%s on [0, 0] after debug_poison 0x%02X: %s" % (name, byte, _where(got, want))
    for visit in (1, 2):
        c.neighbour(multi)
        got = c.run(multi)
        assert got == want, "%s on [0, 0], visit %d behind its neighbour: %s" % (name, visit, _where(got, want))
    with pytest.raises(InvalidParams):
        multi.set_option("debug_poison", 256)

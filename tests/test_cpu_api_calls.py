"""What libstacker_rs_amd/api.py hands to the C ABI, call by call, without a GPU.

A Stacker is built with Stacker.__new__ around a recording stand-in for the library: an object whose stk_* attributes
exist exactly for the names of _ffi.SIGNATURES. Every function of status type is a ctypes callback of that signature, so a
call with a wrong argument count or an argument of the wrong kind fails as it would on the real library; the callback
snapshots what it was given (scalars, the bytes of every parameter struct, the geometry and the bytes of stk_frames, the
host buffers the case names) AT CALL TIME, and returns 0. The context-free host functions (stk_mesh_grid, ...) are the real
library's.

Checked for every name in SIGNATURES that takes stk_frames (but EXEMPT, each with its reason): the C function called, every
scalar, the bytes of every parameter struct, which optional pointers are NULL, that every output address passed is the
address of the array later returned (with its documented shape and dtype), that every host input buffer read through the
passed address at call time holds what the caller gave, the type, length and order of the result for every combination of
the return_* flags, and the refusals the wrapper itself raises."""
import ctypes as C
import itertools

import numpy as np
import pytest

from libstacker_rs_amd import _ffi
from libstacker_rs_amd.api import (BORDER_REFLECT, BORDER_REPLICATE, HOST, RANSAC, CalibrationParameters, DrizzleParameters,
                                   EccMatchParameters, InvalidParams, KeyPointMatchParameters, LocalNormParameters, LocalParameters,
                                   MeshParameters, MotionType, NotEnoughFiles, OpenCvError, QuantileParameters, RejectParameters,
                                   RobustClipParameters, SelectParameters, SigmaClipParameters, Stacker, StarParameters,
                                   WeightParameters, mesh_grid)

CTX = 0x5150
N, H, W, CH = 3, 8, 12, 3
STEP = 8
_rng = np.random.default_rng(5)
U8 = _rng.integers(0, 256, (N, H, W, CH), dtype=np.uint8)
GREY = _rng.integers(0, 256, (N, H, W), dtype=np.uint8)
U16 = _rng.integers(0, 65536, (N, H, W, CH), dtype=np.uint16)
ECC = EccMatchParameters(MotionType.Affine, 50, 1e-3, 3)
KP = KeyPointMatchParameters(RANSAC, 4.0, 0.7, 0.85, BORDER_REPLICATE, (1.0, 2.0, 3.0))
PARAMS = {"ecc": ECC, "keypoint": KP}
SDW = 6.5
ECC_SIZES = "the frames differ in size: the reference fails on such a stack in cv::add (lib.rs:809)"
HOST_FUNCS = {"stk_mesh_grid", "stk_local_norm_estimate", "stk_rank_frames", "stk_star_match_lists", "stk_shard_moving_frames"}
# names that take stk_frames and are not driven here: they need device tensors
EXEMPT = {
    "stk_ecc_match_shard": "sum_out is a device tensor by contract (stk_image_f32 with location DEVICE; _tensor_ready asks torch for its stream)",
    "stk_keypoint_match_shard": "sum_out is a device tensor by contract (as stk_ecc_match_shard)",
    "stk_hybrid_match_shard": "sum_out is a device tensor by contract (as stk_ecc_match_shard)",
}
P_FRAMES, P_IMAGE, P_I32 = C.POINTER(_ffi.Frames), C.POINTER(_ffi.ImageF32), C.POINTER(C.c_int32)
P_STATS, P_WEIGHT, P_GEO, P_CAL = (C.POINTER(_ffi.FrameStats), C.POINTER(_ffi.FrameWeight), C.POINTER(_ffi.FrameGeometry),
                                   C.POINTER(_ffi.Calibration))
P_HG, P_HGOUT = C.POINTER(_ffi.HgProblem), C.POINTER(_ffi.HgOutcome)
SEEN = set()


def _bytes_of(s):
    return bytes(C.string_at(C.addressof(s), C.sizeof(s)))


class Recorder:
    """The stand-in for libstacker_amd.so. reads: {argument index: nbytes | ("tbl", count, nbytes per entry)} to snapshot
    behind void pointers; pokes: {argument index: int or list} written through int32 pointers; status: {frame: status}
    written into the stats; outcomes: [(rc, found, H, n_inliers, models_evaluated)] written into stk_hg_outcome records."""

    def __init__(self):
        self.calls, self.reads, self.pokes, self.status, self.outcomes = [], {}, {}, {}, []
        real = _ffi.load()
        for name, (res, argtypes) in _ffi.SIGNATURES.items():
            if name in HOST_FUNCS:
                fn = getattr(real, name)
            elif res is not _ffi.c_status:
                fn = (lambda *a: None)
            else:
                fn = C.CFUNCTYPE(res, *argtypes)(self._entry(name, argtypes))
            setattr(self, name, fn)

    def _entry(self, name, argtypes):
        def entry(*args):
            SEEN.add(name)
            try:
                self.calls.append((name, self._snapshot(argtypes, args)))
            except Exception as e:                     # an exception cannot cross the callback: handed to last()
                self.calls.append((name, e))
            return 0
        return entry

    def _snapshot(self, argtypes, args):
        assert len(args) == len(argtypes)
        out, n = [], 0
        for i, (t, a) in enumerate(zip(argtypes, args)):
            if t is P_FRAMES:
                f = a.contents
                n = f.n
                row = f.width * f.channels * (f.depth // 8)
                ptrs = [f.data[k] for k in range(n)]
                assert f.row_stride_bytes in (0, row)
                out.append(dict(n=n, width=f.width, height=f.height, channels=f.channels, depth=f.depth, location=f.location,
                                stride=f.row_stride_bytes, ptrs=ptrs, data=[C.string_at(p, row * f.height) for p in ptrs]))
            elif t is P_IMAGE:
                out.append(None if not a else {k: getattr(a.contents, k) for k, _ in _ffi.ImageF32._fields_})
            elif t is P_I32:
                if a and i in self.pokes:
                    for k, v in enumerate(np.atleast_1d(self.pokes[i])):
                        a[k] = int(v)
                out.append(C.addressof(a.contents) if a else None)
            elif t is P_STATS:
                if a:
                    for k, v in self.status.items():
                        a[k].status = v
                out.append(C.addressof(a.contents) if a else None)
            elif t is P_WEIGHT:
                out.append(bytes(C.string_at(C.addressof(a.contents), n * C.sizeof(_ffi.FrameWeight))) if a else None)
            elif t is P_GEO:
                out.append([(a[k].width, a[k].height, a[k].row_stride_bytes) for k in range(n)])
            elif t is P_CAL:
                c = a.contents
                imgs = {k: (None if not getattr(c, k + "_or_null") else
                            {f: getattr(getattr(c, k + "_or_null").contents, f) for f, _ in _ffi.ImageF32._fields_})
                        for k in ("bias", "dark", "flat")}
                scale = c.dark_scale_or_null
                out.append(dict(imgs, dark_scale=None if not scale else bytes(C.string_at(scale, 4 * n)), flat_mean=list(c.flat_mean), flat_min=c.flat_min,
                                pedestal=c.pedestal, defects=c.defects_or_null, defects_location=c.defects_location,
                                defect_step=c.defect_step, out_depth=c.out_depth))
            elif t is P_HG:                                      # `count` problems: the count is the next argument
                out.append([dict(n=a[k].n, src=bytes(C.string_at(a[k].src_pts, 8 * a[k].n)), dst=bytes(C.string_at(a[k].dst_pts, 8 * a[k].n)),
                                 mask=a[k].inlier_mask_or_null) for k in range(args[i + 1])])
            elif t is P_HGOUT:
                for k, (rc, found, Hm, n_in, n_ev) in enumerate(self.outcomes):
                    a[k].rc, a[k].found, a[k].n_inliers, a[k].models_evaluated = rc, found, n_in, n_ev
                    a[k].H[:] = list(Hm)
                out.append(C.addressof(a.contents) if a else None)
            elif isinstance(t, type) and issubclass(t, C._Pointer):
                out.append(_bytes_of(a.contents) if a else None)
            elif t is C.c_void_p and i in self.reads and a:
                spec = self.reads[i]
                if isinstance(spec, tuple):
                    ptrs = list((C.c_void_p * spec[1]).from_address(a))
                    out.append((a, ptrs, [None if p is None else bytes(C.string_at(p, spec[2])) for p in ptrs]))
                else:
                    out.append((a, bytes(C.string_at(a, spec))))
            else:
                out.append(a)
        return out

    def last(self):
        name, snap = self.calls[-1]
        if isinstance(snap, Exception):
            raise snap
        return name, snap


def new_stacker():
    st = Stacker.__new__(Stacker)
    st._lib, st._h, st.device, st.devices, st._bound_stream = Recorder(), C.c_void_p(CTX), 0, [0], None
    return st


def test_the_stand_in_has_exactly_the_declared_names_and_checks_kinds():
    rec = Recorder()
    assert {k for k in vars(rec) if k.startswith("stk_")} == set(_ffi.SIGNATURES)
    with pytest.raises(AttributeError):
        rec.stk_no_such_function
    with pytest.raises(TypeError):
        rec.stk_grey(C.c_void_p(CTX), None)                                # an argument short
    with pytest.raises(C.ArgumentError):
        rec.stk_grey(C.c_void_p(CTX), C.byref(_ffi.ImageF32()), None)       # a pointer of the wrong kind
    assert mesh_grid(W, H, STEP) == (3, 2) and not rec.calls                # the real library's


# ---- descriptors: one per C argument behind ctx -------------------------------------------------------------------------
def addr(a):
    return a.ctypes.data


def frames_of(files):
    a = np.asarray(files)
    return a if a.ndim == 4 else a[..., None]


def run(st, method, cname, descs, *args, pokes=None, status=None, **kw):
    """The call, and the check of every C argument against its descriptor. A descriptor that names a result ("img", "out",
    "outtbl", "planes") takes a function of the result that picks the array (None: the flag is off, the pointer NULL)."""
    rec = st._lib
    rec.reads, rec.pokes, rec.status = {}, dict(pokes or {}), dict(status or {})
    for i, d in enumerate(descs, start=1):
        if d[0] == "buf" and d[1] is not None:
            rec.reads[i] = np.asarray(d[1]).nbytes
        elif d[0] == "tbl" and d[1] is not None:
            rec.reads[i] = ("tbl", len(d[1]), max([np.asarray(p).nbytes for p in d[1] if p is not None] + [0]))
        elif d[0] in ("outtbl", "planes"):
            rec.reads[i] = ("tbl", N, 0)
        elif d[0] == "i32" and d[1] is not None:
            rec.pokes[i] = d[1]
    before = len(rec.calls)
    res = getattr(st, method)(*args, **kw)
    assert len(rec.calls) == before + 1, "one C call per wrapper call"
    name, snap = rec.last()
    assert name == cname
    assert snap[0] == CTX and len(snap) == len(descs) + 1
    for i, (d, s) in enumerate(zip(descs, snap[1:]), start=1):
        kind, where = d[0], "%s argument %d %r" % (cname, i, d[0])
        if kind == "frames":
            fr = frames_of(d[1])
            assert (s["n"], s["height"], s["width"], s["channels"], s["depth"], s["location"], s["stride"]) == \
                (fr.shape[0], fr.shape[1], fr.shape[2], fr.shape[3], fr.itemsize * 8, HOST, 0), where
            assert s["data"] == [fr[k].tobytes() for k in range(fr.shape[0])], where
        elif kind == "val":
            assert s == d[1] and type(s) is type(d[1]), (where, s, d[1])
        elif kind == "struct":
            assert s == (None if d[1] is None else _bytes_of(d[1])), where
        elif kind == "buf":                                      # a host input buffer, or NULL
            assert (s is None) if d[1] is None else (s[1] == np.asarray(d[1]).tobytes()), where
        elif kind == "tbl":                                      # a table of input planes, entries may be NULL
            if d[1] is None:
                assert s is None, where
            else:
                assert [None if p is None else p[:np.asarray(q).nbytes] for p, q in zip(s[2], d[1])] == \
                    [None if q is None else np.asarray(q).tobytes() for q in d[1]], where
        elif kind == "rec":                                      # stk_frame_weight records, or NULL
            assert s == (None if d[1] is None else _bytes_of(d[1])), where
        elif kind == "img":                                      # the stk_image_f32 of a returned array
            a = d[1](res)
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == d[2] and a.flags.c_contiguous, where
            assert s == dict(data=addr(a), width=d[2][1], height=d[2][0], channels=d[2][2], location=HOST, row_stride_bytes=0), where
        elif kind == "out":                                      # an optional output array
            a = d[1](res) if d[1] else None
            if a is None:
                assert s is None, where
            else:
                assert isinstance(a, np.ndarray) and a.dtype == d[2] and a.shape == d[3] and a.flags.c_contiguous, where
                assert s == addr(a), where
        elif kind == "outtbl":                                   # an optional n x plane output array behind a pointer table
            a = d[1](res) if d[1] else None
            if a is None:
                assert s is None, where
            else:
                assert isinstance(a, np.ndarray) and a.dtype == d[2] and a.shape == d[3] and a.flags.c_contiguous, where
                assert s[1] == [addr(a) + k * a[0].nbytes for k in range(a.shape[0])], where
        elif kind == "planes":                                   # optional per-frame norm planes; d[2]: the frames without one
            a = d[1](res) if d[1] else None
            if a is None:
                assert s is None, where
            else:
                assert isinstance(a, list) and len(a) == N and all(p is not None for p in s[1]), where
                for k in range(N):
                    if k in d[2]:
                        assert a[k] is None, where
                    else:
                        assert a[k].dtype == np.float32 and a[k].shape == d[3] and addr(a[k]) == s[1][k], where
        elif kind == "i32":                                      # an int32 the engine writes: never NULL
            assert s is not None, where
        elif kind == "ptr":                                      # stats, applied: never NULL
            assert s is not None, where
        else:
            raise AssertionError(kind)
    return res


def records(gain=None, offset=None, weights=None, c=CH):
    rec = (_ffi.FrameWeight * N)()
    for i in range(N):
        for k in range(4):
            rec[i].gain[k] = float(gain[i][k]) if gain is not None and k < c else 1.0
            rec[i].offset[k] = float(offset[i][k]) if offset is not None and k < c else 0.0
        rec[i].weight = 1.0 if weights is None else float(weights[i])
    return rec


def is_stats(x):
    return isinstance(x, list) and len(x) == N and all(set(s) == {"status", "iterations", "rho", "n_keypoints", "n_matches",
                                                                   "n_inliers", "warp"} and s["warp"].shape == (3, 3) for s in x)


def is_applied(x, c=CH):
    return isinstance(x, list) and len(x) == N and all(set(a) == {"gain", "offset", "weight", "flags"} and a["gain"].shape == (c,)
                                                       for a in x)


# ---- whole-stack forms ---------------------------------------------------------------------------------------------------
WEIGHTS = np.array([1.0, 0.5, 2.0], np.float32)
GRID = mesh_grid(W, H, STEP)[::-1]                               # (gh, gw)
ARR = lambda flag, dtype, shape: (flag, ("arr", dtype, shape))   # noqa: E731


def whole(kind, suffix, kwargs, mid, outs=(), img_shape=(H, W, CH), files=U8, refuse_weights=False, plane_shape=None):
    """Every return_* combination of Stacker.<kind>_match<suffix>: [ctx, frames, params, scale_down_width, *mid, image,
    (dropped if keypoint), *outs, stats]. outs: (flag, spec) in the order of the ABI, which is the order of the result."""
    method, cname, params = "%s_match%s" % (kind, suffix), "stk_%s_match%s" % (kind, suffix), PARAMS[kind]
    flags = [f for f, _ in outs] + ["return_stats"]
    for combo in itertools.product((False, True), repeat=len(flags)):
        on = dict(zip(flags, combo))
        keys = ["image"] + [f for f in flags if on[f]]
        first = 1 if kind == "keypoint" else 0

        def pick(key, keys=keys, first=first):
            if key not in keys:
                return None
            return (lambda res: res[first + keys.index(key)] if isinstance(res, tuple) else res)
        descs = [("frames", files), ("struct", params._c()), ("val", SDW)] + list(mid) + [("img", pick("image"), img_shape)]
        if kind == "keypoint":
            descs.append(("i32", 5))
        for flag, spec in outs:
            if spec[0] == "arr":
                descs.append(("out", pick(flag), spec[1], spec[2]))
            elif spec[0] == "maps":
                descs.append(("outtbl", pick(flag), np.float32, (N, H, W)))
            elif spec[0] == "planes":
                descs.append(("planes", pick(flag), {0, 2} if kind == "keypoint" else {0}, plane_shape))
            else:                                                # "applied", "rejected": always passed
                descs.append(("ptr",))
        descs.append(("ptr",))
        st = new_stacker()
        res = run(st, method, cname, descs, files, params, scale_down_width=SDW, status={2: 1}, **dict(kwargs, **on))
        if kind == "keypoint":                                   # always a tuple that starts with dropped
            assert isinstance(res, tuple) and len(res) == len(keys) + 1 and res[0] == 5
        elif len(keys) == 1:                                     # the bare image
            assert isinstance(res, np.ndarray)
        else:
            assert isinstance(res, tuple) and len(res) == len(keys)
        for flag, spec in outs:
            if on[flag] and spec[0] == "applied":
                assert is_applied(pick(flag)(res), files.shape[3] if files.ndim == 4 else 1)
            if on[flag] and spec[0] == "rejected":
                r = pick(flag)(res)
                assert r.dtype == np.int64 and r.shape == (N,)
            if on[flag] and spec[0] == "maps":
                assert bool((pick(flag)(res) == 1).all())
        if on["return_stats"]:
            assert is_stats(pick("return_stats")(res))
    # scale_down_width None is 0
    st = new_stacker()
    getattr(st, method)(files, params, **kwargs)
    assert st._lib.last()[1][3] == 0.0
    # the refusals, before any C call
    st = new_stacker()
    with pytest.raises(NotEnoughFiles, match="^Not enough files$"):
        getattr(st, method)([], params, **kwargs)
    mixed = [U8[0], U8[1][:, :W - 2], U8[2]]
    if kind == "ecc":
        with pytest.raises(OpenCvError) as e:
            getattr(st, method)(mixed, params, **kwargs)
        assert str(e.value) == ECC_SIZES
    elif suffix:
        with pytest.raises(InvalidParams, match="^all frames must share size, channels and dtype$"):
            getattr(st, method)(mixed, params, **kwargs)
    if refuse_weights:
        with pytest.raises(InvalidParams, match="^one weight per frame expected$"):
            getattr(st, method)(files, params, **dict(kwargs, weights=[1.0, 2.0]))
    assert not st._lib.calls


KINDS = pytest.mark.parametrize("kind", ["ecc", "keypoint"])


@KINDS
def test_match(kind):
    whole(kind, "", {}, [])
    whole(kind, "", {}, [], img_shape=(H, W, 1), files=GREY)
    whole(kind, "", {}, [], files=U16)


@KINDS
def test_match_clipped(kind):
    clip, rclip = SigmaClipParameters(2.5, 3.5, 3), RobustClipParameters(2.0, 4.0, 0.01, 1)
    counts = [ARR("return_counts", np.int32, (H, W, CH))]
    whole(kind, "_clipped", {"clip": clip}, [("struct", clip._c())], counts)
    whole(kind, "_clipped", {}, [("struct", SigmaClipParameters()._c())], counts)
    whole(kind, "_robust_clipped", {"clip": rclip}, [("struct", rclip._c())], counts)
    whole(kind, "_robust_clipped", {}, [("struct", RobustClipParameters()._c())], counts)


@KINDS
def test_match_quantile(kind):
    whole(kind, "_quantile", {"quantile": 0.25}, [("struct", QuantileParameters(0.25)._c())])
    whole(kind, "_quantile", {"quantile": QuantileParameters(0.75)}, [("struct", QuantileParameters(0.75)._c())], files=U16)
    whole(kind, "_quantile", {}, [("struct", QuantileParameters(0.5)._c())])


WEIGHTED_OUTS = [ARR("return_coverage", np.float32, (H, W)), ("return_applied", ("applied",))]


@KINDS
def test_match_weighted(kind):
    wp = WeightParameters(3, True, 2)
    whole(kind, "_weighted", {"weight": wp, "weights": WEIGHTS}, [("struct", wp._c()), ("buf", WEIGHTS)], WEIGHTED_OUTS,
          refuse_weights=True)
    whole(kind, "_weighted", {"weights": [1, 0.5, 2]}, [("struct", WeightParameters()._c()), ("buf", WEIGHTS)], WEIGHTED_OUTS)
    whole(kind, "_weighted", {}, [("struct", WeightParameters()._c()), ("buf", None)], WEIGHTED_OUTS, img_shape=(H, W, 1), files=GREY)


@KINDS
def test_match_local_weighted(kind):
    wp, lp = WeightParameters(1, True, 0), LocalParameters(2, 8, 3, 0.5)
    whole(kind, "_local_weighted", {"local": lp, "weight": wp, "weights": WEIGHTS},
          [("struct", wp._c()), ("buf", WEIGHTS), ("struct", lp._c())], WEIGHTED_OUTS, refuse_weights=True)
    whole(kind, "_local_weighted", {}, [("struct", WeightParameters()._c()), ("buf", None), ("struct", LocalParameters()._c())],
          WEIGHTED_OUTS)


@KINDS
def test_match_local_aligned(kind):
    mp, lp = MeshParameters(step=STEP, radius=4), LocalParameters(2, 8, 3, 0.5)
    whole(kind, "_local_aligned", {"mesh": mp, "local": lp}, [("struct", mp._c()), ("struct", lp._c())])
    whole(kind, "_local_aligned", {}, [("struct", MeshParameters()._c()), ("struct", None)])
    whole(kind, "_local_aligned_pyramid", {"mesh": mp, "levels": 2, "local": lp}, [("struct", mp._c()), ("val", 2), ("struct", lp._c())])
    whole(kind, "_local_aligned_pyramid", {}, [("struct", MeshParameters()._c()), ("val", 3), ("struct", None)])


@KINDS
def test_match_drizzle(kind):
    dz, mp = DrizzleParameters(1.5, 0.8, 0.25, -0.5, 0.125), MeshParameters(step=STEP)
    den = lambda oh, ow: [ARR("return_den", np.float32, (oh, ow))]             # noqa: E731
    whole(kind, "_drizzle", {"drizzle": dz}, [("struct", dz._c())], den(12, 18), img_shape=(12, 18, CH))
    whole(kind, "_drizzle", {}, [("struct", DrizzleParameters()._c())], den(16, 24), img_shape=(16, 24, CH))
    whole(kind, "_drizzle", {"drizzle": dz, "out_shape": (5, 7)}, [("struct", dz._c())], den(5, 7), img_shape=(5, 7, 1), files=GREY)
    whole(kind, "_local_aligned_drizzle", {"mesh": mp, "drizzle": dz}, [("struct", mp._c()), ("struct", dz._c())], den(12, 18),
          img_shape=(12, 18, CH))
    whole(kind, "_local_aligned_drizzle", {"out_shape": (9, 4)}, [("struct", MeshParameters()._c()), ("struct", DrizzleParameters()._c())],
          den(9, 4), img_shape=(9, 4, CH))
    st = new_stacker()
    for suffix in ("_drizzle", "_local_aligned_drizzle"):
        with pytest.raises(InvalidParams, match="^drizzle: the output must be at least one pixel wide and high$"):
            getattr(st, "%s_match%s" % (kind, suffix))(U8, PARAMS[kind], out_shape=(0, 4))


@KINDS
def test_match_drizzle_rejected(kind):
    dz, wp, rp = DrizzleParameters(1.5, 0.8), WeightParameters(2, True, 2), RejectParameters(5.0, 2.5, 1.0, 0.5, 0.01, 0.1, 2)
    outs = [ARR("return_den", np.float32, (12, 18)), ("return_maps", ("maps",)), ("return_rejected", ("rejected",)),
            ("return_applied", ("applied",))]
    whole(kind, "_drizzle_rejected", {"drizzle": dz, "reject": rp, "weight": wp, "weights": WEIGHTS},
          [("struct", dz._c()), ("struct", wp._c()), ("buf", WEIGHTS), ("struct", rp._c())], outs, img_shape=(12, 18, CH),
          refuse_weights=True)
    outs[0] = ARR("return_den", np.float32, (3, 5))
    whole(kind, "_drizzle_rejected", {"out_shape": (3, 5)}, [("struct", DrizzleParameters()._c()), ("struct", WeightParameters()._c()),
                                                            ("buf", None), ("struct", RejectParameters()._c())], outs, img_shape=(3, 5, CH))


@KINDS
def test_match_clipped_and_quantile_weighted(kind):
    wp = WeightParameters(2, True, 2)
    outs = [ARR("return_counts", np.int32, (H, W, CH)), ARR("return_kept_weight", np.float32, (H, W, CH)), ("return_applied", ("applied",))]
    for suffix, clip, default in (("_clipped_weighted", SigmaClipParameters(2.5, 3.5, 3), SigmaClipParameters()),
                                  ("_robust_clipped_weighted", RobustClipParameters(2.0, 4.0, 0.01, 1), RobustClipParameters())):
        whole(kind, suffix, {"clip": clip, "weight": wp, "weights": WEIGHTS}, [("struct", clip._c()), ("struct", wp._c()), ("buf", WEIGHTS)],
              outs, refuse_weights=True)
        whole(kind, suffix, {}, [("struct", default._c()), ("struct", WeightParameters()._c()), ("buf", None)], outs)
    outs = [ARR("return_counts", np.int32, (H, W)), ("return_applied", ("applied",))]
    whole(kind, "_quantile_weighted", {"quantile": 0.25, "weight": wp, "weights": WEIGHTS},
          [("struct", QuantileParameters(0.25)._c()), ("struct", wp._c()), ("buf", WEIGHTS)], outs, refuse_weights=True)
    whole(kind, "_quantile_weighted", {}, [("struct", QuantileParameters()._c()), ("struct", WeightParameters()._c()), ("buf", None)], outs)


@KINDS
def test_match_local_normalized(kind):
    ln = LocalNormParameters(step=STEP, stat_step=2, normalize=1)
    outs = [ARR("return_den", np.float32, (H, W)), ARR("return_counts", np.int32, (H, W)), ("return_norm", ("planes",)),
            ("return_applied", ("applied",))]
    shape = GRID + (2 * CH,)
    whole(kind, "_local_normalized", {"norm": ln, "weights": WEIGHTS}, [("struct", ln._c()), ("struct", None), ("buf", WEIGHTS)], outs,
          refuse_weights=True, plane_shape=shape)
    whole(kind, "_local_normalized", {"norm": ln, "quantile": 0.25}, [("struct", ln._c()), ("struct", QuantileParameters(0.25)._c()),
                                                                      ("buf", None)], outs, plane_shape=shape)
    whole(kind, "_local_normalized", {}, [("struct", LocalNormParameters()._c()), ("struct", None), ("buf", None)], outs,
          plane_shape=mesh_grid(W, H, 64)[::-1] + (2 * CH,))


@KINDS
def test_match_local_normalized_clipped(kind):
    ln, clip, rclip = LocalNormParameters(step=STEP), SigmaClipParameters(2.5, 3.5, 3), RobustClipParameters(2.0, 4.0, 0.01, 1)
    outs = [ARR("return_counts", np.int32, (H, W, CH)), ARR("return_kept_weight", np.float32, (H, W, CH)), ("return_norm", ("planes",)),
            ("return_applied", ("applied",))]
    shape = GRID + (2 * CH,)
    whole(kind, "_local_normalized_clipped", {"norm": ln, "clip": clip, "weights": WEIGHTS},
          [("struct", ln._c()), ("struct", clip._c()), ("struct", None), ("buf", WEIGHTS)], outs, refuse_weights=True, plane_shape=shape)
    whole(kind, "_local_normalized_clipped", {"norm": ln, "clip": rclip},
          [("struct", ln._c()), ("struct", None), ("struct", rclip._c()), ("buf", None)], outs, plane_shape=shape)
    st = new_stacker()
    method = getattr(st, kind + "_match_local_normalized_clipped")
    with pytest.raises(InvalidParams, match="^clip: one of SigmaClipParameters and RobustClipParameters expected, not both$"):
        method(U8, PARAMS[kind], ln, (clip, rclip))
    for none in (None, (clip, None)):
        with pytest.raises(InvalidParams, match="^clip: a SigmaClipParameters or a RobustClipParameters expected$"):
            method(U8, PARAMS[kind], ln, none)
    with pytest.raises(InvalidParams):                            # the clip is judged before the frames
        method([], PARAMS[kind], ln, None)
    assert not st._lib.calls


@KINDS
def test_match_ranked(kind):
    """[ctx, frames, params, scale_down_width, image, (dropped), stats, select, order, kept, scores]: the result carries
    order[:kept] and the stats of the kept list."""
    sel = SelectParameters(2, 5, 1, 0.5, 1)
    for select, want in ((sel, sel), (None, SelectParameters())):
        for return_scores, return_stats in itertools.product((False, True), repeat=2):
            k = 1 if kind == "keypoint" else 0
            descs = [("frames", U8), ("struct", PARAMS[kind]._c()), ("val", SDW), ("img", lambda r, k=k: r[k], (H, W, CH))] \
                + ([("i32", 5)] if kind == "keypoint" else []) \
                + [("ptr",), ("struct", want._c()), ("i32", [2, 0, 1]), ("i32", 2),
                   ("out", lambda r, k=k: r[k + 2], np.float64, (N, 4)) if return_scores else ("ptr",)]
            st = new_stacker()
            res = run(st, kind + "_match_ranked", "stk_%s_match_ranked" % kind, descs, U8, PARAMS[kind], select, SDW,
                      return_scores, return_stats)
            assert isinstance(res, tuple) and len(res) == k + 2 + return_scores + return_stats
            assert res[:k] == (5,)[:k]
            assert res[k + 1].dtype == np.int32 and res[k + 1].tolist() == [2, 0]
            if return_stats:
                assert isinstance(res[-1], list) and len(res[-1]) == 2
    st = new_stacker()
    with pytest.raises(NotEnoughFiles, match="^Not enough files$"):
        getattr(st, kind + "_match_ranked")([], PARAMS[kind])
    if kind == "ecc":
        with pytest.raises(OpenCvError) as e:
            st.ecc_match_ranked([U8[0], U8[1][:, :W - 2]], ECC)
        assert str(e.value) == ECC_SIZES
    assert not st._lib.calls


# ---- caller-held warps ---------------------------------------------------------------------------------------------------
WARPS = [np.eye(3), np.array([[1.0, 0.01, 2.5], [-0.01, 1.0, -1.5]]), np.arange(9.0).reshape(3, 3)]
WARPS9 = np.stack([np.eye(3).reshape(-1), np.array([1.0, 0.01, 2.5, -0.01, 1.0, -1.5, 0.0, 0.0, 1.0]), np.arange(9.0)])
INCLUDE = np.array([1, 0, 1], np.int32)
BORDER = dict(is_affine=True, border_mode=BORDER_REFLECT, border_value=(1.0, 2.0, 3.0), alpha=0.5)
GAIN = np.array([[1.0, 1.0, 1.0], [1.5, 0.5, 2.0], [0.25, 4.0, 1.0]], np.float32)
OFFSET = np.array([[0.0, 0.0, 0.0], [0.1, -0.1, 0.2], [0.3, 0.0, -0.2]], np.float32)
MAPS = _rng.random((N, H, W), dtype=np.float32)
FIELDS = (_rng.random((N,) + GRID + (2,), dtype=np.float32) - 0.5)
NORM = [None] + [_rng.random(GRID + (2 * CH,), dtype=np.float32) for _ in range(N - 1)]


def head(kind, files=U8, include=INCLUDE):
    """The run every caller-held-warps signature starts with; kind "border": with the border pair and alpha; "alpha": alpha
    alone (drizzle, reject); "bare": neither (local_align)."""
    d = [("frames", files), ("buf", WARPS9), ("buf", include), ("val", 1)]
    if kind == "border":
        d += [("val", BORDER_REFLECT), ("buf", np.array([1.0, 2.0, 3.0, 0.0])), ("val", 0.5)]
    elif kind == "alpha":
        d += [("val", 0.5)]
    return d


def head_kw(kind, **kw):
    d = dict(BORDER) if kind == "border" else {"is_affine": True, "alpha": 0.5} if kind == "alpha" else {"is_affine": True}
    return dict(d, include=INCLUDE, **kw)


def first(r):
    return r[0] if isinstance(r, tuple) else r


def flagged(st, method, cname, mk_descs, args, kw, flags):
    """Every combination of `flags`; mk_descs(pick) builds the descriptors, pick(flag) the result picker or None."""
    for combo in itertools.product((False, True), repeat=len(flags)):
        on = dict(zip(flags, combo))
        keys = ["image"] + [f for f in flags if on[f]]

        def pick(key, keys=keys):
            return (lambda res: res[keys.index(key)] if isinstance(res, tuple) else res) if key in keys else None
        res = run(st, method, cname, mk_descs(pick), *args, **dict(kw, **on))
        if len(keys) == 1:
            assert isinstance(res, np.ndarray)
        else:
            assert isinstance(res, tuple) and len(res) == len(keys)


def warp_refusals(method, *args, **kw):
    """Empty stack, wrong warp count, wrong include count: each before any C call, warps before everything behind them."""
    st = new_stacker()
    fn = getattr(st, method)
    with pytest.raises(NotEnoughFiles, match="^Not enough files$"):
        fn([], [], *args, **kw)
    with pytest.raises(InvalidParams, match=r"^one 3x3 \(or 2x3\) warp per frame expected$"):
        fn(U8, WARPS[:2], *args, **kw)
    with pytest.raises(InvalidParams, match=r"^one 3x3 \(or 2x3\) warp per frame expected$"):
        fn(U8, [np.eye(3), np.eye(3), np.eye(4)], *args, **kw)
    with pytest.raises(InvalidParams, match="^one include flag per frame expected$"):
        fn(U8, WARPS, *args, **dict(kw, include=[1, 1]))
    assert not st._lib.calls


def records_refusals(method, *args, **kw):
    st = new_stacker()
    fn = getattr(st, method)
    with pytest.raises(InvalidParams, match="^gain and offset: n x channels, weights: n expected$"):
        fn(U8, WARPS, *args, **dict(kw, weights=[1.0, 2.0]))
    with pytest.raises(InvalidParams, match="^gain and offset: n x channels, weights: n expected$"):
        fn(U8, WARPS, *args, **dict(kw, gain=np.ones((N, 2))))
    with pytest.raises(InvalidParams, match="^one record per frame expected$"):
        fn(U8, WARPS, *args, **dict(kw, applied=[dict(gain=[1] * 3, offset=[0] * 3, weight=1.0)]))
    with pytest.raises(InvalidParams, match=r"^one 3x3 \(or 2x3\) warp per frame expected$"):      # warps come first
        fn(U8, WARPS[:2], *args, **dict(kw, weights=[1.0, 2.0]))
    assert not st._lib.calls


@pytest.mark.parametrize("robust", [False, True])
def test_clip_stack(robust):
    method, cname = ("robust_clip_stack", "stk_robust_clip_stack") if robust else ("clip_stack", "stk_clip_stack")
    clip = RobustClipParameters(2.0, 4.0, 0.01, 1) if robust else SigmaClipParameters(2.5, 3.5, 3)
    flagged(new_stacker(), method, cname, lambda pick: head("border") + [("struct", clip._c()), ("img", pick("image"), (H, W, CH)),
                                                                       ("out", pick("return_counts"), np.int32, (H, W, CH))],
            (U8, WARPS, clip), head_kw("border"), ["return_counts"])
    res = run(new_stacker(), method, cname, [("frames", GREY), ("buf", WARPS9), ("buf", None), ("val", 0), ("val", 0),
                                             ("buf", np.zeros(4)), ("val", 1.0 / 255.0), ("struct", type(clip)()._c()),
                                             ("img", first, (H, W, 1)), ("out", None)], GREY, WARPS)
    assert isinstance(res, np.ndarray)
    warp_refusals(method)


def test_quantile_stack():
    flagged(new_stacker(), "quantile_stack", "stk_quantile_stack",
            lambda pick: head("border") + [("struct", QuantileParameters(0.25)._c()), ("img", pick("image"), (H, W, CH))],
            (U8, WARPS, 0.25), head_kw("border"), [])
    run(new_stacker(), "quantile_stack", "stk_quantile_stack",
        [("frames", U16), ("buf", WARPS9), ("buf", None), ("val", 0), ("val", 0), ("buf", np.zeros(4)), ("val", 1.0 / 255.0),
         ("struct", QuantileParameters()._c()), ("img", first, (H, W, CH))], U16, WARPS)
    warp_refusals("quantile_stack")


def test_weighted_stack():
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), "weighted_stack", "stk_weighted_stack",
            lambda pick: head("border") + [("rec", rec), ("val", 0), ("img", pick("image"), (H, W, CH)),
                                           ("out", pick("return_coverage"), np.float32, (H, W))],
            (U8, WARPS, GAIN, OFFSET, WEIGHTS), head_kw("border", coverage=False), ["return_coverage"])
    applied = [dict(gain=GAIN[i], offset=OFFSET[i], weight=float(WEIGHTS[i]), flags=0) for i in range(N)]
    run(new_stacker(), "weighted_stack", "stk_weighted_stack",           # the records of another call, as given
        head("border") + [("rec", rec), ("val", 1), ("img", first, (H, W, CH)), ("out", None)], U8, WARPS, applied=applied,
        **head_kw("border"))
    run(new_stacker(), "weighted_stack", "stk_weighted_stack",           # nothing given: records are built all the same
        head("border", GREY) + [("rec", records(c=1)), ("val", 1), ("img", first, (H, W, 1)), ("out", None)], GREY, WARPS,
        **head_kw("border"))
    warp_refusals("weighted_stack")
    records_refusals("weighted_stack")


def test_moments():
    run(new_stacker(), "overlap_moments", "stk_overlap_moments",
        head("border") + [("val", 2), ("out", lambda r: r, np.float64, (N, CH, 6))], U8, WARPS, stat_step=2, **head_kw("border"))
    run(new_stacker(), "local_moments", "stk_local_moments",
        head("border") + [("val", STEP), ("val", 2), ("out", lambda r: r, np.float64, (N, 1, 2, CH, 6))], U8, WARPS, STEP, stat_step=2,
        **head_kw("border"))
    run(new_stacker(), "local_moments", "stk_local_moments",             # a bad step is the engine's to refuse
        [("frames", GREY), ("buf", WARPS9), ("buf", None), ("val", 0), ("val", 0), ("buf", np.zeros(4)), ("val", 1.0 / 255.0),
         ("val", 0), ("val", 4), ("out", lambda r: r, np.float64, (N, 1, 1, 1, 6))], GREY, WARPS, 0)
    warp_refusals("overlap_moments")
    warp_refusals("local_moments", STEP)


def norm_refusals(method):
    st = new_stacker()
    fn = getattr(st, method)
    with pytest.raises(InvalidParams, match=r"^one normalisation plane \(or None\) per frame expected$"):
        fn(U8, WARPS, NORM[:2], STEP)
    for bad in (np.zeros(GRID + (CH,), np.float32), np.zeros(GRID, np.float32), np.zeros((5, 5, 2 * CH), np.float32)):
        with pytest.raises(InvalidParams, match="^normalisation planes: gh x gw x 2 channels f32 expected$"):
            fn(U8, WARPS, [None, bad, NORM[2]], STEP)
    with pytest.raises(InvalidParams, match="^gain and offset: n x channels, weights: n expected$"):   # records before planes
        fn(U8, WARPS, NORM[:2], STEP, weights=[1.0])
    assert not st._lib.calls
    fn(U8, WARPS, [None, np.zeros((5, 5, 2 * CH), np.float32), None], 7)        # a bad step is the engine's to refuse
    assert len(st._lib.calls) == 1


def test_local_norm_stack():
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), "local_norm_stack", "stk_local_norm_stack",
            lambda pick: head("border") + [("rec", rec), ("tbl", NORM), ("val", STEP), ("val", 0), ("img", pick("image"), (H, W, CH)),
                                           ("out", pick("return_den"), np.float32, (H, W))],
            (U8, WARPS, NORM, STEP, GAIN, OFFSET, WEIGHTS), head_kw("border", coverage=False), ["return_den"])
    run(new_stacker(), "local_norm_stack", "stk_local_norm_stack",
        head("border") + [("rec", records()), ("buf", None), ("val", STEP), ("val", 1), ("img", first, (H, W, CH)), ("out", None)],
        U8, WARPS, None, STEP, **head_kw("border"))
    warp_refusals("local_norm_stack", NORM, STEP)
    records_refusals("local_norm_stack", NORM, STEP)
    norm_refusals("local_norm_stack")


def test_quantile_stack_local_norm():
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), "quantile_stack_local_norm", "stk_quantile_stack_local_norm",
            lambda pick: head("border") + [("struct", QuantileParameters(0.25)._c()), ("rec", rec), ("tbl", NORM), ("val", STEP), ("val", 1),
                                           ("img", pick("image"), (H, W, CH)), ("out", pick("return_counts"), np.int32, (H, W))],
            (U8, WARPS, NORM, STEP, 0.25, GAIN, OFFSET, WEIGHTS), head_kw("border"), ["return_counts"])
    warp_refusals("quantile_stack_local_norm", NORM, STEP)
    records_refusals("quantile_stack_local_norm", NORM, STEP)
    norm_refusals("quantile_stack_local_norm")


@pytest.mark.parametrize("robust", [False, True])
def test_clip_stack_local_norm(robust):
    method = "robust_clip_stack_local_norm" if robust else "clip_stack_local_norm"
    clip = RobustClipParameters(2.0, 4.0, 0.01, 1) if robust else SigmaClipParameters(2.5, 3.5, 3)
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), method, "stk_" + method,
            lambda pick: head("border") + [("struct", clip._c()), ("rec", rec), ("tbl", NORM), ("val", STEP), ("val", 1),
                                           ("img", pick("image"), (H, W, CH)), ("out", pick("return_counts"), np.int32, (H, W, CH)),
                                           ("out", pick("return_kept_weight"), np.float32, (H, W, CH))],
            (U8, WARPS, NORM, STEP, clip, GAIN, OFFSET, WEIGHTS), head_kw("border"), ["return_counts", "return_kept_weight"])
    run(new_stacker(), method, "stk_" + method,
        head("border") + [("struct", type(clip)()._c()), ("rec", records()), ("tbl", NORM), ("val", STEP), ("val", 1),
                          ("img", first, (H, W, CH)), ("out", None), ("out", None)], U8, WARPS, NORM, STEP, **head_kw("border"))
    warp_refusals(method, NORM, STEP)
    records_refusals(method, NORM, STEP)
    norm_refusals(method)


@pytest.mark.parametrize("robust", [False, True])
def test_clip_stack_weighted(robust):
    method = "robust_clip_stack_weighted" if robust else "clip_stack_weighted"
    clip = RobustClipParameters(2.0, 4.0, 0.01, 1) if robust else SigmaClipParameters(2.5, 3.5, 3)
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), method, "stk_" + method,
            lambda pick: head("border") + [("struct", clip._c()), ("rec", rec), ("val", 0), ("img", pick("image"), (H, W, CH)),
                                           ("out", pick("return_counts"), np.int32, (H, W, CH)),
                                           ("out", pick("return_kept_weight"), np.float32, (H, W, CH))],
            (U8, WARPS, clip, GAIN, OFFSET, WEIGHTS), head_kw("border", coverage=False), ["return_counts", "return_kept_weight"])
    run(new_stacker(), method, "stk_" + method,
        head("border") + [("struct", type(clip)()._c()), ("rec", records()), ("val", 1), ("img", first, (H, W, CH)), ("out", None),
                          ("out", None)], U8, WARPS, **head_kw("border"))
    warp_refusals(method)
    records_refusals(method)


def test_quantile_stack_weighted():
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), "quantile_stack_weighted", "stk_quantile_stack_weighted",
            lambda pick: head("border") + [("struct", QuantileParameters(0.25)._c()), ("rec", rec), ("val", 1),
                                           ("img", pick("image"), (H, W, CH)), ("out", pick("return_counts"), np.int32, (H, W))],
            (U8, WARPS, 0.25, GAIN, OFFSET, WEIGHTS), head_kw("border"), ["return_counts"])
    run(new_stacker(), "quantile_stack_weighted", "stk_quantile_stack_weighted",
        head("border") + [("struct", QuantileParameters()._c()), ("rec", records()), ("val", 1), ("img", first, (H, W, CH)), ("out", None)],
        U8, WARPS, **head_kw("border"))
    warp_refusals("quantile_stack_weighted")
    records_refusals("quantile_stack_weighted")


def maps_refusals(method, *args):
    st = new_stacker()
    fn = getattr(st, method)
    with pytest.raises(InvalidParams, match="^one weight map per frame expected$"):
        fn(U8, WARPS, MAPS[:2], *args)
    with pytest.raises(InvalidParams, match="^weight maps: H x W planes expected$"):
        fn(U8, WARPS, [MAPS[0], MAPS[1][:, :5], MAPS[2]], *args)
    with pytest.raises(InvalidParams, match="^gain and offset: n x channels, weights: n expected$"):   # records before maps
        fn(U8, WARPS, MAPS[:2], *args, weights=[1.0])
    assert not st._lib.calls


def fields_refusals(method, before, after=()):
    st = new_stacker()
    fn = getattr(st, method)
    with pytest.raises(InvalidParams, match="^one field per frame expected$"):
        fn(U8, WARPS, *before, list(FIELDS[:2]), STEP, *after)
    with pytest.raises(InvalidParams, match=r"^fields: gh x gw x 2 planes expected \(mesh_grid\)$"):
        fn(U8, WARPS, *before, [FIELDS[0], FIELDS[1][:, :2], FIELDS[2]], STEP, *after)
    assert not st._lib.calls
    fn(U8, WARPS, *before, [FIELDS[0], FIELDS[1][:, :2], FIELDS[2]], 7, *after)     # a bad step is the engine's to refuse
    assert len(st._lib.calls) == 1


def test_local_weighted_stack():
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), "local_weighted_stack", "stk_local_weighted_stack",
            lambda pick: head("border") + [("rec", rec), ("tbl", list(MAPS)), ("val", 0.5), ("val", 3), ("img", pick("image"), (H, W, CH)),
                                           ("out", pick("return_coverage"), np.float32, (H, W))],
            (U8, WARPS, MAPS.astype(np.float64), GAIN, OFFSET, WEIGHTS), head_kw("border", floor=0.5, power=3), ["return_coverage"])
    run(new_stacker(), "local_weighted_stack", "stk_local_weighted_stack",          # nothing given: NULL records
        head("border") + [("rec", None), ("tbl", list(MAPS)), ("val", 1.0), ("val", 2), ("img", first, (H, W, CH)), ("out", None)],
        U8, WARPS, list(MAPS), **head_kw("border"))
    warp_refusals("local_weighted_stack", MAPS)
    records_refusals("local_weighted_stack", MAPS)
    maps_refusals("local_weighted_stack")


def test_mesh_stacks():
    run(new_stacker(), "mesh_stack", "stk_mesh_stack", head("border") + [("tbl", list(FIELDS)), ("val", STEP), ("img", first, (H, W, CH))],
        U8, WARPS, FIELDS, STEP, **head_kw("border"))
    warp_refusals("mesh_stack", FIELDS, STEP)
    fields_refusals("mesh_stack", ())
    rec = records(GAIN, OFFSET, WEIGHTS)
    flagged(new_stacker(), "mesh_local_weighted_stack", "stk_mesh_local_weighted_stack",
            lambda pick: head("border") + [("rec", rec), ("tbl", list(MAPS)), ("val", 0.5), ("val", 3), ("tbl", list(FIELDS)), ("val", STEP),
                                           ("img", pick("image"), (H, W, CH)), ("out", pick("return_coverage"), np.float32, (H, W))],
            (U8, WARPS, MAPS, FIELDS, STEP, GAIN, OFFSET, WEIGHTS), head_kw("border", floor=0.5, power=3), ["return_coverage"])
    run(new_stacker(), "mesh_local_weighted_stack", "stk_mesh_local_weighted_stack",
        head("border") + [("rec", None), ("tbl", list(MAPS)), ("val", 1.0), ("val", 2), ("tbl", list(FIELDS)), ("val", STEP),
                          ("img", first, (H, W, CH)), ("out", None)], U8, WARPS, MAPS, FIELDS, STEP, **head_kw("border"))
    warp_refusals("mesh_local_weighted_stack", MAPS, FIELDS, STEP)
    records_refusals("mesh_local_weighted_stack", MAPS, FIELDS, STEP)
    maps_refusals("mesh_local_weighted_stack", FIELDS, STEP)
    fields_refusals("mesh_local_weighted_stack", (MAPS,))
    st = new_stacker()
    with pytest.raises(InvalidParams, match="^one weight map per frame expected$"):                   # maps before fields
        st.mesh_local_weighted_stack(U8, WARPS, MAPS[:2], FIELDS[:2], STEP)


def test_drizzle_stacks():
    dz = DrizzleParameters(1.5, 0.8, 0.25, -0.5, 0.125)
    rec = records(GAIN, OFFSET, WEIGHTS)
    some = [MAPS[0], None, MAPS[2]]
    flagged(new_stacker(), "drizzle_stack", "stk_drizzle_stack",
            lambda pick: head("alpha") + [("struct", dz._c()), ("rec", rec), ("tbl", some), ("img", pick("image"), (12, 18, CH)),
                                          ("out", pick("return_den"), np.float32, (12, 18))],
            (U8, WARPS, dz, GAIN, OFFSET, WEIGHTS), head_kw("alpha", maps=some), ["return_den"])
    run(new_stacker(), "drizzle_stack", "stk_drizzle_stack",                         # nothing given: NULL records, NULL maps
        head("alpha") + [("struct", DrizzleParameters()._c()), ("rec", None), ("buf", None), ("img", first, (5, 7, CH)), ("out", None)],
        U8, WARPS, out_shape=(5, 7), **head_kw("alpha"))
    run(new_stacker(), "drizzle_stack", "stk_drizzle_stack",                         # a list of no maps at all is a table of NULLs
        head("alpha") + [("struct", dz._c()), ("rec", None), ("tbl", [None] * N), ("img", first, (12, 18, CH)), ("out", None)],
        U8, WARPS, dz, maps=[None] * N, **head_kw("alpha"))
    some_f = [None, FIELDS[1], None]
    flagged(new_stacker(), "mesh_drizzle_stack", "stk_mesh_drizzle_stack",
            lambda pick: head("alpha") + [("struct", dz._c()), ("rec", rec), ("tbl", some), ("tbl", some_f), ("val", STEP),
                                          ("img", pick("image"), (12, 18, CH)), ("out", pick("return_den"), np.float32, (12, 18))],
            (U8, WARPS, some_f, STEP, dz, GAIN, OFFSET, WEIGHTS), head_kw("alpha", maps=some), ["return_den"])
    run(new_stacker(), "mesh_drizzle_stack", "stk_mesh_drizzle_stack",
        head("alpha") + [("struct", DrizzleParameters()._c()), ("rec", None), ("buf", None), ("tbl", list(FIELDS)), ("val", STEP),
                         ("img", first, (16, 24, CH)), ("out", None)], U8, WARPS, FIELDS, STEP, **head_kw("alpha"))
    for method, args in (("drizzle_stack", ()), ("mesh_drizzle_stack", (FIELDS, STEP))):
        warp_refusals(method, *args)
        records_refusals(method, *args)
        st = new_stacker()
        fn = getattr(st, method)
        with pytest.raises(InvalidParams, match=r"^one weight map \(or None\) per frame expected$"):
            fn(U8, WARPS, *args, maps=[None, None])
        with pytest.raises(InvalidParams, match="^weight maps: H x W planes expected$"):
            fn(U8, WARPS, *args, maps=[None, MAPS[1][:, :5], None])
        with pytest.raises(InvalidParams, match="^drizzle: the output must be at least one pixel wide and high$"):
            fn(U8, WARPS, *args, out_shape=(4, 0))
        with pytest.raises(InvalidParams, match="^gain and offset: n x channels, weights: n expected$"):  # records before maps
            fn(U8, WARPS, *args, weights=[1.0], maps=[None, None])
        assert not st._lib.calls
    fields_refusals("mesh_drizzle_stack", ())
    st = new_stacker()
    with pytest.raises(InvalidParams, match=r"^one weight map \(or None\) per frame expected$"):      # maps before fields
        st.mesh_drizzle_stack(U8, WARPS, FIELDS[:2], STEP, maps=[None, None])


def test_reject_maps():
    rp = RejectParameters(5.0, 2.5, 1.0, 0.5, 0.01, 0.1, 2)
    clean = _rng.random((H, W, CH), dtype=np.float32)
    counts = _rng.integers(0, 4, (H, W), dtype=np.int32)
    rec = records(GAIN, OFFSET)
    out = np.full((N, H, W), 0.5, np.float32)
    some = [MAPS[0], None, MAPS[2]]
    for return_counts in (False, True):
        full = lambda r: r[0] if return_counts else r                          # noqa: E731
        # rejected and judged are always passed: checked as outputs only when they are returned
        tail = [("out", lambda r: r[1], np.int64, (N,)), ("out", lambda r: r[2], np.int64, (N,))] if return_counts else [("ptr",), ("ptr",)]
        res = run(new_stacker(), "reject_maps", "stk_reject_maps",
                  head("alpha") + [("rec", rec), ("buf", clean), ("buf", counts), ("struct", rp._c()), ("tbl", some),
                                   ("outtbl", full, np.float32, (N, H, W))] + tail,
                  U8, WARPS, clean.astype(np.float64), rp, counts.astype(np.int64), GAIN, OFFSET, maps=some, return_counts=return_counts,
                  **head_kw("alpha"))
        assert bool((full(res) == 1).all())                                    # fresh planes are all ones
        assert (isinstance(res, tuple) and len(res) == 3) if return_counts else isinstance(res, np.ndarray)
    # nothing given: NULL records, NULL counts, NULL maps; a caller's array is written in place
    res = run(new_stacker(), "reject_maps", "stk_reject_maps",
              head("alpha") + [("rec", None), ("buf", clean), ("buf", None), ("struct", RejectParameters()._c()), ("buf", None),
                               ("outtbl", lambda r: r, np.float32, (N, H, W)), ("ptr",), ("ptr",)],
              U8, WARPS, clean, out=out, **head_kw("alpha"))
    assert res is out
    # maps as one array, and maps that are `out` itself
    run(new_stacker(), "reject_maps", "stk_reject_maps",
        head("alpha") + [("rec", None), ("buf", clean), ("buf", None), ("struct", RejectParameters()._c()), ("tbl", list(MAPS)),
                         ("outtbl", lambda r: r, np.float32, (N, H, W)), ("ptr",), ("ptr",)], U8, WARPS, clean, maps=MAPS, **head_kw("alpha"))
    st = new_stacker()
    res = run(st, "reject_maps", "stk_reject_maps",
              head("alpha") + [("rec", None), ("buf", clean), ("buf", None), ("struct", RejectParameters()._c()), ("tbl", list(out)),
                               ("outtbl", lambda r: r, np.float32, (N, H, W)), ("ptr",), ("ptr",)], U8, WARPS, clean, maps=out, out=out,
              **head_kw("alpha"))
    assert res is out and st._lib.last()[1][10][1] == st._lib.last()[1][11][1]            # in place: the same addresses
    warp_refusals("reject_maps", clean)
    st = new_stacker()
    with pytest.raises(InvalidParams, match="^gain and offset: n x channels, weights: n expected$"):
        st.reject_maps(U8, WARPS, clean[:4], gain=np.ones((N, 2)))                         # records before the clean image
    with pytest.raises(InvalidParams, match=r"^clean image: shape \(8, 12, 3\) expected$"):
        st.reject_maps(U8, WARPS, clean[:4], counts=counts[:4])                            # the clean image before the counts
    with pytest.raises(InvalidParams, match=r"^counts: shape \(8, 12\) expected$"):
        st.reject_maps(U8, WARPS, clean, counts=counts[:4], out=out[:2])
    with pytest.raises(InvalidParams, match=r"^out: shape \(3, 8, 12\) expected$"):
        st.reject_maps(U8, WARPS, clean, out=out[:2], maps=[None])
    with pytest.raises(InvalidParams, match="^out: a contiguous n x H x W float32 array where the frames live expected$"):
        st.reject_maps(U8, WARPS, clean, out=out.astype(np.float64))
    with pytest.raises(InvalidParams, match=r"^one input map \(or None\) per frame expected$"):
        st.reject_maps(U8, WARPS, clean, maps=[None])
    with pytest.raises(InvalidParams, match=r"^maps: shape \(8, 12\) expected$"):
        st.reject_maps(U8, WARPS, clean, maps=[None, MAPS[1][:, :5], None])
    with pytest.raises(InvalidParams, match=r"^maps: shape \(3, 8, 12\) expected$"):
        st.reject_maps(U8, WARPS, clean, maps=MAPS[:2])
    assert not st._lib.calls


def test_local_align():
    mp = MeshParameters(step=STEP, radius=4)
    fshape, sshape = (N,) + GRID + (2,), (N,) + GRID
    for method, cname, extra, pos in (("local_align", "stk_local_align", [], ()),
                                      ("local_align_pyramid", "stk_local_align_pyramid", [("val", 2)], (2,))):
        for return_status in (False, True):
            res = run(new_stacker(), method, cname,
                      head("bare") + [("struct", mp._c())] + extra
                      + [("outtbl", (lambda r: r[0]) if return_status else (lambda r: r), np.float32, fshape),
                         ("outtbl", (lambda r: r[1]) if return_status else None, np.int32, sshape)],
                      U8, WARPS, mp, *pos, return_status=return_status, **head_kw("bare"))
            assert (isinstance(res, tuple) and len(res) == 2 and not res[0].any() and not res[1].any()) if return_status \
                else (isinstance(res, np.ndarray) and not res.any())
        warp_refusals(method)
    run(new_stacker(), "local_align", "stk_local_align",                     # a bad step is the engine's to refuse
        [("frames", GREY), ("buf", WARPS9), ("buf", None), ("val", 0), ("struct", MeshParameters(step=7)._c()),
         ("outtbl", lambda r: r, np.float32, (N, 1, 1, 2)), ("buf", None)], GREY, WARPS, MeshParameters(step=7))
    run(new_stacker(), "local_align_pyramid", "stk_local_align_pyramid",     # the defaults
        [("frames", U8), ("buf", WARPS9), ("buf", None), ("val", 0), ("struct", MeshParameters()._c()), ("val", 3),
         ("outtbl", lambda r: r, np.float32, (N,) + mesh_grid(W, H, 16)[::-1] + (2,)), ("buf", None)], U8, WARPS)


# ---- the other entry points that take stk_frames ---------------------------------------------------------------------------
def empty_refusal(method, *args):
    st = new_stacker()
    with pytest.raises(NotEnoughFiles, match="^Not enough files$"):
        getattr(st, method)([], *args)
    assert not st._lib.calls


def test_scores_and_maps():
    run(new_stacker(), "stack_sharpness", "stk_stack_sharpness", [("frames", U8), ("val", 5), ("out", lambda r: r, np.float64, (N, 4))], U8, 5)
    empty_refusal("stack_sharpness")
    lp = LocalParameters(2, 8, 3, 0.5)
    run(new_stacker(), "local_sharpness", "stk_local_sharpness",
        [("frames", U8), ("struct", lp._c()), ("outtbl", lambda r: r, np.float32, (N, H, W))], U8, lp)
    empty_refusal("local_sharpness")
    frame = U8[1]
    res = run(new_stacker(), "grey_pyramid", "stk_grey_pyramid", [("frames", frame[None]), ("val", 3), ("ptr",)], frame, 3)
    assert [(p.dtype, p.shape) for p in res] == [(np.uint8, (4, 6)), (np.uint8, (2, 3))] and not any(p.any() for p in res)
    st = new_stacker()
    with pytest.raises(InvalidParams, match="^grey_pyramid: one frame expected$"):
        st.grey_pyramid(U8, 3)
    run(new_stacker(), "grey", "stk_grey", [("frames", frame[None]), ("out", lambda r: r, np.uint8, (H, W))], frame)
    run(new_stacker(), "grey", "stk_grey", [("frames", U16[:1]), ("out", lambda r: r, np.uint16, (H, W))], U16[0])
    run(new_stacker(), "convert_f32", "stk_convert_f32", [("frames", frame[None]), ("val", 0.25), ("out", lambda r: r, np.float32, (H, W, CH))],
        frame, 0.25)
    run(new_stacker(), "convert_f32", "stk_convert_f32", [("frames", GREY[:1]), ("val", 1.0 / 255.0), ("out", lambda r: r, np.float32, (H, W))],
        GREY[0])
    run(new_stacker(), "grey_blur_f32", "stk_grey_blur_f32", [("frames", frame[None]), ("val", 5), ("out", lambda r: r, np.float32, (H, W))],
        frame, 5)


def test_grey_pyramid_table():
    st = new_stacker()
    st._lib.reads = {3: ("tbl", 3, 0)}
    planes = st.grey_pyramid(U8[1], 3)
    assert st._lib.last()[1][3][1] == [None, addr(planes[0]), addr(planes[1])]           # level 0 is the frame itself: NULL


def test_star_entry_points():
    sp = StarParameters(radius=3, max_stars=7, border_value=(1.0, 2.0))
    st = new_stacker()
    st._lib.reads = {}
    lists, peaks = st.star_detect(U8, sp, return_peaks=True)
    name, snap = st._lib.last()
    assert name == "stk_star_detect" and snap[2] == _bytes_of(sp._c()) and all(snap[3:6]) and snap[5] == addr(peaks)
    assert len(lists) == N and all(len(s) == 0 for s in lists) and peaks.dtype == np.int32 and peaks.shape == (N,)
    assert isinstance(st.star_detect(U8), list) and st._lib.last()[1][2] == _bytes_of(StarParameters()._c())
    res = run(new_stacker(), "star_align", "stk_star_align", [("frames", U8), ("struct", sp._c()), ("i32", 5), ("ptr",)], U8, sp)
    assert isinstance(res, tuple) and res[0] == 5 and is_stats(res[1])
    for return_stats in (False, True):
        res = run(new_stacker(), "star_match", "stk_star_match",
                  [("frames", U8), ("struct", sp._c()), ("img", lambda r: r[1], (H, W, CH)), ("i32", 5), ("ptr",)], U8, sp,
                  return_stats=return_stats)
        assert isinstance(res, tuple) and len(res) == 2 + return_stats and res[0] == 5 and (not return_stats or is_stats(res[2]))
    for method in ("star_detect", "star_align", "star_match"):
        empty_refusal(method)


def test_calibration_entry_points():
    bias = _rng.random((H, W, CH), dtype=np.float32)
    defects = (_rng.random((H, W)) < 0.1).astype(np.uint8)
    scale = np.array([1.0, 0.5, 2.0], np.float32)
    st = new_stacker()
    st._lib.reads = {3: ("tbl", N, 0)}
    res = st.calibrate(U8, CalibrationParameters(bias=bias, dark_scale=scale, flat_mean=[2.0, 3.0, 4.0], flat_min=0.5, pedestal=7.0,
                                                 defects=defects, defect_step=2))
    name, snap = st._lib.last()
    assert name == "stk_calibrate" and snap[4] == 0
    cal = snap[2]
    assert cal["bias"] == dict(data=addr(bias), width=W, height=H, channels=CH, location=HOST, row_stride_bytes=0)
    assert cal["dark"] is None and cal["flat"] is None and cal["defects"] == addr(defects) and cal["defects_location"] == HOST
    assert (cal["flat_mean"], cal["flat_min"], cal["pedestal"], cal["defect_step"], cal["out_depth"]) == ([2.0, 3.0, 4.0, 1.0], 0.5, 7.0, 2, 8)
    assert cal["dark_scale"] == scale.tobytes()
    assert res.dtype == np.uint8 and res.shape == (N, H, W, CH) and snap[3][1] == [addr(res) + i * H * W * CH for i in range(N)]
    res = st.calibrate(U16, CalibrationParameters(out_depth=32))
    assert res.dtype == np.float32 and res.shape == (N, H, W, CH) and st._lib.last()[1][2]["out_depth"] == 32
    for bad, message in ((CalibrationParameters(dark_scale=[1.0]), "one dark_scale per frame expected"),
                         (CalibrationParameters(out_depth=12), "out_depth must be 8, 16 or 32"),
                         (CalibrationParameters(defects=defects[:4]), "defects: an H x W uint8 plane expected"),
                         (CalibrationParameters(bias=bias.astype(np.float64)), "bias master: an H x W x C float32 image expected")):
        before = len(st._lib.calls)
        with pytest.raises(InvalidParams) as e:
            st.calibrate(U8, bad)
        assert str(e.value) == message and len(st._lib.calls) == before
    empty_refusal("calibrate", CalibrationParameters())
    clip = RobustClipParameters(2.0, 4.0, 0.01, 1)
    flagged(new_stacker(), "master_stack", "stk_master_stack",
            lambda pick: [("frames", U16), ("val", 2), ("val", 3), ("struct", clip._c()), ("img", pick("image"), (H, W, CH)),
                          ("out", pick("return_counts"), np.int32, (H, W, CH))], (U16, 2, clip), {"stat_step": 3}, ["return_counts"])
    run(new_stacker(), "master_stack", "stk_master_stack",
        [("frames", U8), ("val", 0), ("val", 4), ("struct", RobustClipParameters(3.0, 3.0, 0.5, 2)._c()), ("img", first, (H, W, CH)),
         ("out", None)], U8)
    empty_refusal("master_stack")


def test_hybrid_mixed_and_warp_accumulate():
    for return_stats in (False, True):
        res = run(new_stacker(), "hybrid_match", "stk_hybrid_match",
                  [("frames", U16), ("struct", KP._c()), ("struct", ECC._c()), ("img", first, (H, W, CH)), ("ptr",)], U16, KP, ECC,
                  return_stats=return_stats)
        assert (isinstance(res, tuple) and len(res) == 2 and is_stats(res[1])) if return_stats else isinstance(res, np.ndarray)
    empty_refusal("hybrid_match", KP, ECC)
    # frames of differing size under keypoint_match: stk_keypoint_match_mixed, every frame at its own size into frame 0's
    small = np.zeros(H * W * CH, np.uint8)[:6 * 10 * CH].reshape(6, 10, CH)      # (the stand-in reads frame 0's size from each)
    st = new_stacker()
    st._lib.pokes = {6: 5}
    for return_stats in (False, True):
        res = st.keypoint_match([U8[0], small, U8[2]], KP, SDW, return_stats=return_stats)
        name, snap = st._lib.last()
        assert name == "stk_keypoint_match_mixed" and snap[0] == CTX
        assert (snap[1]["n"], snap[1]["width"], snap[1]["height"], snap[1]["channels"], snap[1]["depth"]) == (N, W, H, CH, 8)
        assert snap[1]["ptrs"][1] == addr(small) and snap[2] == [(W, H, 0), (10, 6, 0), (W, H, 0)]
        assert snap[3] == _bytes_of(KP._c()) and snap[4] == SDW and snap[6] is not None and snap[7] is not None
        assert isinstance(res, tuple) and len(res) == 2 + return_stats and res[0] == 5
        assert res[1].dtype == np.float32 and res[1].shape == (H, W, CH)
        assert snap[5] == dict(data=addr(res[1]), width=W, height=H, channels=CH, location=HOST, row_stride_bytes=0)
    with pytest.raises(OpenCvError, match="^ORB: 8-bit BGR / BGRA frames of one type expected$"):
        st.keypoint_match([GREY[0], GREY[1][:6]], KP)
    M = WARPS[1]
    run(new_stacker(), "warp_accumulate", "stk_warp_accumulate",
        [("frames", U8[1:2]), ("buf", WARPS9[1]), ("val", 1), ("val", BORDER_REFLECT), ("buf", np.array([1.0, 2.0, 3.0, 0.0])), ("val", 0.5),
         ("val", 0), ("img", first, (H, W, CH))], U8[1], M, **BORDER)
    acc = np.zeros((H, W, 1), np.float32)
    res = run(new_stacker(), "warp_accumulate", "stk_warp_accumulate",     # a host accumulator is written in place
              [("frames", GREY[1:2]), ("buf", WARPS9[2]), ("val", 0), ("val", 0), ("buf", np.zeros(4)), ("val", 1.0 / 255.0), ("val", 1),
               ("img", first, (H, W, 1))], GREY[1], WARPS[2], acc=acc)
    assert res is acc


def test_find_homography_batch():
    """[ctx, problems, count, method, threshold, outcomes]: every problem's points as contiguous f32 pairs whatever the caller
    gave, one mask of n bytes per problem whose address is the returned array's, and the result built from the records."""
    src = [_rng.random((5, 2)), _rng.random((3, 2)).astype(np.float32), _rng.random((2 * 7, 2))[::2].tolist()]
    dst = [_rng.random((5, 2)), _rng.random(6).astype(np.float32), _rng.random((7, 2)).astype(np.float32)]
    Hm = np.arange(9.0) + 0.5
    st = new_stacker()
    st._lib.outcomes = [(0, 1, Hm, 4, 32), (3, 0, np.zeros(9), 0, 0), (0, 0, np.zeros(9), 0, 288)]
    res = st.find_homography_batch(list(zip(src, dst)), 4, 2)
    name, snap = st._lib.last()
    assert name == "stk_find_homography_batch" and len(st._lib.calls) == 1
    assert snap[0] == CTX and snap[2:5] == [3, 4, 2.0] and type(snap[4]) is float and snap[5] is not None
    for got, s, d, r in zip(snap[1], src, dst, res):
        want_s, want_d = np.asarray(s, np.float32).reshape(-1, 2), np.asarray(d, np.float32).reshape(-1, 2)
        assert got["n"] == len(want_s) and got["src"] == want_s.tobytes() and got["dst"] == want_d.tobytes()
        assert r["mask"].dtype == np.uint8 and r["mask"].shape == (len(want_s),) and got["mask"] == addr(r["mask"])
        assert set(r) == {"H", "mask", "rc", "n_inliers", "models_evaluated"}
    assert res[0]["H"].dtype == np.float64 and res[0]["H"].shape == (3, 3) and res[0]["H"].ravel().tolist() == Hm.tolist()
    assert (res[0]["rc"], res[0]["n_inliers"], res[0]["models_evaluated"]) == (0, 4, 32)
    assert res[1]["H"] is None and res[1]["rc"] == 3                        # an argument error of one problem: no exception
    assert res[2]["H"] is None and (res[2]["rc"], res[2]["models_evaluated"]) == (0, 288)
    st = new_stacker()                                                     # the defaults: RANSAC, 3.0
    st.find_homography_batch([(src[0], dst[0])])
    assert st._lib.last()[1][2:5] == [1, RANSAC, 3.0]
    st = new_stacker()                                                     # before any C call
    assert st.find_homography_batch([]) == []
    with pytest.raises(InvalidParams, match="^find_homography_batch: src and dst of a problem differ in length$"):
        st.find_homography_batch([(src[0], dst[0]), (src[1], dst[2])])
    assert not st._lib.calls


def test_every_name_that_takes_frames_is_driven_or_exempt():
    takes = {n for n, (_, a) in _ffi.SIGNATURES.items() if P_FRAMES in a}
    assert set(EXEMPT) <= takes
    if not takes - set(EXEMPT) <= SEEN:                                    # run alone: drive the module's cases first
        for name, fn in sorted(globals().items()):
            if name.startswith("test_") and fn is not test_every_name_that_takes_frames_is_driven_or_exempt:
                marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
                for values in itertools.product(*[m.args[1] for m in marks]):
                    fn(*values)
    assert takes - set(EXEMPT) - SEEN == set()
    assert not set(EXEMPT) & SEEN

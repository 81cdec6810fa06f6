"""Cost of the bicubic fold (option "warp_interpolation" = 2) next to the bilinear one on the headline stack: N 4K u8 BGR
frames (device-resident), ECC homography. One process, device events (stk_timing), warmed up; linear and cubic alternate
in every repetition, so that drift hits both alike. Prints, for both settings: the mean fold (warp_ms of ecc_match), one
clip pass (finalize_ms of clip_stack with two iterations minus that with one: clip.cpp runs iterations + 1 passes), the
weighted fold (finalize_ms of weighted_stack), the quantile combine of a 64-frame subset (finalize_ms: band stores +
selections; the selections do not depend on the setting, so the tool also prints cubic - linear, the extra cost of the
cubic band stores), ecc_match end to end (wall), and the weighted fold of a 32-frame subset as u8 and as a float32 copy of
the same values (the u8 BGR fast kernel against the generic one, under both settings):
    python tools/interp_time.py [n=256] [reps=5] [path/to/another/libstacker_amd.so]
With a third argument the linear mean fold of that other build of the engine (the parent commit's: build it in a second
checkout) runs in the same process and the same repetitions, interleaved with this build's, and both are printed."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import EccMatchParameters, MotionType, SigmaClipParameters, Stacker, _ffi, synth  # noqa: E402

LINEAR, CUBIC = 1, 2
NAMES = {LINEAR: "linear", CUBIC: "cubic"}


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    other = None
    if len(sys.argv) > 3:                                         # a second engine build in this process (dlopen is local)
        _ffi._lib, _ffi.LIB_PATH = None, os.path.abspath(sys.argv[3])
        other = Stacker(0)
    p = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    clip1, clip2 = SigmaClipParameters(3.0, 3.0, 1), SigmaClipParameters(3.0, 3.0, 2)
    nq, ng = min(n, 64), min(n, 32)
    _, stats = st.ecc_match(frames, p, return_stats=True)
    warps = [s["warp"] for s in stats]
    sub_q, sub_g = frames[:nq], frames[:ng]
    sub_f = sub_g.to(torch.float32)
    modes = (LINEAR, CUBIC)

    def setting(m):
        st.set_option("warp_interpolation", m)

    def once(m, rec):
        setting(m)
        t0 = time.perf_counter()
        st.ecc_match(frames, p)
        torch.cuda.synchronize()
        rec["ecc wall"].append((time.perf_counter() - t0) * 1e3)
        rec["mean fold"].append(st.timing()["warp_ms"])
        st.clip_stack(frames, warps, clip1)
        two = st.timing()["finalize_ms"]
        st.clip_stack(frames, warps, clip2)
        rec["clip pass"].append(st.timing()["finalize_ms"] - two)
        st.weighted_stack(frames, warps, coverage=True)
        rec["weighted fold"].append(st.timing()["finalize_ms"])
        st.quantile_stack(sub_q, warps[:nq], 0.5)
        rec[f"quantile, {nq} frames"].append(st.timing()["finalize_ms"])
        st.weighted_stack(sub_g, warps[:ng], coverage=True)
        rec[f"weighted fold, {ng} frames u8"].append(st.timing()["finalize_ms"])
        st.weighted_stack(sub_f, warps[:ng], coverage=True, alpha=1.0 / 255.0)
        rec[f"weighted fold, {ng} frames f32"].append(st.timing()["finalize_ms"])

    keys = ["mean fold", "clip pass", "weighted fold", f"quantile, {nq} frames", "ecc wall",
            f"weighted fold, {ng} frames u8", f"weighted fold, {ng} frames f32"]
    try:
        for m in modes:                                           # warm-up: code objects, workspaces
            once(m, {k: [] for k in keys})
        if other:
            other.ecc_match(frames, p)
        rec = {m: {k: [] for k in keys} for m in modes}
        other_fold = []
        for _ in range(reps):
            for m in modes:
                once(m, rec[m])
                if other and m == LINEAR:
                    other.ecc_match(frames, p)
                    other_fold.append(other.timing()["warp_ms"])
    finally:
        setting(LINEAR)
    print(f"{n} x 3840x2160 u8 ECC, medians of {reps} (ms), linear and cubic alternating:")
    print(f"  {'':48s} {'linear':>9s} {'cubic':>9s} {'ratio':>6s}")
    for k in keys:
        a, b = med(rec[LINEAR][k]), med(rec[CUBIC][k])
        print(f"  {k:48s} {a:9.3f} {b:9.3f} {b / a:6.2f}")
    kq = f"quantile, {nq} frames"
    print(f"  cubic - linear quantile combine (the band stores' extra cost): {med(rec[CUBIC][kq]) - med(rec[LINEAR][kq]):.3f} ms")
    fold = rec[LINEAR]["mean fold"]
    if other:
        print(f"  linear mean fold of {sys.argv[3]}: median {med(other_fold):.3f}   this build / that: {med(fold) / med(other_fold):.4f}")
        print(f"  that build, all runs:       {' '.join(f'{v:.3f}' for v in other_fold)}")
    print(f"  linear mean fold, all runs: {' '.join(f'{v:.3f}' for v in fold)}")
    print(f"  cubic mean fold, all runs:  {' '.join(f'{v:.3f}' for v in rec[CUBIC]['mean fold'])}", flush=True)


if __name__ == "__main__":
    main()

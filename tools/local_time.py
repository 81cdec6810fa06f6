"""Cost of the per-pixel weight maps and of the local-weighted fold (stk_local_sharpness, stk_local_weighted_stack,
stk_ecc_match_local_weighted) next to their yardsticks on the headline stack: N 4K u8 BGR frames (device-resident) under
the warps of their own ECC homography run. One process, device events (stk_timing: prep_ms of the map and sharpness passes,
finalize_ms of the folds), warmed up, the candidates alternating in every repetition so that drift hits all alike. Prints
the medians of:
  * the map pass at radius 4 and radius 15, beside stk_stack_sharpness at ksize 3 (the same reads; the map pass also
    writes 4 B per pixel);
  * the local fold (generic kernel + a bilinear map sample) beside stk_weighted_stack on the u8 stack (the u8 BGR fast
    kernel);
  * on an M-frame subset: the local fold beside stk_weighted_stack of an f32 copy of the same values (the generic kernel:
    the fair yardstick for the fold);
  * stk_ecc_match_local_weighted end to end beside stk_ecc_match_weighted (wall clock around the synchronised call).
    python tools/local_time.py [n=256] [reps=5] [m=32]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import (EccMatchParameters, LocalParameters, MotionType, Stacker, WeightParameters, synth)  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    m = min(n, int(sys.argv[3]) if len(sys.argv) > 3 else 32)
    ecc = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    _, stats = st.ecc_match(frames, ecc, return_stats=True)
    warps = [s["warp"] for s in stats]
    lp4, lp15 = LocalParameters(4, 16, 2, 1.0), LocalParameters(15, 16, 2, 1.0)
    wp = WeightParameters(3, True, 0)
    maps = st.local_sharpness(frames, lp4)
    sub = frames[:m]
    sub_f32 = sub.to(torch.float32)                     # the same values: alpha stays 1/255
    keys = ["map pass, radius 4", "map pass, radius 15", "stack_sharpness, ksize 3", "local fold, u8", "weighted fold, u8 (fast kernel)",
            f"local fold, u8, {m} frames", f"weighted fold, f32, {m} frames (generic kernel)", "ecc_match_local_weighted, wall",
            "ecc_match_weighted, wall"]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def once(rec):
        st.local_sharpness(frames, lp4)
        rec[keys[0]].append(st.timing()["prep_ms"])
        st.local_sharpness(frames, lp15)
        rec[keys[1]].append(st.timing()["prep_ms"])
        st.stack_sharpness(frames, 3)
        rec[keys[2]].append(st.timing()["prep_ms"])
        st.local_weighted_stack(frames, warps, maps, floor=1.0, power=2)
        rec[keys[3]].append(st.timing()["finalize_ms"])
        st.weighted_stack(frames, warps, coverage=True)
        rec[keys[4]].append(st.timing()["finalize_ms"])
        st.local_weighted_stack(sub, warps[:m], maps[:m], floor=1.0, power=2)
        rec[keys[5]].append(st.timing()["finalize_ms"])
        st.weighted_stack(sub_f32, warps[:m], coverage=True)
        rec[keys[6]].append(st.timing()["finalize_ms"])
        rec[keys[7]].append(wall(lambda: st.ecc_match_local_weighted(frames, ecc, lp4, wp)))
        rec[keys[8]].append(wall(lambda: st.ecc_match_weighted(frames, ecc, wp)))

    once({k: [] for k in keys})                          # warm-up: code objects, workspaces
    rec = {k: [] for k in keys}
    for _ in range(reps):
        once(rec)
    v = {k: med(rec[k]) for k in keys}
    print(f"{n} x 3840x2160 u8 BGR, device-resident, medians of {reps} (ms):")
    for k in keys:
        print(f"  {k:50s} {v[k]:10.3f}")
    print(f"  map pass r4 / stack_sharpness: {v[keys[0]] / v[keys[2]]:.2f}   r15 / r4: {v[keys[1]] / v[keys[0]]:.2f}")
    print(f"  local fold / weighted fast fold (u8, {n} frames): {v[keys[3]] / v[keys[4]]:.2f}")
    print(f"  local fold / generic weighted fold ({m} frames): {v[keys[5]] / v[keys[6]]:.2f}")
    print(f"  ecc_match_local_weighted / ecc_match_weighted: {v[keys[7]] / v[keys[8]]:.2f}")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

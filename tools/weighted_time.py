"""Cost of the weighted, coverage-aware combine on the headline stack: N 4K u8 BGR frames (device-resident), ECC
homography. Prints the plain fold (warp_ms), the weighted fold alone (finalize_ms of a NONE + coverage call), the moments
pass at stat_step 1 and 4 (finalize_ms of overlap_moments on the call's own warps) and the wall time of the plain call and
of the LINEAR + coverage call at the default step:  python tools/weighted_time.py [n=256] [reps=5]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import EccMatchParameters, MotionType, Stacker, WeightParameters, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    p = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    fold_only = WeightParameters(0, True, 0)
    linear = WeightParameters(3, True, 0)
    for _ in range(2):                                         # warm-up: code objects, workspaces
        _, stats = st.ecc_match(frames, p, return_stats=True)
        st.ecc_match_weighted(frames, p, fold_only)
        st.ecc_match_weighted(frames, p, linear)
    warps = [s["warp"] for s in stats]
    for step in (1, 4):
        st.overlap_moments(frames, warps, stat_step=step)
    torch.cuda.synchronize()
    plain_s, lin_s, warp_ms, fold_ms, lin_ms, mom_ms = [], [], [], [], [], {1: [], 4: []}
    for _ in range(reps):                                      # alternated, so that drift hits all alike
        t0 = time.perf_counter()
        st.ecc_match(frames, p)
        torch.cuda.synchronize()
        plain_s.append(time.perf_counter() - t0)
        warp_ms.append(st.timing()["warp_ms"])
        t0 = time.perf_counter()
        st.ecc_match_weighted(frames, p, linear)
        torch.cuda.synchronize()
        lin_s.append(time.perf_counter() - t0)
        lin_ms.append(st.timing()["finalize_ms"])
        st.ecc_match_weighted(frames, p, fold_only)
        fold_ms.append(st.timing()["finalize_ms"])
        for step in (1, 4):
            st.overlap_moments(frames, warps, stat_step=step)
            mom_ms[step].append(st.timing()["finalize_ms"])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    fold, wfold = med(warp_ms), med(fold_ms)
    print(f"{n} x 3840x2160 u8 ECC, medians of {reps}:")
    print(f"  warp_ms (plain fold)              {fold:8.3f}")
    print(f"  weighted fold (coverage = 1)      {wfold:8.3f}   {wfold / fold:.2f} x the fold, per frame {wfold / n * 1e3:.2f} us")
    for step in (1, 4):
        print(f"  moments pass, stat_step = {step}       {med(mom_ms[step]):8.3f}")
    print(f"  finalize_ms (LINEAR, default step) {med(lin_ms):7.3f}")
    print(f"  plain call    {med(plain_s) * 1e3:8.2f} ms   {n / med(plain_s):8.1f} frames/s")
    print(f"  weighted call {med(lin_s) * 1e3:8.2f} ms   {n / med(lin_s):8.1f} frames/s   (+{(med(lin_s) - med(plain_s)) * 1e3:.2f} ms)",
          flush=True)


if __name__ == "__main__":
    main()

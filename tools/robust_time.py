"""Cost of the normalised, coverage-aware rejection combines on the headline stack: N 4K u8 BGR frames (device-resident),
ECC homography, T clip iterations. The new call and the call it extends alternate in one process. Prints the clip pass
(finalize_ms of ecc_match_clipped / (T + 1)) against the weighted clip pass (finalize_ms of a NONE + coverage call /
(T + 2): the centre pass is one of them), the whole LINEAR + coverage calls against ecc_match_clipped and
ecc_match_quantile, and their finalize_ms (moments + combine):  python tools/robust_time.py [n=256] [T=2] [reps=5]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import EccMatchParameters, MotionType, SigmaClipParameters, Stacker, WeightParameters, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    p = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    clip = SigmaClipParameters(3.0, 3.0, T)
    none, linear = WeightParameters(0, True, 0), WeightParameters(3, True, 0)
    calls = {
        "clipped": lambda: st.ecc_match_clipped(frames, p, clip),
        "clipped_weighted NONE": lambda: st.ecc_match_clipped_weighted(frames, p, clip, none),
        "clipped_weighted LINEAR": lambda: st.ecc_match_clipped_weighted(frames, p, clip, linear),
        "quantile": lambda: st.ecc_match_quantile(frames, p, 0.5),
        "quantile_weighted NONE": lambda: st.ecc_match_quantile_weighted(frames, p, 0.5, none),
        "quantile_weighted LINEAR": lambda: st.ecc_match_quantile_weighted(frames, p, 0.5, linear),
    }
    for _ in range(2):                                         # warm-up: code objects, workspaces
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    wall = {k: [] for k in calls}
    fin = {k: [] for k in calls}
    for _ in range(reps):                                      # alternated, so that drift hits all alike
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[k].append(time.perf_counter() - t0)
            fin[k].append(st.timing()["finalize_ms"])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print(f"{n} x 3840x2160 u8 ECC, T={T}, medians of {reps}:")
    for k in calls:
        print(f"  {k:26s} call {med(wall[k]) * 1e3:8.2f} ms   {n / med(wall[k]):8.1f} frames/s   finalize_ms {med(fin[k]):8.3f}")
    cp, wp = med(fin["clipped"]) / (T + 1), med(fin["clipped_weighted NONE"]) / (T + 2)
    print(f"  clip pass {cp:.3f} ms, weighted clip pass {wp:.3f} ms (+{wp - cp:.3f} ms, {wp / cp:.2f} x)")
    print(f"  clipped_weighted LINEAR - clipped:   +{(med(wall['clipped_weighted LINEAR']) - med(wall['clipped'])) * 1e3:.2f} ms")
    print(f"  quantile_weighted LINEAR - quantile: +{(med(wall['quantile_weighted LINEAR']) - med(wall['quantile'])) * 1e3:.2f} ms "
          f"(combine alone: {med(fin['quantile_weighted NONE']):.3f} against {med(fin['quantile']):.3f} ms)", flush=True)


if __name__ == "__main__":
    main()

"""Cost of the sigma-clipped combine on the headline stack: N 4K u8 BGR frames (device-resident), ECC homography, T clip
iterations. Prints the plain fold (warp_ms), the clip passes (finalize_ms), per pass and per pass-frame, and the wall time
of the plain and the clipped call:  python tools/clip_time.py [n=256] [T=2] [reps=5]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import EccMatchParameters, MotionType, SigmaClipParameters, Stacker, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    p = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    clip = SigmaClipParameters(3.0, 3.0, T)
    for _ in range(2):                                         # warm-up: code objects, workspaces
        st.ecc_match(frames, p)
        st.ecc_match_clipped(frames, p, clip)
    torch.cuda.synchronize()
    plain_s, clip_s, warp_ms, fin_ms = [], [], [], []
    for _ in range(reps):                                      # alternated, so that drift hits both alike
        t0 = time.perf_counter()
        st.ecc_match(frames, p)
        torch.cuda.synchronize()
        plain_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        st.ecc_match_clipped(frames, p, clip)
        torch.cuda.synchronize()
        clip_s.append(time.perf_counter() - t0)
        t = st.timing()
        warp_ms.append(t["warp_ms"]); fin_ms.append(t["finalize_ms"])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    passes = T + 1
    fold, fin = med(warp_ms), med(fin_ms)
    print(f"{n} x 3840x2160 u8 ECC, T={T} ({passes} passes), medians of {reps}:")
    print(f"  warp_ms (plain fold)      {fold:8.3f}")
    print(f"  finalize_ms (clip passes) {fin:8.3f}   per pass {fin / passes:.3f} ms ({fin / passes / fold:.2f} x the fold), "
          f"per pass-frame {fin / passes / n * 1e3:.2f} us")
    print(f"  plain call   {med(plain_s) * 1e3:8.2f} ms   {n / med(plain_s):8.1f} frames/s")
    print(f"  clipped call {med(clip_s) * 1e3:8.2f} ms   {n / med(clip_s):8.1f} frames/s   (+{(med(clip_s) - med(plain_s)) * 1e3:.2f} ms)",
          flush=True)


if __name__ == "__main__":
    main()

"""Cost of the two clip combines through local-normalisation planes next to the weighted clips they extend, on one stack:
N 4K u8 BGR frames (device-resident) under the homographies the synthetic stack was made with, smooth synthetic planes
(gains 0.9 .. 1.1, offsets +-0.02; frame 0 has none), sigma clip and median / MAD clip with 2 iterations. Four pairs:
  * sigma:    stk_clip_stack_weighted beside stk_clip_stack_local_norm at step 128 (both run the u8 BGR fast kernels);
  * generic:  the new call under BORDER_CONSTANT (fast state) beside the same call under BORDER_REPLICATE with coverage 1 (the
              generic state, same bits);
  * mad:      stk_robust_clip_stack_weighted beside stk_robust_clip_stack_local_norm at step 128;
  * vote:     the new call at step 128 (a wave shares its nodes: scalar loads) beside step 32 (per-lane loads).
One process, device events (stk_timing: finalize_ms of each call, the launches alone), one warm-up, the two candidates of a
pair alternating in every repetition so that drift hits both alike. Prints the medians in ms, their ratios and every run.
The scalar-load path against the per-lane path at the SAME step is a second run of this tool on a build of kernels_clip.hip
with -DSTK_NORM_CLIP_NO_VOTE (tools/ab_build.sh novote libstacker_rs_amd/csrc/kernels_clip.hip -DSTK_NORM_CLIP_NO_VOTE, then
STACKER_AMD_LIB=libstacker_rs_amd/ab/libnovote.so): compare the "sigma" pair's second column between the two runs.
    python tools/local_norm_clip_time.py [n=256] [reps=5] [pairs=sigma,generic,mad,vote]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import BORDER_REPLICATE, RobustClipParameters, SigmaClipParameters, Stacker, synth  # noqa: E402
from tools.local_norm_time import med, smooth_planes  # noqa: E402

STEP = 128


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    want = sys.argv[3].split(",") if len(sys.argv) > 3 else ["sigma", "generic", "mad", "vote"]
    w, h = 3840, 2160
    frames, G = synth.make_stack(n, w, h, device="cuda")
    warps = [G[i] for i in range(n)]
    planes = smooth_planes(n, w, h, 3, STEP)
    planes32 = smooth_planes(n, w, h, 3, 32)
    clip, mad = SigmaClipParameters(3.0, 3.0, 2), RobustClipParameters(3.0, 3.0, 0.5 / 255.0, 2)
    st = Stacker(0)
    pairs = {
        "sigma": (lambda: st.clip_stack_weighted(frames, warps, clip), lambda: st.clip_stack_local_norm(frames, warps, planes, STEP, clip)),
        "generic": (lambda: st.clip_stack_local_norm(frames, warps, planes, STEP, clip),
                    lambda: st.clip_stack_local_norm(frames, warps, planes, STEP, clip, border_mode=BORDER_REPLICATE)),
        "mad": (lambda: st.robust_clip_stack_weighted(frames, warps, mad),
                lambda: st.robust_clip_stack_local_norm(frames, warps, planes, STEP, mad)),
        "vote": (lambda: st.clip_stack_local_norm(frames, warps, planes, STEP, clip),
                 lambda: st.clip_stack_local_norm(frames, warps, planes32, 32, clip)),
    }
    pairs = {k: v for k, v in pairs.items() if k in want}

    def once(rec):
        for name, (first, second) in pairs.items():
            for k, call in enumerate((first, second)):
                call()
                t = st.timing()
                rec[(name, k)].append(t["finalize_ms"])
                if name == "mad":                        # the selection launches' share of the call
                    rec[(name, f"select{k}")].append(t["robust_select_us"] / 1000.0)

    def fresh():
        return {(name, k): [] for name in pairs for k in ((0, 1, "select0", "select1") if name == "mad" else (0, 1))}
    once(fresh())                                        # warm-up: code objects, workspaces, output tensors
    rec = fresh()
    for _ in range(reps):
        once(rec)
    print(f"{n} x {w}x{h} u8 BGR, device-resident, homographies, 2 iterations; medians of {reps} (first, second of each pair):")
    for name in pairs:
        a, b = med(rec[(name, 0)]), med(rec[(name, 1)])
        print(f"  {name:8s} first {a:10.3f} ms   second {b:10.3f} ms   second / first {b / a:.3f}")
    for key, v in rec.items():
        print(f"  {key[0]} {key[1]}, all runs: {' '.join(f'{x:.3f}' for x in v)}", flush=True)


if __name__ == "__main__":
    main()

"""Cost of local normalisation next to the combines it extends, on one stack: N 4K u8 BGR frames (device-resident) under the
homographies the synthetic stack was made with, node step 128, smooth synthetic planes (gains 0.9 .. 1.1, offsets +-0.02;
frame 0 has none). Three pairs:
  * the cell moments pass (stk_local_moments, step 128, stat_step 4) beside stk_overlap_moments at step 4;
  * the locally normalised mean (stk_local_norm_stack) beside stk_weighted_stack, once on the u8 BGR stack (the yardstick
    runs the u8 fast kernel, the new fold the generic one) and once on an f32 copy of the first 32 frames (both generic);
  * the locally normalised median (stk_quantile_stack_local_norm) beside stk_quantile_stack_weighted.
One process, device events (stk_timing: finalize_ms of each call, the launches alone), one warm-up, the two candidates of a
pair alternating in every repetition so that drift hits both alike. Prints the medians in ms and their ratios.
    python tools/local_norm_time.py [n=256] [reps=5]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import Stacker, local_norm_grid, synth  # noqa: E402

STEP = 128


def med(v):
    return sorted(v)[len(v) // 2]


def smooth_planes(n, w, h, cn, step, seed=1):
    """n planes gh x gw x 2 cn float32 (None for frame 0): a tilted gain and offset per frame and channel."""
    gh, gw, _, _ = local_norm_grid(w, h, step)
    rng = np.random.default_rng(seed)
    j, k = np.mgrid[0:gh, 0:gw].astype(np.float64)
    planes = [None]
    for _ in range(1, n):
        P = np.empty((gh, gw, 2 * cn), np.float32)
        for c in range(cn):
            a, b = rng.uniform(-0.1, 0.1, 2)
            P[..., c] = 1.0 + a * (k / max(gw - 1, 1) - 0.5) + b * (j / max(gh - 1, 1) - 0.5)
            a, b = rng.uniform(-0.02, 0.02, 2)
            P[..., cn + c] = a * (k / max(gw - 1, 1) - 0.5) + b * (j / max(gh - 1, 1) - 0.5)
        planes.append(P)
    return planes


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 3840, 2160
    frames, G = synth.make_stack(n, w, h, device="cuda")
    warps = [G[i] for i in range(n)]
    planes = smooth_planes(n, w, h, 3, STEP)
    nf = min(n, 32)
    f32 = frames[:nf].float() * (1.0 / 255.0)
    st = Stacker(0)
    pairs = {
        "moments": (lambda: st.overlap_moments(frames, warps, stat_step=4), lambda: st.local_moments(frames, warps, STEP, stat_step=4)),
        "mean u8": (lambda: st.weighted_stack(frames, warps), lambda: st.local_norm_stack(frames, warps, planes, STEP)),
        "mean f32": (lambda: st.weighted_stack(f32, warps[:nf], alpha=1.0), lambda: st.local_norm_stack(f32, warps[:nf], planes[:nf], STEP, alpha=1.0)),
        "median": (lambda: st.quantile_stack_weighted(frames, warps, 0.5), lambda: st.quantile_stack_local_norm(frames, warps, planes, STEP, 0.5)),
    }

    def once(rec):
        for name, (base, new) in pairs.items():
            base()
            rec[(name, "base")].append(st.timing()["finalize_ms"])
            new()
            rec[(name, "local")].append(st.timing()["finalize_ms"])

    def fresh():
        return {(name, k): [] for name in pairs for k in ("base", "local")}
    once(fresh())                                        # warm-up: code objects, workspaces, output tensors
    rec = fresh()
    for _ in range(reps):
        once(rec)
    print(f"{n} x {w}x{h} u8 BGR (mean f32: {nf} frames), device-resident, homographies, step {STEP}; medians of {reps}:")
    for name in pairs:
        a, b = med(rec[(name, "base")]), med(rec[(name, "local")])
        print(f"  {name:9s} yardstick {a:10.3f} ms   local normalisation {b:10.3f} ms   ratio {b / a:.3f}")
    for key, v in rec.items():
        print(f"  {key[0]} {key[1]}, all runs: {' '.join(f'{x:.3f}' for x in v)}", flush=True)


if __name__ == "__main__":
    main()

"""Cost of drizzle integration (stk_drizzle_stack) next to its yardstick on N 1080p u8 BGR frames (device-resident) under
the homographies the synthetic stack was made with: the drizzle launch at (scale, pixfrac) = (1, 1), (2, 0.5) and (3, 0.4)
onto the grid that covers frame 0 at that scale, beside the generic weighted fold (stk_weighted_stack, coverage = 1, on an
f32 copy of the same values, which takes the generic kernel) onto frame 0's grid. One process, device events (stk_timing:
finalize_ms of each call), warmed up, the candidates alternating in every repetition so that drift hits all alike. Prints
the medians in ms and in ns per output pixel and table entry.
    python tools/drizzle_time.py [n=64] [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import DrizzleParameters, Stacker, synth  # noqa: E402

CASES = [(1.0, 1.0), (2.0, 0.5), (3.0, 0.4)]


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 1920, 1080
    frames, G = synth.make_stack(n, w, h, device="cuda")
    warps = [G[i] for i in range(n)]
    f32 = frames.to(torch.float32)                                  # the same values: alpha stays 1/255
    st = Stacker(0)
    keys = [f"drizzle s={s:g} p={p:g}" for s, p in CASES] + ["weighted fold, f32 (generic kernel)"]
    pixels = [DrizzleParameters(scale=s).out_shape(h, w) for s, _ in CASES] + [(h, w)]

    def once(rec):
        for k, (s, p) in zip(keys, CASES):
            st.drizzle_stack(frames, warps, DrizzleParameters(scale=s, pixfrac=p))
            rec[k].append(st.timing()["finalize_ms"])
        st.weighted_stack(f32, warps, coverage=True)
        rec[keys[-1]].append(st.timing()["finalize_ms"])

    once({k: [] for k in keys})                          # warm-up: code objects, workspaces, output tensors
    rec = {k: [] for k in keys}
    for _ in range(reps):
        once(rec)
    print(f"{n} x {w}x{h} u8 BGR, device-resident, homographies; medians of {reps}:")
    for k, (oh, ow) in zip(keys, pixels):
        v = med(rec[k])
        print(f"  {k:40s} {v:9.3f} ms   {ow}x{oh}   {v * 1e6 / (ow * oh * n):7.4f} ns per output pixel and entry")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

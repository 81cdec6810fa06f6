"""Cost of mesh-displaced drizzle (stk_mesh_drizzle_stack) next to plain drizzle (stk_drizzle_stack) on the same stack: N
1080p u8 BGR frames (device-resident) under the homographies the synthetic stack was made with, at (scale, pixfrac) = (1, 1),
(2, 0.5) and (3, 0.4) onto the grid that covers frame 0 at that scale, step 32, smooth synthetic fields (two cosines per
component, up to 2.5 px, wavelengths of 400 to 900 px; frame 0 has none). One process, device events (stk_timing:
finalize_ms of each call, the launch alone), one warm-up, the two candidates alternating in every repetition so that drift
hits both alike. Prints the medians in ms, in ns per output pixel and table entry, and their ratio.
    python tools/mesh_drizzle_time.py [n=64] [reps=5]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import DrizzleParameters, Stacker, mesh_grid, synth  # noqa: E402

CASES = [(1.0, 1.0), (2.0, 0.5), (3.0, 0.4)]
STEP = 32


def med(v):
    return sorted(v)[len(v) // 2]


def smooth_fields(n, w, h, step, seed=1):
    """n x gh x gw x 2 float32: two cosines per component and frame; frame 0's plane is zero (and is not read)."""
    gw, gh = mesh_grid(w, h, step)
    rng = np.random.default_rng(seed)
    j, k = np.mgrid[0:gh, 0:gw].astype(np.float64) * step
    D = np.zeros((n, gh, gw, 2), np.float32)
    for i in range(1, n):
        for c in range(2):
            for _ in range(2):
                lam, th, ph, amp = rng.uniform(400, 900), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 1.25)
                D[i, ..., c] += amp * np.cos(2 * np.pi * (np.cos(th) * k + np.sin(th) * j) / lam + ph)
    return D


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 1920, 1080
    frames, G = synth.make_stack(n, w, h, device="cuda")
    warps = [G[i] for i in range(n)]
    fields = list(torch.from_numpy(smooth_fields(n, w, h, STEP)).cuda())
    fields[0] = None
    st = Stacker(0)

    def once(rec):
        for s, p in CASES:
            dz = DrizzleParameters(scale=s, pixfrac=p)
            st.drizzle_stack(frames, warps, dz)
            rec[(s, p, "plain")].append(st.timing()["finalize_ms"])
            st.mesh_drizzle_stack(frames, warps, fields, STEP, dz)
            rec[(s, p, "mesh")].append(st.timing()["finalize_ms"])

    def fresh():
        return {(s, p, k): [] for s, p in CASES for k in ("plain", "mesh")}
    once(fresh())                                        # warm-up: code objects, workspaces, output tensors
    rec = fresh()
    for _ in range(reps):
        once(rec)
    print(f"{n} x {w}x{h} u8 BGR, device-resident, homographies, step {STEP}; medians of {reps}:")
    for s, p in CASES:
        oh, ow = DrizzleParameters(scale=s).out_shape(h, w)
        a, b = med(rec[(s, p, "plain")]), med(rec[(s, p, "mesh")])
        per = 1e6 / (ow * oh * n)
        print(f"  s={s:g} p={p:g}  {ow}x{oh}   plain {a:9.3f} ms ({a * per:7.4f} ns per output pixel and entry)   "
              f"mesh {b:9.3f} ms ({b * per:7.4f})   ratio {b / a:.3f}")
    for key, v in rec.items():
        print(f"  s={key[0]:g} p={key[1]:g} {key[2]}, all runs: {' '.join(f'{x:.3f}' for x in v)}", flush=True)


if __name__ == "__main__":
    main()

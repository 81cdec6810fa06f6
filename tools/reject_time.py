"""Cost of the blot-and-compare rejection pass (stk_reject_maps) next to its two neighbours on the same stack: the plain
drizzle launch (stk_drizzle_stack at scale 2, pixfrac 0.5) and the coverage-aware median that makes the clean image
(stk_quantile_stack_weighted at 0.5). N 1080p u8 BGR frames (device-resident) under the homographies the synthetic stack was
made with; the reject pass runs with the median's counts, min_count = 3 and no input maps. One process, device events
(stk_timing: finalize_ms of each call), one warm-up, the three candidates alternating in every repetition so that drift hits
all alike. Prints the medians in ms, the reject pass in ns per frame pixel and entry, and the two ratios.
    python tools/reject_time.py [n=64] [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import DrizzleParameters, RejectParameters, Stacker, synth  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 1920, 1080
    frames, G = synth.make_stack(n, w, h, device="cuda")
    warps = [G[i] for i in range(n)]
    st = Stacker(0)
    dz = DrizzleParameters(scale=2.0, pixfrac=0.5)
    rp = RejectParameters()
    maps = torch.ones((n, h, w), dtype=torch.float32, device="cuda")
    state = {}

    def once(rec):
        clean, cnt = st.quantile_stack_weighted(frames, warps, 0.5, coverage=True, return_counts=True)
        rec["median"].append(st.timing()["finalize_ms"])
        _, rej, jud = st.reject_maps(frames, warps, clean, rp, cnt, out=maps, return_counts=True)
        rec["reject"].append(st.timing()["finalize_ms"])
        st.drizzle_stack(frames, warps, dz)
        rec["drizzle"].append(st.timing()["finalize_ms"])
        state["rej"], state["jud"] = int(rej.sum()), int(jud.sum())

    def fresh():
        return {k: [] for k in ("median", "reject", "drizzle")}
    once(fresh())                                        # warm-up: code objects, workspaces, output tensors
    rec = fresh()
    for _ in range(reps):
        once(rec)
    m, r, d = med(rec["median"]), med(rec["reject"]), med(rec["drizzle"])
    print(f"{n} x {w}x{h} u8 BGR, device-resident, homographies; medians of {reps}:")
    print(f"  reject {r:9.3f} ms ({r * 1e6 / (w * h * n):7.4f} ns per frame pixel and entry)   drizzle (2, 0.5) {d:9.3f} ms   "
          f"median {m:9.3f} ms   reject / drizzle {r / d:.3f}   reject / median {r / m:.3f}")
    print(f"  judged {state['jud']} of {n * w * h} pixels, rejected {state['rej']}")
    for key, v in rec.items():
        print(f"  {key}, all runs: {' '.join(f'{x:.3f}' for x in v)}", flush=True)


if __name__ == "__main__":
    main()

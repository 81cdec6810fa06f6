"""Cost of coarse-to-fine local alignment (stk_local_align_pyramid at levels 1 / 2 / 3) beside the single-level pass
(stk_local_align) on the headline stack: N 4K u8 BGR frames (device-resident) under the warps of their own ECC homography
run, step 32, radius 12, epsilon 0.01, max_iters 10. One process, device events (stk_timing: align_ms = the levels'
estimations and fills, prep_ms = the pyramid pass), one warm-up, the candidates alternating in every repetition so that
drift hits all alike. Prints the medians, the pyramid pass's own time beside one read of the stack at a nominal HBM rate,
and the valid nodes and iterations per valid node of level 0.
    python tools/mesh_pyramid_time.py [n=256] [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import EccMatchParameters, MeshParameters, MotionType, Stacker, synth  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 3840, 2160
    ecc = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    mp = MeshParameters(step=32, radius=12, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=2)
    frames, _ = synth.make_stack(n, w, h, device="cuda")
    st = Stacker(0)
    _, stats = st.ecc_match(frames, ecc, return_stats=True)
    warps = [s["warp"] for s in stats]
    keys = ["stk_local_align"] + [f"stk_local_align_pyramid, levels {lv}" for lv in (1, 2, 3)]
    node = {}

    def once(rec, pyr):
        _, s = st.local_align(frames, warps, mp, return_status=True)
        rec[keys[0]].append(st.timing()["align_ms"])
        node[keys[0]] = s
        for lv in (1, 2, 3):
            _, s = st.local_align_pyramid(frames, warps, mp, lv, return_status=True)
            t = st.timing()
            rec[keys[lv]].append(t["align_ms"])
            pyr[lv].append(t["prep_ms"])
            node[keys[lv]] = s

    once({k: [] for k in keys}, {lv: [] for lv in (1, 2, 3)})            # warm-up: code objects, workspaces
    rec, pyr = {k: [] for k in keys}, {lv: [] for lv in (1, 2, 3)}
    for _ in range(reps):
        once(rec, pyr)
    v = {k: med(rec[k]) for k in keys}
    print(f"{n} x {w}x{h} u8 BGR, device-resident, step {mp.step}, radius {mp.radius}, epsilon {mp.epsilon}, max_iters {mp.max_iters}; "
          f"medians of {reps} (ms):")
    for k in keys:
        s = node[k][1:]
        ok = s > 0
        print(f"  {k:40s} estimation + fill {v[k]:9.3f}   x single-level {v[k] / v[keys[0]]:5.2f}   valid nodes {float(ok.float().mean()):.3f}"
              f"   iterations per valid node at level 0 {float(s[ok].float().mean()):.2f}")
    gb = n * w * h * 3 / 1e9
    for lv in (2, 3):
        p = med(pyr[lv])
        print(f"  pyramid pass, levels {lv}: {p:9.3f} ms for {gb:.2f} GB read = {gb / p * 1e3:.0f} GB/s ({p / (gb / 8000.0 * 1e3):.2f} x one read "
              f"of the stack at a nominal 8 TB/s); with the pass, x single-level {(v[keys[lv]] + p) / v[keys[0]]:5.2f}")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}")
    for lv in (2, 3):
        print(f"  pyramid pass, levels {lv}, all runs: {' '.join(f'{x:.3f}' for x in pyr[lv])}", flush=True)


if __name__ == "__main__":
    main()

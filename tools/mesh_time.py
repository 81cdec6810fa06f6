"""Cost of local alignment (stk_local_align, stk_mesh_stack, stk_mesh_local_weighted_stack) next to its yardsticks on the
headline stack: N 4K u8 BGR frames (device-resident) under the warps of their own ECC homography run, step 32, radius 12,
epsilon 0.01, max_iters 10. One process, device events (stk_timing: align_ms of the field pass, finalize_ms of the folds,
warp_ms of stk_clip_stack's plain mean fold), warmed up, the candidates alternating in every repetition so that drift hits
all alike. Prints the medians of:
  * the field pass (estimation and fill) over all frames, beside one ECC iteration pass of the same run (ecc_iter_ms /
    ecc_iter_timed of stk_ecc_match);
  * the mesh mean fold and the mesh local-weighted fold over all frames (the generic kernel's mesh variant), beside
    stk_local_weighted_stack (the generic kernel without fields);
  * on an M-frame subset: the mesh mean fold beside the plain mean fold of an f32 copy of the same values (the generic
    kernel without fields: the fair yardstick for the field's price).
    python tools/mesh_time.py [n=256] [reps=5] [m=32]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import (EccMatchParameters, LocalParameters, MeshParameters, MotionType, SigmaClipParameters, Stacker,  # noqa: E402
                               synth)


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    m = min(n, int(sys.argv[3]) if len(sys.argv) > 3 else 32)
    ecc = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    mp = MeshParameters(step=32, radius=12, max_iters=10, epsilon=0.01, max_shift=8.0, min_eig=1.0, fill=2)
    lp = LocalParameters(4, 16, 2, 1.0)
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    _, stats = st.ecc_match(frames, ecc, return_stats=True)
    t = st.timing()
    ecc_pass = t["ecc_iter_ms"] / max(1, t["ecc_iter_timed"])
    warps = [s["warp"] for s in stats]
    fields, status = st.local_align(frames, warps, mp, return_status=True)
    valid = float((status[1:] > 0).float().mean())
    iters = float(status[1:][status[1:] > 0].float().mean())
    maps = st.local_sharpness(frames, lp)
    sub, sub_f32 = frames[:m], frames[:m].to(torch.float32)          # the same values: alpha stays 1/255
    keys = ["field pass", "mesh mean fold", "mesh local-weighted fold", "local-weighted fold (no fields)",
            f"mesh mean fold, {m} frames", f"plain mean fold, f32, {m} frames (generic kernel)"]

    def once(rec):
        st.local_align(frames, warps, mp)
        rec[keys[0]].append(st.timing()["align_ms"])
        st.mesh_stack(frames, warps, fields, mp.step)
        rec[keys[1]].append(st.timing()["finalize_ms"])
        st.mesh_local_weighted_stack(frames, warps, maps, fields, mp.step, floor=lp.floor, power=lp.power)
        rec[keys[2]].append(st.timing()["finalize_ms"])
        st.local_weighted_stack(frames, warps, maps, floor=lp.floor, power=lp.power)
        rec[keys[3]].append(st.timing()["finalize_ms"])
        st.mesh_stack(sub, warps[:m], fields[:m], mp.step)
        rec[keys[4]].append(st.timing()["finalize_ms"])
        st.clip_stack(sub_f32, warps[:m], SigmaClipParameters())
        rec[keys[5]].append(st.timing()["warp_ms"])

    once({k: [] for k in keys})                          # warm-up: code objects, workspaces
    rec = {k: [] for k in keys}
    for _ in range(reps):
        once(rec)
    v = {k: med(rec[k]) for k in keys}
    print(f"{n} x 3840x2160 u8 BGR, device-resident, step {mp.step}, radius {mp.radius}; medians of {reps} (ms):")
    for k in keys:
        print(f"  {k:55s} {v[k]:10.3f}")
    print(f"  one ECC iteration pass of the same stack (ecc_iter_ms / ecc_iter_timed): {ecc_pass:.3f}")
    print(f"  valid nodes: {valid:.3f}, iterations per valid node: {iters:.2f}")
    print(f"  mesh local-weighted fold / local-weighted fold: {v[keys[2]] / v[keys[3]]:.2f}")
    print(f"  mesh mean fold / plain generic fold ({m} frames): {v[keys[4]] / v[keys[5]]:.2f}")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

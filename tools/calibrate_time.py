"""Cost of frame calibration (stk_calibrate, stk_defect_map, stk_master_stack) on the headline stack: N 4K u8 BGR frames,
device-resident, with all three masters and a defect map that flags 0.1 % of the pixels. One process, warmed up, medians
of `reps` repetitions with the candidates alternating in every repetition so that drift hits all alike. Prints the medians of:
  * stk_calibrate to u8 and to f32 (device events: stk_timing.finalize_ms), each also with the frame chunk forced to 1
    (option "calibrate_chunk": the masters read once per frame instead of once per 16 frames) and, to u8, without the flat
    (no division) and with no master at all (a conversion: the loads and stores alone), beside two yardsticks:
    stk_stack_sharpness at ksize 3 (prep_ms; one read of the stack) and the bytes the call must move (frames in, frames out,
    masters and map once) at the HBM spec peak of 8 TB/s;
  * stk_defect_map on one 4K master (finalize_ms) beside one read of it at that peak;
  * stk_master_stack (normalize 2) of `flats` 4K u8 flats beside stk_robust_clip_stack_weighted called directly on the same
    frames (wall clock around the synchronised calls): the difference is the moments pass and host work.
    python tools/calibrate_time.py [n=256] [reps=5] [flats=32]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import CalibrationParameters, DefectParameters, RobustClipParameters, Stacker  # noqa: E402

HBM_PEAK = 8.0e12           # bytes per second, spec


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    n_flats = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    w, h = 3840, 2160
    px = w * h
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        frames[i] = torch.randint(20, 200, (h, w, 3), generator=gen, device="cuda", dtype=torch.uint8)
    yy = torch.linspace(-1, 1, h, device="cuda")[:, None, None]
    xx = torch.linspace(-1, 1, w, device="cuda")[None, :, None]
    flat = (1000.0 * (1.0 - 0.35 * (xx * xx + yy * yy))).expand(h, w, 3).contiguous()
    bias = 10.0 + torch.rand((h, w, 3), generator=gen, device="cuda")
    dark = 3.0 + torch.rand((h, w, 3), generator=gen, device="cuda")
    hot = torch.rand((h, w, 3), generator=gen, device="cuda") < 0.001 / 3
    dark = torch.where(hot, dark + 80.0, dark)
    st = Stacker(0)
    dmap, counts = st.defect_map(dark, DefectParameters(True, False, 30.0), return_counts=True)
    flagged = float((dmap != 0).sum().item()) / px
    scale = np.linspace(0.5, 2.0, n).astype(np.float32)
    level = st.image_mean(flat)
    out8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    out32 = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")

    def cal(depth):
        return CalibrationParameters(bias=bias, dark=dark, flat=flat, dark_scale=scale, flat_mean=level, flat_min=1.0, defects=dmap,
                                     out_depth=depth)

    no_flat = CalibrationParameters(bias=bias, dark=dark, dark_scale=scale, defects=dmap)
    nothing = CalibrationParameters()

    flats = torch.empty((n_flats, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n_flats):
        lvl = 0.2 * (1.0 + 0.1 * (i % 5))
        flats[i] = torch.clamp(flat * lvl + 3.0 * torch.randn((h, w, 3), generator=gen, device="cuda"), 0, 255).to(torch.uint8)
    eye = [np.eye(3)] * n_flats
    clip = RobustClipParameters(3.0, 3.0, 0.5, 2)
    keys = ["calibrate to u8", "calibrate to f32", "calibrate to u8, chunk 1", "calibrate to f32, chunk 1", "stack_sharpness, ksize 3",
            "defect_map, one master", "master_stack, wall", "robust_clip_stack_weighted, wall", "calibrate to u8, no flat",
            "calibrate to u8, no master"]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def once(rec):
        for chunk, k8, k32 in ((0, keys[0], keys[1]), (1, keys[2], keys[3])):
            st.set_option("calibrate_chunk", chunk)
            st.calibrate(frames, cal(8), out=out8)
            rec[k8].append(st.timing()["finalize_ms"])
            st.calibrate(frames, cal(32), out=out32)
            rec[k32].append(st.timing()["finalize_ms"])
        st.set_option("calibrate_chunk", 0)
        for k, c in ((keys[8], no_flat), (keys[9], nothing)):
            st.calibrate(frames, c, out=out8)
            rec[k].append(st.timing()["finalize_ms"])
        st.stack_sharpness(frames, 3)
        rec[keys[4]].append(st.timing()["prep_ms"])
        st.defect_map(dark, DefectParameters(True, False, 30.0), map=dmap)
        rec[keys[5]].append(st.timing()["finalize_ms"])
        rec[keys[6]].append(wall(lambda: st.master_stack(flats, 2, clip)))
        rec[keys[7]].append(wall(lambda: st.robust_clip_stack_weighted(flats, eye, clip, coverage=False, alpha=1.0)))

    once({k: [] for k in keys})                          # warm-up: code objects, workspaces
    rec = {k: [] for k in keys}
    for _ in range(reps):
        once(rec)
    v = {k: med(rec[k]) for k in keys}
    masters = 3 * px * 12 + px
    need = {keys[0]: n * px * 3 * (1 + 1) + masters, keys[1]: n * px * 3 * (1 + 4) + masters}
    print(f"{n} x {w}x{h} u8 BGR, device-resident, {100 * flagged:.3f} % of the pixels flagged, medians of {reps} (ms):")
    for k in keys:
        print(f"  {k:40s} {v[k]:10.3f}")
    for k in keys[:2]:
        floor_ms = need[k] / HBM_PEAK * 1e3
        print(f"  {k}: {need[k] / 1e9:.2f} GB to move = {floor_ms:.3f} ms at 8 TB/s; measured / that = {v[k] / floor_ms:.2f};"
              f" measured / stack_sharpness = {v[k] / v[keys[4]]:.2f}; chunk 1 / chunk 16 = {v[k + ', chunk 1'] / v[k]:.2f}")
    one_read = px * 12 / HBM_PEAK * 1e3
    print(f"  defect_map: one read of the master = {one_read:.4f} ms at 8 TB/s; measured / that = {v[keys[5]] / one_read:.1f}")
    print(f"  master_stack of {n_flats} flats - the combine alone = {v[keys[6]] - v[keys[7]]:.3f} ms")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

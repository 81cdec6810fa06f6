"""Cost of demosaicing (stk_demosaic) on the headline stack: N 4K u8 Bayer mosaics, device-resident, every method to u8 and
to f32. One process, one warm-up, medians of `reps` repetitions with the candidates alternating in every repetition so that
drift hits all alike; device events throughout (stk_timing.finalize_ms / prep_ms). Beside them, in the same process, two
yardsticks on the B G R stack of that geometry:
  * stk_calibrate with no master and no map to u8: the one other kernel that writes a u8 B G R stack element by element (the
    demosaic writes the same bytes and reads a third of them);
  * stk_stack_sharpness at ksize 3: one read of a B G R stack;
and the bytes each call must move (mosaics in, B G R out) at the HBM spec peak of 8 TB/s.
    python tools/demosaic_time.py [n=256] [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import (CFA_RGGB, DEMOSAIC_BILINEAR, DEMOSAIC_HA, DEMOSAIC_MHC, DEMOSAIC_SUPERPIXEL,  # noqa: E402
                               CalibrationParameters, Stacker)

HBM_PEAK = 8.0e12           # bytes per second, spec
METHODS = [("bilinear", DEMOSAIC_BILINEAR), ("MHC", DEMOSAIC_MHC), ("HA", DEMOSAIC_HA), ("superpixel", DEMOSAIC_SUPERPIXEL)]


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 3840, 2160
    px = w * h
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    mosaics = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        mosaics[i] = torch.randint(20, 200, (h, w), generator=gen, device="cuda", dtype=torch.uint8)
        bgr[i] = torch.randint(20, 200, (h, w, 3), generator=gen, device="cuda", dtype=torch.uint8)
    out8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    out32 = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    half8 = out8.view(-1)[:n * (h // 2) * (w // 2) * 3].view(n, h // 2, w // 2, 3)
    half32 = out32.view(-1)[:n * (h // 2) * (w // 2) * 3].view(n, h // 2, w // 2, 3)
    st = Stacker(0)
    nothing = CalibrationParameters()
    keys = [f"demosaic {name} to {d}" for name, _ in METHODS for d in ("u8", "f32")] + ["calibrate to u8, no master", "stack_sharpness, ksize 3"]

    def once(rec):
        for name, method in METHODS:
            small = method == DEMOSAIC_SUPERPIXEL
            st.demosaic(mosaics, CFA_RGGB, method, out=half8 if small else out8)
            rec[f"demosaic {name} to u8"].append(st.timing()["finalize_ms"])
            st.demosaic(mosaics, CFA_RGGB, method, out_depth=32, out=half32 if small else out32)
            rec[f"demosaic {name} to f32"].append(st.timing()["finalize_ms"])
        st.calibrate(bgr, nothing, out=out8)
        rec[keys[-2]].append(st.timing()["finalize_ms"])
        st.stack_sharpness(bgr, 3)
        rec[keys[-1]].append(st.timing()["prep_ms"])

    once({k: [] for k in keys})                          # warm-up: code objects, workspaces
    rec = {k: [] for k in keys}
    for _ in range(reps):
        once(rec)
    v = {k: med(rec[k]) for k in keys}
    print(f"{n} x {w}x{h} u8 mosaics, device-resident, medians of {reps} (ms):")
    for k in keys:
        print(f"  {k:40s} {v[k]:10.3f}")
    for name, method in METHODS:
        for d, el in (("u8", 1), ("f32", 4)):
            k = f"demosaic {name} to {d}"
            out_px = px // 4 if method == DEMOSAIC_SUPERPIXEL else px
            need = n * (px + out_px * 3 * el)
            floor_ms = need / HBM_PEAK * 1e3
            print(f"  {k}: {need / 1e9:.2f} GB to move = {floor_ms:.3f} ms at 8 TB/s; measured / that = {v[k] / floor_ms:.2f};"
                  f" / calibrate (conversion) = {v[k] / v[keys[-2]]:.2f}; / stack_sharpness = {v[k] / v[keys[-1]]:.2f}")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

"""Cost of Richardson-Lucy deconvolution (stk_deconvolve) on a 4K BGR f32 image, device-resident, 10 iterations, R = 4, 8
and 16, without and with the total-variation regulariser. One process, one warm-up, device events (the call's own stk_timing
fields: finalize_ms = all launches, prep_ms / warp_ms = the ratio and the update launch of the last iteration), medians of
`reps` repetitions with the candidates alternating in every repetition so that drift hits all alike. Prints, per case, the
milliseconds per iteration, those of the ratio and of the update launch, and the fma rate: 2 (2R+1)^2 fmas per pixel, channel
and iteration, 2 flop each, against the chip's f32 vector peak of 157 TFLOP/s. A one-frame f32 -> f32
stk_background_apply of the same image runs beside them as the "one read and one write of this image" yardstick.
    python tools/deconvolve_time.py [reps=5] [iterations=10]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import DeconvolveParameters, Stacker, mesh_grid, psf_model  # noqa: E402

PEAK_TFLOPS = 157.0


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import numpy as np
    import torch
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 5
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    w, h = 3840, 2160
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    sky = 2000 + 300 * x / w + 150 * y / h
    for _ in range(300):
        sx, sy, amp = (float(torch.rand(1, generator=gen, device="cuda")) for _ in range(3))
        x0, y0 = int(sx * (w - 32)), int(sy * (h - 32))
        yy, xx = y[y0:y0 + 32, x0:x0 + 32] - (y0 + 16), x[y0:y0 + 32, x0:x0 + 32] - (x0 + 16)
        sky[y0:y0 + 32, x0:x0 + 32] += 10 ** (2.3 + 1.5 * amp) * torch.exp(-(xx * xx + yy * yy) / 12.0)
    image = (sky[..., None] * torch.tensor([1.0, 0.9, 0.8], device="cuda") + torch.randn((h, w, 3), generator=gen, device="cuda") * 40.0).contiguous()
    out = torch.empty_like(image)
    torch.cuda.synchronize()
    st = Stacker(0)
    gw, gh = mesh_grid(w, h, 64)
    plane = [np.zeros((gh, gw, 3), np.float32)]
    flat_out = [torch.empty_like(image)]
    cases = []
    for R in (4, 8, 16):
        psf = psf_model(R, (R / 3.0) ** 2, (R / 4.0) ** 2, 0.2 * (R / 4.0) ** 2)
        for tv in (False, True):
            p = DeconvolveParameters(iterations=iters, radius=R, lambda_=0.002 if tv else 0.0, tv_eps=1.0)
            cases.append((f"R = {R:2d}, lambda {'> 0' if tv else '= 0'}", R, lambda q=psf, pp=p: st.deconvolve_image(image, q, pp, out=out)))
    cases.append(("stk_background_apply f32 -> f32 (yardstick)", 0, lambda: st.background_apply([image], plane, 64, out=flat_out)))

    def once(rec):
        for name, _, fn in cases:
            fn()
            torch.cuda.synchronize()
            t = st.timing()
            rec[name].append((t["finalize_ms"], t["prep_ms"], t["warp_ms"]))

    once({c[0]: [] for c in cases})                                      # warm-up: code objects, workspaces
    rec = {c[0]: [] for c in cases}
    for _ in range(reps):
        once(rec)
    print(f"{w}x{h} BGR f32, device-resident, {iters} iterations, medians of {reps}:")
    for name, R, _ in cases:
        total, ratio, update = (med([r[k] for r in rec[name]]) for k in range(3))
        if not R:
            print(f"  {name:46s} {total:9.3f} ms")
            continue
        per_it = total / iters
        tflops = 2.0 * 2.0 * (2 * R + 1) ** 2 * w * h * 3 / (per_it * 1e-3) / 1e12
        print(f"  {name:46s} {per_it:9.3f} ms per iteration (ratio {ratio:.3f}, update {update:.3f}; all {total:.2f}), "
              f"{tflops:6.1f} TFLOP/s = {tflops / PEAK_TFLOPS:.2f} of the f32 vector peak")
    for name, _, _ in cases:
        print(f"  {name}, all runs: {' '.join(f'{r[0]:.3f}' for r in rec[name])}", flush=True)


if __name__ == "__main__":
    main()

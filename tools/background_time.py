"""Cost of the background model (stk_background_cells, stk_background_apply, stk_background_flatten) on 4K BGR stacks,
device-resident, u16 and u8, step 64, clip_iters 3. One process, one warm-up, device events (the calls' own stk_timing
fields), medians of `reps` repetitions with the candidates alternating in every repetition so that drift hits all alike.
Prints the medians of:
  * the cells launch (finalize_ms) beside stk_star_detect_deep's launch (prep_ms) and stk_stack_noise (prep_ms) on the same
    stack: both make one read with an exact per-tile selection; the cells pass does 3 channels x up to 4 rounds x 2
    selections, so a small multiple of the deep launch is expected, not parity;
  * the apply launch (finalize_ms) beside stk_calibrate with no master to the same depth (finalize_ms), the element-wise
    yardstick;
  * stk_background_flatten: its two launches (finalize_ms) and the wall clock of the whole call, whose difference is the
    host side: the copy of the records, the estimator per frame, the tables.
The stacks: a sky with a gradient, Gaussian noise and a few hundred stars, made on the device.
    python tools/background_time.py [n=256] [reps=5]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import BackgroundParameters, CalibrationParameters, Stacker, StarParameters  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 3840, 2160
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    sky = 2000 + 300 * x / w + 150 * y / h
    for _ in range(300):
        sx, sy, amp = (float(torch.rand(1, generator=gen, device="cuda")) for _ in range(3))
        x0, y0 = int(sx * (w - 32)), int(sy * (h - 32))
        yy, xx = y[y0:y0 + 32, x0:x0 + 32] - (y0 + 16), x[y0:y0 + 32, x0:x0 + 32] - (x0 + 16)
        sky[y0:y0 + 32, x0:x0 + 32] += 10 ** (2.3 + 1.5 * amp) * torch.exp(-(xx * xx + yy * yy) / 6.0)
    u16 = torch.empty((n, h, w, 3), dtype=torch.uint16, device="cuda")
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        f = sky + torch.randn(sky.shape, generator=gen, device="cuda") * 40.0
        u16[i] = torch.clamp(torch.round(f), 0, 65535).to(torch.int32).to(torch.uint16)[..., None]
        u8[i] = torch.clamp(torch.round(f / 16.0), 0, 255).to(torch.uint8)[..., None]
    torch.cuda.synchronize()
    st = Stacker(0)
    p = BackgroundParameters(step=64, clip_iters=3, target=(1000.0,) * 4)
    p8 = BackgroundParameters(step=64, clip_iters=3, target=(60.0,) * 4)
    sp = StarParameters(min_contrast=8)
    planes = {}

    def flatten(stack, params, key):
        t0 = time.perf_counter()
        out = st.background_flatten(stack, params, return_planes=key not in planes)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if key not in planes:
            planes[key] = out[1]
        return wall

    cases = []
    for key, stack, params in (("u16", u16, p), ("u8", u8, p8)):
        cases += [(f"cells launch, {key}", "finalize_ms", lambda s=stack, q=params: st.background_cells(s, q)),
                  (f"stk_star_detect_deep launch, {key}", "prep_ms", lambda s=stack: st.star_detect_deep(s, sp)),
                  (f"stk_stack_noise, {key}", "prep_ms", lambda s=stack: st.stack_noise(s)),
                  (f"flatten, {key}", "finalize_ms", lambda s=stack, q=params, k=key: flatten(s, q, k)),
                  (f"apply launch, {key}", "finalize_ms", lambda s=stack, q=params, k=key: st.background_apply(s, planes[k], 64, q.target)),
                  (f"stk_calibrate, no master, {key}", "finalize_ms", lambda s=stack: st.calibrate(s, CalibrationParameters()))]

    def once(rec, wall):
        for name, field, fn in cases:
            r = fn()
            torch.cuda.synchronize()
            rec[name].append(st.timing()[field])
            if name.startswith("flatten"):
                wall[name].append(r)
            del r

    once({c[0]: [] for c in cases}, {c[0]: [] for c in cases})       # warm-up: code objects, workspaces, the planes
    rec, wall = {c[0]: [] for c in cases}, {c[0]: [] for c in cases}
    for _ in range(reps):
        once(rec, wall)
    v = {k: med(x) for k, x in rec.items()}
    print(f"{n} x {w}x{h} BGR u16 and u8, device-resident, step 64, clip_iters 3, medians of {reps}:")
    for name, _, _ in cases:
        print(f"  {name:40s} {v[name]:9.3f} ms")
    for key in ("u16", "u8"):
        fw = med(wall[f"flatten, {key}"])
        print(f"  {key}: cells / deep launch {v[f'cells launch, {key}'] / v[f'stk_star_detect_deep launch, {key}']:.2f}, cells / noise "
              f"{v[f'cells launch, {key}'] / v[f'stk_stack_noise, {key}']:.2f}, apply / calibrate "
              f"{v[f'apply launch, {key}'] / v[f'stk_calibrate, no master, {key}']:.2f}; flatten wall {fw:.1f} ms, host side "
              f"{fw - v[f'flatten, {key}']:.1f} ms")
    for name, _, _ in cases:
        print(f"  {name}, all runs: {' '.join(f'{x:.3f}' for x in rec[name])}", flush=True)


if __name__ == "__main__":
    main()

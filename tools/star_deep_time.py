"""Cost of star detection on the 16-bit key (stk_star_detect_deep) on 4K BGR stacks, device-resident. One process, one
warm-up, device events (stk_timing.prep_ms: the detection launch), medians of `reps` repetitions with the candidates
alternating in every repetition so that drift hits all alike. Prints the medians of:
  * the deep launch on N u16 sky frames and on N / 4 f32 sky frames (the same bytes as N u8 frames);
  * beside them, on the u8 stack of that geometry: stk_star_detect's launch (the yardstick) and the deep launch;
  * stk_stack_noise on the u16 stack (prep_ms too), the other exact-histogram pass over 16-bit data;
and each as ms and as ms per GB read, relative to the yardstick.
The stacks: one rendered star field (synth.make_star_stack, `stars` per frame), every frame a whole-pixel shift of it with
its own sensor noise, made on the device; the u16 frames are the u8 field's values times 257 (noise sigma 2 -> 514 counts),
the f32 frames the u16 values as floats (f32_scale 1).
    python tools/star_deep_time.py [n=256] [reps=5] [stars=2000]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import Stacker, StarDeepParameters, StarParameters, synth  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    stars = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    nf = max(n // 4, 1)
    w, h = 3840, 2160
    base, _ = synth.make_star_stack([None], w, h, stars, noise_sigma=0.0, channels=1)
    base = torch.from_numpy(base[0]).cuda().to(torch.float32)
    gen = torch.Generator(device="cuda")
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    u16 = torch.empty((n, h, w, 3), dtype=torch.uint16, device="cuda")
    f32 = torch.empty((nf, h, w, 3), dtype=torch.float32, device="cuda")
    for i in range(n):
        gen.manual_seed(1000 + i)
        f = torch.roll(base, shifts=((7 * i) % 23 - 11, (5 * i) % 31 - 15), dims=(0, 1)) if i else base
        f = f + torch.randn(f.shape, generator=gen, device="cuda") * 2.0
        u8[i] = torch.clamp(torch.round(f), 0, 255).to(torch.uint8)[..., None]
        d = torch.clamp(torch.round(f * 257.0), 0, 65535)
        u16[i] = d.to(torch.int32).to(torch.uint16)[..., None]
        if i < nf:
            f32[i] = d[..., None]
    st = Stacker(0)
    p8, p16, one = StarParameters(), StarParameters(min_contrast=8 * 257), StarDeepParameters(1.0)
    gb = {"u8": u8.numel() / 1e9, "u16": 2 * u16.numel() / 1e9, "f32": 4 * f32.numel() / 1e9}
    cases = [("stk_star_detect launch, u8 (yardstick)", "u8", lambda: st.star_detect(u8, p8)),
             ("deep launch, u8", "u8", lambda: st.star_detect_deep(u8, p8)),
             ("deep launch, u16", "u16", lambda: st.star_detect_deep(u16, p16)),
             ("deep launch, f32", "f32", lambda: st.star_detect_deep(f32, p16, one)),
             ("stk_stack_noise, u16", "u16", lambda: st.stack_noise(u16))]

    def once(rec):
        out = []
        for name, _, fn in cases:
            out.append(fn())
            torch.cuda.synchronize()
            rec[name].append(st.timing()["prep_ms"])
        return out

    once({c[0]: [] for c in cases})                      # warm-up: code objects, workspaces
    rec = {c[0]: [] for c in cases}
    for _ in range(reps):
        out = once(rec)
    v = {k: med(x) for k, x in rec.items()}
    y = v[cases[0][0]] / gb["u8"]
    print(f"{n} x {w}x{h} BGR u8 and u16, {nf} f32, device-resident, {stars} stars per frame, medians of {reps}:")
    for name, kind, _ in cases:
        print(f"  {name:42s} {v[name]:9.3f} ms  {gb[kind]:6.2f} GB  {v[name] / gb[kind]:7.3f} ms/GB  {v[name] / gb[kind] / y:5.2f} x the yardstick per byte")
    print(f"  deep / 8-bit launch on the u8 stack: {v[cases[1][0]] / v[cases[0][0]]:.2f}; u16 / u8 deep launch: {v[cases[2][0]] / v[cases[1][0]]:.2f}")
    same = all(a.tobytes() == b.tobytes() for a, b in zip(out[0], out[1]))
    print(f"  stars kept per frame: u8 {min(map(len, out[0]))} .. {max(map(len, out[0]))} (deep launch the same bits: {same}),"
          f" u16 {min(map(len, out[2]))} .. {max(map(len, out[2]))}, f32 {min(map(len, out[3]))} .. {max(map(len, out[3]))}")
    for name, _, _ in cases:
        print(f"  {name}, all runs: {' '.join(f'{x:.3f}' for x in rec[name])}", flush=True)


if __name__ == "__main__":
    main()

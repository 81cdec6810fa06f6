"""Cost of star measurement (stk_star_measure) beside star detection (stk_star_detect_deep) on a 4K u16 BGR stack,
device-resident. One process, one warm-up, device events (stk_timing.prep_ms: the launches of the call), medians of `reps`
repetitions with the candidates alternating in every repetition so that drift hits all alike. Prints the medians of:
  * the detection launch on the stack (the yardstick: it reads every pixel);
  * the measure launch with 200 and with 2 000 stars per frame (about 1 100 keys per star at the default ring, scattered).
The stack: one rendered star field (synth.make_star_stack), every frame a whole-pixel shift of it with its own sensor noise,
made on the device, the u8 field's values times 257. The lists: the stars detection found in each frame (at most 1 024 of
them), filled up to the count with positions drawn uniformly over the frame: the launch's cost depends on how many apertures
it reads and where they lie, not on what they hold.
    python tools/star_measure_time.py [n=256] [reps=5]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import STAR_DTYPE, Stacker, StarMeasureParameters, StarParameters, synth  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    w, h = 3840, 2160
    base, _ = synth.make_star_stack([None], w, h, 2000, noise_sigma=0.0, channels=1)
    base = torch.from_numpy(base[0]).cuda().to(torch.float32)
    gen = torch.Generator(device="cuda")
    u16 = torch.empty((n, h, w, 3), dtype=torch.uint16, device="cuda")
    for i in range(n):
        gen.manual_seed(1000 + i)
        f = torch.roll(base, shifts=((7 * i) % 23 - 11, (5 * i) % 31 - 15), dims=(0, 1)) if i else base
        f = f + torch.randn(f.shape, generator=gen, device="cuda") * 2.0
        u16[i] = torch.clamp(torch.round(f * 257.0), 0, 65535).to(torch.int32).to(torch.uint16)[..., None]
    st = Stacker(0)
    sp, mp = StarParameters(min_contrast=8 * 257, max_stars=1024), StarMeasureParameters()
    found = st.star_detect_deep(u16, sp)
    rng = np.random.default_rng(1)

    def lists(count):
        out = []
        for s in found:
            l = np.zeros(count, STAR_DTYPE)
            k = min(len(s), count)
            l[:k] = s[:k]
            l["px"][k:], l["py"][k:] = rng.integers(16, w - 16, count - k), rng.integers(16, h - 16, count - k)
            out.append(l)
        return out
    l200, l2000 = lists(200), lists(2000)
    cases = [("stk_star_detect_deep launch (yardstick)", lambda: st.star_detect_deep(u16, sp)),
             ("stk_star_measure launch, 200 stars per frame", lambda: st.star_measure(u16, l200, mp)),
             ("stk_star_measure launch, 2000 stars per frame", lambda: st.star_measure(u16, l2000, mp))]

    def once(rec):
        out = []
        for name, fn in cases:
            out.append(fn())
            torch.cuda.synchronize()
            rec[name].append(st.timing()["prep_ms"])
        return out

    once({c[0]: [] for c in cases})                      # warm-up: code objects, workspaces
    rec = {c[0]: [] for c in cases}
    for _ in range(reps):
        out = once(rec)
    v = {k: med(x) for k, x in rec.items()}
    print(f"{n} x {w}x{h} BGR u16, device-resident, {min(map(len, found))} .. {max(map(len, found))} stars detected per frame, medians of {reps}:")
    for name, _ in cases:
        print(f"  {name:48s} {v[name]:9.3f} ms  {v[name] / v[cases[0][0]]:6.3f} x the detection launch")
    for k, count in ((1, 200), (2, 2000)):
        good = sum(int((s["flags"] == 0).sum()) for s in out[k])
        print(f"  {count} per frame: {v[cases[k][0]] * 1e6 / (n * count):.2f} ns per star, {good} of {n * count} shapes measured (flags == 0)")
    for name, _ in cases:
        print(f"  {name}, all runs: {' '.join(f'{x:.3f}' for x in rec[name])}", flush=True)


if __name__ == "__main__":
    main()

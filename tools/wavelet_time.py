"""Cost of the wavelet layers (stk_wavelet_process, stk_wavelet_sigma) on a 4K BGR f32 image, device-resident. One process,
one warm-up, device events (the call's own stk_timing fields: finalize_ms = all launches, prep_ms = the estimation pass, the
reset and the four histogram and pick launches, warp_ms = the launch of the last level, align_ms = the launch of the level
before it), medians of `reps` repetitions with the candidates alternating in every repetition so that drift hits all alike.
Prints, for both forms of the level kernel (STK_WAVELET_FORM: direct and staged; beyond spacing 32 the direct one runs under
either), the launch of level j (tap spacing 2^j)
  as an inner level, j = 0 .. 6: the level before the last of a (j + 2)-level call. It reads c_j and acc (level 0: c_0 alone)
    and writes c_{j+1} and acc: 4 plane sets moved (level 0: 3), where the yardstick moves 2;
  as the last level, j = 0 .. 7, of a (j + 1)-level call. It reads c_j and acc (level 0: c_0 alone) and writes the interleaved
    output: 3 plane sets moved (level 0: 2);
then the estimation pass and a 4-level and a 6-level call without and with thresholds on an estimated sigma. A one-frame
f32 -> f32 stk_background_apply of the same image runs beside them as the "one read and one write of this image" yardstick
(2 plane sets); every launch is printed as a multiple of it, beside the multiple its own bytes would give.
    python tools/wavelet_time.py [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import Stacker, WaveletParameters, mesh_grid  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import numpy as np
    import torch
    reps = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 5
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
    YARD = "stk_background_apply f32 -> f32 (yardstick)"
    def run(form, p):
        os.environ["STK_WAVELET_FORM"] = form                            # read by the library at every call
        st.wavelet_image(image, p, out=out)

    cases, sets = [], {}
    for form in ("direct", "staged"):
        for j in range(7):
            name = f"{form:6s} level {j} (spacing {2 ** j:3d}), inner, of {j + 2}"
            cases.append((name, "align_ms", lambda f=form, p=WaveletParameters(levels=j + 2, gains=1.5): run(f, p)))
            sets[name] = 4 if j else 3
        for j in range(8):
            name = f"{form:6s} level {j} (spacing {2 ** j:3d}), last of {j + 1}"
            cases.append((name, "warp_ms", lambda f=form, p=WaveletParameters(levels=j + 1, gains=1.5): run(f, p)))
            sets[name] = 3 if j else 2
        for levels in (4, 6):
            cases.append((f"{form:6s} {levels} levels, gains", "finalize_ms", lambda f=form, p=WaveletParameters(levels=levels, gains=1.5): run(f, p)))
            cases.append((f"{form:6s} {levels} levels, thresholds 3, sigma estimated", "finalize_ms",
                          lambda f=form, p=WaveletParameters(levels=levels, thresholds=3.0): run(f, p)))
    cases.append(("the estimation pass (stk_wavelet_sigma)", "prep_ms", lambda: st.wavelet_sigma(image)))
    cases.append((YARD, "finalize_ms", lambda: st.background_apply([image], plane, 64, out=flat_out)))

    def once(rec):
        for name, field, fn in cases:
            fn()
            torch.cuda.synchronize()
            rec[name].append(st.timing()[field])

    once({c[0]: [] for c in cases})                                      # warm-up: code objects, workspaces
    rec = {c[0]: [] for c in cases}
    for _ in range(reps):
        once(rec)
    yard = med(rec[YARD])
    print(f"{w}x{h} BGR f32, device-resident, medians of {reps}:")
    for name, _, _ in cases:
        m = med(rec[name])
        by_bytes = f"  (its bytes: {sets[name] / 2:.1f} x)" if name in sets else ""
        print(f"  {name:52s} {m:9.3f} ms  = {m / yard:6.2f} x the yardstick{by_bytes}")
    for name, _, _ in cases:
        print(f"  {name}, all runs: {' '.join(f'{r:.3f}' for r in rec[name])}", flush=True)


if __name__ == "__main__":
    main()

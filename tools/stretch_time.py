"""Cost of the display stretch (stk_image_stats, stk_stretch, stk_auto_stretch) on a 4K BGR f32 image, device-resident. One
process, one warm-up, device events (the calls' own stk_timing fields: finalize_ms = all launches; for the statistics prep_ms
= the first pass, the counts, min and max and the first digit; warp_ms = one later round, a histogram launch and its pick,
chosen by STK_STRETCH_TIME_ROUND, which the library reads at every call), medians of `reps` repetitions with the candidates
alternating in every repetition so that drift hits all alike.
Prints stk_image_stats on a sky image (a level of 0.02 with a gradient, noise of 0.002, 300 stars: its keys crowd into a few
bins of every round) and on a uniform random image, without and with one quantile (one slot more in every later round), each
round of the call on both images, all of it under both forms of the histogram kernel (STK_STRETCH_HIST_FORM: one LDS atomic
per key, or one per run of equal digits of a thread), stk_stretch to u8, u16 and f32 under each curve and both colour modes, and the whole call.
A one-frame f32 -> f32 stk_background_apply of the same image runs beside them as the "one read and one write of this image"
yardstick, and stk_wavelet_sigma (the other exact selection on an f32 image) beside the statistics; every figure is printed
as a multiple of the yardstick. A round reads the image once and writes nothing, so its bytes are half the yardstick's.
    python tools/stretch_time.py [reps=5]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import (CURVE_ASINH, DEPTH_F32, DEPTH_U8, DEPTH_U16, STRETCH_LINEAR, STRETCH_MTF, STRETCH_TABLE,  # noqa: E402
                               AutoStretchParameters, Stacker, StretchParameters, mesh_grid, stretch_table)


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
    sky = 0.02 + 0.003 * x / w + 0.0015 * y / h
    for _ in range(300):
        sx, sy, amp = (float(torch.rand(1, generator=gen, device="cuda")) for _ in range(3))
        x0, y0 = int(sx * (w - 32)), int(sy * (h - 32))
        yy, xx = y[y0:y0 + 32, x0:x0 + 32] - (y0 + 16), x[y0:y0 + 32, x0:x0 + 32] - (x0 + 16)
        sky[y0:y0 + 32, x0:x0 + 32] += 10 ** (-2.5 + 2.3 * amp) * torch.exp(-(xx * xx + yy * yy) / 12.0)
    images = {"sky": (sky[..., None] * torch.tensor([1.0, 1.4, 0.6], device="cuda") + torch.randn((h, w, 3), generator=gen, device="cuda") * 0.002).contiguous(),
              "random": torch.rand((h, w, 3), generator=gen, device="cuda").contiguous()}
    outs = {DEPTH_U8: torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"), DEPTH_U16: torch.empty((h, w, 3), dtype=torch.uint16, device="cuda"),
            DEPTH_F32: torch.empty((h, w, 3), dtype=torch.float32, device="cuda")}
    torch.cuda.synchronize()
    st = Stacker(0)
    gw, gh = mesh_grid(w, h, 64)
    plane = [np.zeros((gh, gw, 3), np.float32)]
    flat_out = [torch.empty_like(images["sky"])]
    table = stretch_table(CURVE_ASINH, 100.0, 4096)
    rule = st.auto_stretch_image(images["sky"], return_params=True)[1]
    YARD = "stk_background_apply f32 -> f32 (yardstick)"

    def stats(name, quantiles, which=None, form="direct"):
        os.environ["STK_STRETCH_TIME_ROUND"] = which or "v1"                # both read by the library at every call
        os.environ["STK_STRETCH_HIST_FORM"] = form
        st.image_stats(images[name], quantiles=quantiles)

    cases = [(YARD, "finalize_ms", lambda: st.background_apply([images["sky"]], plane, 64, out=flat_out)),
             ("stk_wavelet_sigma, sky image", "finalize_ms", lambda: st.wavelet_sigma(images["sky"]))]
    for name, form in ((n, f) for n in images for f in ("direct", "merged")):
        tag = f"{name}, {form}"
        cases.append((f"stk_image_stats, {tag}", "finalize_ms", lambda n=name, f=form: stats(n, (), None, f)))
        cases.append((f"stk_image_stats, {tag}, one quantile", "finalize_ms", lambda n=name, f=form: stats(n, (0.999,), None, f)))
        cases.append((f"  {tag}: the first pass (count, min, max, digit 0)", "prep_ms", lambda n=name, f=form: stats(n, (), None, f)))
        for which, what in (("v1", "values, round 1"), ("v2", "values, round 2"), ("v3", "values, round 3"), ("m0", "MAD, round 0"), ("m1", "MAD, round 1"),
                            ("m2", "MAD, round 2"), ("m3", "MAD, round 3")):
            cases.append((f"  {tag}: {what}", "warp_ms", lambda n=name, k=which, f=form: stats(n, (), k, f)))
        cases.append((f"  {tag}: values, round 1, one quantile", "warp_ms", lambda n=name, f=form: stats(n, (0.999,), "v1", f)))
    for depth, dname in ((DEPTH_U8, "u8"), (DEPTH_U16, "u16"), (DEPTH_F32, "f32")):
        for curve, cname in ((STRETCH_LINEAR, "linear"), (STRETCH_MTF, "mtf"), (STRETCH_TABLE, "table")):
            for colour in (0, 1):
                p = StretchParameters(curve=curve, colour=colour, out_depth=depth, black=rule.black, white=rule.white, midtone=rule.midtone, table=table)
                cases.append((f"stk_stretch to {dname}, {cname}, colour {colour}", "finalize_ms", lambda p=p, d=depth: st.stretch_image(images["sky"], p, out=outs[d])))

    def whole(depth, form):
        os.environ["STK_STRETCH_HIST_FORM"] = form
        st.auto_stretch_image(images["sky"], AutoStretchParameters(), out_depth=depth, out=outs[depth])

    for depth, dname in ((DEPTH_U8, "u8"), (DEPTH_F32, "f32")):
        for form in ("direct", "merged"):
            cases.append((f"stk_auto_stretch to {dname} (mtf), {form}", "finalize_ms", lambda d=depth, f=form: whole(d, f)))

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
        print(f"  {name:58s} {m:9.4f} ms  = {m / yard:6.2f} x the yardstick  (spread {min(rec[name]) / m:.3f} .. {max(rec[name]) / m:.3f})", flush=True)


if __name__ == "__main__":
    main()

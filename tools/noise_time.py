"""Cost of the noise pass (stk_stack_noise) on the headline stack: N 4K BGR frames, device-resident. One process, device
events (stk_timing.prep_ms), one warm-up, medians of `reps` repetitions with the candidates alternating in every repetition
so that drift hits all alike. Prints the medians of:
  * stk_stack_noise on a u8 SKY stack (a gradient, stars, Gaussian noise of 1.5 .. 8 grey levels: nearly every pixel of a
    wave in a few histogram bins — the concentrated case) and on a u8 UNIFORM RANDOM stack, beside stk_stack_sharpness at
    ksize 3 on the same stacks (one read plus an LDS stencil), with the ratios noise / sharpness and sky / random (what
    same-bin contention costs);
  * the same pass on u16 sky and uniform random stacks of `n16` frames, with the u16 / u8 ratio per byte read;
  * the wall time of the host reduction (stk_noise_from_hist over every frame and channel) at both depths, and the wall
    time of the whole call beside its device time;
  * stk_ecc_match_noise_weighted beside stk_ecc_match_weighted on a synthetic 4K stack of `necc` frames (wall clock around
    the synchronised calls, and stk_timing.finalize_ms).
    python tools/noise_time.py [n=256] [reps=5] [n16=64] [necc=64]"""
import ctypes as C
import json
import os
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import (EccMatchParameters, MotionType, Stacker, WeightParameters, _ffi, synth)  # noqa: E402

SIGMAS = (1.5, 1.5, 2.0, 2.0, 3.0, 4.0, 6.0, 8.0)


def med(v):
    return sorted(v)[len(v) // 2]


def sky_scene(h, w, gen):
    """grey levels, float32 h x w x 3 on the GPU: a gradient per channel and 4000 Gaussian stars"""
    import torch
    import torch.nn.functional as F
    yy = torch.linspace(0, 1, h, device="cuda")[:, None]
    xx = torch.linspace(0, 1, w, device="cuda")[None, :]
    imp = torch.zeros((1, 1, h, w), device="cuda")
    idx = torch.randint(0, h * w, (4000,), generator=gen, device="cuda")
    imp.view(-1)[idx] = 200.0 + 3000.0 * torch.rand(4000, generator=gen, device="cuda") ** 4
    k = torch.arange(-6, 7, device="cuda", dtype=torch.float32)
    g = torch.exp(-k * k / (2 * 1.6 * 1.6))
    g = (g / g.sum())
    stars = F.conv2d(F.conv2d(imp, g.view(1, 1, 1, -1), padding=(0, 6)), g.view(1, 1, -1, 1), padding=(6, 0))[0, 0]
    return torch.stack([20.0 + 6.0 * c + 8.0 * xx + 4.0 * yy + stars for c in range(3)], -1)


def make_stacks(n, h, w, depth, gen):
    import torch
    dt, top, k = (torch.uint8, 255.0, 1.0) if depth == 8 else (torch.uint16, 65535.0, 257.0)
    scene = sky_scene(h, w, gen)
    sky = torch.empty((n, h, w, 3), dtype=dt, device="cuda")
    rnd = torch.empty((n, h, w, 3), dtype=dt, device="cuda")
    for i in range(n):
        f = (scene + torch.randn(scene.shape, generator=gen, device="cuda") * SIGMAS[i % len(SIGMAS)]) * k
        q = torch.clamp(torch.round(f), 0, top)
        sky[i] = q.to(torch.uint8) if depth == 8 else q.to(torch.int32).to(torch.uint16)
        r = torch.randint(0, int(top) + 1, (h, w, 3), generator=gen, device="cuda", dtype=torch.int32)
        rnd[i] = r.to(torch.uint8) if depth == 8 else r.to(torch.uint16)
    return sky, rnd


def reduce_wall(hist, depth):
    """seconds for stk_noise_from_hist over every (frame, channel) of `hist`, called as the engine calls it"""
    lib = _ffi.load()
    bv = 256 if depth == 8 else 65536
    br = hist.shape[2] - bv
    out = _ffi.NoiseStat()
    base, step = hist.ctypes.data, hist.shape[2] * 4
    t0 = time.perf_counter()
    for k in range(hist.shape[0] * hist.shape[1]):
        lib.stk_noise_from_hist(C.c_void_p(base + k * step), bv, C.c_void_p(base + k * step + 4 * bv), br, int(depth == 16), C.byref(out))
    return time.perf_counter() - t0


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    n16 = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    necc = int(sys.argv[4]) if len(sys.argv) > 4 else 64
    w, h = 3840, 2160
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    st = Stacker(0)
    res = {"n": n, "n16": n16, "necc": necc, "reps": reps}

    def noise_ms(frames):
        st.stack_noise(frames)
        return st.timing()["prep_ms"]

    def sharp_ms(frames):
        st.stack_sharpness(frames, 3)
        return st.timing()["prep_ms"]

    # ---- u8
    print("building the u8 stacks", flush=True)
    sky, rnd = make_stacks(n, h, w, 8, gen)
    torch.cuda.synchronize()
    cands = [("noise_sky_u8", noise_ms, sky), ("noise_random_u8", noise_ms, rnd), ("sharpness_sky_u8", sharp_ms, sky), ("sharpness_random_u8", sharp_ms, rnd)]
    for _, fn, fr in cands:
        fn(fr)                                                             # warm-up
    t = {name: [] for name, _, _ in cands}
    for _ in range(reps):
        for name, fn, fr in cands:
            t[name].append(fn(fr))
    for name in t:
        res[name + "_ms"] = round(med(t[name]), 4)
    t0 = time.perf_counter()
    stats, hist = st.stack_noise(sky, return_hist=True)
    res["call_wall_sky_u8_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["reduce_wall_u8_ms"] = round(med([reduce_wall(hist, 8) for _ in range(reps)]) * 1e3, 3)
    est = stats["sigma"][:len(SIGMAS), 0]
    res["sigma_est_first_frames"] = [round(float(v), 3) for v in est]
    del sky, rnd, hist
    torch.cuda.empty_cache()

    # ---- u16
    print("u8 done; building the u16 stacks", flush=True)
    sky16, rnd16 = make_stacks(n16, h, w, 16, gen)
    torch.cuda.synchronize()
    cands = [("noise_sky_u16", noise_ms, sky16), ("noise_random_u16", noise_ms, rnd16)]
    for _, fn, fr in cands:
        fn(fr)
    t = {name: [] for name, _, _ in cands}
    for _ in range(reps):
        for name, fn, fr in cands:
            t[name].append(fn(fr))
    for name in t:
        res[name + "_ms"] = round(med(t[name]), 4)
    t0 = time.perf_counter()
    stats16, hist16 = st.stack_noise(sky16, return_hist=True)
    res["call_wall_sky_u16_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["reduce_wall_u16_ms"] = round(med([reduce_wall(hist16, 16) for _ in range(reps)]) * 1e3, 3)
    res["sigma_est_first_frames_u16_over_257"] = [round(float(v) / 257.0, 3) for v in stats16["sigma"][:len(SIGMAS), 0]]
    del sky16, rnd16, hist16
    torch.cuda.empty_cache()

    # ---- ratios
    res["noise_over_sharpness_sky"] = round(res["noise_sky_u8_ms"] / res["sharpness_sky_u8_ms"], 3)
    res["noise_over_sharpness_random"] = round(res["noise_random_u8_ms"] / res["sharpness_random_u8_ms"], 3)
    res["sky_over_random_u8"] = round(res["noise_sky_u8_ms"] / res["noise_random_u8_ms"], 3)
    res["sky_over_random_u16"] = round(res["noise_sky_u16_ms"] / res["noise_random_u16_ms"], 3)
    res["u16_over_u8_per_byte_sky"] = round((res["noise_sky_u16_ms"] / (n16 * 2)) / (res["noise_sky_u8_ms"] / n), 3)
    res["noise_sky_u8_GBps"] = round(n * h * w * 3 / (res["noise_sky_u8_ms"] * 1e-3) / 1e9, 1)

    # ---- the whole-stack forms
    print("u16 done; building the ECC stack", flush=True)
    frames, _ = synth.make_stack(necc, w, h, device="cuda")
    ecc = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    wp = WeightParameters(2, True, 0)

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(frames, ecc, wp)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, st.timing()["finalize_ms"]
    forms = [("ecc_match_weighted", st.ecc_match_weighted), ("ecc_match_noise_weighted", st.ecc_match_noise_weighted)]
    for _, fn in forms:
        run(fn)
    t = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, fn in forms:
            t[name].append(run(fn))
    for name in t:
        res[name + "_wall_ms"] = round(med([a for a, _ in t[name]]), 3)
        res[name + "_finalize_ms"] = round(med([b for _, b in t[name]]), 3)
    for k, v in res.items():
        print(f"{k:40s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

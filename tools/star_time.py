"""Cost of star registration (stk_star_detect, stk_star_align) on the headline stack: N 4K u8 BGR frames, device-resident.
One process, warmed up, medians of `reps` repetitions with the candidates alternating in every repetition so that drift
hits all alike. Prints the medians of:
  * the detection launch (device events: stk_timing.prep_ms of stk_star_detect) beside stk_stack_sharpness at ksize 3
    (prep_ms too), which has the same one-read-of-the-stack shape;
  * stk_star_detect and stk_star_align end to end (wall clock around the synchronised calls: launch, the two copies back,
    the host merge; for the alignment also triangles, votes and the two batched fits);
  * the host matching alone: stk_star_match_lists of every moving frame's list against frame 0's, one call after the
    other on one thread (wall clock; inside stk_star_align the same work runs on the context's host pool).
The stack: one rendered star field (synth.make_star_stack, `stars` per frame), every frame a whole-pixel shift of it
with its own sensor noise, made on the device.
    python tools/star_time.py [n=256] [reps=5] [stars=2000]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import Stacker, StarParameters, star_match_lists, synth  # noqa: E402


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    import torch
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    stars = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    w, h = 3840, 2160
    base, _ = synth.make_star_stack([None], w, h, stars, noise_sigma=0.0, channels=1)
    base = torch.from_numpy(base[0]).cuda().to(torch.float32)
    gen = torch.Generator(device="cuda")
    frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    for i in range(n):
        gen.manual_seed(1000 + i)
        f = torch.roll(base, shifts=((7 * i) % 23 - 11, (5 * i) % 31 - 15), dims=(0, 1)) if i else base
        f = f + torch.randn(f.shape, generator=gen, device="cuda") * 2.0
        frames[i] = torch.clamp(torch.round(f), 0, 255).to(torch.uint8)[..., None]
    st = Stacker(0)
    p = StarParameters()
    keys = ["star detection launch", "stack_sharpness, ksize 3", "star_detect, wall", "star_align, wall", "host matching alone, wall"]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def once(rec):
        t, lists = wall(lambda: st.star_detect(frames, p))
        rec[keys[0]].append(st.timing()["prep_ms"])
        rec[keys[2]].append(t)
        st.stack_sharpness(frames, 3)
        rec[keys[1]].append(st.timing()["prep_ms"])
        t, (dropped, stats) = wall(lambda: st.star_align(frames, p))
        rec[keys[3]].append(t)
        t, _ = wall(lambda: [star_match_lists(lists[i], lists[0], p) for i in range(1, n)])
        rec[keys[4]].append(t)
        return lists, dropped, stats

    once({k: [] for k in keys})                          # warm-up: code objects, workspaces
    rec = {k: [] for k in keys}
    for _ in range(reps):
        lists, dropped, stats = once(rec)
    v = {k: med(rec[k]) for k in keys}
    print(f"{n} x {w}x{h} u8 BGR, device-resident, {stars} stars per frame, medians of {reps} (ms):")
    for k in keys:
        print(f"  {k:40s} {v[k]:10.3f}")
    print(f"  detection launch / stack_sharpness: {v[keys[0]] / v[keys[1]]:.2f}")
    print(f"  stars kept per frame: {min(len(a) for a in lists)} .. {max(len(a) for a in lists)}; dropped {dropped} of {n - 1};"
          f" inliers {min(s['n_inliers'] for s in stats[1:])} .. {max(s['n_inliers'] for s in stats[1:])}")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{x:.3f}' for x in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

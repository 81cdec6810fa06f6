"""Cost of scoring and ranking the headline stack: N 4K u8 BGR frames (device-resident). Prints medians of alternated
repetitions of: the scoring pass's device time (prep_ms of stack_sharpness) at ksize 3 and 7, the wall time of
stack_sharpness, the wall time of the per-frame route (stk_grey + four stk_sharpness calls per frame, all on device
memory) and the wall time of ecc_match_ranked beside ecc_match on the already ordered list.
  python tools/quality_time.py [n=256] [reps=5] [--per-frame-only]
--per-frame-only times the per-frame route alone and uses only symbols every earlier build of the library has, so the same
file gives the baseline on a build of the commit before the scoring pass existed."""
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import EccMatchParameters, MotionType, Stacker, _ffi, synth  # noqa: E402


def per_frame_route(st, frames, grey, ksize):
    """main.rs:40-47 frame by frame: grey into device memory, then LAPM, LAPV, TENG(ksize), GLVN of it."""
    n, h, w, c = frames.shape
    step = h * w * c
    out = C.c_double(0.0)
    scores = []
    for i in range(n):
        ptr = (C.c_void_p * 1)(frames.data_ptr() + i * step)
        fr = _ffi.Frames(C.cast(ptr, C.POINTER(C.c_void_p)), 1, w, h, c, 8, 1, 0)
        st._check(st._lib.stk_grey(st._h, C.byref(fr), C.c_void_p(grey.data_ptr())))
        row = []
        for metric in range(4):
            st._check(st._lib.stk_sharpness(st._h, C.c_void_p(grey.data_ptr()), 8, w, h, 1, metric, ksize, C.byref(out)))
            row.append(out.value)
        scores.append(row)
    return scores


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only = "--per-frame-only" in sys.argv
    n = int(args[0]) if len(args) > 0 else 256
    reps = int(args[1]) if len(args) > 1 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    grey = torch.empty((2160, 3840), dtype=torch.uint8, device="cuda")
    st = Stacker(0)
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    per_frame_route(st, frames[:2], grey, 3)                   # warm-up: code objects, workspaces
    if only:
        pf, pf7 = [], []
        for _ in range(reps):                                  # alternated, so that drift hits both alike
            pf.append(wall(lambda: per_frame_route(st, frames, grey, 3))[0])
            pf7.append(wall(lambda: per_frame_route(st, frames, grey, 7))[0])
        print(f"{n} x 3840x2160 u8, medians of {reps}:")
        for k, v in ((3, pf), (7, pf7)):
            print(f"  per-frame route (grey + 4 sharpness calls per frame), ksize {k} {med(v) * 1e3:9.2f} ms   all: "
                  + " ".join(f"{t * 1e3:.2f}" for t in v), flush=True)
        return

    from libstacker_rs_amd import SelectParameters
    p = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    sel = SelectParameters()
    order, n_kept, scores, _ = st.rank(frames, sel)
    ordered = [frames[int(i)] for i in order]
    for _ in range(2):
        st.stack_sharpness(frames, 3)
        st.stack_sharpness(frames, 7)
        st.ecc_match(ordered, p)
        st.ecc_match_ranked(ordered, p, sel)
    pf, pf7, ss, ss7, dev, dev7, plain, ranked, ranked_prep = [], [], [], [], [], [], [], [], []
    ref = None
    for _ in range(reps):                                      # alternated, so that drift hits all alike
        t, ref = wall(lambda: per_frame_route(st, frames, grey, 3))
        pf.append(t)
        t, got = wall(lambda: st.stack_sharpness(frames, 3))
        ss.append(t)
        dev.append(st.timing()["prep_ms"])
        assert got.tolist() == ref, "the pass and the per-frame route disagree"
        pf7.append(wall(lambda: per_frame_route(st, frames, grey, 7))[0])
        ss7.append(wall(lambda: st.stack_sharpness(frames, 7))[0])
        dev7.append(st.timing()["prep_ms"])
        plain.append(wall(lambda: st.ecc_match(ordered, p))[0])
        plain_prep = st.timing()["prep_ms"]
        ranked.append(wall(lambda: st.ecc_match_ranked(ordered, p, sel))[0])
        ranked_prep.append(st.timing()["prep_ms"] - plain_prep)
    px = n * 3840 * 2160
    print(f"{n} x 3840x2160 u8, medians of {reps}:")
    for k, d, s, f in ((3, dev, ss, pf), (7, dev7, ss7, pf7)):
        print(f"  ksize {k}: pass device time {med(d):8.3f} ms   {px * 3 / med(d) / 1e9:.2f} TB/s of frame bytes   {med(d) * 1e6 / px * 1e3:.3f} ps/px")
        print(f"           stack_sharpness wall {med(s) * 1e3:8.2f} ms   per-frame route wall {med(f) * 1e3:9.2f} ms   ratio {med(f) / med(s):.1f} x")
    print(f"  ecc_match on the ordered list {med(plain) * 1e3:8.2f} ms   ecc_match_ranked {med(ranked) * 1e3:8.2f} ms   "
          f"(+{(med(ranked) - med(plain)) * 1e3:.2f} ms; prep_ms grew by {med(ranked_prep):.3f})", flush=True)


if __name__ == "__main__":
    main()

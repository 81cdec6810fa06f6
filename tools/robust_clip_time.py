"""Cost of the median / MAD clip (stk_robust_clip_stack) next to the other two rejection combines on the headline stack: N
4K u8 BGR frames (device-resident) under the warps of their own ECC homography run. One process, device events
(stk_timing.finalize_ms: the combine's device time), warmed up, the combines alternating in every repetition so that drift
hits all alike. Prints the medians of: the robust clip at 1, 2 and 3 iterations with the selection kernel's share of each
(stk_get_counter "robust_select_us"), the median combine (stk_quantile_stack, q = 0.5), the plain clip at 2 iterations
(stk_clip_stack: finalize_ms covers its 3 passes, not the mean fold they start from), and the ratios.
    python tools/robust_clip_time.py [n=256] [reps=5]
A pixel-channel leaves the selection's rounds when a round rejects nothing, so the time of iterations 2 and 3 depends on
the data: the synthetic stack (libstacker_rs_amd.synth) has noise but no planted outliers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import (EccMatchParameters, MotionType, RobustClipParameters, SigmaClipParameters, Stacker,  # noqa: E402
                               synth)


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    _, stats = st.ecc_match(frames, EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5), return_stats=True)
    warps = [s["warp"] for s in stats]
    robust = {T: RobustClipParameters(3.0, 3.0, 0.5 / 255.0, T) for T in (1, 2, 3)}
    clip = SigmaClipParameters(3.0, 3.0, 2)
    keys = [f"robust clip, {T} iteration{'s' if T > 1 else ''}" for T in robust] + ["median (quantile 0.5)", "plain clip, 2 iterations"]

    def once(rec, sel):
        for T, k in zip(robust, keys):
            _, cnt = st.robust_clip_stack(frames, warps, robust[T], return_counts=True)
            t = st.timing()
            rec[k].append(t["finalize_ms"])
            sel[k].append(t["robust_select_us"] / 1000.0)
            rejected = float((cnt < n).float().mean())
        st.quantile_stack(frames, warps, 0.5)
        rec[keys[3]].append(st.timing()["finalize_ms"])
        st.clip_stack(frames, warps, clip)
        rec[keys[4]].append(st.timing()["finalize_ms"])
        return rejected

    once({k: [] for k in keys}, {k: [] for k in keys})            # warm-up: code objects, workspaces
    rec, sel = {k: [] for k in keys}, {k: [] for k in keys}
    for _ in range(reps):
        rejected = once(rec, sel)
    q, c = med(rec[keys[3]]), med(rec[keys[4]])
    print(f"{n} x 3840x2160 u8 BGR, device-resident, medians of {reps} (ms of stk_timing.finalize_ms):")
    print(f"  {'':30s} {'combine':>9s} {'select':>9s} {'share':>6s} {'/ median':>9s} {'/ clip':>7s}")
    for k in keys[:3]:
        a, s = med(rec[k]), med(sel[k])
        print(f"  {k:30s} {a:9.3f} {s:9.3f} {s / a:6.2f} {a / q:9.2f} {a / c:7.2f}")
    print(f"  {keys[3]:30s} {q:9.3f}")
    print(f"  {keys[4]:30s} {c:9.3f}")
    print(f"  pixel-channels the 3-iteration robust clip rejected a sample from: {100.0 * rejected:.2f} %")
    for k in keys:
        print(f"  {k}, all runs: {' '.join(f'{v:.3f}' for v in rec[k])}", flush=True)


if __name__ == "__main__":
    main()

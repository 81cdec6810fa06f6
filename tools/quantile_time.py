"""Cost of the median combine on the headline stack: N 4K u8 BGR frames (device-resident), ECC homography, q = 0.5.
Prints the plain call and the quantile call (wall time; the combine's device time, finalize_ms), the store and selection
launches per band and in total (from the torch profiler's kernel records), and stk_quantile_stack on 1024 small u16
frames (the large-N selection path):  python tools/quantile_time.py [n=256] [reps=5]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libstacker_rs_amd import BORDER_REPLICATE, EccMatchParameters, MotionType, QuantileParameters, Stacker, synth  # noqa: E402

med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731


def kernel_split(fn):
    """(store ms per launch, select ms per launch) of one call of fn, from the profiler's device records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    store, select = [], []
    for e in prof.events():
        ms = e.device_time / 1e3 if hasattr(e, "device_time") else e.cuda_time / 1e3
        if "FoldStore" in e.name:
            store.append(ms)
        elif "quantile_select" in e.name:
            select.append(ms)
    return store, select


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    frames, _ = synth.make_stack(n, 3840, 2160, device="cuda")
    st = Stacker(0)
    p = EccMatchParameters(MotionType.Homography, 5000, 1e-5, 5)
    q = QuantileParameters(0.5)
    for _ in range(2):                                         # warm-up: code objects, workspaces
        st.ecc_match(frames, p)
        st.ecc_match_quantile(frames, p, q)
    torch.cuda.synchronize()
    plain_s, quant_s, warp_ms, fin_ms = [], [], [], []
    for _ in range(reps):                                      # alternated, so that drift hits both alike
        t0 = time.perf_counter()
        st.ecc_match(frames, p)
        torch.cuda.synchronize()
        plain_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        st.ecc_match_quantile(frames, p, q)
        torch.cuda.synchronize()
        quant_s.append(time.perf_counter() - t0)
        t = st.timing()
        warp_ms.append(t["warp_ms"]); fin_ms.append(t["finalize_ms"])
    print(f"{n} x 3840x2160 u8 ECC homography, q = 0.5, medians of {reps}:")
    print(f"  warp_ms (plain fold)          {med(warp_ms):8.3f}")
    print(f"  finalize_ms (median combine)  {med(fin_ms):8.3f}")
    print(f"  plain call    {med(plain_s) * 1e3:8.2f} ms   {n / med(plain_s):8.1f} frames/s")
    print(f"  median call   {med(quant_s) * 1e3:8.2f} ms   {n / med(quant_s):8.1f} frames/s   "
          f"(+{(med(quant_s) - med(plain_s)) * 1e3:.2f} ms; target +36 ms)", flush=True)
    try:
        store, select = kernel_split(lambda: st.ecc_match_quantile(frames, p, q))
    except Exception as e:                                     # a profiler without device records
        print(f"  store / selection split: not available ({e})")
    else:
        print(f"  bands {len(store)}: store {' '.join(f'{v:.2f}' for v in store)} ms; "
              f"select {' '.join(f'{v:.2f}' for v in select)} ms")
        print(f"  store total {sum(store):.2f} ms, selection total {sum(select):.2f} ms", flush=True)
    # large N: 1024 frames of 256 x 64 u16 BGR, quantile 0.5, caller-held warps
    big = torch.from_numpy(np.random.default_rng(1).integers(0, 65536, (1024, 64, 256, 3), dtype=np.uint16)).cuda()
    warps = [np.eye(3)] * 1024
    kw = dict(border_mode=BORDER_REPLICATE, alpha=1.0 / 65535.0)
    st.quantile_stack(big, warps, q, **kw)
    ms = []
    for _ in range(reps):
        st.quantile_stack(big, warps, q, **kw)
        ms.append(st.timing()["finalize_ms"])
    print(f"stk_quantile_stack, 1024 x 256x64 u16 BGR, q = 0.5: combine {med(ms):.2f} ms", flush=True)
    st.close()


if __name__ == "__main__":
    main()

// kernels_quantile.hip — median and quantile stacking (stk_quantile_stack and the *_quantile entry points; definition in
// include/stacker.h). Two launches per band of destination rows:
//   * store: the fold kernels of warp_body.h in their store mode write each sample of the band to HBM (frame-major,
//     band[i * m + k] for the k-th pixel-channel of the band and table entry i) — the very values the mean fold adds;
//   * select: per pixel-channel, the exact order statistics s_(j) and s_(j+1) of its n samples, then the formula.
// Selection (select_body.h: the keys, the lane split, the staging and the bisection, shared with robust_select_kernel):
// s_(j) by MSB-first bisection: 32 rounds of "how many keys <= prefix | (2^b - 1)". s_(j+1) (only where g != 0) by one
// more round: s_(j) again if at least j + 2 keys are <= s_(j), else the smallest key above it.
#include "fold_launch.h"
#include "select_body.h"

namespace stk {

struct QuantileSelectArgs {
    const float* band;       // n x m samples, frame-major
    float* out;              // m outputs
    size_t m;
    int n;
    int log2_splits;         // S = 2^log2_splits lanes per pixel-channel (<= 64), Tw = 64 / S pixel-channels per wave
    int j;                   // lo = s_(j)
    float g;                 // the fraction; 0: lo itself, no s_(j+1) needed
};

// Plain keys (NaN: the largest key, and the output NaN); j and g are uniform, from the argument block.
template <int G>
__global__ __launch_bounds__(SEL_THREADS) void quantile_select_kernel(QuantileSelectArgs a) {
    constexpr int KPT = 4 * G;                          // keys per lane
    const int ls = a.log2_splits, Tw = 64 >> ls;
    const SelLane l = sel_stage<G>(a.band, a.m, a.n, ls, SelKeyPlain{});
    uint32_t key[KPT];
    sel_load<G>(key);
    // NaN samples: the largest key at a frame index < n (beyond n it is padding)
    uint32_t nan = 0;
#pragma unroll
    for (int e = 0; e < KPT; e++) nan += (key[e] == SEL_PAD) & (l.s * KPT + e < a.n);
    nan = sel_sum(nan, Tw);

    const uint32_t need = (uint32_t)a.j + 1;
    uint32_t lo;
    SEL_BISECT(lo, key, KPT, 31, need, Tw)
    // s_(j+1) only where it is used (a uniform branch; g != 0 implies j + 1 <= n - 1: one exists)
    uint32_t hi = lo;
    if (a.g != 0.0f) hi = sel_next<KPT>(key, lo, need, Tw);
    if (l.s != 0 || l.col >= a.m) return;
    a.out[l.col] = nan ? __builtin_nanf("") : sel_mid(sel_value(lo), sel_value(hi), a.g);
}

hipError_t launch_quantile_select(const float* band, size_t m, int n, int j, float g, float* out, hipStream_t s) {
    if (n < 1 || n > QUANTILE_MAX_SAMPLES || m == 0) return hipErrorInvalidValue;
    const SelectPlan p = select_plan(m, n);
    QuantileSelectArgs a{};
    a.band = band; a.out = out; a.m = m; a.n = n; a.log2_splits = p.ls; a.j = j; a.g = g;
    return launch_select<SEL_KERNELS(quantile_select_kernel)>(p, a, s);
}

// The store launch of both quantile forms: State = FoldStore, or FoldStoreW (which needs c.coef)
template <template <int> class State>
static hipError_t launch_store(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0 || c.band_rows <= 0 || a.dh != c.y0 + c.band_rows) return hipErrorInvalidValue;
    return launch_fold<State<3>, State>(a, c, depth, c.band_rows, s);
}

hipError_t launch_quantile_store(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    return launch_store<FoldStore>(a, c, depth, s);
}

// ---- the quantile with participation (stk_quantile_stack_weighted and the *_quantile_weighted entry points) ---------
// The band holds normalised samples and QUANTILE_ABSENT_BITS (a signalling NaN, which no sample is) for an entry that is
// no sample of the pixel (FoldStoreW, warp_body.h). Masked keys (select_body.h): an absent entry takes the padding key,
// which no bisection candidate with a clear bit counts — except the last one below the NaN key, which is why NaN gets the
// key below it and is counted like a sample: it ranks last, as in the plain kernel, and makes the output NaN. N_p is one
// more count round (keys below the padding key); j, g and the bisection threshold j + 1 are per-lane values (sel_rank).
struct QuantileSelectMaskedArgs {
    const float* band;       // n x m samples, frame-major
    float* out;              // m outputs
    int* counts;             // m / cn pixel counts N_p (optional)
    size_t m;
    int n;
    int log2_splits;
    int cn;
    float q;
};

template <int G>
__global__ __launch_bounds__(SEL_THREADS) void quantile_select_masked_kernel(QuantileSelectMaskedArgs a) {
    constexpr int KPT = 4 * G;
    const int ls = a.log2_splits, Tw = 64 >> ls;
    const SelLane l = sel_stage<G>(a.band, a.m, a.n, ls, SelKeyMasked{1});
    uint32_t key[KPT];
    sel_load<G>(key);
    // N_p: the keys below the padding key; NaN samples: the key just below it
    uint32_t np = 0, nan = 0;
#pragma unroll
    for (int e = 0; e < KPT; e++) { np += key[e] != SEL_PAD; nan += key[e] == SEL_NAN; }
    np = sel_sum(np, Tw);
    nan = sel_sum(nan, Tw);
    uint32_t need;
    float gq;
    sel_rank(np, a.q, need, gq);
    uint32_t lo;
    SEL_BISECT(lo, key, KPT, 31, need, Tw)
    const uint32_t hi = sel_next<KPT>(key, lo, need, Tw);
    if (l.s != 0 || l.col >= a.m) return;
    float r;
    if (np == 0) r = 0.0f;
    else if (nan) r = __builtin_nanf("");
    else r = sel_mid(sel_value(lo), sel_value(hi), gq);
    a.out[l.col] = r;
    if (a.counts && l.col % (size_t)a.cn == 0) a.counts[l.col / (size_t)a.cn] = (int)np;
}

hipError_t launch_quantile_select_masked(const float* band, size_t m, int n, float q, int cn, float* out, int* counts, hipStream_t s) {
    if (n < 1 || n > QUANTILE_MAX_SAMPLES || m == 0 || cn < 1 || m % (size_t)cn != 0) return hipErrorInvalidValue;
    const SelectPlan p = select_plan(m, n);
    QuantileSelectMaskedArgs a{};
    a.band = band; a.out = out; a.counts = counts; a.m = m; a.n = n; a.log2_splits = p.ls; a.cn = cn; a.q = q;
    return launch_select<SEL_KERNELS(quantile_select_masked_kernel)>(p, a, s);
}

hipError_t launch_quantile_store_weighted(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (!c.coef) return hipErrorInvalidValue;
    return launch_store<FoldStoreW>(a, c, depth, s);
}

}  // namespace stk

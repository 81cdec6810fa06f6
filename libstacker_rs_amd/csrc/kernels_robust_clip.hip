// kernels_robust_clip.hip — median / MAD sigma clipping (stk_robust_clip_stack and the *_robust_clipped entry points;
// definition in include/stacker.h). Per band of destination rows the combine is the quantile's store launch
// (kernels_quantile.hip, unchanged) and the selection kernel below, which turns the band's samples into the centre c and
// the bounds L, U of every pixel-channel and writes them straight into the clip planes; after the last band ONE last clip
// pass (kernels_clip.hip, unchanged) sums the kept samples in fold order.
// The kernel is a body over the shared selection core (select_body.h), with quantile_select_masked_kernel's keys:
// order-preserving u32 keys (an absent entry and the padding beyond n: all ones; NaN: the key below), staged once through
// LDS into the owner lanes' 16-byte slots, 4G keys per lane in registers (fully unrolled, no scratch), S lanes of one wave
// per pixel-channel, counts meeting by lane shuffles, no barrier after the staging one. The median's rank is sel_rank at
// q = 0.5f. The staged keys stay in LDS for the kernel's life: K only shrinks, so the keys of a
// round are the staged ones filtered by [L, U] (a lane reads back only the slots it owns), and the registers can hold the
// deviation keys in between. A round:
//   1. deviation keys in place: e = |value(key) - c| is a non-negative f32 (or NaN: the largest key, 0x7fffffff), so its
//      bits order as an integer with bit 31 clear: 31 bisection rounds for e_(j), one more for e_(j+1);
//   2. sigma and the bounds;
//   3. the slots again from LDS, keys outside [L, U] replaced by the padding key, k recounted, and the 32-round bisection
//      for the median of what is left.
// A pixel-channel is done when k < 3, or when a round rejected nothing (the next round would find the same c, mad and
// bounds); a wave leaves the loop when all its pixel-channels are done.
#include "select_body.h"

namespace stk {

struct RobustSelectArgs {
    const float* band;       // n x m samples, frame-major
    float* c;                // m centres, lower and upper bounds (the clip planes at the band's first row)
    float* L;
    float* U;
    size_t m;
    int n;
    int log2_splits;         // S = 2^log2_splits lanes per pixel-channel (<= 64), Tw = 64 / S pixel-channels per wave
    int masked;              // the band marks absent entries with QUANTILE_ABSENT_BITS (FoldStoreW)
    int iterations;
    float kappa_low, kappa_high, sigma_floor;
};

template <int G>
__global__ __launch_bounds__(SEL_THREADS) void robust_select_kernel(RobustSelectArgs a) {
    constexpr int KPT = 4 * G;
    const int ls = a.log2_splits, Tw = 64 >> ls;
    const SelLane l = sel_stage<G>(a.band, a.m, a.n, ls, SelKeyMasked{a.masked});
    const int tid = threadIdx.x;
    uint32_t key[KPT];
    sel_load<G>(key);
    uint32_t k = 0, nan = 0;
#pragma unroll
    for (int e = 0; e < KPT; e++) { k += key[e] != SEL_PAD; nan += key[e] == SEL_NAN; }
    k = sel_sum(k, Tw);
    nan = sel_sum(nan, Tw);

    // c = med(all samples); a NaN sample: c = NaN and nothing is clipped (the last pass makes the output NaN); no sample
    // at all (the participation form): c = 0
    uint32_t need, lo, hi;
    float g;
    sel_rank(k, 0.5f, need, g);
    sel_pair<KPT, 31>(key, need, Tw, lo, hi);
    float c = sel_mid(sel_value(lo), sel_value(hi), g);
    if (nan) c = __builtin_nanf("");
    if (k == 0) c = 0.0f;
    float L = -__builtin_inff(), U = __builtin_inff();
    bool live = (nan == 0) & (k >= 3);

    for (int round = 0; round < a.iterations; round++) {
        if (__ballot(live) == 0) break;
        // (lanes of a pixel-channel that is done go along: their c, L, U and k stay)
#pragma unroll
        for (int e = 0; e < KPT; e++) {
            const float d = __builtin_fabsf(sel_value(key[e]) - c);
            key[e] = key[e] == SEL_PAD ? SEL_PAD : (d != d ? 0x7fffffffu : __float_as_uint(d));
        }
        sel_pair<KPT, 30>(key, need, Tw, lo, hi);
        const float mad = sel_mid(__uint_as_float(lo), __uint_as_float(hi), g);
        const float sigma = __builtin_fmaxf(1.4826f * mad, a.sigma_floor);
        if (live) {
            L = __builtin_fmaxf(L, c - a.kappa_low * sigma);
            U = __builtin_fminf(U, c + a.kappa_high * sigma);
        }
        // the staged keys again, from LDS (not kept in registers: see the header)
        uint32_t kk = 0;
#pragma unroll
        for (int gi = 0; gi < G; gi++) {
            const uint4 v = sel_keys4[gi * SEL_THREADS + tid];
            const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float sv = sel_value(q[e]);
                const bool in = (q[e] != SEL_PAD) & (L <= sv) & (sv <= U);
                key[4 * gi + e] = in ? q[e] : SEL_PAD;
                kk += in;
            }
        }
        kk = sel_sum(kk, Tw);
        uint32_t need2;
        float g2;
        sel_rank(kk, 0.5f, need2, g2);
        sel_pair<KPT, 31>(key, need2, Tw, lo, hi);
        if (live) {
            if (kk > 0) c = sel_mid(sel_value(lo), sel_value(hi), g2);
            live = (kk >= 3) & (kk != k);
            k = kk; need = need2; g = g2;
        }
    }
    if (l.s != 0 || l.col >= a.m) return;
    a.c[l.col] = c; a.L[l.col] = L; a.U[l.col] = U;
}

hipError_t launch_robust_select(const float* band, size_t m, int n, int masked, const stk_robust_clip_params& p, float* c, float* L,
                                float* U, hipStream_t s) {
    if (n < 1 || n > QUANTILE_MAX_SAMPLES || m == 0) return hipErrorInvalidValue;
    const SelectPlan plan = select_plan(m, n);
    RobustSelectArgs a{};
    a.band = band; a.c = c; a.L = L; a.U = U; a.m = m; a.n = n; a.log2_splits = plan.ls; a.masked = masked;
    a.iterations = p.iterations; a.kappa_low = p.kappa_low; a.kappa_high = p.kappa_high; a.sigma_floor = p.sigma_floor;
    return launch_select<SEL_KERNELS(robust_select_kernel)>(plan, a, s);
}

}  // namespace stk

// kernels_quantile.hip — median and quantile stacking (stk_quantile_stack and the *_quantile entry points; definition in
// include/stacker.h). Two launches per band of destination rows:
//   * store: the fold kernels of warp_body.h in their store mode write each sample of the band to HBM (frame-major,
//     band[i * m + k] for the k-th pixel-channel of the band and table entry i) — the very values the mean fold adds;
//   * select: per pixel-channel, the exact order statistics s_(j) and s_(j+1) of its n samples, then the formula.
// Selection works on order-preserving u32 keys (negative floats: all bits flipped; others: the sign bit set; NaN: the
// largest key, and the output NaN). Each pixel-channel's keys are split over S = 1 .. 64 lanes of ONE wave (lane = s * Tw +
// t, Tw = 64 / S pixel-channels per wave), each lane holding 4G keys in registers (G = 1, 2, 4, 8 or 16, a template
// parameter: fully unrolled, no scratch), so the partial counts meet by lane shuffles and no round needs a barrier.
// A workgroup (4 waves, T = 256 / S pixel-channels) stages its keys once through LDS: coalesced frame-row loads of T
// consecutive pixel-channels, 4 frames per 16-byte LDS store into the owner lane's slot, one barrier, then each lane reads
// its G slots (keys[g * 256 + tid], consecutive lanes on consecutive 16-byte slots: conflict-free ds_read_b128).
// s_(j) by MSB-first bisection: 32 rounds of "how many keys <= prefix | (2^b - 1)". s_(j+1) (only where g != 0) by one
// more round: s_(j) again if at least j + 2 keys are <= s_(j), else the smallest key above it.
#include "warp_cubic_body.h"

namespace stk {

constexpr int QSEL_THREADS = 256;

struct QuantileSelectArgs {
    const float* band;       // n x m samples, frame-major
    float* out;              // m outputs
    size_t m;
    int n;
    int log2_splits;         // S = 2^log2_splits lanes per pixel-channel (<= 64), Tw = 64 / S pixel-channels per wave
    int j;                   // lo = s_(j)
    float g;                 // the fraction; 0: lo itself, no s_(j+1) needed
};

__device__ __forceinline__ uint32_t quantile_key(float v) {
    const uint32_t u = __float_as_uint(v);
    if (v != v) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float quantile_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// sum / min over the S lanes of a pixel-channel (lane bits log2(Tw) .. 5)
__device__ __forceinline__ uint32_t qsel_sum(uint32_t v, int Tw) {
    for (int d = Tw; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t qsel_min(uint32_t v, int Tw) {
    for (int d = Tw; d < 64; d <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

template <int G>
__global__ __launch_bounds__(QSEL_THREADS) void quantile_select_kernel(QuantileSelectArgs a) {
    extern __shared__ uint4 keys4[];                    // [G][256]: slot g of lane tid at keys4[g * 256 + tid]
    constexpr int KPT = 4 * G;                          // keys per lane
    const int ls = a.log2_splits, S = 1 << ls, Tw = 64 >> ls, T = QSEL_THREADS >> ls;
    const int tid = threadIdx.x;

    // stage: thread (phase p, column c) loads frame groups q = p, p + S, ... (4 frames each) of column c: the T lanes of a
    // phase read T consecutive floats of a frame row. Group q belongs to split s = q / G, slot q % G of the owner lane.
    {
        const int c = tid & (T - 1), p = tid >> (8 - ls);
        const size_t col = (size_t)blockIdx.x * T + c;
        const int owner = (c / Tw) * 64 + (c % Tw);     // the lane of split 0 of column c
        for (int q = p; q < S * G; q += S) {
            uint32_t k[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = q * 4 + e;
                k[e] = (col < a.m && i < a.n) ? quantile_key(a.band[(size_t)i * a.m + col]) : 0xffffffffu;
            }
            keys4[(q % G) * QSEL_THREADS + owner + (q / G) * Tw] = uint4{k[0], k[1], k[2], k[3]};
        }
    }
    __syncthreads();
    const int lane = tid & 63, s = lane / Tw, t = (tid >> 6) * Tw + (lane % Tw);
    const size_t col = (size_t)blockIdx.x * T + t;
    uint32_t key[KPT];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint4 v = keys4[g * QSEL_THREADS + tid];
        key[4 * g] = v.x; key[4 * g + 1] = v.y; key[4 * g + 2] = v.z; key[4 * g + 3] = v.w;
    }
    // NaN samples: the largest key at a frame index < n (beyond n it is padding)
    uint32_t nan = 0;
#pragma unroll
    for (int e = 0; e < KPT; e++) nan += (key[e] == 0xffffffffu) & (s * KPT + e < a.n);
    nan = qsel_sum(nan, Tw);

    // s_(j): bit b of the answer is 0 iff at least j + 1 keys are <= (the bits above b) | (2^b - 1). That candidate has
    // bit b clear, so it is never the all-ones key: padding is never counted.
    const uint32_t need = (uint32_t)a.j + 1;
    uint32_t lo = 0;
    for (int b = 31; b >= 0; b--) {
        const uint32_t cand = lo | ((1u << b) - 1u);
        uint32_t c0 = 0, c1 = 0;
#pragma unroll
        for (int e = 0; e < KPT; e += 2) { c0 += key[e] <= cand; c1 += key[e + 1] <= cand; }
        if (qsel_sum(c0 + c1, Tw) < need) lo |= 1u << b;
    }
    // s_(j+1): lo again if j + 2 keys are <= lo, else the smallest key above lo (g != 0 implies j + 1 <= n - 1: one exists)
    uint32_t hi = lo;
    if (a.g != 0.0f) {
        uint32_t c = 0, above = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < KPT; e++) {
            c += key[e] <= lo;
            above = min(above, key[e] > lo ? key[e] : 0xffffffffu);
        }
        c = qsel_sum(c, Tw);
        above = qsel_min(above, Tw);
        hi = c >= need + 1 ? lo : above;
    }
    if (s != 0 || col >= a.m) return;
    float r;
    if (nan) r = __builtin_nanf("");
    else {
        const float l = quantile_value(lo);
        if (a.g == 0.0f) r = l;
        else {
            const float h = quantile_value(hi), d = h - l;
            r = a.g >= 0.5f ? h - d * (1.0f - a.g) : l + d * a.g;
        }
    }
    a.out[col] = r;
}

hipError_t launch_quantile_select(const float* band, size_t m, int n, int j, float g, float* out, hipStream_t s) {
    if (n < 1 || n > QUANTILE_MAX_SAMPLES || m == 0) return hipErrorInvalidValue;
    QuantileSelectArgs a{};
    a.band = band; a.out = out; a.m = m; a.n = n; a.j = j; a.g = g;
    // the fewest lanes per pixel-channel that hold its keys at 32 per lane (64 beyond 64 lanes), keys per lane rounded up
    // to the next instantiation
    const int groups = (n + 3) / 4;
    int ls = 0;
    while (ls < 6 && (groups + (1 << ls) - 1) >> ls > 8) ls++;
    const int per = (groups + (1 << ls) - 1) >> ls;           // <= 16 (n <= 64 lanes x 64 keys)
    const int G = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;
    a.log2_splits = ls;
    const int T = QSEL_THREADS >> ls;
    const dim3 grid((unsigned)((m + T - 1) / T));
    const size_t lds = (size_t)QSEL_THREADS * G * sizeof(uint4);
    switch (G) {
        case 1: quantile_select_kernel<1><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        case 2: quantile_select_kernel<2><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        case 4: quantile_select_kernel<4><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        case 8: quantile_select_kernel<8><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        default: quantile_select_kernel<16><<<grid, QSEL_THREADS, lds, s>>>(a); break;
    }
    return hipGetLastError();
}

hipError_t launch_quantile_store(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0 || c.band_rows <= 0 || a.dh != c.y0 + c.band_rows) return hipErrorInvalidValue;
    if (a.interp == STK_INTER_CUBIC) {
        const dim3 g((a.dw + 63) / 64, (c.band_rows + 3) / 4);
        if (warp_u8c3_applies(a, depth)) return launch_warp_cubic_u8c3<true, FoldStore<3>>(a, c, g, s);
        return launch_warp_cubic<true, FoldStore>(a, c, depth, g, s);
    }
    if (warp_u8c3_applies(a, depth)) {
        // the mean fold's default launch shape (one wave per row of 64 pixels, four frames in flight)
        const dim3 g((a.dw + 63) / 64, (c.band_rows + 3) / 4);
        if (a.is_affine) warp_accumulate_u8c3_kernel<true, 1, 4, true, FoldStore<3>><<<g, 256, 0, s>>>(a, c);
        else warp_accumulate_u8c3_kernel<false, 1, 4, true, FoldStore<3>><<<g, 256, 0, s>>>(a, c);
        return hipGetLastError();
    }
    const dim3 grid((a.dw + 63) / 64, (c.band_rows + 3) / 4);
#define STK_STORE_CASE(T, CN) warp_accumulate_kernel<T, CN, true, FoldStore<CN>><<<grid, 256, 0, s>>>(a, c)
    if (depth == 8 && a.cn == 3) STK_STORE_CASE(uint8_t, 3);
    else if (depth == 8 && a.cn == 1) STK_STORE_CASE(uint8_t, 1);
    else if (depth == 8 && a.cn == 4) STK_STORE_CASE(uint8_t, 4);
    else if (depth == 16 && a.cn == 3) STK_STORE_CASE(uint16_t, 3);
    else if (depth == 16 && a.cn == 1) STK_STORE_CASE(uint16_t, 1);
    else if (depth == 16 && a.cn == 4) STK_STORE_CASE(uint16_t, 4);
    else if (depth == 32 && a.cn == 3) STK_STORE_CASE(float, 3);
    else if (depth == 32 && a.cn == 1) STK_STORE_CASE(float, 1);
    else if (depth == 32 && a.cn == 4) STK_STORE_CASE(float, 4);
    else return hipErrorInvalidValue;
#undef STK_STORE_CASE
    return hipGetLastError();
}

// ---- the quantile with participation (stk_quantile_stack_weighted and the *_quantile_weighted entry points) ---------
// The band holds normalised samples and QUANTILE_ABSENT_BITS (a signalling NaN, which no sample is) for an entry that is
// no sample of the pixel (FoldStoreW, warp_body.h). Keys: an absent entry takes the padding key (all ones), which no
// bisection candidate with a clear bit counts — except the last one below the NaN key, which is why NaN gets the key
// below it and is counted like a sample: it ranks last, as in the plain kernel, and makes the output NaN. N_p is one more
// count round (keys below the padding key); j, g and the bisection threshold j + 1 are per-lane values.
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

__device__ __forceinline__ uint32_t quantile_key_masked(float v) {
    const uint32_t u = __float_as_uint(v);
    if (u == QUANTILE_ABSENT_BITS) return 0xffffffffu;
    if (v != v) return 0xfffffffeu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int G>
__global__ __launch_bounds__(QSEL_THREADS) void quantile_select_masked_kernel(QuantileSelectMaskedArgs a) {
    extern __shared__ uint4 keys4[];                    // [G][256], as in quantile_select_kernel
    constexpr int KPT = 4 * G;
    const int ls = a.log2_splits, S = 1 << ls, Tw = 64 >> ls, T = QSEL_THREADS >> ls;
    const int tid = threadIdx.x;
    {
        const int c = tid & (T - 1), p = tid >> (8 - ls);
        const size_t col = (size_t)blockIdx.x * T + c;
        const int owner = (c / Tw) * 64 + (c % Tw);
        for (int q = p; q < S * G; q += S) {
            uint32_t k[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = q * 4 + e;
                k[e] = (col < a.m && i < a.n) ? quantile_key_masked(a.band[(size_t)i * a.m + col]) : 0xffffffffu;
            }
            keys4[(q % G) * QSEL_THREADS + owner + (q / G) * Tw] = uint4{k[0], k[1], k[2], k[3]};
        }
    }
    __syncthreads();
    const int lane = tid & 63, s = lane / Tw, t = (tid >> 6) * Tw + (lane % Tw);
    const size_t col = (size_t)blockIdx.x * T + t;
    uint32_t key[KPT];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint4 v = keys4[g * QSEL_THREADS + tid];
        key[4 * g] = v.x; key[4 * g + 1] = v.y; key[4 * g + 2] = v.z; key[4 * g + 3] = v.w;
    }
    // N_p: the keys below the padding key; NaN samples: the key just below it
    uint32_t np = 0, nan = 0;
#pragma unroll
    for (int e = 0; e < KPT; e++) { np += key[e] != 0xffffffffu; nan += key[e] == 0xfffffffeu; }
    np = qsel_sum(np, Tw);
    nan = qsel_sum(nan, Tw);
    // j and g of this pixel-channel, in f32, each operation rounded on its own (N_p == 0: unused)
    const float vi = (float)((int)np - 1) * a.q;
    const float jf = __builtin_floorf(vi);
    const float gq = vi - jf;
    const uint32_t need = np ? (uint32_t)(int)jf + 1 : 1;

    uint32_t lo = 0;
    for (int b = 31; b >= 0; b--) {
        const uint32_t cand = lo | ((1u << b) - 1u);
        uint32_t c0 = 0, c1 = 0;
#pragma unroll
        for (int e = 0; e < KPT; e += 2) { c0 += key[e] <= cand; c1 += key[e + 1] <= cand; }
        if (qsel_sum(c0 + c1, Tw) < need) lo |= 1u << b;
    }
    // s_(j+1), used where g != 0 (then j + 1 <= N_p - 1: a present key above or equal exists)
    uint32_t hi;
    {
        uint32_t c = 0, above = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < KPT; e++) {
            c += key[e] <= lo;
            above = min(above, key[e] > lo ? key[e] : 0xffffffffu);
        }
        c = qsel_sum(c, Tw);
        above = qsel_min(above, Tw);
        hi = c >= need + 1 ? lo : above;
    }
    if (s != 0 || col >= a.m) return;
    float r;
    if (np == 0) r = 0.0f;
    else if (nan) r = __builtin_nanf("");
    else {
        const float l = quantile_value(lo);
        if (gq == 0.0f) r = l;
        else {
            const float h = quantile_value(hi), d = h - l;
            r = gq >= 0.5f ? h - d * (1.0f - gq) : l + d * gq;
        }
    }
    a.out[col] = r;
    if (a.counts && col % (size_t)a.cn == 0) a.counts[col / (size_t)a.cn] = (int)np;
}

hipError_t launch_quantile_select_masked(const float* band, size_t m, int n, float q, int cn, float* out, int* counts, hipStream_t s) {
    if (n < 1 || n > QUANTILE_MAX_SAMPLES || m == 0 || cn < 1 || m % (size_t)cn != 0) return hipErrorInvalidValue;
    QuantileSelectMaskedArgs a{};
    a.band = band; a.out = out; a.counts = counts; a.m = m; a.n = n; a.cn = cn; a.q = q;
    // the plain selection's split of a pixel-channel's keys over lanes
    const int groups = (n + 3) / 4;
    int ls = 0;
    while (ls < 6 && (groups + (1 << ls) - 1) >> ls > 8) ls++;
    const int per = (groups + (1 << ls) - 1) >> ls;
    const int G = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;
    a.log2_splits = ls;
    const int T = QSEL_THREADS >> ls;
    const dim3 grid((unsigned)((m + T - 1) / T));
    const size_t lds = (size_t)QSEL_THREADS * G * sizeof(uint4);
    switch (G) {
        case 1: quantile_select_masked_kernel<1><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        case 2: quantile_select_masked_kernel<2><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        case 4: quantile_select_masked_kernel<4><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        case 8: quantile_select_masked_kernel<8><<<grid, QSEL_THREADS, lds, s>>>(a); break;
        default: quantile_select_masked_kernel<16><<<grid, QSEL_THREADS, lds, s>>>(a); break;
    }
    return hipGetLastError();
}

hipError_t launch_quantile_store_weighted(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0 || c.band_rows <= 0 || a.dh != c.y0 + c.band_rows || !c.coef) return hipErrorInvalidValue;
    if (a.interp == STK_INTER_CUBIC) {
        const dim3 g((a.dw + 63) / 64, (c.band_rows + 3) / 4);
        if (warp_u8c3_applies(a, depth)) return launch_warp_cubic_u8c3<true, FoldStoreW<3>>(a, c, g, s);
        return launch_warp_cubic<true, FoldStoreW>(a, c, depth, g, s);
    }
    if (warp_u8c3_applies(a, depth)) {
        const dim3 g((a.dw + 63) / 64, (c.band_rows + 3) / 4);
        if (a.is_affine) warp_accumulate_u8c3_kernel<true, 1, 4, true, FoldStoreW<3>><<<g, 256, 0, s>>>(a, c);
        else warp_accumulate_u8c3_kernel<false, 1, 4, true, FoldStoreW<3>><<<g, 256, 0, s>>>(a, c);
        return hipGetLastError();
    }
    const dim3 grid((a.dw + 63) / 64, (c.band_rows + 3) / 4);
#define STK_STOREW_CASE(T, CN) warp_accumulate_kernel<T, CN, true, FoldStoreW<CN>><<<grid, 256, 0, s>>>(a, c)
    if (depth == 8 && a.cn == 3) STK_STOREW_CASE(uint8_t, 3);
    else if (depth == 8 && a.cn == 1) STK_STOREW_CASE(uint8_t, 1);
    else if (depth == 8 && a.cn == 4) STK_STOREW_CASE(uint8_t, 4);
    else if (depth == 16 && a.cn == 3) STK_STOREW_CASE(uint16_t, 3);
    else if (depth == 16 && a.cn == 1) STK_STOREW_CASE(uint16_t, 1);
    else if (depth == 16 && a.cn == 4) STK_STOREW_CASE(uint16_t, 4);
    else if (depth == 32 && a.cn == 3) STK_STOREW_CASE(float, 3);
    else if (depth == 32 && a.cn == 1) STK_STOREW_CASE(float, 1);
    else if (depth == 32 && a.cn == 4) STK_STOREW_CASE(float, 4);
    else return hipErrorInvalidValue;
#undef STK_STOREW_CASE
    return hipGetLastError();
}

}  // namespace stk

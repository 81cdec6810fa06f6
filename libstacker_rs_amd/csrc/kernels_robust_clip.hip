// kernels_robust_clip.hip — median / MAD sigma clipping (stk_robust_clip_stack and the *_robust_clipped entry points;
// definition in include/stacker.h). Per band of destination rows the combine is the quantile's store launch
// (kernels_quantile.hip, unchanged) and the selection kernel below, which turns the band's samples into the centre c and
// the bounds L, U of every pixel-channel and writes them straight into the clip planes; after the last band ONE last clip
// pass (kernels_clip.hip, unchanged) sums the kept samples in fold order.
// The kernel keeps quantile_select_masked_kernel's layout: order-preserving u32 keys (an absent entry and the padding
// beyond n: all ones; NaN: the key below), staged once through LDS into the owner lanes' 16-byte slots, 4G keys per lane
// in registers (fully unrolled, no scratch), S lanes of one wave per pixel-channel, counts meeting by lane shuffles, no
// barrier after the staging one. The staged keys stay in LDS for the kernel's life: K only shrinks, so the keys of a
// round are the staged ones filtered by [L, U] (a lane reads back only the slots it owns), and the registers can hold the
// deviation keys in between. A round:
//   1. deviation keys in place: e = |value(key) - c| is a non-negative f32 (or NaN: the largest key, 0x7fffffff), so its
//      bits order as an integer with bit 31 clear: 31 bisection rounds for e_(j), one more for e_(j+1);
//   2. sigma and the bounds;
//   3. the slots again from LDS, keys outside [L, U] replaced by the padding key, k recounted, and the 32-round bisection
//      for the median of what is left.
// A pixel-channel is done when k < 3, or when a round rejected nothing (the next round would find the same c, mad and
// bounds); a wave leaves the loop when all its pixel-channels are done.
#include "warp_cubic_body.h"

namespace stk {

constexpr int RSEL_THREADS = 256;
constexpr uint32_t RSEL_PAD = 0xffffffffu, RSEL_NAN = 0xfffffffeu;

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

__device__ __forceinline__ uint32_t rsel_key(float v, int masked) {
    const uint32_t u = __float_as_uint(v);
    if (masked && u == QUANTILE_ABSENT_BITS) return RSEL_PAD;
    if (v != v) return RSEL_NAN;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rsel_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ uint32_t rsel_sum(uint32_t v, int Tw) {
    for (int d = Tw; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t rsel_min(uint32_t v, int Tw) {
    for (int d = Tw; d < 64; d <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// rank and fraction of the median of k keys (include/stacker.h: vi = (float)(k - 1) * 0.5f); k == 0: unused
__device__ __forceinline__ void rsel_rank(uint32_t k, uint32_t& need, float& g) {
    const float vi = (float)((int)k - 1) * 0.5f;
    const float jf = __builtin_floorf(vi);
    g = vi - jf;
    need = k ? (uint32_t)(int)jf + 1 : 1;
}

// lo = the need-th smallest key (from 1), hi = the next one, by MSB-first bisection from bit TOP. A candidate has a clear
// bit, so the padding key (and with TOP = 30 every key with bit 31 set) is never counted. hi is valid where a key >= lo
// other than the first `need` exists, which g != 0 implies.
template <int KPT, int TOP>
__device__ __forceinline__ void rsel_pair(const uint32_t (&key)[KPT], uint32_t need, int Tw, uint32_t& lo, uint32_t& hi) {
    lo = 0;
    for (int b = TOP; b >= 0; b--) {
        const uint32_t cand = lo | ((1u << b) - 1u);
        uint32_t c0 = 0, c1 = 0;
#pragma unroll
        for (int e = 0; e < KPT; e += 2) { c0 += key[e] <= cand; c1 += key[e + 1] <= cand; }
        if (rsel_sum(c0 + c1, Tw) < need) lo |= 1u << b;
    }
    uint32_t c = 0, above = RSEL_PAD;
#pragma unroll
    for (int e = 0; e < KPT; e++) {
        c += key[e] <= lo;
        above = min(above, key[e] > lo ? key[e] : RSEL_PAD);
    }
    c = rsel_sum(c, Tw);
    above = rsel_min(above, Tw);
    hi = c >= need + 1 ? lo : above;
}

__device__ __forceinline__ float rsel_mid(float l, float h, float g) {
    if (g == 0.0f) return l;
    const float d = h - l;
    return g >= 0.5f ? h - d * (1.0f - g) : l + d * g;
}

template <int G>
__global__ __launch_bounds__(RSEL_THREADS) void robust_select_kernel(RobustSelectArgs a) {
    extern __shared__ uint4 keys4[];                    // [G][256]: slot g of lane tid at keys4[g * 256 + tid]
    constexpr int KPT = 4 * G;
    const int ls = a.log2_splits, S = 1 << ls, Tw = 64 >> ls, T = RSEL_THREADS >> ls;
    const int tid = threadIdx.x;
    // stage, as quantile_select_kernel does: thread (phase p, column c) loads frame groups q = p, p + S, ... of column c
    {
        const int c = tid & (T - 1), p = tid >> (8 - ls);
        const size_t col = (size_t)blockIdx.x * T + c;
        const int owner = (c / Tw) * 64 + (c % Tw);
        for (int q = p; q < S * G; q += S) {
            uint32_t k[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = q * 4 + e;
                k[e] = (col < a.m && i < a.n) ? rsel_key(a.band[(size_t)i * a.m + col], a.masked) : RSEL_PAD;
            }
            keys4[(q % G) * RSEL_THREADS + owner + (q / G) * Tw] = uint4{k[0], k[1], k[2], k[3]};
        }
    }
    __syncthreads();
    const int lane = tid & 63, s = lane / Tw, t = (tid >> 6) * Tw + (lane % Tw);
    const size_t col = (size_t)blockIdx.x * T + t;
    uint32_t key[KPT];
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint4 v = keys4[g * RSEL_THREADS + tid];
        key[4 * g] = v.x; key[4 * g + 1] = v.y; key[4 * g + 2] = v.z; key[4 * g + 3] = v.w;
    }
    uint32_t k = 0, nan = 0;
#pragma unroll
    for (int e = 0; e < KPT; e++) { k += key[e] != RSEL_PAD; nan += key[e] == RSEL_NAN; }
    k = rsel_sum(k, Tw);
    nan = rsel_sum(nan, Tw);

    // c = med(all samples); a NaN sample: c = NaN and nothing is clipped (the last pass makes the output NaN); no sample
    // at all (the participation form): c = 0
    uint32_t need, lo, hi;
    float g;
    rsel_rank(k, need, g);
    rsel_pair<KPT, 31>(key, need, Tw, lo, hi);
    float c = rsel_mid(rsel_value(lo), rsel_value(hi), g);
    if (nan) c = __builtin_nanf("");
    if (k == 0) c = 0.0f;
    float L = -__builtin_inff(), U = __builtin_inff();
    bool live = (nan == 0) & (k >= 3);

    for (int round = 0; round < a.iterations; round++) {
        if (__ballot(live) == 0) break;
        // (lanes of a pixel-channel that is done go along: their c, L, U and k stay)
#pragma unroll
        for (int e = 0; e < KPT; e++) {
            const float d = __builtin_fabsf(rsel_value(key[e]) - c);
            key[e] = key[e] == RSEL_PAD ? RSEL_PAD : (d != d ? 0x7fffffffu : __float_as_uint(d));
        }
        rsel_pair<KPT, 30>(key, need, Tw, lo, hi);
        const float mad = rsel_mid(__uint_as_float(lo), __uint_as_float(hi), g);
        const float sigma = __builtin_fmaxf(1.4826f * mad, a.sigma_floor);
        if (live) {
            L = __builtin_fmaxf(L, c - a.kappa_low * sigma);
            U = __builtin_fminf(U, c + a.kappa_high * sigma);
        }
        uint32_t kk = 0;
#pragma unroll
        for (int gi = 0; gi < G; gi++) {
            const uint4 v = keys4[gi * RSEL_THREADS + tid];
            const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float sv = rsel_value(q[e]);
                const bool in = (q[e] != RSEL_PAD) & (L <= sv) & (sv <= U);
                key[4 * gi + e] = in ? q[e] : RSEL_PAD;
                kk += in;
            }
        }
        kk = rsel_sum(kk, Tw);
        uint32_t need2;
        float g2;
        rsel_rank(kk, need2, g2);
        rsel_pair<KPT, 31>(key, need2, Tw, lo, hi);
        if (live) {
            if (kk > 0) c = rsel_mid(rsel_value(lo), rsel_value(hi), g2);
            live = (kk >= 3) & (kk != k);
            k = kk; need = need2; g = g2;
        }
    }
    if (s != 0 || col >= a.m) return;
    a.c[col] = c; a.L[col] = L; a.U[col] = U;
}

hipError_t launch_robust_select(const float* band, size_t m, int n, int masked, const stk_robust_clip_params& p, float* c, float* L,
                                float* U, hipStream_t s) {
    if (n < 1 || n > QUANTILE_MAX_SAMPLES || m == 0) return hipErrorInvalidValue;
    RobustSelectArgs a{};
    a.band = band; a.c = c; a.L = L; a.U = U; a.m = m; a.n = n; a.masked = masked;
    a.iterations = p.iterations; a.kappa_low = p.kappa_low; a.kappa_high = p.kappa_high; a.sigma_floor = p.sigma_floor;
    // the quantile selection's split of a pixel-channel's keys over lanes (launch_quantile_select)
    const int groups = (n + 3) / 4;
    int ls = 0;
    while (ls < 6 && (groups + (1 << ls) - 1) >> ls > 8) ls++;
    const int per = (groups + (1 << ls) - 1) >> ls;           // <= 16 (n <= 64 lanes x 64 keys)
    const int G = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;
    a.log2_splits = ls;
    const int T = RSEL_THREADS >> ls;
    const dim3 grid((unsigned)((m + T - 1) / T));
    const size_t lds = (size_t)RSEL_THREADS * G * sizeof(uint4);
    switch (G) {
        case 1: robust_select_kernel<1><<<grid, RSEL_THREADS, lds, s>>>(a); break;
        case 2: robust_select_kernel<2><<<grid, RSEL_THREADS, lds, s>>>(a); break;
        case 4: robust_select_kernel<4><<<grid, RSEL_THREADS, lds, s>>>(a); break;
        case 8: robust_select_kernel<8><<<grid, RSEL_THREADS, lds, s>>>(a); break;
        default: robust_select_kernel<16><<<grid, RSEL_THREADS, lds, s>>>(a); break;
    }
    return hipGetLastError();
}

}  // namespace stk

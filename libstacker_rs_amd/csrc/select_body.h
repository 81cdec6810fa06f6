// select_body.h — the selection core of the three selection kernels: quantile_select_kernel and
// quantile_select_masked_kernel (kernels_quantile.hip) and robust_select_kernel (kernels_robust_clip.hip). Each of them
// is a short body over the pieces below: __forceinline__ functions, and the bisection as text (SEL_BISECT), so that a
// kernel compiles to the instructions it had when it carried its own copy ("One selection core", has the diff).
// The layout they share: order-preserving u32 keys; a pixel-channel's keys split over S = 1 .. 64 lanes of ONE wave
// (lane = s * Tw + t, Tw = 64 / S pixel-channels per wave), each lane holding 4G keys in registers (G = 1, 2, 4, 8 or 16, a
// template parameter: fully unrolled, no scratch), so the partial counts meet by lane shuffles and no round needs a
// barrier. A workgroup (4 waves, T = 256 / S pixel-channels) stages its keys once through LDS: coalesced frame-row loads
// of T consecutive pixel-channels, 4 frames per 16-byte LDS store into the owner lane's slot, one barrier, then each lane
// reads its G slots (sel_keys4[g * 256 + tid], consecutive lanes on consecutive 16-byte slots: conflict-free
// ds_read_b128).
// Host side: select_plan is the ONE place that turns a sample count into the launch class (S, G), and launch_select the
// one switch over G.
#pragma once
#include "common.h"

namespace stk {

constexpr int SEL_THREADS = 256;
// the padding key (frames beyond n, columns beyond m, and an absent entry of the masked forms), which no bisection
// candidate counts, and the masked forms' NaN key just below it
constexpr uint32_t SEL_PAD = 0xffffffffu, SEL_NAN = 0xfffffffeu;

extern __shared__ uint4 sel_keys4[];                    // [G][256]: slot g of lane tid at sel_keys4[g * 256 + tid]

// ---- keys ---------------------------------------------------------------------------------------------------------
// Negative floats: all bits flipped; others: the sign bit set. Two policies for what is no number, each a functor that
// sel_stage takes:
//   * SelKeyPlain: NaN takes the largest key, which is also the padding key; the kernel tells the two apart by the frame
//     index;
//   * SelKeyMasked: an absent entry (QUANTILE_ABSENT_BITS, a signalling NaN which no sample is) takes the padding key, and
//     NaN the key below it: it is counted like a sample and ranks last. masked = 0 (a band without absence marks): the
//     absent-bits pattern is an ordinary NaN.
__device__ __forceinline__ uint32_t sel_key_ordered(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
struct SelKeyPlain {
    __device__ __forceinline__ uint32_t operator()(float v) const {
        const uint32_t u = __float_as_uint(v);
        if (v != v) return SEL_PAD;
        return sel_key_ordered(u);
    }
};
struct SelKeyMasked {
    int masked;
    __device__ __forceinline__ uint32_t operator()(float v) const {
        const uint32_t u = __float_as_uint(v);
        if (masked && u == QUANTILE_ABSENT_BITS) return SEL_PAD;
        if (v != v) return SEL_NAN;
        return sel_key_ordered(u);
    }
};
__device__ __forceinline__ float sel_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- sum / min over the S lanes of a pixel-channel (lane bits log2(Tw) .. 5) -----------------------------------------
__device__ __forceinline__ uint32_t sel_sum(uint32_t v, int Tw) {
    for (int d = Tw; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}
__device__ __forceinline__ uint32_t sel_min(uint32_t v, int Tw) {
    for (int d = Tw; d < 64; d <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// ---- staging ------------------------------------------------------------------------------------------------------
// after staging, a lane holds split s of pixel-channel col (it writes the result where s == 0 and col < m)
struct SelLane { int s; size_t col; };

// The band (n x m samples, frame-major) into sel_keys4, INCLUDING the barrier after it; returns the lane's place. Thread
// (phase p, column c) loads frame groups q = p, p + S, ... (4 frames each) of column c: the T lanes of a phase read T
// consecutive floats of a frame row. Group q belongs to split s = q / G, slot q % G of the owner lane. keyfn: SelKeyPlain
// or SelKeyMasked.
// (One function for the staging and the lane's place, which share S, Tw, T and the workgroup's first column: as two
// helpers the shared values were computed on both sides of the staging branch and met in vector registers.)
template <int G, class KeyFn>
__device__ __forceinline__ SelLane sel_stage(const float* band, size_t m, int n, int ls, KeyFn keyfn) {
    const int S = 1 << ls, Tw = 64 >> ls, T = SEL_THREADS >> ls;
    const int tid = threadIdx.x;
    {
        const int c = tid & (T - 1), p = tid >> (8 - ls);
        const size_t col = (size_t)blockIdx.x * T + c;
        const int owner = (c / Tw) * 64 + (c % Tw);     // the lane of split 0 of column c
        for (int q = p; q < S * G; q += S) {
            uint32_t k[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int i = q * 4 + e;
                k[e] = (col < m && i < n) ? keyfn(band[(size_t)i * m + col]) : SEL_PAD;
            }
            sel_keys4[(q % G) * SEL_THREADS + owner + (q / G) * Tw] = uint4{k[0], k[1], k[2], k[3]};
        }
    }
    __syncthreads();
    const int lane = tid & 63, t = (tid >> 6) * Tw + (lane % Tw);
    return SelLane{lane / Tw, (size_t)blockIdx.x * T + t};
}

// the lane's G slots into key[4G]
template <int G>
__device__ __forceinline__ void sel_load(uint32_t (&key)[4 * G]) {
#pragma unroll
    for (int g = 0; g < G; g++) {
        const uint4 v = sel_keys4[g * SEL_THREADS + threadIdx.x];
        key[4 * g] = v.x; key[4 * g + 1] = v.y; key[4 * g + 2] = v.z; key[4 * g + 3] = v.w;
    }
}

// ---- order statistics ---------------------------------------------------------------------------------------------
// rank and fraction of the q-quantile of k keys, per lane (include/stacker.h: vi = (float)(k - 1) * q, each operation
// rounded on its own); need = j + 1. k == 0: unused
__device__ __forceinline__ void sel_rank(uint32_t k, float q, uint32_t& need, float& g) {
    const float vi = (float)((int)k - 1) * q;
    const float jf = __builtin_floorf(vi);
    g = vi - jf;
    need = k ? (uint32_t)(int)jf + 1 : 1;
}

// lo = the need-th smallest key (from 1) by MSB-first bisection from bit TOP: bit b of the answer is 0 iff at least `need`
// keys are <= (the bits above b) | (2^b - 1). That candidate has bit b clear, so the padding key (and with TOP = 30 every
// key with bit 31 set) is never counted.
// Text, not a function (the one piece here that is; compare the note at warp_accumulate_kernel): a helper is optimised on
// its own before it is inlined, its count loop already unrolled when the kernel's passes see it, and they then merge the
// two count chains into one — for the quantile kernels, whose bisection stood in the kernel body, more registers at
// G = 4 and 8 ("One selection core"). As text each kernel keeps the loop it had: the quantile kernels expand it
// in their bodies, robust_select_kernel inside sel_pair.
#define SEL_BISECT(lo, key, KPT, TOP, need, Tw)                                                          \
    lo = 0;                                                                                              \
    for (int b = TOP; b >= 0; b--) {                                                                     \
        const uint32_t cand = lo | ((1u << b) - 1u);                                                     \
        uint32_t c0 = 0, c1 = 0;                                                                         \
        _Pragma("unroll")                                                                                \
        for (int e = 0; e < KPT; e += 2) { c0 += key[e] <= cand; c1 += key[e + 1] <= cand; }             \
        if (sel_sum(c0 + c1, Tw) < need) lo |= 1u << b;                                                  \
    }

// The key after lo = the need-th smallest: lo again if need + 1 keys are <= lo, else the smallest key above lo. Valid
// where a key >= lo other than the first `need` exists, which g != 0 implies.
template <int KPT>
__device__ __forceinline__ uint32_t sel_next(const uint32_t (&key)[KPT], uint32_t lo, uint32_t need, int Tw) {
    uint32_t c = 0, above = SEL_PAD;
#pragma unroll
    for (int e = 0; e < KPT; e++) {
        c += key[e] <= lo;
        above = min(above, key[e] > lo ? key[e] : SEL_PAD);
    }
    c = sel_sum(c, Tw);
    above = sel_min(above, Tw);
    return c >= need + 1 ? lo : above;
}
template <int KPT, int TOP>
__device__ __forceinline__ void sel_pair(const uint32_t (&key)[KPT], uint32_t need, int Tw, uint32_t& lo, uint32_t& hi) {
    SEL_BISECT(lo, key, KPT, TOP, need, Tw)
    hi = sel_next<KPT>(key, lo, need, Tw);
}

// the value at fraction g between l = s_(j) and h = s_(j+1)
__device__ __forceinline__ float sel_mid(float l, float h, float g) {
    if (g == 0.0f) return l;
    const float d = h - l;
    return g >= 0.5f ? h - d * (1.0f - g) : l + d * g;
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct SelectPlan { int ls, G; dim3 grid; size_t lds; };

// The launch class of n samples: the fewest lanes per pixel-channel that hold its keys at 32 per lane (64 beyond 64
// lanes), keys per lane rounded up to the next instantiation. (tests/selection_classes.py restates these lines.)
inline SelectPlan select_plan(size_t m, int n) {
    const int groups = (n + 3) / 4;
    int ls = 0;
    while (ls < 6 && (groups + (1 << ls) - 1) >> ls > 8) ls++;
    const int per = (groups + (1 << ls) - 1) >> ls;           // <= 16 (n <= 64 lanes x 64 keys)
    const int G = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : 16;
    const int T = SEL_THREADS >> ls;
    return SelectPlan{ls, G, dim3((unsigned)((m + T - 1) / T)), (size_t)SEL_THREADS * G * sizeof(uint4)};
}

// K1 .. K16: a selection kernel's instantiations for G = 1, 2, 4, 8, 16 (SEL_KERNELS names them)
#define SEL_KERNELS(kernel) kernel<1>, kernel<2>, kernel<4>, kernel<8>, kernel<16>
template <auto K1, auto K2, auto K4, auto K8, auto K16, class Args>
hipError_t launch_select(const SelectPlan& p, const Args& a, hipStream_t s) {
    switch (p.G) {
        case 1: K1<<<p.grid, SEL_THREADS, p.lds, s>>>(a); break;
        case 2: K2<<<p.grid, SEL_THREADS, p.lds, s>>>(a); break;
        case 4: K4<<<p.grid, SEL_THREADS, p.lds, s>>>(a); break;
        case 8: K8<<<p.grid, SEL_THREADS, p.lds, s>>>(a); break;
        default: K16<<<p.grid, SEL_THREADS, p.lds, s>>>(a); break;
    }
    return hipGetLastError();
}

}  // namespace stk

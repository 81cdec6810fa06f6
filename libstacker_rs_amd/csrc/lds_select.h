// lds_select.h — the exact k-th smallest of a set of 16-bit keys held in LDS, by a two-level radix selection: one definition
// for kernels_star_deep.hip, kernels_background.hip (a workgroup of 256 threads per set) and kernels_star_measure.hip (a wave
// per set). Device code only; everything inlines. select16 is four steps, each thread walking its own share of the keys:
//   fill   a 256-bin histogram of the high byte of every key, by integer LDS atomics;
//   pick   the histogram is summed, prefix-summed in registers by wave shuffles and searched for the bin that holds rank k;
//          k becomes the rank inside that bin, and the histogram is zero again;
//   fill   a 256-bin histogram of the low byte of the keys whose high byte is that bin;
//   pick   the low byte, at the rank the first pick left.
// The counts are integers and the sums are taken in a fixed order: nothing depends on the order in which the atomics land.
// The barriers belong to the pick: it opens with the scope's barrier (the histogram is complete) and closes with one (its
// zeroes and the answer are in place before the next fill). A caller zeroes the histogram before the first selection only.
// A scope gives a thread its histogram copy (bins) and pick(k, total): the bin that holds the k-th smallest (k counted from
// 1) of the values counted, k's rank inside that bin, the total; the same in every thread of the scope.
#pragma once
#include "common.h"

namespace stk {

// LDS written by one lane of the wave is read by another: order the accesses for the compiler and the hardware
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// 256 threads, every one calls pick; hist[4][256], one copy per wave so that the waves' atomics do not meet. K0_MEDIAN: k == 0
// on entry asks for the lower median of what was counted (the caller does not know the total yet); without it 1 <= k <= total.
template <bool K0_MEDIAN>
struct WorkgroupSelect {
    static constexpr int HIST_INTS = 4 * 256, PICK_INTS = 2, WSUM_INTS = 4;      // the ints of LDS it needs, in this order
    static constexpr int PICK_AT = HIST_INTS, WSUM_AT = PICK_AT + PICK_INTS, INTS = WSUM_AT + WSUM_INTS;
    int* hist; int* answer; int* wsum;               // hist[4][256], pick[2]: the answer, wsum[4]: the waves' totals
    int t, wave;                                     // threadIdx.x and threadIdx.x >> 6, as the kernel has them
    __device__ __forceinline__ int* bins() const { return &hist[wave * 256]; }
    __device__ __forceinline__ int pick(int& k, int& total) const {
        __syncthreads();                                                  // the histogram is complete
        const int v = hist[t] + hist[256 + t] + hist[512 + t] + hist[768 + t];
        hist[t] = 0; hist[256 + t] = 0; hist[512 + t] = 0; hist[768 + t] = 0;
        int x = v;                                                        // inclusive prefix sum over the wave's 64 bins
        const int lane = t & 63;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if constexpr (K0_MEDIAN) { if (k == 0) k = (total + 1) / 2; }
        for (int i = 0; i < wave; i++) x += wsum[i];
        if (x >= k && x - v < k) { answer[0] = t; answer[1] = k - (x - v); }   // exactly one bin (total >= k >= 1)
        __syncthreads();                                                  // (and the zeroes are in place before the next fill)
        k = answer[1];
        return answer[0];
    }
};

// One wave alone, every lane calls pick, 1 <= k <= total; hist[256], 16-byte aligned, four bins per lane; wave fences and wave barriers only.
struct WaveSelect {
    int* hist; int lane;
    __device__ __forceinline__ int* bins() const { return hist; }
    __device__ __forceinline__ int pick(int& k, int& total) const {
        wave_sync();                                                      // the histogram is complete
        const int4 v = *reinterpret_cast<const int4*>(&hist[4 * lane]);
        *reinterpret_cast<int4*>(&hist[4 * lane]) = make_int4(0, 0, 0, 0);
        const int s = v.x + v.y + v.z + v.w;
        int x = s;                                                        // inclusive prefix sum over the lanes
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
        total = __shfl(x, 63, 64);
        int bin = -1, rank = 0;
        if (x >= k && x - s < k) {                                        // exactly one lane
            int r = k - (x - s);
            if (r <= v.x) { bin = 0; rank = r; }
            else if ((r -= v.x) <= v.y) { bin = 1; rank = r; }
            else if ((r -= v.y) <= v.z) { bin = 2; rank = r; }
            else { bin = 3; rank = r - v.z; }
            bin += 4 * lane;
        }
        const unsigned long long m = __ballot(bin >= 0);
        const int src = m ? __ffsll((long long)m) - 1 : 0;
        k = __shfl(rank, src, 64);
        bin = __shfl(bin, src, 64);
        wave_sync();                                                      // the zeroes are in place before the next fill
        return max(bin, 0);
    }
};

// The key transforms: a median and a MAD are two selections at one rank: of the keys, then of their distances from the median.
struct SelectKey { __device__ __forceinline__ int operator()(int g) const { return g; } };
struct SelectAbsDev { int med; __device__ __forceinline__ int operator()(int g) const { return abs(g - med); } };

// A thread's share of the set, in the thread's own order: the positions i = begin, begin + step, ... below end for which
// has(i) holds; at(i) is the key there. Both are pure and capture by value, and the functions below take scope, share and
// transform by value: behind references the fills' loops do not compile to the hand-written ones.
template <typename Has, typename At> struct SelectShare { int begin, end, step; Has has; At at; };
template <typename Has, typename At>
__device__ __forceinline__ SelectShare<Has, At> select_share(int begin, int end, int step, Has has, At at) { return {begin, end, step, has, at}; }

// The high-byte fill: an atomic per key, or one per RUN of equal bins among the thread's consecutive keys (flat sky).
enum class SelectFill { Direct, Merged };

// The first level: the high-byte fill and its pick. Returns the high byte of the k-th smallest transformed key, k: its rank
// among the keys that share it, total: the size of the set (background's rounds stop here when the set has not shrunk).
template <SelectFill FILL, typename Scope, typename Share, typename Transform>
__device__ __forceinline__ int select_high(const Scope scope, const Share share, const Transform transform, int& k, int& total) {
    int* bins = scope.bins();
    if constexpr (FILL == SelectFill::Merged) {
        int run = 0, bin = 0;
        for (int i = share.begin; i < share.end; i += share.step) {
            if (!share.has(i)) continue;
            const int b = transform(share.at(i)) >> 8;
            if (run && b != bin) { atomicAdd(&bins[bin], run); run = 0; }
            bin = b; run++;
        }
        if (run) atomicAdd(&bins[bin], run);
    } else {
        for (int i = share.begin; i < share.end; i += share.step)
            if (share.has(i)) atomicAdd(&bins[transform(share.at(i)) >> 8], 1);
    }
    return scope.pick(k, total);
}

// The second level: the low-byte fill, restricted to the bin `high`, and its pick. Returns the whole 16-bit value.
template <typename Scope, typename Share, typename Transform>
__device__ __forceinline__ int select_low(const Scope scope, const Share share, const Transform transform, int high, int k) {
    int* bins = scope.bins();
    for (int i = share.begin; i < share.end; i += share.step) {
        if (!share.has(i)) continue;
        const int d = transform(share.at(i));
        if ((d >> 8) == high) atomicAdd(&bins[d & 255], 1);
    }
    int total;
    return (high << 8) | scope.pick(k, total);
}

// The exact k-th smallest (k counted from 1) of transform(key) over the set.
template <SelectFill FILL, typename Scope, typename Share, typename Transform>
__device__ __forceinline__ int select16(const Scope scope, const Share share, const Transform transform, int k) {
    int total;
    const int high = select_high<FILL>(scope, share, transform, k, total);
    return select_low(scope, share, transform, high, k);
}

}  // namespace stk

// kernels_background.hip — the background model (include/stacker.h, stk_background_params): the window
// records of every node of every frame, and the subtraction of the interpolated level planes.
//
// background_cells_kernel. One workgroup of 256 threads per (node, frame): blockIdx.x = node, blockIdx.y = frame of the launch.
// Per colour channel c < min(CN, 3), one after the other:
//   1. the window's rows are read from the interleaved frame, lanes along x, turned into the 16-bit key (the sample, or
//      key_f32 of star_key.h) and kept in LDS as u16: at most 129 x 129 keys = 33 282 bytes at step 128, so that several
//      workgroups fit a CU. Masked pixels are left out: the keys are compacted (a ballot per wave, one integer LDS atomic
//      per wave and 256 pixels for the wave's base). The ORDER of the keys in LDS therefore depends on the order in which
//      the waves arrive; nothing below depends on the order, only on the multiset. A position outside the frame or the
//      window forms NO address: x and y are taken from [a, b] of the window, which lies inside the frame.
//   2. rounds t = 0 .. T over S_t = the keys in [lo_t, hi_t]: the exact median and MAD by two selections of lds_select.h
//      at workgroup scope. A thread's share is every 256th key of the compacted window that lies in [lo_t, hi_t]; the
//      high-byte passes add merged runs (on sky nearly every key shares its high byte). |S_t| is the total that the
//      round's first pick reports; where it equals |S_{t-1}| the rounds stop there, before the low-byte pass, since every
//      later round would repeat the last one.
//   3. kept, and sum and sum2 over S_T as int64 shuffle trees, four wave partials through LDS, added by thread 0.
// Counts and sums are integers: the record does not depend on the order in which the atomics land.
// No global atomics, no floating-point atomics, no scratch.
//
// background_apply_kernel. Element-wise: a workgroup owns a BG_TW x BG_TH tile of one frame (blockIdx.z), a wave BG_ROWS
// 64-pixel row segments of it, whose samples it requests together. The four node offsets of a lane come from the
// local-normalisation chain (k, j, k1, j1); per row a wave vote (all lanes' equal the first lane's, as ClipNormU8C3's
// VotedPlane does) decides whether the node values are read through the first lane's offsets, wave-uniform, or by every
// lane for itself: from a node spacing of 64 on a segment lies in one cell. Both paths run the same sub, fma, sub, fma,
// sub, fma on the same values. Frames and outputs are read and written element by element, pixel bytes only (row padding
// keeps its contents). No LDS, no atomics, no scratch.
#include <type_traits>

#include "common.h"
#include "lds_select.h"
#include "star_key.h"

namespace stk {

namespace {

// A frame pointer comes out of a table, so the compiler cannot tell its address space and would use flat loads and stores;
// frames, planes and outputs are global memory by the entry points' contract, and these casts say so.
#define BG_GLOBAL __attribute__((address_space(1)))

using BgSelect = WorkgroupSelect<true>;             // a round asks for the lower median of a set it has yet to count
// the dynamic LDS block: the selection's ints (histograms, pick, wsum), count and a pad, sum and sum2 of the four waves, the keys
constexpr int BG_COUNT_INTS = 2, BG_SUM_BYTES = (4 + 4) * 8;
constexpr int BG_HIST_BYTES = BgSelect::HIST_INTS * 4, BG_MISC_BYTES = (BgSelect::INTS - BgSelect::HIST_INTS + BG_COUNT_INTS) * 4 + BG_SUM_BYTES;
constexpr int BG_SUM_OFFSET = BG_HIST_BYTES + BG_MISC_BYTES - BG_SUM_BYTES;
constexpr int BG_KEY_OFFSET = BG_HIST_BYTES + BG_MISC_BYTES;
static_assert(BG_SUM_OFFSET % 8 == 0 && BG_KEY_OFFSET % 16 == 0, "the int64 partials and the keys are aligned");

template <typename T>
__device__ __forceinline__ uint32_t bg_key(T v, float scale) {
    if constexpr (sizeof(T) == 4) return key_f32(v, scale);
    else return v;
}

template <typename O>
__device__ __forceinline__ O bg_out(float v) {
    if constexpr (std::is_same<O, float>::value) return v;
    else {
        constexpr float hi = sizeof(O) == 1 ? 255.0f : 65535.0f;
        const float r = __builtin_rintf(v);
        return (O)__builtin_fminf(__builtin_fmaxf(r, 0.0f), hi);       // fmaxf: a NaN gives 0 (stk_calibrate's rule)
    }
}

template <typename T, int CN>
__global__ __launch_bounds__(256) void background_cells_kernel(BgCellsArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    extern __shared__ __align__(16) unsigned char bg_lds[];
    int* hist = reinterpret_cast<int*>(bg_lds);
    int* s_count = hist + BgSelect::INTS;
    long long* s_sum = reinterpret_cast<long long*>(bg_lds + BG_SUM_OFFSET);
    uint16_t* key = reinterpret_cast<uint16_t*>(bg_lds + BG_KEY_OFFSET);

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int node = blockIdx.x, j = node / a.gw, k = node - j * a.gw;
    const int half = a.step >> 1;
    const int ax = max(k * a.step - half, 0), bx = min(k * a.step + half, a.w - 1);
    const int ay = max(j * a.step - half, 0), by = min(j * a.step + half, a.h - 1);
    const int ww = max(bx - ax + 1, 0), wh = max(by - ay + 1, 0), total = ww * wh;      // 0: an empty window
    const BG_GLOBAL uint8_t* src = (const BG_GLOBAL uint8_t*)a.frames[blockIdx.y];
    const BG_GLOBAL uint8_t* mask = (const BG_GLOBAL uint8_t*)a.mask;
    stk_bg_cell* out = a.cells + ((size_t)blockIdx.y * gridDim.x + node) * CC;
    const BgSelect sel{hist, hist + BgSelect::PICK_AT, hist + BgSelect::WSUM_AT, t, wave};
    for (int i = t; i < BgSelect::HIST_INTS; i += 256) hist[i] = 0;

    for (int c = 0; c < CC; c++) {
        if (t == 0) *s_count = 0;
        __syncthreads();                                                  // (and the last channel's keys are no longer read)
        // ---- 1. the window's unmasked keys of channel c into LDS, compacted
        for (int base = 0; base < total; base += 256) {
            const int i = base + t;
            bool in = i < total;
            uint32_t g = 0;
            if (in) {
                const int r = i / ww, x = ax + (i - r * ww), y = ay + r;
                if (mask && mask[(size_t)y * a.w + x]) in = false;
                else g = bg_key<T>(((const BG_GLOBAL T*)(src + (size_t)y * a.stride))[(size_t)x * CN + c], a.f32_scale);
            }
            const unsigned long long m = __ballot(in);
            int wbase = 0;
            if (lane == 0 && m) wbase = atomicAdd(s_count, (int)__popcll(m));
            wbase = __shfl(wbase, 0, 64);
            if (in) key[wbase + (int)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)g;
        }
        __syncthreads();
        const int n = *s_count;
        if (n == 0) {                                                     // (the same in every thread)
            if (t == 0) out[c] = stk_bg_cell{0, 0, 0, 0, 0, 0, {0, 0}, 0, 0};
            continue;
        }

        // ---- 2. the rounds
        int lo = 0, hi = 65535, med = 0, mad = 0, kept = 0;
        for (int round = 0;; round++) {
            const auto window = select_share(t, n, 256, [=](int i) { return key[i] >= lo && key[i] <= hi; }, [=](int i) { return (int)key[i]; });
            int kk = 0, tot;                                              // k = 0: the lower median of a set yet to be counted
            const int hb = select_high<SelectFill::Merged>(sel, window, SelectKey{}, kk, tot);
            if (tot == kept) break;                                       // S_t = S_{t-1}: every later round repeats the last
            kept = tot;
            med = select_low(sel, window, SelectKey{}, hb, kk);
            mad = select16<SelectFill::Merged>(sel, window, SelectAbsDev{med}, (kept + 1) / 2);
            if (round >= a.clip_iters) break;
            const int d = max((int)fminf(ceilf(a.ks * (float)mad), 65536.0f), 1);
            lo = max(lo, med - d);
            hi = min(hi, med + d);
        }

        // ---- 3. the sums over S_T
        long long s1 = 0;
        unsigned long long s2 = 0;
        for (int i = t; i < n; i += 256) {
            const int g = key[i];
            if (g >= lo && g <= hi) { s1 += g; s2 += (unsigned long long)((unsigned)g * (unsigned)g); }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
        if (lane == 0) { s_sum[wave] = s1; s_sum[4 + wave] = (long long)s2; }
        __syncthreads();
        if (t == 0) {
            stk_bg_cell r{n, kept, med, mad, lo, hi, {0, 0}, 0, 0};
            r.sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
            r.sum2 = (unsigned long long)s_sum[4] + (unsigned long long)s_sum[5] + (unsigned long long)s_sum[6] + (unsigned long long)s_sum[7];
            out[c] = r;
        }
    }
}

template <typename T, typename O, int CN>
__global__ __launch_bounds__(256) void background_apply_kernel(BgApplyArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    const int t = threadIdx.x;
    const int x = blockIdx.x * BG_TW + (t & 63);
    const int y0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * BG_TH + (t >> 6) * BG_ROWS));   // a wave: BG_ROWS row segments
    if (y0 >= a.h) return;                                                // the whole wave
    const int rows = min(BG_ROWS, a.h - y0);
    const BgFrame fr = a.frames[blockIdx.z];
    const bool in = x < a.w;

    // the raw samples of all the wave's rows are requested before the first of them is stored, so a thread has that many rows'
    // loads in flight (stores may alias loads for all the compiler knows: one row per iteration would wait out a full memory
    // latency per row, as kernels_calibrate.hip found for its frames)
    float raw[BG_ROWS][CN];
#pragma unroll
    for (int r = 0; r < BG_ROWS; r++) {
        if (in && r < rows) {
            const BG_GLOBAL T* p = (const BG_GLOBAL T*)((const BG_GLOBAL uint8_t*)fr.src + (size_t)(y0 + r) * a.in_stride) + (size_t)x * CN;
#pragma unroll
            for (int c = 0; c < CN; c++) raw[r][c] = (float)p[c];
        }
    }
    const BG_GLOBAL float* P = (const BG_GLOBAL float*)fr.plane;
    const int xc = min(x, a.w - 1);                                       // a lane beyond the row votes with the last pixel's nodes
    const int k = xc >> a.shift, k1 = min(k + 1, a.gw - 1);
    const float u = (float)(xc - (k << a.shift)) * a.inv;
#pragma unroll
    for (int r = 0; r < BG_ROWS; r++) {
        if (r >= rows) break;                                             // (the same in every lane)
        const int y = y0 + r;
        float B[CC];
#pragma unroll
        for (int c = 0; c < CC; c++) B[c] = 0.0f;
        if (P) {                                                          // (the same in every lane)
            const int jn = y >> a.shift, j1 = min(jn + 1, a.gh - 1);
            const float v = (float)(y - (jn << a.shift)) * a.inv;
            const int o00 = (jn * a.gw + k) * CC, o01 = (jn * a.gw + k1) * CC, o10 = (j1 * a.gw + k) * CC, o11 = (j1 * a.gw + k1) * CC;
            const int s00 = __builtin_amdgcn_readfirstlane(o00), s01 = __builtin_amdgcn_readfirstlane(o01);
            const int s10 = __builtin_amdgcn_readfirstlane(o10), s11 = __builtin_amdgcn_readfirstlane(o11);
            const bool uniform = __all((o00 == s00) & (o01 == s01) & (o10 == s10) & (o11 == s11)) != 0;
#pragma unroll
            for (int c = 0; c < CC; c++) {
                float p00, p01, p10, p11;
                if (uniform) { p00 = P[s00 + c]; p01 = P[s01 + c]; p10 = P[s10 + c]; p11 = P[s11 + c]; }
                else { p00 = P[o00 + c]; p01 = P[o01 + c]; p10 = P[o10 + c]; p11 = P[o11 + c]; }
                const float t0 = __builtin_fmaf(u, p01 - p00, p00);
                const float t1 = __builtin_fmaf(u, p11 - p10, p10);
                B[c] = __builtin_fmaf(v, t1 - t0, t0);
            }
        }
        if (in) {
            BG_GLOBAL O* o = (BG_GLOBAL O*)((BG_GLOBAL uint8_t*)fr.dst + (size_t)y * a.out_stride) + (size_t)x * CN;
#pragma unroll
            for (int c = 0; c < CN; c++) {
                float q = raw[r][c];
                if (c < CC) { q = q - B[c < CC ? c : 0]; q = q + a.target[c]; }
                o[c] = bg_out<O>(q);
            }
        }
    }
}

template <typename T>
hipError_t cells_launch_cn(const BgCellsArgs& a, int cn, dim3 grid, size_t lds, hipStream_t s) {
    if (cn == 1) background_cells_kernel<T, 1><<<grid, 256, lds, s>>>(a);
    else if (cn == 3) background_cells_kernel<T, 3><<<grid, 256, lds, s>>>(a);
    else if (cn == 4) background_cells_kernel<T, 4><<<grid, 256, lds, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

template <typename T, typename O>
hipError_t apply_launch_cn(const BgApplyArgs& a, int cn, dim3 grid, hipStream_t s) {
    if (cn == 1) background_apply_kernel<T, O, 1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) background_apply_kernel<T, O, 3><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) background_apply_kernel<T, O, 4><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

// A missing kernel is an error: every (depth, channels) the entry point admits has its instantiation here.
hipError_t launch_background_cells(const BgCellsArgs& a, int n, int depth, int cn, hipStream_t s) {
    if (n <= 0 || n > 65535 || !a.frames || !a.cells || a.w <= 0 || a.h <= 0 || (a.step != 16 && a.step != 32 && a.step != 64 && a.step != 128) ||
        a.gw != (a.w - 1 + a.step - 1) / a.step + 1 || a.gh != (a.h - 1 + a.step - 1) / a.step + 1 || a.clip_iters < 0 || a.clip_iters > 5 ||
        a.stride % (size_t)(depth / 8 ? depth / 8 : 1) || a.stride < (size_t)a.w * cn * (depth / 8))
        return hipErrorInvalidValue;
    const size_t keys = (size_t)(a.step + 1) * (a.step + 1) * sizeof(uint16_t);
    const size_t lds = BG_KEY_OFFSET + ((keys + 15) & ~(size_t)15);
    const dim3 grid((unsigned)(a.gw * a.gh), (unsigned)n);
    if (depth == 8) return cells_launch_cn<uint8_t>(a, cn, grid, lds, s);
    if (depth == 16) return cells_launch_cn<uint16_t>(a, cn, grid, lds, s);
    if (depth == 32) return cells_launch_cn<float>(a, cn, grid, lds, s);
    return hipErrorInvalidValue;
}

hipError_t launch_background_apply(const BgApplyArgs& a, int depth, int out_depth, int cn, hipStream_t s) {
    if (a.n <= 0 || a.n > 65535 || !a.frames || a.w <= 0 || a.h <= 0 || a.shift < 4 || a.shift > 7 ||
        a.gw != ((a.w - 1 + (1 << a.shift) - 1) >> a.shift) + 1 || a.gh != ((a.h - 1 + (1 << a.shift) - 1) >> a.shift) + 1)
        return hipErrorInvalidValue;
    const dim3 grid((a.w + BG_TW - 1) / BG_TW, (a.h + BG_TH - 1) / BG_TH, (unsigned)a.n);
    if (grid.y > 65535) return hipErrorInvalidValue;
    if (depth == 8 && out_depth == 8) return apply_launch_cn<uint8_t, uint8_t>(a, cn, grid, s);
    if (depth == 8 && out_depth == 32) return apply_launch_cn<uint8_t, float>(a, cn, grid, s);
    if (depth == 16 && out_depth == 16) return apply_launch_cn<uint16_t, uint16_t>(a, cn, grid, s);
    if (depth == 16 && out_depth == 32) return apply_launch_cn<uint16_t, float>(a, cn, grid, s);
    if (depth == 32 && out_depth == 32) return apply_launch_cn<float, float>(a, cn, grid, s);
    return hipErrorInvalidValue;
}

}  // namespace stk

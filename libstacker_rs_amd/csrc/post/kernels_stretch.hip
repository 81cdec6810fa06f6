// kernels_stretch.hip — the display stretch of a finished stack (include/stacker.h, "display stretch"): the
// exact per-channel statistics (count, min, max, median, quantiles, MAD) by radix histograms, and the stretch itself: black
// and white point, curve and output conversion in one launch.
//
// The statistics. A key is the sign-flipped bits of a value (negative: every bit flipped; else the sign bit set), -0 counted
// as +0 on the bits, so keys order as the values do; in the MAD's phase the key is bits(fabsf(v - median)), which is its
// own order. Four rounds of 8 bits from the top. A round reads the interleaved image once, every colour channel in that one
// pass, and counts per (channel, slot) the next digit of the keys whose higher bits equal the prefix the slot has found so
// far: per-workgroup LDS histograms filled by integer LDS atomics, non-zero bins flushed by integer global atomics. Counts
// are exact, so no result depends on the order or on the tiling. A slot is one rank (the median, up to four quantiles, the
// MAD); round 0 has no prefix, so one histogram serves every slot, and the smallest and largest key ride on it (integer
// atomicMin / atomicMax). stretch_stat_pick_kernel walks the 256 counts of each (channel, slot), takes the digit that holds
// the rank, and zeroes the counts for the next round. After the last round the prefix is the key. A workgroup is 64
// columns x 4 rows, rows strided by the grid, which is sized to about ST_TARGET_BLOCKS workgroups so that the flush of a
// workgroup's histograms is paid once per many rows.
//
// The stretch. A thread owns runs of 4 consecutive pixels of a row: 4 CN floats in, read as CN 16-byte loads where the
// input's base and row stride are 16-byte aligned, and 4 CN elements out, written as CN 16-byte (f32), 8-byte (u16) or
// dword (u8) stores where the output's base and row stride are aligned to that size; a run of 4 pixels starts at a byte
// offset that is a multiple of either. Rows that are not aligned, and the last w % 4 pixels of a row, go element by element:
// the same arithmetic, the same bits. A thread reads its pixels before it writes them and no other thread touches them, so
// an f32 output may be the input. The parameters are uniform: scalar operands. The table is read from device memory.
// No scratch, no float atomics.
#include "../common.h"

namespace stk {

namespace {

__device__ __forceinline__ uint32_t st_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float st_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

constexpr int ST_LDS_SLOTS = ST_SLOTS - 1;   // the slots of one phase at most: the values' five

__global__ __launch_bounds__(64) void stretch_stat_reset_kernel(StStatArgs a) {
    const int words = (int)st_state_words(a.channels);
    for (int i = threadIdx.x; i < words; i += 64)
        a.state[i] = (i < a.channels * ST_HEAD && !(i & 1)) ? 0xFFFFFFFFu : 0u;   // (the smallest key so far, the largest)
}

// MERGE: the merged form. A thread's samples of one channel are consecutive rows of one column, and on a sky most of them
// share their digit: the thread keeps the digit and the length of its current run in registers and adds the run with one
// LDS atomic when the digit changes (and at the end). It applies where a channel has one histogram (round 0, or one slot);
// with several slots the direct adds run. Counts are integers: both forms give the same words.
template <int CN, bool MERGE>
__global__ __launch_bounds__(256) void stretch_stat_hist_kernel(StStatArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    __shared__ uint32_t bins[CC * ST_LDS_SLOTS * ST_BINS];
    __shared__ uint32_t pre[CC * ST_LDS_SLOTS];
    __shared__ uint32_t ext[CC * 2];
    const bool mad = a.slot0 == ST_MAD, first = a.round == 0;
    const int nt = first ? 1 : a.slots, shift = 32 - ST_DIGIT_BITS * (a.round + 1);
    for (int i = threadIdx.x; i < CC * nt * ST_BINS; i += 256) bins[i] = 0;
    if (threadIdx.x < CC * nt) pre[threadIdx.x] = a.state[st_sel_at(CC, threadIdx.x / nt, a.slot0 + threadIdx.x % nt)];
    if (threadIdx.x < CC * 2) ext[threadIdx.x] = (threadIdx.x & 1) ? 0u : 0xFFFFFFFFu;
    float med[CC];
#pragma unroll
    for (int c = 0; c < CC; c++) med[c] = mad ? st_value(a.state[st_sel_at(CC, c, 0)]) : 0.0f;
    __syncthreads();
    uint32_t kmin[CC], kmax[CC], run_d[CC], run_n[CC];
#pragma unroll
    for (int c = 0; c < CC; c++) { kmin[c] = 0xFFFFFFFFu; kmax[c] = 0u; run_d[c] = 0u; run_n[c] = 0u; }
    const bool merge = MERGE && nt == 1;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x < a.w) {
        for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < a.h; y += gridDim.y * 4) {
            const float* p = a.in + (size_t)y * a.in_stride + (size_t)x * CN;
            float v[CC];
#pragma unroll
            for (int c = 0; c < CC; c++) v[c] = p[c];
            if (a.mask && !(a.mask[(size_t)y * a.mask_stride + x] > 0.0f)) continue;
#pragma unroll
            for (int c = 0; c < CC; c++) {
                uint32_t b = __float_as_uint(v[c]);
                if ((b & 0x7F800000u) == 0x7F800000u) continue;              // not finite
                if (b == 0x80000000u) b = 0u;                                 // -0 counts as +0
                const uint32_t key = mad ? __float_as_uint(__builtin_fabsf(__uint_as_float(b) - med[c])) : st_key(b);
                const uint32_t digit = (key >> shift) & (ST_BINS - 1);
                if (first) { kmin[c] = min(kmin[c], key); kmax[c] = max(kmax[c], key); }
                if (MERGE && merge) {
                    if (!first && ((key >> shift) >> ST_DIGIT_BITS) != pre[c]) continue;
                    if (run_n[c] && digit == run_d[c]) {
                        run_n[c]++;
                    } else {
                        if (run_n[c]) atomicAdd(&bins[c * ST_BINS + run_d[c]], run_n[c]);
                        run_d[c] = digit; run_n[c] = 1u;
                    }
                } else if (first) {
                    atomicAdd(&bins[c * ST_BINS + digit], 1u);
                } else {
                    // (a shift by 32 is not defined, so the upper part is taken in two steps)
                    const uint32_t upper = (key >> shift) >> ST_DIGIT_BITS;
                    for (int t = 0; t < nt; t++)
                        if (upper == pre[c * nt + t]) atomicAdd(&bins[(c * nt + t) * ST_BINS + digit], 1u);
                }
            }
        }
    }
    if (MERGE && merge) {
#pragma unroll
        for (int c = 0; c < CC; c++)
            if (run_n[c]) atomicAdd(&bins[c * ST_BINS + run_d[c]], run_n[c]);
    }
    if (first && !mad) {
#pragma unroll
        for (int c = 0; c < CC; c++)
            if (kmin[c] <= kmax[c]) { atomicMin(&ext[2 * c], kmin[c]); atomicMax(&ext[2 * c + 1], kmax[c]); }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CC * nt * ST_BINS; i += 256) {
        const uint32_t n = bins[i];
        if (n) atomicAdd(&a.state[st_bins_at(CC, i / (nt * ST_BINS), a.slot0 + (i / ST_BINS) % nt) + i % ST_BINS], n);
    }
    if (first && !mad && threadIdx.x < CC && ext[2 * threadIdx.x] <= ext[2 * threadIdx.x + 1]) {
        atomicMin(&a.state[threadIdx.x * ST_HEAD], ext[2 * threadIdx.x]);
        atomicMax(&a.state[threadIdx.x * ST_HEAD + 1], ext[2 * threadIdx.x + 1]);
    }
}

// one lane per (channel, slot): the digit whose bin holds the rank-th smallest (rank counts from 1), then the counts zeroed.
// In round 0 the slots of a channel share one histogram (the phase's first slot's) and take their ranks from the arguments.
__global__ __launch_bounds__(64) void stretch_stat_pick_kernel(StStatArgs a) {
    const int l = threadIdx.x, n = a.channels * a.slots, c = l / a.slots, t = l % a.slots;
    uint32_t digit = ST_BINS - 1, rank = 0;
    if (l < n) {
        const uint32_t* bins = a.state + st_bins_at(a.channels, c, a.slot0 + (a.round == 0 ? 0 : t));
        rank = a.round == 0 ? a.rank[c][a.slot0 + t] : a.state[st_sel_at(a.channels, c, a.slot0 + t) + 1];
        bool found = false;
        for (int b = 0; b < ST_BINS; b++) {
            const uint32_t m = bins[b];
            if (!found) {
                if (rank <= m) { digit = (uint32_t)b; found = true; }
                else rank -= m;
            }
        }
    }
    __syncthreads();
    for (int i = l; i < n * ST_BINS; i += 64)
        a.state[st_bins_at(a.channels, i / (a.slots * ST_BINS), a.slot0 + (i / ST_BINS) % a.slots) + i % ST_BINS] = 0u;
    if (l < n) {
        uint32_t* sel = a.state + st_sel_at(a.channels, c, a.slot0 + t);
        sel[0] = a.round == 0 ? digit : ((sel[0] << ST_DIGIT_BITS) | digit);
        sel[1] = rank;
    }
}

// ---- the stretch --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float st_curve(const StStretchArgs& a, int c, float x) {
    if (a.curve == STK_STRETCH_MTF)
        return __builtin_fminf(__builtin_fmaxf((a.mm1[c] * x) / __builtin_fmaf(a.k[c], x, -a.mid[c]), 0.0f), 1.0f);
    if (a.curve == STK_STRETCH_TABLE) {
        const float t = x * (float)a.knots;
        const int i = min((int)t, a.knots - 1);
        const float fr = t - (float)i, t0 = a.table[i], t1 = a.table[i + 1];
        return __builtin_fmaf(t1 - t0, fr, t0);
    }
    return x;
}

template <typename T> __device__ __forceinline__ T st_convert(float y, float out_scale);
template <> __device__ __forceinline__ float st_convert<float>(float y, float out_scale) { return y * out_scale; }
template <> __device__ __forceinline__ uint8_t st_convert<uint8_t>(float y, float) {
    return (uint8_t)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(y * 255.0f), 0.0f), 255.0f);
}
template <> __device__ __forceinline__ uint16_t st_convert<uint16_t>(float y, float) {
    return (uint16_t)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(y * 65535.0f), 0.0f), 65535.0f);
}

// one pixel: v[CN] -> o[CN]
template <int CN, typename T>
__device__ __forceinline__ void st_pixel(const StStretchArgs& a, const float* v, T* o) {
    constexpr int CC = CN < 3 ? CN : 3;
    float xs[CC], ys[CC];
#pragma unroll
    for (int c = 0; c < CC; c++) xs[c] = __builtin_fminf(__builtin_fmaxf((v[c] - a.black[c]) / a.r[c], 0.0f), 1.0f);
    bool scaled = false;
    if constexpr (CC == 3) {
        if (a.colour) {
            const float L = ((xs[0] + xs[1]) + xs[2]) / 3.0f;
            const float g = st_curve(a, 0, L);
            const float s = L > 0.0f ? g / L : 0.0f;
#pragma unroll
            for (int c = 0; c < CC; c++) ys[c] = __builtin_fminf(xs[c] * s, 1.0f);
            scaled = true;
        }
    }
    if (!scaled) {
#pragma unroll
        for (int c = 0; c < CC; c++) ys[c] = st_curve(a, c, xs[c]);
    }
#pragma unroll
    for (int c = 0; c < CC; c++) o[c] = st_convert<T>(ys[c], a.out_scale);
    if constexpr (CN == 4) o[3] = st_convert<T>(__builtin_fminf(__builtin_fmaxf(v[3], 0.0f), 1.0f), a.out_scale);
}

constexpr int ST_RUN = 4;                    // pixels of one run

template <int CN, typename T>
__global__ __launch_bounds__(256) void stretch_kernel(StStretchArgs a, int vec_in, int vec_out) {
    constexpr int E = ST_RUN * CN;            // elements of a run
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * ST_RUN;
    if (x0 >= a.w) return;
    const int n = min(ST_RUN, a.w - x0);
    const bool whole = n == ST_RUN;
    for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < a.h; y += gridDim.y * 4) {
        const float* p = a.in + (size_t)y * a.in_stride + (size_t)x0 * CN;
        T* q = (T*)a.out + (size_t)y * a.out_stride + (size_t)x0 * CN;
        float v[E];
        if (vec_in && whole) {
#pragma unroll
            for (int k = 0; k < CN; k++) {
                const float4 f = ((const float4*)p)[k];
                v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; i++) v[i] = i < n * CN ? p[i] : 0.0f;
        }
        T o[E];
#pragma unroll
        for (int k = 0; k < ST_RUN; k++) st_pixel<CN, T>(a, v + k * CN, o + k * CN);
        if (vec_out && whole) {
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int k = 0; k < CN; k++) ((float4*)q)[k] = make_float4((float)o[4 * k], (float)o[4 * k + 1], (float)o[4 * k + 2], (float)o[4 * k + 3]);
            } else if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int k = 0; k < CN; k++)
                    ((uint2*)q)[k] = make_uint2((uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 16), (uint32_t)o[4 * k + 2] | ((uint32_t)o[4 * k + 3] << 16));
            } else {
#pragma unroll
                for (int k = 0; k < CN; k++)
                    ((uint32_t*)q)[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) | ((uint32_t)o[4 * k + 3] << 24);
            }
        } else {
#pragma unroll
            for (int i = 0; i < E; i++)
                if (i < n * CN) q[i] = o[i];
        }
    }
}

bool st_stat_ok(const StStatArgs& a) {
    return a.state && a.channels >= 1 && a.channels <= 3 && a.round >= 0 && a.round < ST_ROUNDS && a.slots >= 1 &&
           ((a.slot0 == 0 && a.slots <= ST_LDS_SLOTS) || (a.slot0 == ST_MAD && a.slots == 1));
}

template <int CN, typename T>
hipError_t st_launch(const StStretchArgs& a, hipStream_t s) {
    const size_t ebytes = sizeof(T), out_vec = ebytes == 4 ? 16 : ebytes == 2 ? 8 : 4;
    const int vec_in = (uintptr_t)a.in % 16 == 0 && (a.in_stride * 4) % 16 == 0;
    const int vec_out = (uintptr_t)a.out % out_vec == 0 && (a.out_stride * ebytes) % out_vec == 0;
    const int runs = (a.w + ST_RUN - 1) / ST_RUN, rows = (a.h + 3) / 4;
    const dim3 grid((runs + 63) / 64, (unsigned)(rows < 65535 ? rows : 65535));
    stretch_kernel<CN, T><<<grid, 256, 0, s>>>(a, vec_in, vec_out);
    return hipGetLastError();
}

template <int CN>
hipError_t st_launch_depth(const StStretchArgs& a, hipStream_t s) {
    if (a.depth == STK_DEPTH_U8) return st_launch<CN, uint8_t>(a, s);
    if (a.depth == STK_DEPTH_U16) return st_launch<CN, uint16_t>(a, s);
    if (a.depth == STK_DEPTH_F32) return st_launch<CN, float>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_stretch_stat_reset(const StStatArgs& a, hipStream_t s) {
    if (!a.state || a.channels < 1 || a.channels > 3) return hipErrorInvalidValue;
    stretch_stat_reset_kernel<<<1, 64, 0, s>>>(a);
    return hipGetLastError();
}

// A missing kernel is an error: every channel count the entry points admit has its instantiation here.
hipError_t launch_stretch_stat_hist(const StStatArgs& a, hipStream_t s) {
    if (!st_stat_ok(a) || !a.in || a.w <= 0 || a.h <= 0 || a.in_stride < (size_t)a.w * a.cn || (a.mask && a.mask_stride < (size_t)a.w) ||
        a.channels != (a.cn < 3 ? a.cn : 3))
        return hipErrorInvalidValue;
    const int gx = (a.w + 63) / 64, rows = (a.h + 3) / 4;
    const int gy = std::min(std::min(rows, 65535), std::max(1, ST_TARGET_BLOCKS / gx));
    const dim3 grid(gx, gy);
    if (a.form != ST_FORM_DIRECT && a.form != ST_FORM_MERGED) return hipErrorInvalidValue;
    const bool merged = a.form == ST_FORM_MERGED;
    if (a.cn == 1) { if (merged) stretch_stat_hist_kernel<1, true><<<grid, 256, 0, s>>>(a); else stretch_stat_hist_kernel<1, false><<<grid, 256, 0, s>>>(a); }
    else if (a.cn == 3) { if (merged) stretch_stat_hist_kernel<3, true><<<grid, 256, 0, s>>>(a); else stretch_stat_hist_kernel<3, false><<<grid, 256, 0, s>>>(a); }
    else if (a.cn == 4) { if (merged) stretch_stat_hist_kernel<4, true><<<grid, 256, 0, s>>>(a); else stretch_stat_hist_kernel<4, false><<<grid, 256, 0, s>>>(a); }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_stretch_stat_pick(const StStatArgs& a, hipStream_t s) {
    if (!st_stat_ok(a)) return hipErrorInvalidValue;
    stretch_stat_pick_kernel<<<1, 64, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_stretch(const StStretchArgs& a, hipStream_t s) {
    if (!a.in || !a.out || a.w <= 0 || a.h <= 0 || a.in_stride < (size_t)a.w * a.cn || a.out_stride < (size_t)a.w * a.cn ||
        (a.curve != STK_STRETCH_LINEAR && a.curve != STK_STRETCH_MTF && a.curve != STK_STRETCH_TABLE) ||
        (a.curve == STK_STRETCH_TABLE && (!a.table || a.knots < 2 || a.knots > 65536)))
        return hipErrorInvalidValue;
    if (a.cn == 1) return st_launch_depth<1>(a, s);
    if (a.cn == 3) return st_launch_depth<3>(a, s);
    if (a.cn == 4) return st_launch_depth<4>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace stk

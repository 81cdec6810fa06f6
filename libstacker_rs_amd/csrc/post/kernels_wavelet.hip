// kernels_wavelet.hip — the a trous wavelet layers of a finished stack (include/stacker.h, "wavelet layers"):
// the initialisation, one launch per level (the dilated 5 x 5 separable B3 spline fused with the layer operation, the
// running reconstruction and, on the last level, the output step) and the exact selection of the first layer's median
// magnitude by radix histograms.
//
// Work planes. wavelet_init_kernel de-interleaves the image once into one tightly packed f32 plane per colour channel
// (c_0 = d where it is finite and at most 1e30 in magnitude, else 0), so the level launches never see the channel count:
// blockIdx.z is the plane. Only the output step (and the layers form) writes interleaved pixels again.
//
// A level. One workgroup of 256 threads = WV_TW columns x 4 thread rows of one plane, thread rows strided by the grid. At
// spacing s the rows of the image split into residue classes modulo s, and inside a class the vertical filter is dense: a
// thread owns one column and WV_RUN = 4 outputs of ONE class, y0 + k s, which share their rows of hx: 8 rows of hx (40
// loads) serve 4 outputs where 4 separate outputs take 20 rows (100 loads). Thread row R owns class R % s of the block of
// 4 s image rows R / s, so the four thread rows of a workgroup are four consecutive image rows, four times over. This is
// the direct form: the taps are read from global memory, the five columns reflected once per thread; a wave reads 64
// consecutive floats per tap (256 bytes, coalesced), and every tap but the halo is read again by a neighbouring lane or
// row, so the loads are served by the caches. It runs at every spacing s = 1 .. 128: at s >= 64 the halo of a staged
// tile would outgrow the tile, and at s <= 32 the form that stages a class in LDS (wavelet_level_staged_kernel, below)
// measured 1.04 - 1.36 x slower; it stays as the measured alternative, chosen only by the launch's `form`. hx of a row is the definition's chain, c_{j+1} the same chain over the five hx; nothing is reassociated,
// and hx of a reflected row is hx of the row it reflects to, so sharing it changes no bit.
// The layer operation runs in registers: no layer is stored by the process form. Under LAYERS the same kernel stores w_j
// (and on the last level c_J) interleaved instead.
//
// The selection. Keys are bits(fabsf(w_0)): finite and non-negative, so they order as the values do. Four rounds of 8 bits
// from the top: a round counts, per channel, the next digit of the keys whose higher bits equal the prefix found so far
// (w_0 is recomputed from c_0 in every round: level 0 is cheap and nothing is stored); per-workgroup LDS histograms filled
// by integer LDS atomics, non-zero bins flushed by integer global atomics: counts are exact, so no result depends on the
// order. wavelet_pick_kernel then walks the 256 counts of each channel, takes the digit that holds the rank, and zeroes
// the counts for the next round. After the last round the prefix is the key.
// No scratch; no atomics in the level kernels; no result depends on scheduling or on the tiling.
#include "../common.h"

namespace stk {

namespace {

// BORDER_REFLECT_101 of an index at most n - 1 outside [0, n); anything further out is clamped (the size check of the entry
// points rules that out)
__device__ __forceinline__ int wv_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float wv_chain(float v0, float v1, float v2, float v3, float v4) {
    float a = 0.0625f * v0;
    a = __builtin_fmaf(0.25f, v1, a);
    a = __builtin_fmaf(0.375f, v2, a);
    a = __builtin_fmaf(0.25f, v3, a);
    a = __builtin_fmaf(0.0625f, v4, a);
    return a;
}

constexpr int WV_RUN = 4;                    // outputs of one residue class per thread

// c_{j+1}(x, y0 + k s), k = 0 .. WV_RUN - 1, of the plane `c` (w x h, tightly packed); xs: the five reflected columns
// x - 2s .. x + 2s; centre[k]: c_j(x, y0 + k s). Rows beyond one reflection are clamped: they serve only outputs below the
// image, which the caller does not store.
__device__ __forceinline__ void wv_smooth(const float* c, const int (&xs)[5], int y0, int w, int h, int s, float (&next)[WV_RUN], float (&centre)[WV_RUN]) {
    float hx[WV_RUN + 4];
#pragma unroll
    for (int k = 0; k < WV_RUN + 4; k++) {
        const float* row = c + (size_t)wv_reflect(y0 + (k - 2) * s, h) * w;
        const float v2 = row[xs[2]];
        hx[k] = wv_chain(row[xs[0]], row[xs[1]], v2, row[xs[3]], row[xs[4]]);
        if (k >= 2 && k < WV_RUN + 2) centre[k - 2] = v2;
    }
#pragma unroll
    for (int k = 0; k < WV_RUN; k++) next[k] = wv_chain(hx[k], hx[k + 1], hx[k + 2], hx[k + 3], hx[k + 4]);
}

// the thread rows of a plane at spacing s: s classes in each block of WV_RUN s image rows
__host__ __device__ __forceinline__ int wv_thread_rows(int h, int s) { return (h + WV_RUN * s - 1) / (WV_RUN * s) * s; }

__device__ __forceinline__ float wv_sanitise(float d) {
    return __builtin_fabsf(d) <= 1e30f ? d : 0.0f;                        // (a NaN fails the test, an infinity too)
}

// (the rows of a launch are strided by the grid: an image may have more rows than 4 x 65535)
template <int CN>
__global__ __launch_bounds__(256) void wavelet_init_kernel(WvInitArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= a.w) return;
    for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < a.h; y += gridDim.y * 4) {
        const float* p = a.in + (size_t)y * a.in_stride + (size_t)x * CN;
        float v[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) v[c] = p[c];
        float* c0 = a.c0 + (size_t)y * a.w + x;
#pragma unroll
        for (int c = 0; c < CC; c++) c0[(size_t)c * a.plane] = wv_sanitise(v[c]);
        if constexpr (CN == 4)
            for (int k = 0; k < a.n_alpha; k++) a.alpha[k][(size_t)y * a.alpha_stride[k] + (size_t)x * 4 + 3] = v[3];
    }
}

// what a level does with one output: c = c_j(x, y), next = c_{j+1}(x, y), t the threshold of the plane z
template <bool LAYERS>
__device__ __forceinline__ void wv_emit(const WvLevelArgs& a, int z, int x, int y, float c, float next, float t) {
    const size_t po = (size_t)z * a.plane, at = (size_t)y * a.w + x;
    const float wj = c - next;
    if constexpr (LAYERS) {
        a.wout[(size_t)y * a.wout_stride + (size_t)x * a.cn + z] = wj;
        if (a.last) a.cout[(size_t)y * a.cout_stride + (size_t)x * a.cn + z] = next;
        else a.dst[po + at] = next;
    } else {
        const float m = __builtin_fabsf(wj);
        float wp;
        if (a.mode == STK_WAVELET_HARD) {
            wp = m < t ? wj * a.keep : wj;
        } else {
            const float zz = __builtin_copysignf(__builtin_fmaxf(m - t, 0.0f), wj);
            wp = __builtin_fmaf(a.layer_amount, zz - wj, wj);
        }
        const float g = a.gain * wp;
        const float acc = a.first ? g : a.acc[po + at] + g;
        if (!a.last) {
            a.dst[po + at] = next;
            a.acc[po + at] = acc;
        } else {
            const float res = __builtin_fmaf(a.residual_gain, next, acc);
            float mm = a.amount;
            if (a.mask) mm = a.amount * a.mask[(size_t)y * a.mask_stride + x];
            float o = res;
            if (mm != 1.0f) {
                const float D = wv_sanitise(a.in[(size_t)y * a.in_stride + (size_t)x * a.cn + z]);
                o = __builtin_fmaf(mm, res - D, D);
            }
            a.out[(size_t)y * a.out_stride + (size_t)x * a.cn + z] = o;
        }
    }
}

// the direct form
template <bool LAYERS>
__global__ __launch_bounds__(256) void wavelet_level_kernel(WvLevelArgs a) {
    const int x = blockIdx.x * WV_TW + (threadIdx.x & (WV_TW - 1));
    if (x >= a.w) return;
    const int z = blockIdx.z, s = a.s;
    const float* src = a.src + (size_t)z * a.plane;
    int xs[5];
#pragma unroll
    for (int k = 0; k < 5; k++) xs[k] = wv_reflect(x + (k - 2) * s, a.w);
    const float t = a.t[z];
    const int rows = wv_thread_rows(a.h, s);
    for (int R = blockIdx.y * 4 + threadIdx.x / WV_TW; R < rows; R += gridDim.y * 4) {
        const int y0 = (R / s) * (WV_RUN * s) + R % s;
        float nexts[WV_RUN], cs[WV_RUN];
        wv_smooth(src, xs, y0, a.w, a.h, s, nexts, cs);
#pragma unroll
        for (int n = 0; n < WV_RUN; n++) {
            const int y = y0 + n * s;
            if (y < a.h) wv_emit<LAYERS>(a, z, x, y, cs[n], nexts[n], t);
        }
    }
}

// the staged form, s <= WV_STAGED_MAX_S. A workgroup takes WV_TW columns x WV_TH rows of ONE residue class: unit U (strided
// by the grid) is class U % s of the block U / s of WV_TH s image rows. It stages the WV_TH + 4 rows of the class it needs
// (two on either side) with a halo of 2 s columns in LDS, rows WV_TW + 4 s floats apart, every coordinate reflected (and
// clamped beyond one reflection: such cells serve only outputs outside the image): every input row segment is read from
// global memory once. A thread then owns one column and WV_RUN consecutive rows of the class, as in the direct form, and
// reads its 8 x 5 taps from LDS (consecutive lanes read consecutive floats: no bank conflict). The same chains, the same bits.
template <bool LAYERS>
__global__ __launch_bounds__(256) void wavelet_level_staged_kernel(WvLevelArgs a) {
    extern __shared__ __align__(16) float wv_tile[];
    const int z = blockIdx.z, s = a.s, pitch = WV_TW + 4 * s;
    const int X0 = blockIdx.x * WV_TW, tx = threadIdx.x & (WV_TW - 1), ty = threadIdx.x / WV_TW;
    const float* src = a.src + (size_t)z * a.plane;
    const float t = a.t[z];
    const int units = (a.h + WV_TH * s - 1) / (WV_TH * s) * s;
    for (int U = blockIdx.y; U < units; U += gridDim.y) {
        const int Y0 = (U / s) * (WV_TH * s) + U % s;                     // row 0 of the tile; row i is Y0 + i s
        for (int m = ty; m < WV_TH + 4; m += 4) {
            const float* row = src + (size_t)wv_reflect(Y0 + (m - 2) * s, a.h) * a.w;
            for (int n = tx; n < pitch; n += WV_TW) wv_tile[m * pitch + n] = row[wv_reflect(X0 - 2 * s + n, a.w)];
        }
        __syncthreads();
        float hx[WV_RUN + 4], centre[WV_RUN];
#pragma unroll
        for (int k = 0; k < WV_RUN + 4; k++) {
            const float* row = wv_tile + (WV_RUN * ty + k) * pitch + tx;
            const float v2 = row[2 * s];
            hx[k] = wv_chain(row[0], row[s], v2, row[3 * s], row[4 * s]);
            if (k >= 2 && k < WV_RUN + 2) centre[k - 2] = v2;
        }
        const int x = X0 + tx;
#pragma unroll
        for (int n = 0; n < WV_RUN; n++) {
            const int y = Y0 + (WV_RUN * ty + n) * s;
            if (x < a.w && y < a.h) wv_emit<LAYERS>(a, z, x, y, centre[n], wv_chain(hx[n], hx[n + 1], hx[n + 2], hx[n + 3], hx[n + 4]), t);
        }
        __syncthreads();                                                  // the tile is staged again for the next unit
    }
}

__global__ __launch_bounds__(64) void wavelet_select_reset_kernel(WvSelectArgs a) {
    for (int i = threadIdx.x; i < a.channels * (2 + WV_BINS); i += 64)
        a.state[i] = i < 2 * a.channels ? ((i & 1) ? a.rank : 0u) : 0u;
}

__global__ __launch_bounds__(256) void wavelet_select_hist_kernel(WvSelectArgs a) {
    __shared__ uint32_t bins[WV_BINS];
    const int z = blockIdx.z, shift = 32 - WV_DIGIT_BITS * (a.round + 1);
    const uint32_t prefix = a.state[2 * z];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const int x = blockIdx.x * WV_TW + (threadIdx.x & (WV_TW - 1));
    if (x < a.w) {
        const float* c0 = a.c0 + (size_t)z * a.plane;
        int xs[5];
#pragma unroll
        for (int k = 0; k < 5; k++) xs[k] = wv_reflect(x + (k - 2), a.w);
        const int rows = wv_thread_rows(a.h, 1);
        for (int R = blockIdx.y * 4 + threadIdx.x / WV_TW; R < rows; R += gridDim.y * 4) {
            float nexts[WV_RUN], cs[WV_RUN];
            wv_smooth(c0, xs, R * WV_RUN, a.w, a.h, 1, nexts, cs);
#pragma unroll
            for (int n = 0; n < WV_RUN; n++) {
                if (R * WV_RUN + n >= a.h) continue;
                const uint32_t key = __float_as_uint(__builtin_fabsf(cs[n] - nexts[n]));
                // (round 0 has no prefix: a shift by 32 is not defined, so the upper part is taken in two steps)
                const uint32_t upper = (key >> shift) >> WV_DIGIT_BITS;
                if (a.round == 0 || upper == prefix) atomicAdd(&bins[(key >> shift) & (WV_BINS - 1)], 1u);
            }
        }
    }
    __syncthreads();
    const uint32_t n = bins[threadIdx.x];
    if (n) atomicAdd(&a.state[2 * a.channels + z * WV_BINS + threadIdx.x], n);
}

// one lane per channel: the digit whose bin holds the rank-th smallest (rank counts from 1), then the counts zeroed
__global__ __launch_bounds__(64) void wavelet_select_pick_kernel(WvSelectArgs a) {
    const int z = threadIdx.x;
    if (z >= a.channels) return;
    uint32_t* bins = a.state + 2 * a.channels + z * WV_BINS;
    uint32_t rank = a.state[2 * z + 1], digit = WV_BINS - 1;
    bool found = false;
    for (int b = 0; b < WV_BINS; b++) {
        const uint32_t n = bins[b];
        bins[b] = 0;
        if (!found) {
            if (rank <= n) { digit = (uint32_t)b; found = true; }
            else rank -= n;
        }
    }
    a.state[2 * z] = (a.state[2 * z] << WV_DIGIT_BITS) | digit;
    a.state[2 * z + 1] = rank;
}

bool wv_grid(int w, int h, int s, int channels, dim3& grid) {
    if (w <= 0 || h <= 0 || s < 1 || channels < 1 || channels > 3) return false;
    const int rows = (wv_thread_rows(h, s) + 3) / 4;
    grid = dim3((w + WV_TW - 1) / WV_TW, (unsigned)(rows < 65535 ? rows : 65535), (unsigned)channels);
    return true;
}

}  // namespace

// A missing kernel is an error: every channel count the entry points admit has its instantiation here.
hipError_t launch_wavelet_init(const WvInitArgs& a, int cn, hipStream_t s) {
    if (!a.in || !a.c0 || a.w <= 0 || a.h <= 0 || a.in_stride < (size_t)a.w * cn || a.plane < (size_t)a.w * a.h || a.n_alpha < 0 || a.n_alpha > 9)
        return hipErrorInvalidValue;
    for (int k = 0; k < a.n_alpha; k++)
        if (cn == 4 && (!a.alpha[k] || a.alpha_stride[k] < (size_t)a.w * cn)) return hipErrorInvalidValue;
    const dim3 grid((a.w + 63) / 64, (unsigned)((a.h + 3) / 4 < 65535 ? (a.h + 3) / 4 : 65535));
    if (cn == 1) wavelet_init_kernel<1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) wavelet_init_kernel<3><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) wavelet_init_kernel<4><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_wavelet_level(const WvLevelArgs& a, hipStream_t s) {
    dim3 grid;
    if (!wv_grid(a.w, a.h, a.s, a.channels, grid) || !a.src || a.plane < (size_t)a.w * a.h || a.s < 1 || a.s > 128 || (a.s & (a.s - 1)) ||
        a.w < 2 * a.s + 1 || a.h < 2 * a.s + 1 || (a.cn != 1 && a.cn != 3 && a.cn != 4) || a.channels != (a.cn < 3 ? a.cn : 3))
        return hipErrorInvalidValue;
    const size_t row = (size_t)a.w * a.cn;
    if (a.form != WV_FORM_DIRECT && a.form != WV_FORM_STAGED) return hipErrorInvalidValue;
    const bool staged = a.form == WV_FORM_STAGED && a.s <= WV_STAGED_MAX_S;
    size_t lds = 0;
    if (staged) {
        const int units = (a.h + WV_TH * a.s - 1) / (WV_TH * a.s) * a.s;
        grid.y = (unsigned)(units < 65535 ? units : 65535);
        lds = (size_t)(WV_TH + 4) * (WV_TW + 4 * a.s) * sizeof(float);
    }
    if (a.layers) {
        if (!a.wout || a.wout_stride < row || (a.last ? (!a.cout || a.cout_stride < row) : !a.dst)) return hipErrorInvalidValue;
        if (staged) wavelet_level_staged_kernel<true><<<grid, 256, lds, s>>>(a);
        else wavelet_level_kernel<true><<<grid, 256, 0, s>>>(a);
    } else {
        if ((a.mode != STK_WAVELET_HARD && a.mode != STK_WAVELET_SOFT) || (!a.first && !a.acc)) return hipErrorInvalidValue;
        if (a.last ? (!a.out || a.out_stride < row || !a.in || a.in_stride < row || (a.mask && a.mask_stride < (size_t)a.w)) : (!a.dst || !a.acc))
            return hipErrorInvalidValue;
        if (staged) wavelet_level_staged_kernel<false><<<grid, 256, lds, s>>>(a);
        else wavelet_level_kernel<false><<<grid, 256, 0, s>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch_wavelet_select_reset(const WvSelectArgs& a, hipStream_t s) {
    if (!a.state || a.channels < 1 || a.channels > 3 || a.rank < 1) return hipErrorInvalidValue;
    wavelet_select_reset_kernel<<<1, 64, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_wavelet_select_hist(const WvSelectArgs& a, hipStream_t s) {
    dim3 grid;
    if (!wv_grid(a.w, a.h, 1, a.channels, grid) || !a.c0 || !a.state || a.plane < (size_t)a.w * a.h || a.w < 3 || a.h < 3 || a.round < 0 || a.round >= WV_ROUNDS)
        return hipErrorInvalidValue;
    wavelet_select_hist_kernel<<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_wavelet_select_pick(const WvSelectArgs& a, hipStream_t s) {
    if (!a.state || a.channels < 1 || a.channels > 3) return hipErrorInvalidValue;
    wavelet_select_pick_kernel<<<1, 64, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace stk

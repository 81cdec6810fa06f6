// kernels_noise.hip — per-frame, per-channel noise histograms (include/stacker.h, stk_noise_stat): for every
// frame and channel of a u8 or u16 stack the exact histogram HV of the values and the exact histogram HR of
// min(|r|, BR - 1) over the interior pixels, r = Immerkaer's mask
//     1 -2  1
//    -2  4 -2        = the outer product of [1 -2 1] with itself,
//     1 -2  1
// in integers, on the frame's own grid. Counts are uint32 and exact, so tiling, launch shape and the order of the adds
// cannot change a bit.
//
// The pass is of the family of quality_kernel and star_detect_kernel. One workgroup of 256 threads per tile of 64 x TH
// pixels of one frame (blockIdx.x = tile, blockIdx.y = frame of the launch; the frames are an array of pointers with one
// row stride):
//   1. the tile and a halo of one pixel are copied into LDS as they are, interleaved (as dwords where the frame's base and
//      row stride allow it, element by element otherwise and for the up to three odd bytes at either end of a row). A
//      position outside the frame forms NO address; its LDS bytes are never written and whatever they hold reaches no
//      result: a value is counted only for a pixel inside the frame, a residual only for a pixel whose whole 3 x 3
//      neighbourhood is.
//   2. per channel: a lane walks down TH / 4 rows of one tile column with the row passes [1 -2 1] of the last three rows in
//      registers, and adds one value key and one residual key per pixel to the channel's two LDS histograms (integer LDS
//      atomics; Guideline 12: partial sums first). At depth 8 the LDS histograms hold every bin (256 + 2041 ints); at depth
//      16 they are windows of NOISE_WIN16 bins — the value window around the mean of a sparse pre-sample of the frame
//      (noise_presample_kernel), the residual window at 0 — and a key outside its window goes straight to the frame's
//      global histogram with an integer global atomic. Any window gives the same counts.
//   3. the non-zero bins of the LDS histograms are added to the frame's global histogram with integer global atomics; the
//      host driver zeroes the global histograms on the call's stream inside the call.
// Same-bin contention: a sky frame puts nearly every pixel of a wave into two or three value bins. The adds are plain LDS
// atomics all the same: merging equal keys within the wave first (broadcast the first pending lane's key, count its lanes
// with one ballot, let one lane add the count, up to four keys) was built and measured 1.7 x SLOWER on a sky stack and 1.15 x
// slower on a random one; without it a three-level frame costs 1.28 x a uniform random one.
// No scratch: the per-lane state is a handful of integers, and every loop over rows has a compile-time trip count.
#include "common.h"

namespace stk {

constexpr int NT_W = 64;                     // pixels per tile row
constexpr int NOISE_BR8 = 2041;              // |r| <= 8 * 255
constexpr int NOISE_WIN16 = 4096;            // bins per LDS window at depth 16

struct NoiseArgs {
    const void* const* frames;   // device array: the frames of this launch (blockIdx.y)
    uint32_t* hist;              // [frame][channel][BV + BR], zeroed
    const int32_t* origin;       // [frame][channel]: first bin of the value window (depth 16), or null = 0
    int w, h;
    size_t stride;               // bytes per frame row
    int tiles_x;
};

// T: uint8_t or uint16_t. WV / WR: bins of the value / residual LDS histograms; BV / BR: bins of the global ones.
template <typename T, int CN, int TH, int WV, int WR, int BV, int BR>
__global__ __launch_bounds__(256) void noise_hist_kernel(NoiseArgs a) {
    constexpr int ES = (int)sizeof(T);
    constexpr int PADB = (CN * ES + 3) & ~3;                         // LDS bytes in front of a row: the left neighbour of column 0
    constexpr int PITCH = (PADB + (NT_W + 3) * CN * ES + 4 + 3) & ~3;   // LDS bytes per tile row
    constexpr int ROWS = TH + 2, LANE_ROWS = TH / 4;
    static_assert(ROWS * PITCH + (WV + WR) * 4 <= 64 * 1024, "LDS");
    __shared__ __align__(16) uint8_t tile[ROWS * PITCH];
    __shared__ uint32_t hv[WV];
    __shared__ uint32_t hr[WR];
    const int w = a.w, h = a.h, t = threadIdx.x;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * NT_W, y0 = ty * TH;
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.frames[blockIdx.y]);

    // ---- 1. tile + halo into LDS. Row bytes [bb0, bb1) of the frame row are pixels max(x0 - 1, 0) .. min(x0 + 65, w) - 1;
    //         frame byte b of row r lands at tile[r * PITCH + PADB + b - base].
    const int bb0 = max(x0 - 1, 0) * CN * ES, bb1 = min(x0 + NT_W + 1, w) * CN * ES;
    const int base = bb0 & ~3;
    const int r_lo = y0 == 0 ? 1 : 0, r_hi = min(ROWS, h - y0 + 1);    // tile rows whose image row y0 - 1 + r is inside the frame
    const int nrows = r_hi - r_lo;
    const int d0 = (bb0 + 3) & ~3, d1 = bb1 & ~3;
    if (((reinterpret_cast<uintptr_t>(src) | a.stride) & 3) == 0 && d1 > d0) {
        const int ndw = (d1 - d0) >> 2;
        for (int i = t; i < nrows * ndw; i += 256) {
            const int r = i / ndw, q = i - r * ndw;
            const uint8_t* p = src + (size_t)(y0 - 1 + r_lo + r) * a.stride + d0 + 4 * q;
            *reinterpret_cast<uint32_t*>(&tile[(r_lo + r) * PITCH + PADB + d0 - base + 4 * q]) = *reinterpret_cast<const uint32_t*>(p);
        }
        const int nh = (d0 - bb0) / ES, nt = (bb1 - d1) / ES;          // the odd elements at either end
        for (int i = t; i < nrows * (nh + nt); i += 256) {
            const int r = i / (nh + nt), e = i - r * (nh + nt);
            const int b = e < nh ? bb0 + e * ES : d1 + (e - nh) * ES;
            const uint8_t* p = src + (size_t)(y0 - 1 + r_lo + r) * a.stride + b;
            *reinterpret_cast<T*>(&tile[(r_lo + r) * PITCH + PADB + b - base]) = *reinterpret_cast<const T*>(p);
        }
    } else {
        const int ne = (bb1 - bb0) / ES;
        for (int i = t; i < nrows * ne; i += 256) {
            const int r = i / ne, e = i - r * ne;
            const uint8_t* p = src + (size_t)(y0 - 1 + r_lo + r) * a.stride + bb0 + e * ES;
            *reinterpret_cast<T*>(&tile[(r_lo + r) * PITCH + PADB + bb0 - base + e * ES]) = *reinterpret_cast<const T*>(p);
        }
    }

    // ---- 2. per channel: the two LDS histograms of the tile
    const int cx = t & 63, rr0 = (t >> 6) * LANE_ROWS;
    const int x = x0 + cx;
    const bool x_in = x < w, x_int = x >= 1 && x <= w - 2;
    for (int c = 0; c < CN; c++) {
        for (int i = t; i < WV; i += 256) hv[i] = 0;
        for (int i = t; i < WR; i += 256) hr[i] = 0;
        __syncthreads();                                               // (first channel: the tile is complete too)
        uint32_t* __restrict__ g = a.hist + ((size_t)blockIdx.y * CN + c) * (BV + BR);
        const int org = (WV < BV && a.origin) ? a.origin[(size_t)blockIdx.y * CN + c] : 0;
        // element (x, channel c) of tile row r: byte PADB + (x * CN + c) * ES - base of the row
        const uint8_t* col = &tile[PADB + (x * CN + c) * ES - base];
        int a0 = 0, a1 = 0;                                            // the row passes [1 -2 1] of the two rows above
#pragma unroll
        for (int j = 0; j < LANE_ROWS + 2; j++) {
            const uint8_t* p = col + (rr0 + j) * PITCH;                // tile row rr0 + j = image row y0 - 1 + rr0 + j
            const int pl = *reinterpret_cast<const T*>(p - CN * ES), pc = *reinterpret_cast<const T*>(p), pr = *reinterpret_cast<const T*>(p + CN * ES);
            const int a2 = pl - 2 * pc + pr;
            if (j >= 1 && j <= LANE_ROWS) {                            // the value of image row y0 + rr0 + j - 1
                const int y = y0 + rr0 + j - 1;
                const bool ok = x_in && y < h;
                const int k = pc - org;
                const bool win = WV >= BV || (unsigned)k < (unsigned)WV;
                if (ok && win) atomicAdd(&hv[k], 1u);
                if (WV < BV) { if (ok && !win) atomicAdd(&g[pc], 1u); }
            }
            if (j >= 2) {                                              // the residual of image row y0 + rr0 + j - 2
                const int y = y0 + rr0 + j - 2;
                const bool ok = x_int && y >= 1 && y <= h - 2;
                int rs = a0 - 2 * a1 + a2;
                rs = min(rs < 0 ? -rs : rs, BR - 1);
                const bool win = WR >= BR || rs < WR;
                if (ok && win) atomicAdd(&hr[rs], 1u);
                if (WR < BR) { if (ok && !win) atomicAdd(&g[BV + rs], 1u); }
            }
            a0 = a1; a1 = a2;
        }
        __syncthreads();
        // ---- 3. the non-zero bins to the frame's histogram
        for (int i = t; i < WV; i += 256) { const uint32_t v = hv[i]; if (v) atomicAdd(&g[org + i], v); }
        for (int i = t; i < WR; i += 256) { const uint32_t v = hr[i]; if (v) atomicAdd(&g[BV + i], v); }
        __syncthreads();
    }
}

// depth 16: the first bin of each (frame, channel)'s value window — the mean of 32 x 32 pixels on a sparse grid, less half
// a window, clamped to the histogram. One workgroup per frame.
template <int CN>
__global__ __launch_bounds__(256) void noise_presample_kernel(const void* const* frames, int w, int h, size_t stride, int32_t* origin) {
    __shared__ int sum[4];
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(frames[blockIdx.x]);
    if (threadIdx.x < 4) sum[threadIdx.x] = 0;
    __syncthreads();
    int s[CN] = {};
    for (int k = 0; k < 4; k++) {
        const int i = threadIdx.x * 4 + k;                             // 0 .. 1023
        const int sx = (int)(((long long)(2 * (i & 31) + 1) * w) >> 6), sy = (int)(((long long)(2 * (i >> 5) + 1) * h) >> 6);   // < w, < h
        const uint16_t* p = reinterpret_cast<const uint16_t*>(src + (size_t)sy * stride) + (size_t)sx * CN;
        for (int c = 0; c < CN; c++) s[c] += p[c];
    }
    for (int c = 0; c < CN; c++) {
        int v = s[c];                                                  // 1024 x 65535 < 2^31
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&sum[c], v);
    }
    __syncthreads();
    if (threadIdx.x < CN) origin[(size_t)blockIdx.x * CN + threadIdx.x] = min(max((sum[threadIdx.x] >> 10) - NOISE_WIN16 / 2, 0), 65536 - NOISE_WIN16);
}

size_t noise_hist_bins(int depth) { return depth == 8 ? (size_t)256 + NOISE_BR8 : (size_t)65536 * 2; }

hipError_t launch_noise_hist(const void* const* frames_dev, int n, int cn, int depth, int w, int h, size_t stride_bytes, uint32_t* hist,
                             int32_t* origin, hipStream_t s) {
    if (n <= 0 || n > 65535 || (cn != 1 && cn != 3 && cn != 4) || (depth != 8 && depth != 16) || w < 3 || h < 3) return hipErrorInvalidValue;
    const int th = depth == 8 ? 64 : 32;
    NoiseArgs a{frames_dev, hist, depth == 16 ? origin : nullptr, w, h, stride_bytes, (w + NT_W - 1) / NT_W};
    const dim3 grid((unsigned)(a.tiles_x * ((h + th - 1) / th)), (unsigned)n);
#define STK_NOISE8(CN) noise_hist_kernel<uint8_t, CN, 64, 256, NOISE_BR8, 256, NOISE_BR8><<<grid, 256, 0, s>>>(a)
#define STK_NOISE16(CN)                                                                                     \
    do {                                                                                                    \
        noise_presample_kernel<CN><<<n, 256, 0, s>>>(frames_dev, w, h, stride_bytes, origin);               \
        noise_hist_kernel<uint16_t, CN, 32, NOISE_WIN16, NOISE_WIN16, 65536, 65536><<<grid, 256, 0, s>>>(a); \
    } while (0)
    if (depth == 8) { if (cn == 1) STK_NOISE8(1); else if (cn == 3) STK_NOISE8(3); else STK_NOISE8(4); }
    else { if (cn == 1) STK_NOISE16(1); else if (cn == 3) STK_NOISE16(3); else STK_NOISE16(4); }
#undef STK_NOISE16
#undef STK_NOISE8
    return hipGetLastError();
}

}  // namespace stk

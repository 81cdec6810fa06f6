// kernels_quality.hip — the four sharpness metrics (lib.rs:1030-1166: LAPM, LAPV, TENG(ksize), GLVN) of EVERY frame of an
// 8-bit stack in one pass: what examples/main.rs:35-49 computes file by file before it ranks the stack.
//
// One workgroup per 64 x 64 tile of one frame (blockIdx.x = tile, blockIdx.y = frame of the launch; the frames are an
// array of pointers, any distance apart):
//   1. the tile and a 3-pixel halo are read from the interleaved frame (as dwords where the frame's base and row stride
//      allow it, four pixels per lane like grey_u8x4_kernel), turned into the integer grey (grey.h: the function stk_grey
//      uses) and kept in LDS as bytes — the grey image never exists in memory. Off-image halo pixels are filled by
//      BORDER_REFLECT_101, what LAPM and TENG read there; LAPV (BORDER_REPLICATE, see kernels_sharp.hip) clamps its
//      neighbour index into the image instead and never reads a reflected pixel.
//   2. a lane walks down 16 rows of one tile column. Per row it forms the row passes of the separable filters from the
//      2 RD + 1 grey bytes around it and keeps the last 2 RD + 1 of them in registers (the loop is unrolled: the window is
//      renamed, not moved); the column passes come from that window. Every pixel of the tile is read from LDS
//      (16 + 2 RD) / 16 times per tap instead of once per (row tap x column tap).
//   3. six sums per tile: LAPM x4, LAPV sum and sum of squares, TENG, GLVN sum and sum of squares. All of them exact
//      integers, so tiling, reduction order and launch shape cannot change the result. A lane's 16 pixels fit 32 bits
//      for all but TENG (LAPV: 16 x 2040^2 = 6.7e7); TENG is 64-bit from the first pixel: |gx|, |gy| <= 64 x 10 x 255 =
//      163 200 at ksize 7 fit 32 bits, so gx^2 + acc is ONE 32 x 32 -> 64 multiply-add (v_mad_i64_i32), never a 64-bit
//      multiply. Bound of the per-frame sums: gx^2 + gy^2 <= 5.33e10 per pixel, 4.4e17 at 3840 x 2160, and inside int64
//      (9.2e18) up to QUALITY_MAX_PIXELS = 2^27 pixels per frame, which the host driver enforces.
//   quality_reduce_kernel then adds a frame's tile partials into its record of six int64: no atomics, one record per frame.
#include "common.h"
#include "grey.h"

namespace stk {

constexpr int QT_W = 64, QT_H = 64;       // output pixels per tile
constexpr int QT_HALO = 3;                // TENG ksize 7
constexpr int QT_LEFT = 4;                // LDS column of the tile's first pixel: the interior is stored as aligned dwords
constexpr int QT_STRIDE = 72;             // LDS bytes per tile row (QT_LEFT + QT_W + QT_HALO = 71, rounded to a dword)
constexpr int QT_ROWS = QT_H + 2 * QT_HALO;
constexpr int QT_LANE_ROWS = QT_H / 4;    // rows per lane: 256 lanes = 64 columns x 4 row groups

__device__ __forceinline__ int quality_reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

template <int CN>
__device__ __forceinline__ uint8_t quality_grey_px(const uint8_t* p) {
    if constexpr (CN == 1) return p[0];
    else return grey_u8(p[0], p[1], p[2]);
}

// four consecutive pixels starting at a dword-aligned address -> four greys in one dword
template <int CN>
__device__ __forceinline__ uint32_t quality_grey_x4(const uint32_t* p) {
    if constexpr (CN == 1) return p[0];
    else if constexpr (CN == 3) {
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];   // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
        const uint32_t g0 = grey_u8(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
        const uint32_t g1 = grey_u8(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
        const uint32_t g2 = grey_u8((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
        const uint32_t g3 = grey_u8((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
        return g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    } else {
        uint32_t g = 0;
        for (int k = 0; k < 4; k++) { const uint32_t d = p[k]; g |= (uint32_t)grey_u8(d & 255u, (d >> 8) & 255u, (d >> 16) & 255u) << (8 * k); }
        return g;
    }
}

// getDerivKernels' integer taps, as launch_sharpness (kernels_sharp.hip) hands them to the per-frame kernel:
// ksize 1: smooth {1}, derivative {-1 0 1}; 3: {1 2 1}, {-1 0 1}; 5: {1 4 6 4 1}, {-1 -2 0 2 1}; 7: {1 6 15 20 15 6 1}, {-1 -4 -5 0 5 4 1}
template <int KS> struct QualityTaps;
template <> struct QualityTaps<1> { static constexpr int RS = 0, RD = 1; static constexpr int smooth[1] = {1}; static constexpr int deriv[3] = {-1, 0, 1}; };
template <> struct QualityTaps<3> { static constexpr int RS = 1, RD = 1; static constexpr int smooth[3] = {1, 2, 1}; static constexpr int deriv[3] = {-1, 0, 1}; };
template <> struct QualityTaps<5> { static constexpr int RS = 2, RD = 2; static constexpr int smooth[5] = {1, 4, 6, 4, 1}; static constexpr int deriv[5] = {-1, -2, 0, 2, 1}; };
template <> struct QualityTaps<7> { static constexpr int RS = 3, RD = 3; static constexpr int smooth[7] = {1, 6, 15, 20, 15, 6, 1}; static constexpr int deriv[7] = {-1, -4, -5, 0, 5, 4, 1}; };

struct QualityArgs {
    const void* const* frames;   // device array: the frames of this launch (blockIdx.y)
    int w, h;
    size_t stride;               // bytes per frame row
    int tiles_x, tiles;          // tiles per row of tiles, tiles per frame
    long long* partials;         // [frame][tile][6]
};

template <int CN, int KS>
__global__ __launch_bounds__(256) void quality_kernel(QualityArgs a) {
    using K = QualityTaps<KS>;
    constexpr int RD = K::RD, RS = K::RS, NW = 2 * RD + 1;
    static_assert(RD <= QT_HALO && RD >= 1, "halo");
    __shared__ __align__(16) uint8_t tile[QT_ROWS * QT_STRIDE];
    __shared__ long long red[4][6];
    const int w = a.w, h = a.h;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * QT_W, y0 = ty * QT_H;
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.frames[blockIdx.y]);

    // ---- 1. grey tile + halo into LDS (every address read lies inside the frame: both indices are reflected into it)
    const bool dwords = x0 + QT_W <= w && ((reinterpret_cast<uintptr_t>(src) | a.stride) & 3) == 0;   // x0 * CN is a multiple of 4
    if (dwords) {
        for (int i = threadIdx.x; i < QT_ROWS * (QT_W / 4); i += 256) {
            const int r = i / (QT_W / 4), q = i - r * (QT_W / 4);
            const int yy = quality_reflect101(y0 - QT_HALO + r, h);
            const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (size_t)yy * a.stride + (size_t)(x0 + 4 * q) * CN);
            *reinterpret_cast<uint32_t*>(&tile[r * QT_STRIDE + QT_LEFT + 4 * q]) = quality_grey_x4<CN>(p);
        }
        for (int i = threadIdx.x; i < QT_ROWS * 2 * QT_HALO; i += 256) {
            const int r = i / (2 * QT_HALO), c = i - r * (2 * QT_HALO);
            const int lx = c < QT_HALO ? c - QT_HALO : QT_W + c - QT_HALO;
            const int yy = quality_reflect101(y0 - QT_HALO + r, h), xx = quality_reflect101(x0 + lx, w);
            tile[r * QT_STRIDE + QT_LEFT + lx] = quality_grey_px<CN>(src + (size_t)yy * a.stride + (size_t)xx * CN);
        }
    } else {
        constexpr int COLS = QT_W + 2 * QT_HALO;
        for (int i = threadIdx.x; i < QT_ROWS * COLS; i += 256) {
            const int r = i / COLS, lx = i - r * COLS - QT_HALO;
            const int yy = quality_reflect101(y0 - QT_HALO + r, h), xx = quality_reflect101(x0 + lx, w);
            tile[r * QT_STRIDE + QT_LEFT + lx] = quality_grey_px<CN>(src + (size_t)yy * a.stride + (size_t)xx * CN);
        }
    }
    __syncthreads();

    // ---- 2. a lane walks down QT_LANE_ROWS rows of column c
    const int c = threadIdx.x & (QT_W - 1), r0 = (threadIdx.x >> 6) * QT_LANE_ROWS;
    const int x = x0 + c;
    const bool left_in = x > 0, right_in = x < w - 1;                 // LAPV: x -+ 1 exists (else BORDER_REPLICATE: the pixel itself)
    int wd[NW] = {}, ws[NW] = {};                                      // TENG row passes: derivative / smoothing along x
    int wm[NW] = {}, wg[NW] = {};                                      // LAPM row passes: [-1 2 -1] and [1 2 1] along x
    int wc[NW] = {}, wp[NW] = {};                                      // LAPV: p(x-1) + p(x+1) under REPLICATE; the pixel
    unsigned lapm = 0, lapv_q = 0, gl_s = 0, gl_q = 0;
    int lapv_s = 0;
    long long teng = 0;
#pragma unroll
    for (int j = 0; j < QT_LANE_ROWS + 2 * RD; j++) {
        const uint8_t* t = &tile[(QT_HALO + r0 - RD + j) * QT_STRIDE + QT_LEFT + c];
        int p[NW];
#pragma unroll
        for (int i = 0; i < NW; i++) p[i] = t[i - RD];
#pragma unroll
        for (int i = 0; i + 1 < NW; i++) { wd[i] = wd[i + 1]; ws[i] = ws[i + 1]; wm[i] = wm[i + 1]; wg[i] = wg[i + 1]; wc[i] = wc[i + 1]; wp[i] = wp[i + 1]; }
        int d = 0, s = 0;
#pragma unroll
        for (int i = 0; i < NW; i++) d += K::deriv[i] * p[i];
#pragma unroll
        for (int i = 0; i <= 2 * RS; i++) s += K::smooth[i] * p[RD - RS + i];
        const int pl = p[RD - 1], pc = p[RD], pr = p[RD + 1];
        wd[NW - 1] = d; ws[NW - 1] = s;
        wm[NW - 1] = 2 * pc - pl - pr; wg[NW - 1] = pl + 2 * pc + pr;
        wc[NW - 1] = (left_in ? pl : pc) + (right_in ? pr : pc); wp[NW - 1] = pc;
        if (j < 2 * RD) continue;
        const int y = y0 + r0 + j - 2 * RD;                            // the window holds rows y - RD .. y + RD
        if (x >= w || y >= h) continue;
        int gx = 0, gy = 0;
#pragma unroll
        for (int i = 0; i <= 2 * RS; i++) gx += K::smooth[i] * wd[RD - RS + i];
#pragma unroll
        for (int i = 0; i < NW; i++) gy += K::deriv[i] * ws[i];
        teng += (long long)gx * gx;
        teng += (long long)gy * gy;
        const int lx = wm[RD - 1] + 2 * wm[RD] + wm[RD + 1];           // column [1 2 1] of the [-1 2 -1] rows (x4: the host divides)
        const int ly = 2 * wg[RD] - wg[RD - 1] - wg[RD + 1];
        lapm += (unsigned)((lx < 0 ? -lx : lx) + (ly < 0 ? -ly : ly));
        const int v = 2 * (y > 0 ? wc[RD - 1] : wc[RD]) + 2 * (y < h - 1 ? wc[RD + 1] : wc[RD]) - 8 * wp[RD];
        lapv_s += v; lapv_q += (unsigned)(v * v);
        gl_s += (unsigned)wp[RD]; gl_q += (unsigned)(wp[RD] * wp[RD]);
    }

    // ---- 3. six exact sums per tile: wavefront, then workgroup
    long long v[6] = {(long long)lapm, (long long)lapv_s, (long long)lapv_q, teng, (long long)gl_s, (long long)gl_q};
#pragma unroll
    for (int k = 0; k < 6; k++)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; k++) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 6)
        a.partials[((size_t)blockIdx.y * a.tiles + blockIdx.x) * 6 + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one workgroup per frame: its tile partials -> its record of six sums
__global__ __launch_bounds__(256) void quality_reduce_kernel(const long long* __restrict__ partials, int tiles, long long* __restrict__ records) {
    __shared__ long long red[4][6];
    const long long* p = partials + (size_t)blockIdx.x * tiles * 6;
    long long v[6] = {};
    for (int t = threadIdx.x; t < tiles; t += 256)
        for (int k = 0; k < 6; k++) v[k] += p[(size_t)t * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; k++)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; k++) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 6)
        records[(size_t)blockIdx.x * 6 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

int quality_tiles(int w, int h) { return ((w + QT_W - 1) / QT_W) * ((h + QT_H - 1) / QT_H); }

hipError_t launch_quality(const void* const* frames_dev, int n, int cn, int w, int h, size_t stride_bytes, int ksize,
                          long long* partials, long long* records, hipStream_t s) {
    QualityArgs a{frames_dev, w, h, stride_bytes, (w + QT_W - 1) / QT_W, quality_tiles(w, h), partials};
    if (n <= 0 || n > 65535 || (cn != 1 && cn != 3 && cn != 4) || (ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.tiles, (unsigned)n);
#define STK_QUALITY(CN, KS) quality_kernel<CN, KS><<<grid, 256, 0, s>>>(a)
#define STK_QUALITY_K(CN) \
    switch (ksize) { case 1: STK_QUALITY(CN, 1); break; case 3: STK_QUALITY(CN, 3); break; case 5: STK_QUALITY(CN, 5); break; default: STK_QUALITY(CN, 7); break; }
    if (cn == 1) { STK_QUALITY_K(1) } else if (cn == 3) { STK_QUALITY_K(3) } else { STK_QUALITY_K(4) }
#undef STK_QUALITY_K
#undef STK_QUALITY
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    quality_reduce_kernel<<<n, 256, 0, s>>>(partials, a.tiles, records);
    return hipGetLastError();
}

}  // namespace stk

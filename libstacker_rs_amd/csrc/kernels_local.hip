// kernels_local.hip — per-pixel weights (include/stacker.h, stk_local_params): the local quality map of
// every frame of an 8-bit stack, and the launch of the fold whose weight varies per pixel (FoldLocal<CN>, warp_body.h).
//
// The map pass is modelled on quality_kernel (kernels_quality.hip). One workgroup per 64 x 64 tile of one frame
// (blockIdx.x = tile, blockIdx.y = frame of the launch; frames and map planes are arrays of pointers):
//   1. the tile and a halo of radius + 1 are read from the interleaved frame (as dwords where the frame's base and row
//      stride allow it and the tile is whole, byte by byte otherwise), turned into the integer grey (grey.h) and kept in
//      LDS as bytes. Both indices are reflected (BORDER_REFLECT_101, iterated) BEFORE an address is formed: LDS position
//      p holds g(r101(p)), for halo pixels and for the columns and rows of a partial tile alike, so a frame smaller than
//      the halo forms no address outside itself.
//   2. mlT = the thresholded modified Laplacian of the tile plus a halo of radius, from the LDS greys, as u16 (<= 1020).
//      The reflected extension is mirror-symmetric about every turning point and ml reads x - 1 and x + 1 alike, so ml of
//      the extension at p IS ml(r101(p)): the box sum below adds the terms of the definition.
//   3. a separable box sum with running sums: along the rows (a lane owns 16 columns of one row; a row's sum is
//      <= 31 x 1020 = 31 620, u16), then down the columns (a lane owns 16 rows of one column, as that kernel's lanes walk):
//      per output 2 LDS reads and 2 adds per direction instead of 2 radius + 1.
//   4. the f32 rows are written 256 contiguous bytes per wave. Every value is an integer below 2^24: tiling, summation
//      order and launch shape cannot change a bit.
// LDS rows are padded to an odd number of dwords where lanes of one wave walk different rows.
#include "grey.h"
#include "warp_cubic_body.h"

namespace stk {

constexpr int LT = 64;                        // output pixels per tile side
constexpr int LT_RMAX = 15;                   // largest radius
constexpr int LT_LEFT = LT_RMAX + 1;          // LDS column of the tile's first pixel: the interior is stored as aligned dwords
constexpr int LT_GS = LT + 2 * (LT_RMAX + 1); // grey: bytes per LDS row = rows = 96
constexpr int LT_MW = LT + 2 * LT_RMAX;       // mlT: columns = rows at the largest radius = 94
constexpr int LT_MS = 98;                     // mlT: u16 per LDS row (49 dwords: lanes of the row pass sit in different rows)
constexpr int LT_HS = 66;                     // row sums: u16 per LDS row (33 dwords)

__device__ __forceinline__ int local_reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

template <int CN>
__device__ __forceinline__ uint8_t local_grey_px(const uint8_t* p) {
    if constexpr (CN == 1) return p[0];
    else return grey_u8(p[0], p[1], p[2]);
}

// four consecutive pixels starting at a dword-aligned address -> four greys in one dword
template <int CN>
__device__ __forceinline__ uint32_t local_grey_x4(const uint32_t* p) {
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

struct LocalMapArgs {
    const void* const* frames;   // device array: the frames of this launch (blockIdx.y)
    float* const* maps;          // device array: their map planes, w x h f32, tightly packed
    int w, h;
    size_t stride;               // bytes per frame row
    int tiles_x;                 // tiles per row of tiles
    int radius, threshold;
};

template <int CN>
__global__ __launch_bounds__(256) void local_map_kernel(LocalMapArgs a) {
    __shared__ __align__(16) uint8_t grey[LT_GS * LT_GS];
    __shared__ __align__(16) uint16_t ml[LT_MW * LT_MS];
    __shared__ __align__(16) uint16_t hs[LT_MW * LT_HS];
    const int w = a.w, h = a.h, R = a.radius;
    const int halo = R + 1, gn = LT + 2 * halo, mn = LT + 2 * R;      // grey rows (= columns) and mlT rows (= columns) in use
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * LT, y0 = ty * LT;
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.frames[blockIdx.y]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // ---- 1. grey tile + halo into LDS: grey row r <-> image row y0 - halo + r, grey column LT_LEFT + lx <-> image column
    //         x0 + lx, lx in [-halo, LT + halo). Every address read lies inside the frame: both indices are reflected into it.
    const bool dwords = x0 + LT <= w && ((reinterpret_cast<uintptr_t>(src) | a.stride) & 3) == 0;   // x0 * CN is a multiple of 4
    if (dwords) {
        // 16 lanes per row, a row group of 16 rows per step; unrolled, so that the loads of all steps are in flight together
        const int q = threadIdx.x & 15;
#pragma unroll
        for (int k = 0; k < LT_GS / 16; k++) {
            const int r = (threadIdx.x >> 4) + 16 * k;
            if (r < gn) {
                const int yy = local_reflect101(y0 - halo + r, h);
                const uint32_t* p = reinterpret_cast<const uint32_t*>(src + (size_t)yy * a.stride + (size_t)(x0 + 4 * q) * CN);
                *reinterpret_cast<uint32_t*>(&grey[r * LT_GS + LT_LEFT + 4 * q]) = local_grey_x4<CN>(p);
            }
        }
        // the halo columns, all rows, spread over the workgroup
        const int h2 = 2 * halo;
        for (int i = threadIdx.x; i < gn * h2; i += 256) {
            const int r = i / h2, c = i - r * h2;
            const int lx = c < halo ? c - halo : LT + c - halo;
            const int yy = local_reflect101(y0 - halo + r, h), xx = local_reflect101(x0 + lx, w);
            grey[r * LT_GS + LT_LEFT + lx] = local_grey_px<CN>(src + (size_t)yy * a.stride + (size_t)xx * CN);
        }
    } else {
        // (r, c) walks the gn x gn region in steps of 256 positions: gn >= 66, so a step crosses at most four rows
        int r = 0, c = threadIdx.x;
        while (c >= gn) { c -= gn; r++; }
        while (r < gn) {
            const int lx = c - halo;
            const int yy = local_reflect101(y0 - halo + r, h), xx = local_reflect101(x0 + lx, w);
            grey[r * LT_GS + LT_LEFT + lx] = local_grey_px<CN>(src + (size_t)yy * a.stride + (size_t)xx * CN);
            c += 256;
            while (c >= gn) { c -= gn; r++; }
        }
    }
    __syncthreads();

    // ---- 2. mlT: row mr <-> grey row mr + 1, column mc <-> grey column LT_LEFT - R + mc
    {
        int mr = 0, mc = threadIdx.x;                                   // the same walk over the mn x mn region
        while (mc >= mn) { mc -= mn; mr++; }
        while (mr < mn) {
            const uint8_t* g = &grey[(mr + 1) * LT_GS + LT_LEFT - R + mc];
            const int c2 = 2 * (int)g[0];
            const int lx = c2 - (int)g[-1] - (int)g[1], ly = c2 - (int)g[-LT_GS] - (int)g[LT_GS];
            const int v = (lx < 0 ? -lx : lx) + (ly < 0 ? -ly : ly);
            ml[mr * LT_MS + mc] = (uint16_t)(v >= a.threshold ? v : 0);
            mc += 256;
            while (mc >= mn) { mc -= mn; mr++; }
        }
    }
    __syncthreads();

    // ---- 3a. row sums: hs[r][c] = sum of ml[r][c .. c + 2 R], c < LT; a thread owns 16 columns of one row
    for (int t = threadIdx.x; t < mn * 4; t += 256) {
        const int r = t >> 2, c0 = (t & 3) * 16;
        const uint16_t* m = &ml[r * LT_MS + c0];
        int acc = 0;
        for (int k = 0; k <= 2 * R; k++) acc += m[k];
        uint16_t* o = &hs[r * LT_HS + c0];
        o[0] = (uint16_t)acc;
#pragma unroll
        for (int i = 1; i < 16; i++) {
            acc += (int)m[i + 2 * R] - (int)m[i - 1];
            o[i] = (uint16_t)acc;
        }
    }
    __syncthreads();

    // ---- 3b / 4. column sums: Q[y0 + j][x0 + c] = sum of hs[j .. j + 2 R][c]; a lane walks down 16 rows of column c
    const int x = x0 + lane, j0 = wave * 16;
    if (x >= w || y0 + j0 >= h) return;
    float* __restrict__ out = a.maps[blockIdx.y];
    const uint16_t* q = &hs[j0 * LT_HS + lane];
    int acc = 0;
    for (int k = 0; k <= 2 * R; k++) acc += q[k * LT_HS];
    out[(size_t)(y0 + j0) * w + x] = (float)acc;
#pragma unroll
    for (int i = 1; i < 16; i++) {
        acc += (int)q[(i + 2 * R) * LT_HS] - (int)q[(i - 1) * LT_HS];
        if (y0 + j0 + i < h) out[(size_t)(y0 + j0 + i) * w + x] = (float)acc;
    }
}

int local_map_tiles(int w, int h) { return ((w + LT - 1) / LT) * ((h + LT - 1) / LT); }

hipError_t launch_local_maps(const void* const* frames_dev, float* const* maps_dev, int n, int cn, int w, int h, size_t stride_bytes,
                             int radius, int threshold, hipStream_t s) {
    if (n <= 0 || n > 65535 || (cn != 1 && cn != 3 && cn != 4) || radius < 1 || radius > LT_RMAX) return hipErrorInvalidValue;
    const LocalMapArgs a{frames_dev, maps_dev, w, h, stride_bytes, (w + LT - 1) / LT, radius, threshold};
    const dim3 grid((unsigned)local_map_tiles(w, h), (unsigned)n);
    if (cn == 1) local_map_kernel<1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) local_map_kernel<3><<<grid, 256, 0, s>>>(a);
    else local_map_kernel<4><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

// The local-weighted fold over the frames of `a` (c.coef, c.maps / c.map_stride, c.floor, c.power, c.out / c.out_stride,
// c.den / c.den_stride): the generic kernels, linear or cubic. The u8 BGR fast kernels do not serve this state.
hipError_t launch_local_fold(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0 || !c.maps || c.power < 1 || c.power > 4) return hipErrorInvalidValue;
    const dim3 grid((a.dw + 63) / 64, (a.dh + 3) / 4);
    if (a.interp == STK_INTER_CUBIC) return launch_warp_cubic<true, FoldLocal>(a, c, depth, grid, s);
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        warp_accumulate_kernel<decltype(t), CN, true, FoldLocal<CN>><<<grid, 256, 0, s>>>(a, c);
    });
}

}  // namespace stk

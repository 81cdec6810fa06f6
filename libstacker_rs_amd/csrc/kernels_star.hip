// kernels_star.hip — star detection (include/stacker.h, stk_star_params): the peaks of every frame of an
// 8-bit stack with their background-subtracted first moments, all in integers.
//
// The pass is modelled on local_map_kernel (kernels_local.hip). One workgroup of 256 threads per 64 x 64 tile of one frame
// (blockIdx.x = tile, blockIdx.y = frame of the launch; the frames are an array of pointers with one row stride):
//   1. the tile and a halo of `radius` (<= 7) are read from the interleaved frame (as dwords where the frame's base and row
//      stride allow it and the tile is whole in x, byte by byte otherwise), turned into the integer grey (grey.h) and kept
//      in LDS as bytes. A position outside the frame forms NO address: its LDS byte is 0 and is never used, because a peak
//      needs its whole window inside the frame and the statistics count the tile's own pixels inside the frame only.
//   2. a 256-bin histogram of the tile's pixels inside the frame (no halo), one copy per wave (integer LDS atomics;
//      Guideline 12: partial sums first), summed and prefix-summed: med = the k-th smallest grey, k = (n + 1) / 2; mad = the
//      k-th smallest |g - med|, from the same sums: #{|g - med| <= d} = cum(med + d) - cum(med - d - 1);
//      thr = med + max((int)ceilf(ks * (float)mad), min_contrast) — the one float multiply and ceil of the pass. (Spreading
//      the counts further, over 32 partial histograms by lane, measured 0.8 % on a 256 x 4K sky stack and was not kept:
//      the atomics' contention is not what the pass waits for)
//   3. a thread tests 16 pixels of the tile: admissible (window inside the frame), g >= thr, the maximum of its window
//      (strictly above what precedes it in raster order, not below what follows: a plateau yields its raster-first pixel),
//      at least min_pixels window pixels >= thr. A peak's moments over the window, v = max(g - med, 0): S, Sx, Sy (int32;
//      S <= 225 * 255). Peaks go to an LDS list in any order (an LDS atomic hands out the slot).
//   4. every peak counts the peaks that precede it under the key (S descending, py ascending, px ascending) and is written
//      to global slot `rank` when rank < STK_STAR_TILE_CAP: no global atomics, and the same bits whatever the order in
//      which the list was filled.
// Two peaks are never within each other's window (the later one in raster order would have to be both above and not above
// the earlier), so they lie >= radius + 1 apart in x or in y: a tile holds at most ceil(64 / (radius + 1))^2 of them,
// 22^2 = 484 at the smallest radius, 2. The list has that many slots.
#include "common.h"
#include "grey.h"

namespace stk {

constexpr int ST = 64;                       // pixels per tile side
constexpr int ST_RMAX = 7;                   // largest radius
constexpr int ST_LEFT = 8;                   // LDS column of the tile's first pixel: the interior is stored as aligned dwords
constexpr int ST_GS = ST + 2 * ST_LEFT;      // bytes per LDS row = 80
constexpr int ST_ROWS = ST + 2 * ST_RMAX;    // rows at the largest radius = 78
constexpr int ST_LIST = 484;                 // ceil(64 / 3)^2: the bound above at radius 2

template <int CN>
__device__ __forceinline__ uint8_t star_grey_px(const uint8_t* p) {
    if constexpr (CN == 1) return p[0];
    else return grey_u8(p[0], p[1], p[2]);
}

// four consecutive pixels starting at a dword-aligned address -> four greys in one dword (kernels_local.hip's
// local_grey_x4, restated: that file's kernels stay as they are)
template <int CN>
__device__ __forceinline__ uint32_t star_grey_x4(const uint32_t* p) {
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

template <int CN>
__global__ __launch_bounds__(256) void star_detect_kernel(StarDetectArgs a) {
    __shared__ __align__(16) uint8_t grey[ST_ROWS * ST_GS];
    __shared__ int hist[4 * 256];             // one histogram per wave, then [0, 256): the sums, [256, 512): scan scratch
    __shared__ int list[ST_LIST * 7];
    __shared__ int s_med, s_mad, s_count;
    const int w = a.w, h = a.h, R = a.radius;
    const int gn = ST + 2 * R;                                         // grey rows (= columns) in use
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * ST, y0 = ty * ST;
    const uint8_t* __restrict__ src = static_cast<const uint8_t*>(a.frames[blockIdx.y]);
    const int t = threadIdx.x;

    // ---- 1. grey tile + halo into LDS: grey row r <-> image row y0 - R + r, grey column ST_LEFT + lx <-> image column
    //         x0 + lx, lx in [-R, ST + R). Outside the frame: 0, and no address.
    for (int i = t; i < 4 * 256; i += 256) hist[i] = 0;
    if (t == 0) s_count = 0;
    const bool dwords = x0 + ST <= w && ((reinterpret_cast<uintptr_t>(src) | a.stride) & 3) == 0;   // x0 * CN is a multiple of 4
    if (dwords) {
        const int q = t & 15;
#pragma unroll
        for (int k = 0; k < (ST_ROWS + 15) / 16; k++) {
            const int r = (t >> 4) + 16 * k;
            if (r < gn) {
                const int yy = y0 - R + r;
                uint32_t g = 0;
                if (yy >= 0 && yy < h) g = star_grey_x4<CN>(reinterpret_cast<const uint32_t*>(src + (size_t)yy * a.stride + (size_t)(x0 + 4 * q) * CN));
                *reinterpret_cast<uint32_t*>(&grey[r * ST_GS + ST_LEFT + 4 * q]) = g;
            }
        }
        const int h2 = 2 * R;                                           // the halo columns, all rows
        for (int i = t; i < gn * h2; i += 256) {
            const int r = i / h2, c = i - r * h2;
            const int lx = c < R ? c - R : ST + c - R;
            const int yy = y0 - R + r, xx = x0 + lx;
            uint8_t g = 0;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) g = star_grey_px<CN>(src + (size_t)yy * a.stride + (size_t)xx * CN);
            grey[r * ST_GS + ST_LEFT + lx] = g;
        }
    } else {
        for (int i = t; i < gn * gn; i += 256) {
            const int r = i / gn, lx = i - r * gn - R;
            const int yy = y0 - R + r, xx = x0 + lx;
            uint8_t g = 0;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) g = star_grey_px<CN>(src + (size_t)yy * a.stride + (size_t)xx * CN);
            grey[r * ST_GS + ST_LEFT + lx] = g;
        }
    }
    __syncthreads();

    // ---- 2. tile statistics. A thread owns column (t & 63) of rows (t >> 6) * 16 .. + 15: its wave's histogram.
    const int lx = t & 63, ly0 = (t >> 6) * 16;
    const int tw = min(ST, w - x0), th = min(ST, h - y0);               // the tile's pixels inside the frame
    {
        int* hw = &hist[(t >> 6) * 256];
        if (lx < tw)
            for (int i = 0; i < 16 && ly0 + i < th; i++) atomicAdd(&hw[grey[(R + ly0 + i) * ST_GS + ST_LEFT + lx]], 1);
    }
    __syncthreads();
    int v = hist[t] + hist[256 + t] + hist[512 + t] + hist[768 + t];
    __syncthreads();
    // inclusive prefix sums of 256 bins, ping-pong between hist[0, 256) and hist[256, 512)
    int* cur = hist; int* nxt = hist + 256;
    cur[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        nxt[t] = cur[t] + (t >= d ? cur[t - d] : 0);
        __syncthreads();
        int* sw = cur; cur = nxt; nxt = sw;
    }
    const int* cum = cur;
    const int kth = (tw * th + 1) / 2;
    if (cum[t] >= kth && (t == 0 || cum[t - 1] < kth)) s_med = t;       // exactly one bin
    __syncthreads();
    const int med = s_med;
    {
        // thread d: #{|g - med| <= d} and the same for d - 1 (monotone in d; d = 255 covers every grey)
        const int hi = min(med + t, 255), lo = med - t - 1;
        const int cd = cum[hi] - (lo >= 0 ? cum[lo] : 0);
        int cp = 0;
        if (t > 0) { const int hi1 = min(med + t - 1, 255), lo1 = med - t; cp = cum[hi1] - (lo1 >= 0 ? cum[lo1] : 0); }
        if (cd >= kth && (t == 0 || cp < kth)) s_mad = t;
    }
    __syncthreads();
    const int dT = max((int)ceilf(a.ks * (float)s_mad), a.min_contrast);
    const int thr = med + dT;

    // ---- 3. peaks of this thread's 16 pixels
    const int px = x0 + lx;
    if (px >= R && px < w - R) {
        for (int i = 0; i < 16; i++) {
            const int py = y0 + ly0 + i;
            if (py < R || py >= h - R) continue;
            const uint8_t* c = &grey[(R + ly0 + i) * ST_GS + ST_LEFT + lx];
            const int g = c[0];
            if (g < thr) continue;
            bool peak = true;
            for (int dy = -R; dy <= R && peak; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const int q = c[dy * ST_GS + dx];
                    const bool before = dy < 0 || (dy == 0 && dx < 0);
                    if (before ? q >= g : q > g) { peak = false; break; }
                }
            if (!peak) continue;
            int npix = 0, S = 0, Sx = 0, Sy = 0;
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const int q = c[dy * ST_GS + dx];
                    npix += q >= thr;
                    const int vv = max(q - med, 0);
                    S += vv; Sx += vv * dx; Sy += vv * dy;
                }
            if (npix < a.min_pixels) continue;
            const int slot = atomicAdd(&s_count, 1);
            if (slot < ST_LIST) {                                       // (always: the bound in the header comment)
                int* o = &list[slot * 7];
                o[0] = px; o[1] = py; o[2] = S; o[3] = Sx; o[4] = Sy; o[5] = g; o[6] = npix;
            }
        }
    }
    __syncthreads();

    // ---- 4. rank and write
    const int count = min(s_count, ST_LIST);
    const size_t cell = (size_t)blockIdx.y * a.tiles + blockIdx.x;
    if (t == 0) a.counts[cell] = count;
    for (int i = t; i < count; i += 256) {
        const int S = list[i * 7 + 2], py = list[i * 7 + 1], pxi = list[i * 7];
        int rank = 0;
        for (int j = 0; j < count; j++) {
            const int Sj = list[j * 7 + 2], yj = list[j * 7 + 1], xj = list[j * 7];
            rank += Sj > S || (Sj == S && (yj < py || (yj == py && xj < pxi)));
        }
        if (rank < STAR_TILE_CAP) {
            StarRecord rec;
            rec.px = pxi; rec.py = py; rec.S = S; rec.Sx = list[i * 7 + 3]; rec.Sy = list[i * 7 + 4];
            rec.peak = list[i * 7 + 5]; rec.npix = list[i * 7 + 6]; rec.pad = 0;
            a.records[cell * STAR_TILE_CAP + rank] = rec;
        }
    }
}

int star_tiles(int w, int h) { return ((w + ST - 1) / ST) * ((h + ST - 1) / ST); }

hipError_t launch_star_detect(const void* const* frames_dev, int n, int cn, int w, int h, size_t stride_bytes, int radius, float ks,
                              int min_contrast, int min_pixels, int32_t* counts, StarRecord* records, hipStream_t s) {
    if (n <= 0 || n > 65535 || (cn != 1 && cn != 3 && cn != 4) || radius < 2 || radius > ST_RMAX || w <= 0 || h <= 0) return hipErrorInvalidValue;
    const StarDetectArgs a{frames_dev, counts, records, w, h, stride_bytes, (w + ST - 1) / ST, star_tiles(w, h), radius, ks, min_contrast, min_pixels};
    const dim3 grid((unsigned)a.tiles, (unsigned)n);
    if (cn == 1) star_detect_kernel<1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) star_detect_kernel<3><<<grid, 256, 0, s>>>(a);
    else star_detect_kernel<4><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace stk

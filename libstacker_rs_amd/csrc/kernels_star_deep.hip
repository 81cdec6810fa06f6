// kernels_star_deep.hip — star detection on 8-bit, 16-bit and f32 frames (include/stacker.h, stk_star_deep_params; DESIGN
// §4.28): kernels_star.hip's pass on a 16-bit integer key, all in integers behind the key.
//
// One workgroup of 256 threads per 64 x 64 tile of one frame (blockIdx.x = tile, blockIdx.y = frame of the launch):
//   1. the tile and a halo of `radius` (<= 7) are read from the interleaved frame, turned into the key (deep_key below)
//      and kept in LDS as u16, 78 rows of 80 = 12 480 bytes. The tile's own columns go four pixels per thread from dwords
//      (u8, u16) or float4s (f32) where the frame's base and row stride are aligned to that unit and the tile is whole in x,
//      element by element otherwise; both routes compute every key with the same function on the same values, so the LDS
//      contents are the same. A position outside the frame forms NO address: its key is 0 and is never used.
//   2. the exact median and MAD of the tile's (up to 4096) keys inside the frame: two selections of lds_select.h at workgroup
//      scope, four passes over the LDS tile. A thread's share is its 16 pixels of one column; on a sky tile nearly every key
//      shares its high byte, so the high-byte passes add merged runs.
//      thr = med + max((int)fminf(ceilf(ks * (float)mad), 65536.0f), min_contrast).
//   3. the peak test, the window walk (S <= 225 * 65535, |Sx|, |Sy| <= 840 * 65535: int32), the LDS list,
//   4. the rank by (S descending, py, px) and the record slots are kernels_star.hip's, to the letter.
// No global atomics, no floating-point atomics, no scratch.
#include "common.h"
#include "grey.h"
#include "lds_select.h"
#include "star_key.h"

namespace stk {

namespace {

constexpr int SD = 64;                       // pixels per tile side
constexpr int SD_RMAX = 7;                   // largest radius
constexpr int SD_LEFT = 8;                   // LDS column of the tile's first pixel
constexpr int SD_GS = SD + 2 * SD_LEFT;      // keys per LDS row = 80 (160 bytes: a group of four keys is 8-byte aligned)
constexpr int SD_ROWS = SD + 2 * SD_RMAX;    // rows at the largest radius = 78
constexpr int SD_LIST = 484;                 // ceil(64 / 3)^2 peaks at the smallest radius (kernels_star.hip's bound)

// key_f32 and deep_key, the key of one pixel: star_key.h

// four consecutive pixels from an aligned address (4 bytes for u8 / u16, 16 for f32) -> four keys, k[0] the first pixel
template <typename T, int CN>
__device__ __forceinline__ void deep_key_x4(const T* p, float scale, uint32_t k[4]) {
    if constexpr (sizeof(T) == 1) {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(p);
        if constexpr (CN == 1) {
            const uint32_t d0 = d[0];
            k[0] = d0 & 255u; k[1] = (d0 >> 8) & 255u; k[2] = (d0 >> 16) & 255u; k[3] = d0 >> 24;
        } else if constexpr (CN == 3) {
            const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];               // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            k[0] = grey_u8(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
            k[1] = grey_u8(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
            k[2] = grey_u8((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
            k[3] = grey_u8((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) { const uint32_t v = d[i]; k[i] = grey_u8(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u); }
        }
    } else if constexpr (sizeof(T) == 2) {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(p);
        if constexpr (CN == 1) {
            const uint32_t d0 = d[0], d1 = d[1];
            k[0] = d0 & 0xffffu; k[1] = d0 >> 16; k[2] = d1 & 0xffffu; k[3] = d1 >> 16;
        } else if constexpr (CN == 3) {
            const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], d5 = d[5];   // b0 g0 | r0 b1 | g1 r1 | b2 g2 | r2 b3 | g3 r3
            k[0] = grey_u16(d0 & 0xffffu, d0 >> 16, d1 & 0xffffu);
            k[1] = grey_u16(d1 >> 16, d2 & 0xffffu, d2 >> 16);
            k[2] = grey_u16(d3 & 0xffffu, d3 >> 16, d4 & 0xffffu);
            k[3] = grey_u16(d4 >> 16, d5 & 0xffffu, d5 >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) { const uint32_t lo = d[2 * i], hi = d[2 * i + 1]; k[i] = grey_u16(lo & 0xffffu, lo >> 16, hi & 0xffffu); }
        }
    } else {
        const float4* d = reinterpret_cast<const float4*>(p);
        if constexpr (CN == 1) {
            const float4 a = d[0];
            k[0] = key_f32(a.x, scale); k[1] = key_f32(a.y, scale); k[2] = key_f32(a.z, scale); k[3] = key_f32(a.w, scale);
        } else if constexpr (CN == 3) {
            const float4 a = d[0], b = d[1], c = d[2];                    // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            k[0] = key_f32(grey_f32(a.x, a.y, a.z), scale); k[1] = key_f32(grey_f32(a.w, b.x, b.y), scale);
            k[2] = key_f32(grey_f32(b.z, b.w, c.x), scale); k[3] = key_f32(grey_f32(c.y, c.z, c.w), scale);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) { const float4 a = d[i]; k[i] = key_f32(grey_f32(a.x, a.y, a.z), scale); }
        }
    }
}

using DeepSelect = WorkgroupSelect<false>;    // the rank is known: (tile pixels inside the frame + 1) / 2 >= 1

template <typename T, int CN>
__global__ __launch_bounds__(256) void star_detect_deep_kernel(StarDetectArgs a, float scale) {
    __shared__ __align__(16) uint16_t key[SD_ROWS * SD_GS];
    __shared__ int hist[DeepSelect::HIST_INTS];
    __shared__ int list[SD_LIST * 7];
    __shared__ int s_pick[DeepSelect::PICK_INTS], s_wsum[DeepSelect::WSUM_INTS], s_count;
    const int w = a.w, h = a.h, R = a.radius;
    const int gn = SD + 2 * R;                                            // key rows (= columns) in use
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * SD, y0 = ty * SD;
    const char* __restrict__ src = static_cast<const char*>(a.frames[blockIdx.y]);
    const int t = threadIdx.x;
    auto px_at = [&](int yy, int xx) { return reinterpret_cast<const T*>(src + (size_t)yy * a.stride) + (size_t)xx * CN; };

    // ---- 1. keys of the tile + halo into LDS: row r <-> image row y0 - R + r, column SD_LEFT + lx <-> image column x0 + lx,
    //         lx in [-R, SD + R). Outside the frame: 0, and no address.
    for (int i = t; i < DeepSelect::HIST_INTS; i += 256) hist[i] = 0;
    if (t == 0) s_count = 0;
    constexpr uintptr_t UNIT = sizeof(T) == 4 ? 15 : 3;                   // x0 * CN * sizeof(T) is a multiple of 16
    const bool wide = x0 + SD <= w && ((reinterpret_cast<uintptr_t>(src) | a.stride) & UNIT) == 0;
    if (wide) {
        const int q = t & 15;
#pragma unroll
        for (int kk = 0; kk < (SD_ROWS + 15) / 16; kk++) {
            const int r = (t >> 4) + 16 * kk;
            if (r < gn) {
                const int yy = y0 - R + r;
                uint32_t k4[4] = {0u, 0u, 0u, 0u};
                if (yy >= 0 && yy < h) deep_key_x4<T, CN>(px_at(yy, x0 + 4 * q), scale, k4);
                *reinterpret_cast<uint2*>(&key[r * SD_GS + SD_LEFT + 4 * q]) = make_uint2(k4[0] | (k4[1] << 16), k4[2] | (k4[3] << 16));
            }
        }
        const int h2 = 2 * R;                                             // the halo columns, all rows
        for (int i = t; i < gn * h2; i += 256) {
            const int r = i / h2, c = i - r * h2;
            const int lx = c < R ? c - R : SD + c - R;
            const int yy = y0 - R + r, xx = x0 + lx;
            uint32_t g = 0;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) g = deep_key<T, CN>(px_at(yy, xx), scale);
            key[r * SD_GS + SD_LEFT + lx] = (uint16_t)g;
        }
    } else {
        for (int i = t; i < gn * gn; i += 256) {
            const int r = i / gn, lx = i - r * gn - R;
            const int yy = y0 - R + r, xx = x0 + lx;
            uint32_t g = 0;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) g = deep_key<T, CN>(px_at(yy, xx), scale);
            key[r * SD_GS + SD_LEFT + lx] = (uint16_t)g;
        }
    }
    __syncthreads();

    // ---- 2. tile statistics. A thread owns column (t & 63) of rows (t >> 6) * 16 .. + 15: its wave's histogram.
    const int lx = t & 63, ly0 = (t >> 6) * 16;
    const int tw = min(SD, w - x0), th = min(SD, h - y0);                  // the tile's pixels inside the frame
    const int rows = lx < tw ? max(min(16, th - ly0), 0) : 0;             // this thread's pixels
    const uint16_t* col = &key[(R + ly0) * SD_GS + SD_LEFT + lx];
    const DeepSelect sel{hist, s_pick, s_wsum, t, t >> 6};
    const int kth = (tw * th + 1) / 2;
    const auto column = select_share(0, rows, 1, [](int) { return true; }, [=](int i) { return (int)col[i * SD_GS]; });
    const int med = select16<SelectFill::Merged>(sel, column, SelectKey{}, kth);
    const int mad = select16<SelectFill::Merged>(sel, column, SelectAbsDev{med}, kth);
    const int dT = max((int)fminf(ceilf(a.ks * (float)mad), 65536.0f), a.min_contrast);
    const int thr = med + dT;

    // ---- 3. peaks of this thread's 16 pixels
    const int px = x0 + lx;
    if (px >= R && px < w - R) {
        for (int i = 0; i < 16; i++) {
            const int py = y0 + ly0 + i;
            if (py < R || py >= h - R) continue;
            const uint16_t* c = col + i * SD_GS;
            const int g = c[0];
            if (g < thr) continue;
            bool peak = true;
            for (int dy = -R; dy <= R && peak; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const int q = c[dy * SD_GS + dx];
                    const bool before = dy < 0 || (dy == 0 && dx < 0);
                    if (before ? q >= g : q > g) { peak = false; break; }
                }
            if (!peak) continue;
            int npix = 0, S = 0, Sx = 0, Sy = 0;
            for (int dy = -R; dy <= R; dy++)
                for (int dx = -R; dx <= R; dx++) {
                    const int q = c[dy * SD_GS + dx];
                    npix += q >= thr;
                    const int vv = max(q - med, 0);
                    S += vv; Sx += vv * dx; Sy += vv * dy;
                }
            if (npix < a.min_pixels) continue;
            const int slot = atomicAdd(&s_count, 1);
            if (slot < SD_LIST) {                                         // (always: kernels_star.hip's bound)
                int* o = &list[slot * 7];
                o[0] = px; o[1] = py; o[2] = S; o[3] = Sx; o[4] = Sy; o[5] = g; o[6] = npix;
            }
        }
    }
    __syncthreads();

    // ---- 4. rank and write
    const int count = min(s_count, SD_LIST);
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

template <typename T>
void deep_launch_cn(int cn, dim3 grid, hipStream_t s, const StarDetectArgs& a, float scale) {
    if (cn == 1) star_detect_deep_kernel<T, 1><<<grid, 256, 0, s>>>(a, scale);
    else if (cn == 3) star_detect_deep_kernel<T, 3><<<grid, 256, 0, s>>>(a, scale);
    else star_detect_deep_kernel<T, 4><<<grid, 256, 0, s>>>(a, scale);
}

}  // namespace

hipError_t launch_star_detect_deep(const void* const* frames_dev, int n, int depth, int cn, int w, int h, size_t stride_bytes, int radius,
                                   float ks, int min_contrast, int min_pixels, float f32_scale, int32_t* counts, StarRecord* records,
                                   hipStream_t s) {
    if (n <= 0 || n > 65535 || (cn != 1 && cn != 3 && cn != 4) || (depth != 8 && depth != 16 && depth != 32) || radius < 2 ||
        radius > SD_RMAX || w <= 0 || h <= 0 || stride_bytes % (size_t)(depth / 8) || stride_bytes < (size_t)w * cn * (depth / 8))
        return hipErrorInvalidValue;
    const StarDetectArgs a{frames_dev, counts, records, w, h, stride_bytes, (w + SD - 1) / SD, star_tiles(w, h), radius, ks, min_contrast, min_pixels};
    const dim3 grid((unsigned)a.tiles, (unsigned)n);
    if (depth == 8) deep_launch_cn<uint8_t>(cn, grid, s, a, f32_scale);
    else if (depth == 16) deep_launch_cn<uint16_t>(cn, grid, s, a, f32_scale);
    else deep_launch_cn<float>(cn, grid, s, a, f32_scale);
    return hipGetLastError();
}

}  // namespace stk

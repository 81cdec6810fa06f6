// kernels_demosaic.hip — colour-filter mosaics (include/stacker.h, stk_mosaic): the stencil pass that turns a
// stack of single-channel Bayer mosaics into B G R stacks, the superpixel pass, and the colour mask of a pattern.
//
// demosaic_kernel. A workgroup of 256 threads owns a DEM_TW x DEM_TH tile of one frame (blockIdx.z); a thread owns one
// 2 x 2 cell of it. The cell grid is shifted by the pattern so that a cell's top-left pixel is always a red site: the tile's
// origin is (64 bx - rx, 16 by - ry) with (rx, ry) the parity of the red sites, so every lane runs the same code on one R,
// two G and one B site, the four patterns are four grid origins of one kernel, and the pixels of an edge cell that fall
// outside the frame are masked one by one. The tile plus a halo (1 bilinear, 2 MHC, 3 HA) is staged in LDS in the
// accumulator type (int32 for integer mosaics, f32 for f32 ones) with BORDER_REFLECT_101 applied to the indices on the way
// in; a position further than the halo outside the frame holds 0 and is read by masked pixels only. HA keeps a second plane
// of G8 at the R / B positions of the tile plus a halo of 1, written from the first plane behind one barrier: G8 at a
// position outside the frame is the formula on the reflected mosaic. 6 KB + 4.6 KB of LDS, no atomics, no scratch.
// Addresses. A load forms the address of an in-frame sample only (the reflected index of a position at most `halo` outside);
// a store that of an in-frame pixel only; frames and outputs are read and written element by element, pixel bytes only.
#include <type_traits>

#include "common.h"

namespace stk {

namespace {

enum { DEM_BILINEAR = 0, DEM_MHC = 1, DEM_HA = 2 };

// A frame pointer comes out of the record table: the casts say that it is global memory (see kernels_calibrate.hip).
#define DEM_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const DEM_GLOBAL T* dem_src_row(const void* base, size_t byte_offset) {
    return (const DEM_GLOBAL T*)((const DEM_GLOBAL uint8_t*)base + byte_offset);
}
template <typename T>
__device__ __forceinline__ DEM_GLOBAL T* dem_dst_row(void* base, size_t byte_offset) {
    return (DEM_GLOBAL T*)((DEM_GLOBAL uint8_t*)base + byte_offset);
}

template <typename T> struct DemAcc { using type = int; };
template <> struct DemAcc<float> { using type = float; };

// BORDER_REFLECT_101 of an index at most 3 outside [0, n), n >= 3 (n = 3 takes the second reflection)
__device__ __forceinline__ int dem_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i < 0 ? -i : i;
}

__device__ __forceinline__ int dem_abs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ float dem_abs(float v) { return __builtin_fabsf(v); }

// numerator s over 2^K as an output sample: integers round half up by floor((s + D / 2) / D) and saturate; f32 multiplies
// by 1 / D (K = 0: the sample itself)
template <typename O, int K, typename A>
__device__ __forceinline__ O dem_out(A s) {
    if constexpr (std::is_same<A, float>::value) return K ? s * (1.0f / (float)(1 << K)) : s;
    else if constexpr (std::is_same<O, float>::value) return (float)s * (1.0f / (float)(1 << K));
    else {
        constexpr int hi = sizeof(O) == 1 ? 255 : 65535;
        const int r = (s + ((1 << K) >> 1)) >> K;                   // arithmetic shift: floor
        return (O)min(max(r, 0), hi);
    }
}

// Hamilton-Adams green in eighths at an R / B position p of the staged plane (row pitch LW)
template <typename A, int LW>
__device__ __forceinline__ A dem_g8(const A* s, int p) {
    const A two = (A)2;
    const A c2 = two * s[p];
    const A W = s[p - 1], E = s[p + 1], N = s[p - LW], S = s[p + LW];
    const A tH = (c2 - s[p - 2]) - s[p + 2], tV = (c2 - s[p - 2 * LW]) - s[p + 2 * LW];
    const A dH = dem_abs(W - E) + dem_abs(tH), dV = dem_abs(N - S) + dem_abs(tV);
    const A gH = two * (W + E) + tH, gV = two * (N + S) + tV;
    return dH < dV ? two * gH : (dV < dH ? two * gV : gH + gV);
}

// an R / B site at p (q: its place in the G8 plane): the green and the opposite colour there
template <int M, typename O, int LW, int GW, typename A>
__device__ __forceinline__ void dem_rb_site(const A* s, const A* g, int p, int q, O& green, O& opp) {
    const A c = s[p];
    if constexpr (M == DEM_HA) {
        const A G8 = g[q];
        const A dNW = (A)8 * s[p - LW - 1] - g[q - GW - 1], dNE = (A)8 * s[p - LW + 1] - g[q - GW + 1];
        const A dSW = (A)8 * s[p + LW - 1] - g[q + GW - 1], dSE = (A)8 * s[p + LW + 1] - g[q + GW + 1];
        green = dem_out<O, 3>(G8);
        opp = dem_out<O, 5>(((A)4 * G8 + (dNW + dNE)) + (dSW + dSE));
    } else {
        const A x1 = (s[p - LW] + s[p + LW]) + (s[p - 1] + s[p + 1]);
        const A d = (s[p - LW - 1] + s[p - LW + 1]) + (s[p + LW - 1] + s[p + LW + 1]);
        if constexpr (M == DEM_BILINEAR) {
            green = dem_out<O, 2>(x1);
            opp = dem_out<O, 2>(d);
        } else {
            const A x2 = (s[p - 2 * LW] + s[p + 2 * LW]) + (s[p - 2] + s[p + 2]);
            green = dem_out<O, 4>((A)8 * c + (A)4 * x1 - (A)2 * x2);
            opp = dem_out<O, 4>((A)12 * c + (A)4 * d - (A)3 * x2);
        }
    }
}

// a G site at p: the colour of its row neighbours and the colour of its column neighbours there
template <int M, typename O, int LW, int GW, typename A>
__device__ __forceinline__ void dem_g_site(const A* s, const A* g, int p, int q, O& rowc, O& colc) {
    const A c = s[p];
    if constexpr (M == DEM_HA) {
        const A G8 = (A)8 * c;
        const A dW = (A)8 * s[p - 1] - g[q - 1], dE = (A)8 * s[p + 1] - g[q + 1];
        const A dN = (A)8 * s[p - LW] - g[q - GW], dS = (A)8 * s[p + LW] - g[q + GW];
        rowc = dem_out<O, 4>(((A)2 * G8 + dW) + dE);
        colc = dem_out<O, 4>(((A)2 * G8 + dN) + dS);
    } else {
        const A h1 = s[p - 1] + s[p + 1], v1 = s[p - LW] + s[p + LW];
        if constexpr (M == DEM_BILINEAR) {
            rowc = dem_out<O, 1>(h1);
            colc = dem_out<O, 1>(v1);
        } else {
            const A h2 = s[p - 2] + s[p + 2], v2 = s[p - 2 * LW] + s[p + 2 * LW];
            const A d = (s[p - LW - 1] + s[p - LW + 1]) + (s[p + LW - 1] + s[p + LW + 1]);
            rowc = dem_out<O, 4>((A)10 * c + (A)8 * h1 - (A)2 * d - (A)2 * h2 + v2);
            colc = dem_out<O, 4>((A)10 * c + (A)8 * v1 - (A)2 * d - (A)2 * v2 + h2);
        }
    }
}

template <typename O>
__device__ __forceinline__ void dem_store(const DemArgs& a, void* dst, int x, int y, O b, O g, O r) {
    if ((unsigned)x >= (unsigned)a.w || (unsigned)y >= (unsigned)a.h) return;
    DEM_GLOBAL O* o = dem_dst_row<O>(dst, (size_t)y * a.out_stride) + (size_t)x * 3;
    o[0] = b; o[1] = g; o[2] = r;
}

}  // namespace

template <typename T, typename O, int M>
__global__ __launch_bounds__(256) void demosaic_kernel(DemArgs a) {
    using A = typename DemAcc<T>::type;
    constexpr int H = M == DEM_HA ? 3 : (M == DEM_MHC ? 2 : 1);
    constexpr int LW = DEM_TW + 2 * H, LH = DEM_TH + 2 * H;
    constexpr int GW = DEM_TW + 2, GH = DEM_TH + 2;
    __shared__ A sM[LW * LH];
    __shared__ A sG[M == DEM_HA ? GW * GH : 1];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * DEM_TW - (a.pattern & 1), y0 = blockIdx.y * DEM_TH - (a.pattern >> 1);
    const DemFrame fr = a.frames[blockIdx.z];

    for (int idx = t; idx < LW * LH; idx += 256) {
        const int ly = idx / LW, lx = idx - ly * LW;
        const int gx = x0 - H + lx, gy = y0 - H + ly;
        A v = (A)0;
        if (gx >= -H && gx < a.w + H && gy >= -H && gy < a.h + H)
            v = (A)dem_src_row<T>(fr.src, (size_t)dem_reflect(gy, a.h) * a.in_stride)[dem_reflect(gx, a.w)];
        sM[idx] = v;
    }
    __syncthreads();
    if constexpr (M == DEM_HA) {
        // the R / B positions of the G8 plane: (col + row) even, its origin being one left of and above a red site
        constexpr int HALF = GW / 2;
        for (int idx = t; idx < HALF * GH; idx += 256) {
            const int row = idx / HALF, col = 2 * (idx - row * HALF) + (row & 1);
            sG[row * GW + col] = dem_g8<A, LW>(sM, (row + H - 1) * LW + col + H - 1);
        }
        __syncthreads();
    }

    const int lx = 2 * (t & 31), ly = 2 * (t >> 5);
    const int p = (ly + H) * LW + lx + H, q = (ly + 1) * GW + lx + 1;
    const int x = x0 + lx, y = y0 + ly;
    O green, opp, rowc, colc;
    dem_rb_site<M, O, LW, GW>(sM, sG, p, q, green, opp);                                // red: B = opp
    dem_store<O>(a, fr.dst, x, y, opp, green, dem_out<O, 0>(sM[p]));
    dem_g_site<M, O, LW, GW>(sM, sG, p + 1, q + 1, rowc, colc);                         // green on a red row: R = row, B = column
    dem_store<O>(a, fr.dst, x + 1, y, colc, dem_out<O, 0>(sM[p + 1]), rowc);
    dem_g_site<M, O, LW, GW>(sM, sG, p + LW, q + GW, rowc, colc);                       // green on a blue row: B = row, R = column
    dem_store<O>(a, fr.dst, x, y + 1, rowc, dem_out<O, 0>(sM[p + LW]), colc);
    dem_rb_site<M, O, LW, GW>(sM, sG, p + LW + 1, q + GW + 1, green, opp);              // blue: R = opp
    dem_store<O>(a, fr.dst, x + 1, y + 1, dem_out<O, 0>(sM[p + LW + 1]), green, opp);
}

// one thread per output pixel = one cell of the pattern itself (not shifted): B and R are its samples, G the mean of its two
template <typename T, typename O>
__global__ __launch_bounds__(256) void superpixel_kernel(DemArgs a) {
    using A = typename DemAcc<T>::type;
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * DEM_SP_TH + (threadIdx.x >> 6);
    if (X >= a.w / 2 || Y >= a.h / 2) return;
    const DemFrame fr = a.frames[blockIdx.z];
    const int rx = a.pattern & 1, ry = a.pattern >> 1;
    const DEM_GLOBAL T* r0 = dem_src_row<T>(fr.src, (size_t)(2 * Y) * a.in_stride) + 2 * (size_t)X;
    const DEM_GLOBAL T* r1 = dem_src_row<T>(fr.src, (size_t)(2 * Y + 1) * a.in_stride) + 2 * (size_t)X;
    const A m00 = (A)r0[0], m01 = (A)r0[1], m10 = (A)r1[0], m11 = (A)r1[1];
    const A red = ry ? (rx ? m11 : m10) : (rx ? m01 : m00);
    const A blue = ry ? (rx ? m00 : m01) : (rx ? m10 : m11);
    const A greens = rx == ry ? m01 + m10 : m00 + m11;
    DEM_GLOBAL O* o = dem_dst_row<O>(fr.dst, (size_t)Y * a.out_stride) + (size_t)X * 3;
    o[0] = dem_out<O, 0>(blue); o[1] = dem_out<O, 1>(greens); o[2] = dem_out<O, 0>(red);
}

template <typename T, typename O>
static hipError_t demosaic_launch_method(const DemArgs& a, int method, hipStream_t s) {
    if (method == 3) {
        const dim3 grid((a.w / 2 + 63) / 64, (a.h / 2 + DEM_SP_TH - 1) / DEM_SP_TH, a.n);
        if (a.w < 2 || a.h < 2 || grid.y > 65535) return hipErrorInvalidValue;
        superpixel_kernel<T, O><<<grid, 256, 0, s>>>(a);
        return hipGetLastError();
    }
    const dim3 grid((a.w + (a.pattern & 1) + DEM_TW - 1) / DEM_TW, (a.h + (a.pattern >> 1) + DEM_TH - 1) / DEM_TH, a.n);
    if (a.w < 3 || a.h < 3 || grid.y > 65535) return hipErrorInvalidValue;
    if (method == DEM_BILINEAR) demosaic_kernel<T, O, DEM_BILINEAR><<<grid, 256, 0, s>>>(a);
    else if (method == DEM_MHC) demosaic_kernel<T, O, DEM_MHC><<<grid, 256, 0, s>>>(a);
    else if (method == DEM_HA) demosaic_kernel<T, O, DEM_HA><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// A missing kernel is an error: every (depth, out_depth, method) the entry point admits has its instantiation here.
hipError_t launch_demosaic(const DemArgs& a, int depth, int out_depth, int method, hipStream_t s) {
    if (a.n <= 0 || a.n > 65535 || !a.frames || a.pattern < 0 || a.pattern > 3) return hipErrorInvalidValue;
    if (depth == 8 && out_depth == 8) return demosaic_launch_method<uint8_t, uint8_t>(a, method, s);
    if (depth == 8 && out_depth == 32) return demosaic_launch_method<uint8_t, float>(a, method, s);
    if (depth == 16 && out_depth == 16) return demosaic_launch_method<uint16_t, uint16_t>(a, method, s);
    if (depth == 16 && out_depth == 32) return demosaic_launch_method<uint16_t, float>(a, method, s);
    if (depth == 32 && out_depth == 32) return demosaic_launch_method<float, float>(a, method, s);
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cfa_mask_kernel(float* __restrict__ plane, int w, int h, int pattern, int channel) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const int rx = pattern & 1, ry = pattern >> 1;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const bool cx = (x & 1) == rx, cy = (y & 1) == ry;
        const int colour = cx && cy ? 2 : (!cx && !cy ? 0 : 1);
        plane[(size_t)y * w + x] = colour == channel ? 1.0f : 0.0f;
    }
}

hipError_t launch_cfa_mask(float* plane, int w, int h, int pattern, int channel, hipStream_t s) {
    if (!plane || w <= 0 || h <= 0 || pattern < 0 || pattern > 3 || channel < 0 || channel > 2) return hipErrorInvalidValue;
    const dim3 grid((w + 255) / 256, h < 65535 ? h : 65535);
    cfa_mask_kernel<<<grid, 256, 0, s>>>(plane, w, h, pattern, channel);
    return hipGetLastError();
}

}  // namespace stk

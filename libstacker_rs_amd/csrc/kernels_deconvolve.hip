// kernels_deconvolve.hip — Richardson-Lucy deconvolution (include/stacker.h, "deconvolution"): the
// initialisation, the ratio pass (A = P * u, r = D / fmaxf(A, floor)) and the update pass (C = P correlated with r, v = u C,
// the total-variation regulariser, and on the last iteration the output step).
//
// Work planes. deconv_init_kernel de-interleaves the image once into one tightly packed f32 plane per colour channel
// (D = d + pedestal, not finite or below 0 -> 0; u_0 = D is the same plane), so the two passes never see the channel count:
// blockIdx.z is the plane. Only the output step writes interleaved pixels again (pixel stride a.cn), and for four
// channels the initialisation copies alpha to the output.
//
// A pass. One workgroup of 256 threads per DCV_TW x DCV_TH tile of one plane. The tile and its halo (R rows above and
// below, H columns left and right; H = 8 for R <= 8, else 16: the radius class, a template parameter of the two passes)
// are staged in LDS, rows DCV_PITCH floats apart, coordinates outside the image mapped by BORDER_REFLECT_101 (one
// reflection: the halo is at most R <= min(w, h) - 1 wide; positions further out, which only tiles that overhang the image
// and the padding columns have, are clamped and reach no output). A thread owns DCV_NY runs of 4 outputs along x, 16 rows
// apart. Per tap row j it reads its window of the staged row as H / 2 + 1 aligned float4s (ds_read_b128; lanes 0 .. 15 of
// a quarter wave read consecutive float4s, the next quarter the next row, DCV_PITCH = 0 mod 64 banks apart:
// conflict-free) and runs 16 DCV_NY fmas per float4. The taps of a row are 2 H + 7 consecutive floats of the padded tap
// table (dcv_pad_taps), the same for every lane: they are read through the constant address space at wave-uniform
// addresses, all at the head of the row, and are scalar operands of the fmas. With H a constant the float4s of a row are
// expanded in line, so a row waits once for its loads (with H at run time every float4 waited for its own: 1.2 - 1.3 x
// slower at R = 8 and 16).
// Order. Every output's accumulator starts at 0.0f and takes acc = fmaf(P, value, acc) with j = -R .. R outermost and
// i = -R .. R inside it, as the definition says: the correlation walks the staged row upwards (i grows with the position),
// the convolution downwards (i = x - position), float4 by float4 and element by element; the four outputs of a run are
// four independent accumulators. A (position, output) pair whose |i| exceeds R is skipped, not multiplied by a zero tap:
// the test is wave-uniform, and a float4 all of whose sixteen pairs are inside takes a path without tests.
// Built with -fno-slp-vectorize (Makefile): paired into packed fmas the tap loop costs the same slots plus the moves.
// No MFMA, no atomics, no scratch; no result depends on the tiling.
#include "common.h"

namespace stk {

namespace {

#define DCV_GLOBAL __attribute__((address_space(1)))
#define DCV_CONST __attribute__((address_space(4)))

static_assert(DCV_NY == 1 || DCV_NY == 2, "DCV_NY: 1 or 2 rows of outputs per thread");
static_assert(DCV_TW + 2 * 16 <= DCV_PITCH && DCV_PITCH % 64 == 0, "a staged row holds the tile and both halos");

// BORDER_REFLECT_101 of an index at most n - 1 outside [0, n); anything further out is clamped (it reaches no output)
__device__ __forceinline__ int dcv_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// the tile of plane `src` at (X0, Y0) with its halo into LDS; ends with the barrier
__device__ __forceinline__ void dcv_stage(float* tile, const DCV_GLOBAL float* src, int w, int h, int X0, int Y0, int R, int H) {
    const int t = threadIdx.x, lx = t & (DCV_PITCH - 1), LW = DCV_TW + 2 * H, LH = DCV_TH + 2 * R;
    if (lx < LW) {
        const int gx = dcv_reflect(X0 - H + lx, w);
        for (int ly = t / DCV_PITCH; ly < LH; ly += 256 / DCV_PITCH) {
            const int gy = dcv_reflect(Y0 - R + ly, h);
            tile[ly * DCV_PITCH + lx] = src[(size_t)gy * w + gx];
        }
    }
    __syncthreads();
}


// one float4 of a thread's window: the positions 4 m - H .. 4 m + 3 - H from the run's first output, against the four
// outputs; tap: the whole padded row of taps. m and H are constants where this is expanded; a float4 that may straddle an
// end of the tap row for some radius of the class takes a wave-uniform test, and then skips the pairs with |i| > R
template <bool CONV, int H>
__device__ __forceinline__ void dcv_chunk(const float* row, const float (&tap)[2 * H + 7], int m, int R, float (&acc)[DCV_NY][4]) {
    float v[DCV_NY][4];
#pragma unroll
    for (int n = 0; n < DCV_NY; n++) {
        const float4 q = *reinterpret_cast<const float4*>(row + n * 16 * DCV_PITCH + 4 * m);
        v[n][0] = q.x; v[n][1] = q.y; v[n][2] = q.z; v[n][3] = q.w;
    }
    const int tb = CONV ? 2 * H - 4 * m : 4 * m, p0 = 4 * m - H;
    if (p0 - 3 >= -R && p0 + 3 <= R) {                                    // all sixteen pairs inside the tap row
#pragma unroll
        for (int ee = 0; ee < 4; ee++) {
            const int e = CONV ? 3 - ee : ee;
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int n = 0; n < DCV_NY; n++) acc[n][k] = __builtin_fmaf(tap[tb + (CONV ? k - e + 3 : e - k + 3)], v[n][e], acc[n][k]);
        }
    } else {
#pragma unroll
        for (int ee = 0; ee < 4; ee++) {
            const int e = CONV ? 3 - ee : ee;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int d = p0 + e - k;                                 // +i of the correlation, -i of the convolution
                if (d >= -R && d <= R) {
#pragma unroll
                    for (int n = 0; n < DCV_NY; n++) acc[n][k] = __builtin_fmaf(tap[tb + (CONV ? k - e + 3 : e - k + 3)], v[n][e], acc[n][k]);
                }
            }
        }
    }
}

// the DCV_NY x 4 sums of a thread; CONV: the true convolution of the ratio pass, else the correlation of the update pass.
// H: the halo of the radius class (dcv_halo), H - 8 < R <= H. Per tap row the 2 H + 7 taps are read at once (wide scalar
// loads) and the H / 2 + 1 float4s of the window are expanded in line, so that a row waits once for its loads
template <bool CONV, int H>
__device__ __forceinline__ void dcv_accumulate(const float* tile, const DCV_CONST float* taps, int R, float (&acc)[DCV_NY][4]) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    constexpr int pitch = 2 * H + 8, chunks = H / 2 + 1;                  // (2 H + 4) / 4 float4s per window
    __builtin_assume(R > H - 8 && R <= H);
#pragma unroll
    for (int n = 0; n < DCV_NY; n++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[n][k] = 0.0f;
    for (int jj = 0; jj <= 2 * R; jj++) {                                 // j = jj - R
        const float* row = tile + (CONV ? ty + 2 * R - jj : ty + jj) * DCV_PITCH + 4 * tx;
        const DCV_CONST float* trow = taps + jj * pitch;
        float tap[2 * H + 7];
#pragma unroll
        for (int q = 0; q < 2 * H + 7; q++) tap[q] = trow[q];
#pragma unroll
        for (int mm = 0; mm < chunks; mm++)                               // the convolution walks downwards: i = x - position grows
            dcv_chunk<CONV, H>(row, tap, CONV ? chunks - 1 - mm : mm, R, acc);
    }
}

// (the rows of a launch are strided by the grid: an image may have more rows than 4 x 65535)
template <int CN>
__global__ __launch_bounds__(256) void deconv_init_kernel(DeconvInitArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= a.w) return;
    for (int y = blockIdx.y * 4 + (threadIdx.x >> 6); y < a.h; y += gridDim.y * 4) {
        const DCV_GLOBAL float* p = (const DCV_GLOBAL float*)a.in + (size_t)y * a.in_stride + (size_t)x * CN;
        float v[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) v[c] = p[c];
        DCV_GLOBAL float* D = (DCV_GLOBAL float*)a.D + (size_t)y * a.w + x;
#pragma unroll
        for (int c = 0; c < CC; c++) {
            const float d = v[c] + a.pedestal;
            D[(size_t)c * a.plane] = (__builtin_fabsf(d) < __builtin_inff() && d >= 0.0f) ? d : 0.0f;   // (a NaN fails both tests)
        }
        if constexpr (CN == 4) ((DCV_GLOBAL float*)a.out)[(size_t)y * a.out_stride + (size_t)x * 4 + 3] = v[3];
    }
}

template <int H>
__global__ __launch_bounds__(256) void deconv_ratio_kernel(DeconvPassArgs a) {
    extern __shared__ __align__(16) float dcv_tile[];
    const int X0 = blockIdx.x * DCV_TW, Y0 = blockIdx.y * DCV_TH, R = a.radius;
    const size_t po = (size_t)blockIdx.z * a.plane;
    dcv_stage(dcv_tile, (const DCV_GLOBAL float*)a.src + po, a.w, a.h, X0, Y0, R, H);
    float acc[DCV_NY][4];
    dcv_accumulate<true, H>(dcv_tile, (const DCV_CONST float*)a.taps, R, acc);
    const DCV_GLOBAL float* D = (const DCV_GLOBAL float*)a.D + po;
    DCV_GLOBAL float* dst = (DCV_GLOBAL float*)a.dst + po;
    const int x0 = X0 + 4 * (threadIdx.x & 15);
#pragma unroll
    for (int n = 0; n < DCV_NY; n++) {
        const int y = Y0 + (threadIdx.x >> 4) + 16 * n;
        if (y >= a.h) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = x0 + k;
            if (x < a.w) dst[(size_t)y * a.w + x] = D[(size_t)y * a.w + x] / __builtin_fmaxf(acc[n][k], a.floor);
        }
    }
}

// (px, py) of the regulariser at (x, y), a pixel of the plane
__device__ __forceinline__ void dcv_unit_gradient(const DCV_GLOBAL float* u, int x, int y, int w, int h, float e2, float& px, float& py) {
    const float c = u[(size_t)y * w + x];
    const float gx = x + 1 < w ? u[(size_t)y * w + x + 1] - c : 0.0f;
    const float gy = y + 1 < h ? u[(size_t)(y + 1) * w + x] - c : 0.0f;
    const float n = __builtin_sqrtf(__builtin_fmaf(gx, gx, __builtin_fmaf(gy, gy, e2)));
    px = gx / n;
    py = gy / n;
}

template <bool TV, int H>
__global__ __launch_bounds__(256) void deconv_update_kernel(DeconvPassArgs a) {
    extern __shared__ __align__(16) float dcv_tile[];
    const int X0 = blockIdx.x * DCV_TW, Y0 = blockIdx.y * DCV_TH, R = a.radius;
    const size_t po = (size_t)blockIdx.z * a.plane;
    dcv_stage(dcv_tile, (const DCV_GLOBAL float*)a.src + po, a.w, a.h, X0, Y0, R, H);
    float acc[DCV_NY][4];
    dcv_accumulate<false, H>(dcv_tile, (const DCV_CONST float*)a.taps, R, acc);
    const DCV_GLOBAL float* u = (const DCV_GLOBAL float*)a.u + po;
    const int x0 = X0 + 4 * (threadIdx.x & 15);
#pragma unroll
    for (int n = 0; n < DCV_NY; n++) {
        const int y = Y0 + (threadIdx.x >> 4) + 16 * n;
        if (y >= a.h) continue;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = x0 + k;
            if (x >= a.w) continue;
            const size_t at = (size_t)y * a.w + x;
            float un = u[at] * acc[n][k];
            if constexpr (TV) {
                float px, py, qx = 0.0f, qy = 0.0f, t;
                dcv_unit_gradient(u, x, y, a.w, a.h, a.e2, px, py);
                if (x > 0) dcv_unit_gradient(u, x - 1, y, a.w, a.h, a.e2, qx, t);
                if (y > 0) dcv_unit_gradient(u, x, y - 1, a.w, a.h, a.e2, t, qy);
                const float div = (px - qx) + (py - qy);
                un = un / __builtin_fmaxf(__builtin_fmaf(-a.lambda, div, 1.0f), 0.5f);
            }
            if (!a.last) {
                ((DCV_GLOBAL float*)a.dst)[po + at] = un;
            } else {
                const float D = ((const DCV_GLOBAL float*)a.D)[po + at];
                float m = a.amount;
                if (a.mask) m = a.amount * ((const DCV_GLOBAL float*)a.mask)[(size_t)y * a.mask_stride + x];
                const float o = m == 1.0f ? un - a.pedestal : __builtin_fmaf(m, un - D, D) - a.pedestal;
                ((DCV_GLOBAL float*)a.out)[(size_t)y * a.out_stride + (size_t)x * a.cn + blockIdx.z] = o;
            }
        }
    }
}

bool dcv_pass_ok(const DeconvPassArgs& a, dim3& grid, size_t& lds) {
    if (!a.taps || !a.src || !a.D || a.w <= 0 || a.h <= 0 || a.radius < 1 || a.radius > 16 || a.w < a.radius + 1 || a.h < a.radius + 1 ||
        a.channels < 1 || a.channels > 3 || a.plane < (size_t)a.w * a.h)
        return false;
    grid = dim3((a.w + DCV_TW - 1) / DCV_TW, (a.h + DCV_TH - 1) / DCV_TH, (unsigned)a.channels);
    lds = (size_t)(DCV_TH + 2 * a.radius) * DCV_PITCH * sizeof(float);
    return grid.y <= 65535;
}

}  // namespace

// A missing kernel is an error: every channel count the entry point admits has its instantiation here.
hipError_t launch_deconv_init(const DeconvInitArgs& a, int cn, hipStream_t s) {
    if (!a.in || !a.D || a.w <= 0 || a.h <= 0 || a.in_stride < (size_t)a.w * cn || a.plane < (size_t)a.w * a.h ||
        (cn == 4 && (!a.out || a.out_stride < (size_t)a.w * cn)))
        return hipErrorInvalidValue;
    const dim3 grid((a.w + 63) / 64, (unsigned)((a.h + 3) / 4 < 65535 ? (a.h + 3) / 4 : 65535));
    if (cn == 1) deconv_init_kernel<1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) deconv_init_kernel<3><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) deconv_init_kernel<4><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_deconv_ratio(const DeconvPassArgs& a, hipStream_t s) {
    dim3 grid;
    size_t lds = 0;
    if (!dcv_pass_ok(a, grid, lds) || !a.dst) return hipErrorInvalidValue;
    if (dcv_halo(a.radius) == 8) deconv_ratio_kernel<8><<<grid, 256, lds, s>>>(a);
    else deconv_ratio_kernel<16><<<grid, 256, lds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_deconv_update(const DeconvPassArgs& a, hipStream_t s) {
    dim3 grid;
    size_t lds = 0;
    if (!dcv_pass_ok(a, grid, lds) || !a.u) return hipErrorInvalidValue;
    if (a.last ? (!a.out || a.out_stride < (size_t)a.w * a.cn || (a.cn != 1 && a.cn != 3 && a.cn != 4) || a.channels != (a.cn < 3 ? a.cn : 3) ||
                  (a.mask && a.mask_stride < (size_t)a.w))
               : !a.dst)
        return hipErrorInvalidValue;
    const bool tv = a.lambda > 0.0f;
    if (dcv_halo(a.radius) == 8) {
        if (tv) deconv_update_kernel<true, 8><<<grid, 256, lds, s>>>(a);
        else deconv_update_kernel<false, 8><<<grid, 256, lds, s>>>(a);
    } else {
        if (tv) deconv_update_kernel<true, 16><<<grid, 256, lds, s>>>(a);
        else deconv_update_kernel<false, 16><<<grid, 256, lds, s>>>(a);
    }
    return hipGetLastError();
}

}  // namespace stk

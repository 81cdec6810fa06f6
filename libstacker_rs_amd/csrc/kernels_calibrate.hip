// kernels_calibrate.hip — frame calibration (include/stacker.h, stk_calibration / stk_defect_params): the
// per-pixel pass that applies bias, dark and flat masters to a stack and repairs defective pixels, the stencil pass that
// finds defects in a master, and the per-channel sums of an f32 image.
//
// calibrate_kernel. The masters are the traffic (12 B per pixel each as f32 BGR against 3 B of a u8 frame), so the grid is
// tiles x frame chunks: a workgroup of 256 threads owns a CAL_TW x CAL_TH tile (one pixel per thread) and the frames
// [blockIdx.z * chunk, + chunk). A thread loads its pixel's master values and its map byte ONCE and keeps them in registers
// across the chunk. Defective pixels are rare: one ballot per wave, before the frame loop, decides whether the wave ever
// enters the neighbour path; there a defective lane recomputes the calibrated value of each admissible neighbour from global
// memory (raw sample and masters, the formula of its own pixel, so nothing cascades) and takes the median through a
// 19-comparator network on order-preserving integer keys — no runtime-indexed array, no scratch, no LDS.
// Addresses. A thread forms addresses of its own pixel (x < w, y < h) and of neighbours that passed the in-frame test only;
// frames and outputs are read and written element by element, pixel bytes only (row padding keeps its contents); the map
// is w x h bytes. No atomics here.
//
// defect_map_kernel. An LDS-tiled stencil: DEF_TW x DEF_TH pixels plus a halo of `step` per workgroup, per channel one f32
// plane in LDS; positions outside the master hold 0 and are never ranked (the in-frame test is on the coordinates). Counts:
// one ballot + popcount per wave, row and channel, one integer atomic per wave and channel (integers: any order gives the
// same sums), as kernels_reject.hip does.
//
// image sums. A wave per row, lanes striding the row in f64, a fixed shuffle tree; a second launch adds the rows' partials
// in row order: the order is fixed by the geometry alone.
#include <type_traits>

#include "common.h"

namespace stk {

namespace {

constexpr int CAL_GROUP = 4;                       // frames whose loads a thread keeps in flight
constexpr uint32_t CAL_KEY_NAN = 0xFFFFFFFEu;      // every NaN: above every number
constexpr uint32_t CAL_KEY_ABSENT = 0xFFFFFFFFu;   // no neighbour: above everything

// the total order of the definition as unsigned integers: -inf < .. < -0 < +0 < .. < +inf < NaN
__device__ __forceinline__ uint32_t cal_key(float v) {
    const uint32_t b = __float_as_uint(v);
    if (v != v) return CAL_KEY_NAN;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cal_unkey(uint32_t k) {
    if (k == CAL_KEY_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

#define CAL_CX(i, j) { const uint32_t lo_ = min(k[i], k[j]), hi_ = max(k[i], k[j]); k[i] = lo_; k[j] = hi_; }
// the median rule over the m present keys of k[0 .. 8) (absent slots hold CAL_KEY_ABSENT); m >= 1
__device__ __forceinline__ float cal_median8(uint32_t (&k)[8], int m) {
    CAL_CX(0, 1) CAL_CX(2, 3) CAL_CX(4, 5) CAL_CX(6, 7)
    CAL_CX(0, 2) CAL_CX(1, 3) CAL_CX(4, 6) CAL_CX(5, 7)
    CAL_CX(1, 2) CAL_CX(5, 6) CAL_CX(0, 4) CAL_CX(3, 7)
    CAL_CX(1, 5) CAL_CX(2, 6)
    CAL_CX(1, 4) CAL_CX(3, 6)
    CAL_CX(2, 4) CAL_CX(3, 5)
    CAL_CX(3, 4)
    const int jl = (m - 1) >> 1, jh = m >> 1;
    uint32_t kl = k[0], kh = k[0];
#pragma unroll
    for (int i = 1; i < 8; i++) { if (i == jl) kl = k[i]; if (i == jh) kh = k[i]; }
    const float lo = cal_unkey(kl);
    if (m & 1) return lo;
    return (lo + cal_unkey(kh)) * 0.5f;
}
#undef CAL_CX

// offset k of the eight: raster order without the centre
__device__ __forceinline__ constexpr int cal_dx(int k) { return (k < 4 ? k : k + 1) % 3 - 1; }
__device__ __forceinline__ constexpr int cal_dy(int k) { return (k < 4 ? k : k + 1) / 3 - 1; }

template <typename O>
__device__ __forceinline__ O cal_out(float v) {
    if constexpr (std::is_same<O, float>::value) return v;
    else {
        constexpr float hi = sizeof(O) == 1 ? 255.0f : 65535.0f;
        const float r = __builtin_rintf(v);
        return (O)__builtin_fminf(__builtin_fmaxf(r, 0.0f), hi);       // fmaxf: a NaN gives 0
    }
}

// A frame pointer comes out of the record table, so the compiler cannot tell its address space and would use flat loads and
// stores; the frames and outputs are global memory by the entry point's contract, and these casts say so.
#define CAL_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const CAL_GLOBAL T* cal_src_row(const void* base, size_t byte_offset) {
    return (const CAL_GLOBAL T*)((const CAL_GLOBAL uint8_t*)base + byte_offset);
}
template <typename T>
__device__ __forceinline__ CAL_GLOBAL T* cal_dst_row(void* base, size_t byte_offset) {
    return (CAL_GLOBAL T*)((CAL_GLOBAL uint8_t*)base + byte_offset);
}

// the calibrated, unrepaired value of channel c at (x, y) of a frame, from global memory: the neighbour path
template <typename T, int CN>
__device__ __forceinline__ float cal_value_at(const CalArgs& a, const void* src, int x, int y, int c, float s) {
    const size_t q = (size_t)x * CN + c;
    float v = (float)cal_src_row<T>(src, (size_t)y * a.in_stride)[q];
    if (a.bias) v = v - a.bias[(size_t)y * a.bias_stride + q];
    if (a.dark) { const float d = s * a.dark[(size_t)y * a.dark_stride + q]; v = v - d; }
    if (a.flat) { const float t = v * a.flat_mean[c]; v = t / __builtin_fmaxf(a.flat[(size_t)y * a.flat_stride + q], a.flat_min); }
    return v + a.pedestal;
}

}  // namespace

template <typename T, typename O, int CN>
__global__ __launch_bounds__(256) void calibrate_kernel(CalArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    const int t = threadIdx.x;
    const int x = blockIdx.x * CAL_TW + (t & 63), y = blockIdx.y * CAL_TH + (t >> 6);
    const bool in = x < a.w && y < a.h;
    const int f0 = blockIdx.z * a.chunk, f1 = min(a.n, f0 + a.chunk);
    const int step = a.step;

    // the tile's masters and map byte, once per chunk
    float B[CC], D[CC], F[CC];
    unsigned dm = 0;
    unsigned nb[CC];                      // bit k: neighbour k is inside the frame and its bit of this channel is clear
#pragma unroll
    for (int c = 0; c < CC; c++) { B[c] = 0.0f; D[c] = 0.0f; F[c] = 1.0f; nb[c] = 0; }
    if (in) {
        const size_t q = (size_t)x * CN;
#pragma unroll
        for (int c = 0; c < CC; c++) {
            if (a.bias) B[c] = a.bias[(size_t)y * a.bias_stride + q + c];
            if (a.dark) D[c] = a.dark[(size_t)y * a.dark_stride + q + c];
            if (a.flat) F[c] = __builtin_fmaxf(a.flat[(size_t)y * a.flat_stride + q + c], a.flat_min);
        }
        if (a.defects) dm = a.defects[(size_t)y * a.w + x] & ((1u << CC) - 1u);
        if (dm) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int nx = x + cal_dx(k) * step, ny = y + cal_dy(k) * step;
                if ((unsigned)nx < (unsigned)a.w && (unsigned)ny < (unsigned)a.h) {
                    const unsigned byte = a.defects[(size_t)ny * a.w + nx];
#pragma unroll
                    for (int c = 0; c < CC; c++)
                        if (!((byte >> c) & 1u)) nb[c] |= 1u << k;
                }
            }
        }
    }
    const bool wave_repairs = __ballot(dm != 0) != 0;      // every lane of the wave is here: no lane has left the kernel

    // CAL_GROUP frames at a time: their records and raw samples are all requested before the first of them is stored, so a
    // thread has that many frames' loads in flight (stores may alias loads for all the compiler knows: one frame per
    // iteration would wait out a full memory latency per frame, and the launch would be bound by that, not by bandwidth)
    const CalFrame* __restrict__ table = a.frames;
    for (int g0 = f0; g0 < f1; g0 += CAL_GROUP) {
        CalFrame fr[CAL_GROUP];
        float v[CAL_GROUP][CN];
#pragma unroll
        for (int u = 0; u < CAL_GROUP; u++) fr[u] = table[min(g0 + u, f1 - 1)];
        if (in) {
#pragma unroll
            for (int u = 0; u < CAL_GROUP; u++) {
                const CAL_GLOBAL T* p = cal_src_row<T>(fr[u].src, (size_t)y * a.in_stride) + (size_t)x * CN;
#pragma unroll
                for (int c = 0; c < CN; c++) v[u][c] = (float)p[c];
            }
        }
#pragma unroll
        for (int u = 0; u < CAL_GROUP; u++) {
            if (!in || g0 + u >= f1) continue;                // (a group's tail repeats the last frame's loads and drops them)
#pragma unroll
            for (int c = 0; c < CC; c++) {
                float q = v[u][c];
                if (a.bias) q = q - B[c];
                if (a.dark) { const float d = fr[u].dark_scale * D[c]; q = q - d; }
                if (a.flat) { const float tt = q * a.flat_mean[c]; q = tt / F[c]; }
                v[u][c] = q + a.pedestal;
            }
            if (wave_repairs) {
                if (dm) {
                    const void* src = fr[u].src;
#pragma unroll
                    for (int c = 0; c < CC; c++) {
                        if (!((dm >> c) & 1u) || nb[c] == 0) continue;
                        uint32_t key[8];
#pragma unroll
                        for (int k = 0; k < 8; k++) {
                            key[k] = CAL_KEY_ABSENT;
                            if ((nb[c] >> k) & 1u)
                                key[k] = cal_key(cal_value_at<T, CN>(a, src, x + cal_dx(k) * step, y + cal_dy(k) * step, c, fr[u].dark_scale));
                        }
                        v[u][c] = cal_median8(key, __popc(nb[c]));
                    }
                }
            }
            CAL_GLOBAL O* o = cal_dst_row<O>(fr[u].dst, (size_t)y * a.out_stride) + (size_t)x * CN;
#pragma unroll
            for (int c = 0; c < CN; c++) o[c] = cal_out<O>(v[u][c]);
        }
    }
}

template <typename T, typename O>
static hipError_t calibrate_launch_cn(const CalArgs& a, int cn, dim3 grid, hipStream_t s) {
    if (cn == 1) calibrate_kernel<T, O, 1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) calibrate_kernel<T, O, 3><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) calibrate_kernel<T, O, 4><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// A missing kernel is an error: every (depth, out_depth, channels) the entry point admits has its instantiation here.
hipError_t launch_calibrate(const CalArgs& a, int depth, int out_depth, int cn, hipStream_t s) {
    if (a.n <= 0 || a.chunk <= 0 || a.w <= 0 || a.h <= 0 || !a.frames || (a.step != 1 && a.step != 2)) return hipErrorInvalidValue;
    const dim3 grid((a.w + CAL_TW - 1) / CAL_TW, (a.h + CAL_TH - 1) / CAL_TH, (a.n + a.chunk - 1) / a.chunk);
    if (grid.y > 65535 || grid.z > 65535) return hipErrorInvalidValue;
    if (depth == 8 && out_depth == 8) return calibrate_launch_cn<uint8_t, uint8_t>(a, cn, grid, s);
    if (depth == 8 && out_depth == 32) return calibrate_launch_cn<uint8_t, float>(a, cn, grid, s);
    if (depth == 16 && out_depth == 16) return calibrate_launch_cn<uint16_t, uint16_t>(a, cn, grid, s);
    if (depth == 16 && out_depth == 32) return calibrate_launch_cn<uint16_t, float>(a, cn, grid, s);
    if (depth == 32 && out_depth == 32) return calibrate_launch_cn<float, float>(a, cn, grid, s);
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
struct DefectArgs {
    const float* master;
    size_t stride;
    int w, h;
    int tests;
    float high_abs, low_ratio;
    int step, accumulate;
    uint8_t* map;
    unsigned long long* counts;
};

template <int CN>
__global__ __launch_bounds__(256) void defect_map_kernel(DefectArgs a) {
    constexpr int CC = CN < 3 ? CN : 3;
    __shared__ float sX[CC][(DEF_TH + 4) * (DEF_TW + 4)];
    const int t = threadIdx.x, step = a.step;
    const int RW = DEF_TW + 2 * step, RH = DEF_TH + 2 * step;
    const int x0 = blockIdx.x * DEF_TW, y0 = blockIdx.y * DEF_TH;
    for (int idx = t; idx < RW * RH; idx += 256) {
        const int ry = idx / RW, rx = idx - ry * RW;
        const int gx = x0 - step + rx, gy = y0 - step + ry;
        const bool inside = (unsigned)gx < (unsigned)a.w && (unsigned)gy < (unsigned)a.h;
        const float* p = a.master + (inside ? (size_t)gy * a.stride + (size_t)gx * CN : 0);
#pragma unroll
        for (int c = 0; c < CC; c++) sX[c][idx] = inside ? p[c] : 0.0f;
    }
    __syncthreads();

    const int tx = t & 63, x = x0 + tx;
    unsigned cnt[CC];
#pragma unroll
    for (int c = 0; c < CC; c++) cnt[c] = 0;
#pragma unroll
    for (int r = 0; r < DEF_TH / 4; r++) {
        const int ty = (t >> 6) + 4 * r, y = y0 + ty;
        const bool in = x < a.w && y < a.h;
        unsigned byte = 0;
        if (in) {
            const int centre = (ty + step) * RW + tx + step;
#pragma unroll
            for (int c = 0; c < CC; c++) {
                const float X = sX[c][centre];
                uint32_t key[8];
                int m = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int ddx = cal_dx(k) * step, ddy = cal_dy(k) * step;
                    const bool inside = (unsigned)(x + ddx) < (unsigned)a.w && (unsigned)(y + ddy) < (unsigned)a.h;
                    key[k] = inside ? cal_key(sX[c][centre + ddy * RW + ddx]) : CAL_KEY_ABSENT;
                    m += inside ? 1 : 0;
                }
                bool flag = !(__builtin_fabsf(X) < __builtin_inff());          // NaN and +-inf
                if (m > 0) {
                    const float med = cal_median8(key, m);
                    if (a.tests & 1) flag = flag | (X - med > a.high_abs);
                    if (a.tests & 2) flag = flag | (X < a.low_ratio * med);
                }
                byte |= flag ? (1u << c) : 0u;
            }
            const size_t o = (size_t)y * a.w + x;
            if (a.accumulate) byte |= a.map[o];
            a.map[o] = (uint8_t)byte;
        }
#pragma unroll
        for (int c = 0; c < CC; c++) cnt[c] += (unsigned)__popcll(__ballot((byte >> c) & 1u));
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int c = 0; c < CC; c++)
            if (cnt[c]) atomicAdd(a.counts + c, (unsigned long long)cnt[c]);
    }
}

hipError_t launch_defect_map(const float* master, size_t stride, int w, int h, int cn, int tests, float high_abs, float low_ratio,
                             int step, int accumulate, uint8_t* map, unsigned long long* counts, hipStream_t s) {
    if (!master || !map || !counts || w <= 0 || h <= 0 || (step != 1 && step != 2)) return hipErrorInvalidValue;
    const dim3 grid((w + DEF_TW - 1) / DEF_TW, (h + DEF_TH - 1) / DEF_TH);
    if (grid.y > 65535) return hipErrorInvalidValue;
    const DefectArgs a{master, stride, w, h, tests, high_abs, low_ratio, step, accumulate, map, counts};
    if (cn == 1) defect_map_kernel<1><<<grid, 256, 0, s>>>(a);
    else if (cn == 3) defect_map_kernel<3><<<grid, 256, 0, s>>>(a);
    else if (cn == 4) defect_map_kernel<4><<<grid, 256, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
template <int CN>
__global__ __launch_bounds__(256) void image_row_sums_kernel(const float* __restrict__ image, size_t stride, int w, int h,
                                                             double* __restrict__ partials) {
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= h) return;                                      // the whole wave: y is the wave's
    const float* row = image + (size_t)y * stride;
    double s[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) s[c] = 0.0;
    for (int x = lane; x < w; x += 64) {
#pragma unroll
        for (int c = 0; c < CN; c++) s[c] = s[c] + (double)row[(size_t)x * CN + c];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < CN; c++) s[c] = s[c] + __shfl_down(s[c], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) partials[(size_t)y * 4 + c] = c < CN ? s[c < CN ? c : 0] : 0.0;
    }
}

__global__ __launch_bounds__(64) void image_sums_finish_kernel(const double* __restrict__ partials, int h, double* __restrict__ sums) {
    const int c = threadIdx.x;
    if (c >= 4) return;
    double acc = 0.0;
    for (int y = 0; y < h; y++) acc = acc + partials[(size_t)y * 4 + c];
    sums[c] = acc;
}

hipError_t launch_image_sums(const float* image, size_t stride, int w, int h, int cn, double* partials, double* sums, hipStream_t s) {
    if (!image || !partials || !sums || w <= 0 || h <= 0) return hipErrorInvalidValue;
    const dim3 grid((h + 3) / 4);
    if (cn == 1) image_row_sums_kernel<1><<<grid, 256, 0, s>>>(image, stride, w, h, partials);
    else if (cn == 3) image_row_sums_kernel<3><<<grid, 256, 0, s>>>(image, stride, w, h, partials);
    else if (cn == 4) image_row_sums_kernel<4><<<grid, 256, 0, s>>>(image, stride, w, h, partials);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    image_sums_finish_kernel<<<1, 64, 0, s>>>(partials, h, sums);
    return hipGetLastError();
}

}  // namespace stk

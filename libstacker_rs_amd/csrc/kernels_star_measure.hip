// kernels_star_measure.hip — the shape of every detected star (include/stacker.h, stk_star_measure_params): the
// background ring's exact median and MAD, and the thresholded aperture's zeroth, first and second moments, on the 16-bit key
// of star detection (star_key.h), all in integers behind the key.
//
// One WAVE per star, four stars per 256-thread workgroup (blockIdx.x * 4 + wave = the star of the frame's list, blockIdx.y =
// frame of the launch). A wave works alone: it returns early where its frame has no such star, and there is no workgroup
// barrier anywhere in the kernel.
//   1. the (2 Ro + 1)^2 box of keys around the star (at most 33 x 33) goes to the wave's LDS as u16, lane l taking elements
//      l, l + 64, ... A position outside the frame forms NO address: its key is 0 and is never used. Each lane keeps a bit
//      per element it loaded: inside the frame and inside the ring.
//   2. bg and mad by two selections of lds_select.h at wave scope: a 256-bin histogram in the wave's LDS, four bins per lane.
//      A lane's share is the ring elements it loaded; every key gets an atomic of its own (the direct fill).
//   3. the aperture's sums: per lane in int32 (at most 10 pixels of at most 65535 x 144 each), then wave-shuffle trees on
//      int64; every lane ends with the totals, lane 0 writes the record.
// No global atomics, no floating-point atomics, no scratch.
#include "common.h"
#include "grey.h"
#include "lds_select.h"
#include "star_key.h"

namespace stk {

namespace {

constexpr int SM_RMAX = 12;                                  // largest aperture radius
constexpr int SM_RO_MAX = 16;                                // largest ring radius
constexpr int SM_BOX = 2 * SM_RO_MAX + 1;                    // 33
constexpr int SM_KEYS = (SM_BOX * SM_BOX + 7) & ~7;          // 1096 u16 per wave: the waves' boxes stay 16-byte aligned
constexpr int SM_ITERS = (SM_BOX * SM_BOX + 63) / 64;        // 18 elements per lane at most

template <typename V>
__device__ __forceinline__ V wave_sum(V x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

template <typename T, int CN>
__global__ __launch_bounds__(256) void star_measure_kernel(StarMeasureArgs a, float scale) {
    __shared__ __align__(16) uint16_t s_key[4][SM_KEYS];
    __shared__ __align__(16) int s_hist[4][256];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int frame = blockIdx.y;
    const int j = blockIdx.x * 4 + wv;
    if (j >= a.max_stars || j >= a.counts[frame]) return;                 // the same for the whole wave
    const size_t slot = (size_t)frame * a.max_stars + j;
    const int px = a.stars[2 * slot], py = a.stars[2 * slot + 1];
    const int w = a.w, h = a.h, R = a.radius, Ro = a.ring_outer;
    StarMeasureRecord rec{};
    if (px < R || py < R || px > w - 1 - R || py > h - 1 - R) {           // (the host keeps such a star off the list) no address
        rec.flags = 1;
        if (lane == 0) a.records[slot] = rec;
        return;
    }
    uint16_t* key = s_key[wv];
    int* hist = s_hist[wv];
    *reinterpret_cast<int4*>(&hist[4 * lane]) = make_int4(0, 0, 0, 0);

    // ---- 1. the box: element i <-> (dy, dx) = (i / B - Ro, i % B - Ro)
    const char* __restrict__ src = static_cast<const char*>(a.frames[frame]);
    const int B = 2 * Ro + 1, nbox = B * B;
    const int Ri2 = a.ring_inner * a.ring_inner, Ro2 = Ro * Ro;
    uint32_t ring = 0;                                                    // bit it: element it * 64 + lane is a ring pixel
#pragma unroll 6
    for (int it = 0; it < SM_ITERS; it++) {
        const int i = it * 64 + lane;
        if (i < nbox) {
            const int r = i / B, dy = r - Ro, dx = i - r * B - Ro;
            const int yy = py + dy, xx = px + dx;
            uint32_t g = 0;
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
                g = deep_key<T, CN>(reinterpret_cast<const T*>(src + (size_t)yy * a.stride) + (size_t)xx * CN, scale);
                const int d2 = dx * dx + dy * dy;
                if (d2 >= Ri2 && d2 <= Ro2) ring |= 1u << it;
            }
            key[i] = (uint16_t)g;
        }
    }
    wave_sync();

    // ---- 2. the ring's median and MAD; a lane reads back the elements it wrote
    const int n_ring = wave_sum((int)__popc(ring));
    int bg = 0, mad = 0;
    if (n_ring > 0) {
        const int kth = (n_ring + 1) / 2;
        const WaveSelect sel{hist, lane};
        const uint16_t* own = key + lane;                                 // element it * 64 + lane
        const auto ring_keys = select_share(0, SM_ITERS, 1, [=](int it) { return ((ring >> it) & 1u) != 0; }, [=](int it) { return (int)own[it * 64]; });
        bg = select16<SelectFill::Direct>(sel, ring_keys, SelectKey{}, kth);
        mad = select16<SelectFill::Direct>(sel, ring_keys, SelectAbsDev{bg}, kth);
    }
    const int thr = max((int)fminf(ceilf(a.ks * (float)mad), 65536.0f), a.min_contrast);

    // ---- 3. the aperture: wholly inside the frame (the guard above) and inside the box (R < Ro)
    const int A = 2 * R + 1, nap = A * A, R2 = R * R;
    int npix = 0, peak = 0, S = 0, Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
    for (int i = lane; i < nap; i += 64) {
        const int r = i / A, dy = r - R, dx = i - r * A - R;
        if (dx * dx + dy * dy <= R2) {
            const int g = key[(dy + Ro) * B + dx + Ro];
            peak = max(peak, g);
            const int v = g - bg;
            if (v >= thr) {                                               // thr >= 1: v > 0
                npix++;
                S += v; Sx += v * dx; Sy += v * dy; Sxx += v * dx * dx; Syy += v * dy * dy; Sxy += v * dx * dy;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) peak = max(peak, __shfl_xor(peak, d, 64));
    npix = wave_sum(npix);
    rec.S = wave_sum((long long)S); rec.Sx = wave_sum((long long)Sx); rec.Sy = wave_sum((long long)Sy);
    rec.Sxx = wave_sum((long long)Sxx); rec.Syy = wave_sum((long long)Syy); rec.Sxy = wave_sum((long long)Sxy);
    rec.bg = bg; rec.mad = mad; rec.thr = thr; rec.npix = npix; rec.peak = peak; rec.n_ring = n_ring;
    rec.flags = ((a.saturation > 0 && peak >= a.saturation) ? 2 : 0) | ((npix < a.min_pixels || rec.S == 0) ? 4 : 0);
    if (lane == 0) a.records[slot] = rec;
}

template <typename T>
void measure_launch_cn(int cn, dim3 grid, hipStream_t s, const StarMeasureArgs& a, float scale) {
    if (cn == 1) star_measure_kernel<T, 1><<<grid, 256, 0, s>>>(a, scale);
    else if (cn == 3) star_measure_kernel<T, 3><<<grid, 256, 0, s>>>(a, scale);
    else star_measure_kernel<T, 4><<<grid, 256, 0, s>>>(a, scale);
}

}  // namespace

hipError_t launch_star_measure(const StarMeasureArgs& a, int n, int depth, int cn, float f32_scale, hipStream_t s) {
    if (n <= 0 || n > 65535 || (cn != 1 && cn != 3 && cn != 4) || (depth != 8 && depth != 16 && depth != 32) || a.radius < 2 ||
        a.radius > SM_RMAX || a.ring_inner <= a.radius || a.ring_inner > 15 || a.ring_outer < a.ring_inner || a.ring_outer > SM_RO_MAX ||
        a.max_stars < 1 || a.max_stars > 4096 || a.w <= 0 || a.h <= 0 || a.stride % (size_t)(depth / 8) ||
        a.stride < (size_t)a.w * cn * (depth / 8))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.max_stars + 3) / 4), (unsigned)n);
    if (depth == 8) measure_launch_cn<uint8_t>(cn, grid, s, a, f32_scale);
    else if (depth == 16) measure_launch_cn<uint16_t>(cn, grid, s, a, f32_scale);
    else measure_launch_cn<float>(cn, grid, s, a, f32_scale);
    return hipGetLastError();
}

}  // namespace stk

// kernels_reject.hip — blot-and-compare rejection maps for drizzle (include/stacker.h, stk_reject_params).
// One workgroup of 256 threads owns a 64 x 16 tile of ONE entry's pixel grid (the entry index is blockIdx.z) and runs the
// definition's three stencil levels out of LDS, separated by barriers:
//   1. every lattice point of the tile plus a halo of 2 (68 x 20): the fold's coordinate fragment (warp_coords.inc.h at
//      STK_SUBPIX == 0) with the entry's FORWARD matrix, `valid`, and the bilinear model B_c from the four gathered taps of
//      the clean image, into LDS. The halo is 2 because the first flag is needed one pixel out (the grow step) and needs the
//      gradient, which needs B one pixel further out. Lattice points outside the frame's pixel grid are computed like any
//      other: B is a function of the lattice point.
//   2. the tile plus a halo of 1 (66 x 18): judged, the gradient D_c from LDS, the frame's own sample (read here, once per
//      tile and halo), and BOTH tests, as three bits per point into LDS. A halo point outside the frame is not judged and
//      reads nothing.
//   3. the tile's pixels: the 3 x 3 OR of the first flags, the result, the store, and the counts: one ballot + popcount per
//      wave and row, one integer atomic per wave and counter (integers: any order gives the same sums).
// Every address is inside by construction: C and cnt are read at (ix .. ix + 1, iy .. iy + 1) of valid points only
// (0 <= ix, ix + 1 <= sw - 1, likewise iy); the frame and the maps at 0 <= x < sw, 0 <= y < sh only; LDS indices are those of
// the 68 x 20 and 66 x 18 blocks, the neighbours of a 66 x 18 point lie inside the 68 x 20 block. No floating-point atomics,
// no scratch. The directory compiles with -ffp-contract=off: the only fused operations are the fragment's and the lerp
// chain's.
#include "reject.h"
#include "warp_body.h"

namespace stk {

namespace {
constexpr int BW = REJECT_TW + 4, BH = REJECT_TH + 4;       // the model block: tile + halo 2
constexpr int FW = REJECT_TW + 2, FH = REJECT_TH + 2;       // the flag block: tile + halo 1
constexpr unsigned FLAG_JUDGED = 1, FLAG_FIRST = 2, FLAG_SECOND = 4;
}  // namespace

template <typename T, int CN, bool PERSPECTIVE>
__global__ __launch_bounds__(256) void reject_kernel(RejectArgs ra) {
    __shared__ float sB[CN][BW * BH];
    __shared__ unsigned char sV[BW * BH];
    __shared__ unsigned char sF[FW * FH];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * REJECT_TW, y0 = blockIdx.y * REJECT_TH;
    const RejectEntry* __restrict__ ent = ra.entries + blockIdx.z;
    const WarpFrame* fr = &ent->f;
    const int sw = ra.sw, sh = ra.sh;
    const float* __restrict__ C = ra.clean;
    const int* __restrict__ cnt = ra.counts;

    // 1. valid and B on the tile + 2
    for (int idx = tid; idx < BW * BH; idx += 256) {
        const int by = idx / BW, bx = idx - by * BW;
        const int px = x0 - 2 + bx, py = y0 - 2 + by;
        const float fx = (float)px, fy = (float)py;
        // the fragment reads a.is_affine: a constant here, so that the division exists in the perspective kernels only
        constexpr struct { int is_affine; } a{PERSPECTIVE ? 0 : 1};
#define STK_SUBPIX 0
#include "warp_coords.inc.h"
#undef STK_SUBPIX
        (void)w00; (void)w01; (void)w10; (void)w11;
        bool valid = finite & (ix >= 0) & (ix + 1 <= sw - 1) & (iy >= 0) & (iy + 1 <= sh - 1);
        const size_t p00 = valid ? (size_t)iy * sw + ix : 0, p10 = p00 + sw;
        if (valid && cnt) {
            const int mc = ra.min_count;
            valid = (cnt[p00] >= mc) & (cnt[p00 + 1] >= mc) & (cnt[p10] >= mc) & (cnt[p10 + 1] >= mc);
        }
        if (valid) {
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const float c00 = C[p00 * CN + c], c01 = C[(p00 + 1) * CN + c];
                const float c10 = C[p10 * CN + c], c11 = C[(p10 + 1) * CN + c];
                const float t0 = __builtin_fmaf(ax, c01 - c00, c00);
                const float t1 = __builtin_fmaf(ax, c11 - c10, c10);
                sB[c][idx] = __builtin_fmaf(ay, t1 - t0, t0);
            }
        }
        sV[idx] = valid ? 1 : 0;
    }
    __syncthreads();

    // 2. judged and the two tests on the tile + 1
    const T* __restrict__ src = (const T*)fr->src;
    const float* __restrict__ min_ = ent->map_in;
    const float alpha = ra.alpha;
    for (int idx = tid; idx < FW * FH; idx += 256) {
        const int gy = idx / FW, gx = idx - gy * FW;
        const int x = x0 - 1 + gx, y = y0 - 1 + gy;
        const int b = (gy + 1) * BW + (gx + 1);
        bool judged = (sV[b] != 0) & ((unsigned)x < (unsigned)sw) & ((unsigned)y < (unsigned)sh);
        if (judged && min_) judged = min_[(size_t)y * sw + x] > 0.0f;
        unsigned flags = 0;
        if (judged) {
            const bool vl = sV[b - 1] != 0, vr = sV[b + 1] != 0, vu = sV[b - BW] != 0, vd = sV[b + BW] != 0;
            const T* __restrict__ p = src + (size_t)y * ra.src_stride + (size_t)x * CN;
            bool first = false, second = false;
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const float B = sB[c][b];
                float D = 0.0f;
                if (vl) D = __builtin_fmaxf(D, __builtin_fabsf(sB[c][b - 1] - B));
                if (vr) D = __builtin_fmaxf(D, __builtin_fabsf(sB[c][b + 1] - B));
                if (vu) D = __builtin_fmaxf(D, __builtin_fabsf(sB[c][b - BW] - B));
                if (vd) D = __builtin_fmaxf(D, __builtin_fabsf(sB[c][b + BW] - B));
                const float u = ((float)p[c] * alpha) * ent->gain[c] + ent->offset[c];
                const float e = __builtin_fabsf(u - B);
                const float sigma = __builtin_sqrtf(ra.rn2 + ra.pg * __builtin_fmaxf(B, 0.0f));
                first = first | (e > ra.scale1 * D + ra.snr1 * sigma);
                second = second | (e > ra.scale2 * D + ra.snr2 * sigma);
            }
            flags = FLAG_JUDGED | (first ? FLAG_FIRST : 0u) | (second ? FLAG_SECOND : 0u);
        }
        sF[idx] = (unsigned char)flags;
    }
    __syncthreads();

    // 3. grow, the result, the counts
    const int tx = tid & 63, x = x0 + tx;
    float* __restrict__ mout = ent->map_out;
    unsigned n_rej = 0, n_jud = 0;              // (lane 0's are the wave's)
#pragma unroll
    for (int r = 0; r < REJECT_TH / 4; r++) {
        const int ty = (tid >> 6) + 4 * r, y = y0 + ty;
        const int f = (ty + 1) * FW + (tx + 1);
        const unsigned fl = sF[f];
        const unsigned around = sF[f - FW - 1] | sF[f - FW] | sF[f - FW + 1] | sF[f - 1] | fl | sF[f + 1] |
                                sF[f + FW - 1] | sF[f + FW] | sF[f + FW + 1];
        const bool judged = (fl & FLAG_JUDGED) != 0;
        const bool rej = judged & (((fl & FLAG_FIRST) != 0) | (((around & FLAG_FIRST) != 0) & ((fl & FLAG_SECOND) != 0)));
        if (x < sw && y < sh) {                  // (a judged point is inside the frame)
            const size_t o = (size_t)y * sw + x;
            const float keep = min_ ? min_[o] : 1.0f;
            mout[o] = rej ? 0.0f : keep;
        }
        n_rej += (unsigned)__popcll(__ballot(rej));
        n_jud += (unsigned)__popcll(__ballot(judged));
    }
    if ((tid & 63) == 0) {
        if (n_rej) atomicAdd(ra.tallies + 2 * (size_t)blockIdx.z, (unsigned long long)n_rej);
        if (n_jud) atomicAdd(ra.tallies + 2 * (size_t)blockIdx.z + 1, (unsigned long long)n_jud);
    }
}

template <typename T, int CN>
static void reject_launch(const RejectArgs& a, dim3 grid, hipStream_t s) {
    if (a.is_affine) reject_kernel<T, CN, false><<<grid, 256, 0, s>>>(a);
    else reject_kernel<T, CN, true><<<grid, 256, 0, s>>>(a);
}

// A missing kernel is an error: every depth and channel count the entry point admits has its instantiation here.
hipError_t launch_reject(const RejectArgs& a, int depth, hipStream_t s) {
    if (a.n_entries <= 0 || a.n_entries > 65535 || a.sw <= 0 || a.sh <= 0 || !a.entries || !a.clean || !a.tallies)
        return hipErrorInvalidValue;
    const dim3 grid((a.sw + REJECT_TW - 1) / REJECT_TW, (a.sh + REJECT_TH - 1) / REJECT_TH, a.n_entries);
    if (grid.y > 65535) return hipErrorInvalidValue;
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) { reject_launch<decltype(t), decltype(ch)::value>(a, grid, s); });
}

}  // namespace stk

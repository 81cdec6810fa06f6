// kernels_local_norm.hip — local normalisation (include/stacker.h, "Local normalisation"): the cell moments
// pass, and the launches of the two folds whose gain and offset come from a node grid (FoldNorm<CN> / FoldStoreNorm<CN>:
// the weighted mean and the store with participation over the plane source, warp_body.h).
//
// The moments pass. One wave owns one (cell, entry): blockIdx.x * 4 + wave = the cell in row-major order, blockIdx.y + 1 =
// the table entry. Its lanes walk the cell's stepped pixels (x % step == 0, y % step == 0) lane-strided in row-major order;
// per pixel a lane samples entry 0 and then the entry with the generic fold's own text (warp_coords.inc.h,
// warp_linear_sample.inc.h: the LINEAR sample whatever the context's interpolation — these are statistics, not an image)
// and adds the six terms per channel to private f64 sums where kappa == 1.0f. An xor-shuffle tree over the wave follows
// and lane 0 writes the cell's record. No partials buffer, no second kernel, no LDS, no atomics: the order of the additions
// is fixed by the geometry, the cell size and the step alone. Every address is formed by the fragments' in-frame logic
// from a destination pixel inside the destination; the record is addressed by (entry, cell), both checked against the
// launch.
#include "warp_cubic_body.h"

namespace stk {

// FoldMoments' sums (MomentSums, warp_body.h: wants_kappa is all it asks of the sample fragment) without the stepped-grid
// bookkeeping and its mask: every pixel the wave visits is a stepped pixel of the cell.
template <int CN> struct CellMoments : MomentSums<CN, false> {};

template <typename T, int CN>
__global__ __launch_bounds__(256) void local_moments_kernel(WarpArgs a, ClipArgs ca) {
    const int lane = threadIdx.x & 63;
    const int cell = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= ca.cell_w * ca.cell_h) return;                       // (the whole wave)
    const int J = cell / ca.cell_w, K = cell - J * ca.cell_w;
    const int side = 1 << ca.cell_shift, st = ca.step;
    const int xa = K << ca.cell_shift, ya = J << ca.cell_shift;
    const int xb = min(xa + side, a.dw), yb = min(ya + side, a.dh);
    // the cell's stepped columns are st * [sx0, sx1), its stepped rows st * [sy0, sy1)
    const int sx0 = (xa + st - 1) / st, sx1 = (xb + st - 1) / st;
    const int sy0 = (ya + st - 1) / st, sy1 = (yb + st - 1) / st;
    const int nx = sx1 - sx0, npix = nx * (sy1 - sy0);
    CellMoments<CN> cs;
    cs.zero();
    const int mode = a.border_mode;
    for (int i = lane; i < npix; i += 64) {
        const int ry = i / nx, rx = i - ry * nx;
        const int px = (sx0 + rx) * st, py = (sy0 + ry) * st;       // < a.dw, < a.dh
        const float fx = (float)px, fy = (float)py;
        for (int f = 0; f < 2; f++) {
            const WarpFrame* fr = a.frames + f * (1 + (int)blockIdx.y);
            const T* __restrict__ src = (const T*)fr->src;
#define STK_SUBPIX a.subpixel_bits
#define STK_SAMPLE(c, v) cs.add(c, v)
#include "warp_coords.inc.h"
#include "warp_linear_sample.inc.h"
#undef STK_SAMPLE
#undef STK_SUBPIX
        }
    }
    // every lane of the wave is here: lanes without a pixel carry zeros
#pragma unroll
    for (int k = 0; k < CellMoments<CN>::NM; k++) {
        double v = cs.S[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
        cs.S[k] = v;
    }
    if (lane == 0) {
        double* o = ca.cells + ((size_t)blockIdx.y * ((size_t)ca.cell_w * ca.cell_h) + cell) * (CN * 6);
#pragma unroll
        for (int c = 0; c < CN; c++) {
            o[c * 6] = cs.S[0];
#pragma unroll
            for (int k = 1; k <= 5; k++) o[c * 6 + k] = cs.S[k + 5 * c];
        }
    }
}

hipError_t launch_local_moments(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames < 2 || a.n_frames - 1 > 65535 || !c.cells || c.step < 1 || c.cell_shift < 3 || c.cell_shift > 8) return hipErrorInvalidValue;
    const int side = 1 << c.cell_shift;
    if (c.cell_w != (a.dw + side - 1) / side || c.cell_h != (a.dh + side - 1) / side) return hipErrorInvalidValue;
    const dim3 grid(((unsigned)c.cell_w * c.cell_h + 3) / 4, (unsigned)(a.n_frames - 1));
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        local_moments_kernel<decltype(t), decltype(ch)::value><<<grid, 256, 0, s>>>(a, c);
    });
}

// The locally normalised mean over the frames of `a`: the generic kernels, linear or cubic. The u8 BGR fast kernels do not
// serve these states (they have no add2 / add3k): a matter of these two launchers, not of the states' traits.
hipError_t launch_norm_fold(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (!norm_args_ok(a, c) || !c.out) return hipErrorInvalidValue;
    const dim3 grid((a.dw + 63) / 64, (a.dh + 3) / 4);
    if (a.interp == STK_INTER_CUBIC) return launch_warp_cubic<true, FoldNorm>(a, c, depth, grid, s);
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        warp_accumulate_kernel<decltype(t), CN, true, FoldNorm<CN>><<<grid, 256, 0, s>>>(a, c);
    });
}

// The locally normalised store launch for the band c.y0 .. c.y0 + c.band_rows (a.dh = its end; c.norm_gh is the whole
// destination's, hence the >= above).
hipError_t launch_norm_store(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (!norm_args_ok(a, c) || !c.band || c.band_rows <= 0) return hipErrorInvalidValue;
    const dim3 grid((a.dw + 63) / 64, (c.band_rows + 3) / 4);
    if (a.interp == STK_INTER_CUBIC) return launch_warp_cubic<true, FoldStoreNorm>(a, c, depth, grid, s);
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        warp_accumulate_kernel<decltype(t), CN, true, FoldStoreNorm<CN>><<<grid, 256, 0, s>>>(a, c);
    });
}

}  // namespace stk

// kernels_weighted.hip — the weighted, coverage-aware mean over the aligned frames and the overlap moments its
// normalisation is estimated from (stk_weighted_stack, stk_overlap_moments and the *_weighted entry points; definition in
// include/stacker.h, stk_weight_params). Both are modes of the fold kernels of warp_body.h, so the sample they see is the
// mean's by construction:
//   * the weighted fold: FoldWeighted<CN> in the generic kernel and in the u8 BGR fast kernel. Per sample, over the mean's
//     work: two multiplies and two adds per channel plus one add for den (interior path), and kappa's lerp chain and two
//     more multiplies on the rim. One launch, the result written once;
//   * the moments pass: FoldMoments<CN> in the generic kernel (every depth; its samples are the fast kernel's bit for
//     bit), grid z = entry - 1. A thread walks `reps` stepped rows of one entry privately in f64 before its wave reduces by
//     lane shuffles and writes one partial; moments_reduce_kernel then adds an entry's partials in index order. The order
//     of every addition is fixed by the geometry and the step alone: the same bits on every call. No atomics.
#include "fold_launch.h"

namespace stk {

// one workgroup per entry, one thread per moment: partials in index order (four loads in flight, added in order)
__global__ __launch_bounds__(64) void moments_reduce_kernel(const double* __restrict__ partials, size_t parts, int nm, int cn,
                                                            double* __restrict__ moments) {
    const int k = threadIdx.x;
    if (k >= nm) return;
    const double* p = partials + (size_t)blockIdx.x * parts * nm + k;
    double s = 0.0;
    size_t i = 0;
    for (; i + 4 <= parts; i += 4) {
        const double v0 = p[i * nm], v1 = p[(i + 1) * nm], v2 = p[(i + 2) * nm], v3 = p[(i + 3) * nm];
        s = s + v0; s = s + v1; s = s + v2; s = s + v3;
    }
    for (; i < parts; i++) s = s + p[i * nm];
    // partial layout: n, then per channel (sum X, sum Y, sum X^2, sum Y^2, sum XY); output: per channel (n, the five sums)
    double* o = moments + (size_t)blockIdx.x * cn * 6;
    if (k == 0) { for (int c = 0; c < cn; c++) o[c * 6] = s; }
    else o[((k - 1) / 5) * 6 + 1 + (k - 1) % 5] = s;
}

hipError_t launch_weighted_fold(const WarpArgs& a, const ClipArgs& c, int depth, hipStream_t s) {
    if (a.n_frames <= 0) return hipErrorInvalidValue;
    return launch_fold<FoldWeighted<3>, FoldWeighted>(a, c, depth, a.dh, s);
}

hipError_t launch_overlap_moments(const WarpArgs& a, ClipArgs c, int depth, int step, double* moments, hipStream_t s) {
    if (a.n_frames < 2 || step < 1) return hipErrorInvalidValue;
    const MomentsPlan p = moments_plan(a.dw, a.dh, step);
    c.step = step; c.reps = p.reps;
    const dim3 grid(p.bx, p.by, a.n_frames - 1);
    hipError_t e;
    if (a.interp == STK_INTER_CUBIC) e = launch_warp_cubic<true, FoldMoments>(a, c, depth, grid, s);
    else e = dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        warp_accumulate_kernel<decltype(t), CN, true, FoldMoments<CN>><<<grid, 256, 0, s>>>(a, c);
    });
    if (e != hipSuccess) return e;
    moments_reduce_kernel<<<a.n_frames - 1, 64, 0, s>>>(c.partials, p.parts(), 1 + 5 * a.cn, a.cn, moments);
    return hipGetLastError();
}

}  // namespace stk

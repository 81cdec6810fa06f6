// fold_launch.h — the one launcher of the combines whose fold has a u8 BGR fast state (host side): the sigma-clipping
// passes (kernels_clip.hip), the weighted mean (kernels_weighted.hip) and the quantile store launches
// (kernels_quantile.hip). Which kernel a combine runs is decided here and nowhere else:
//   cubic,  u8 BGR  -> warp_accumulate_cubic_u8c3_kernel<AFFINE, 2, true, FastState>
//   cubic,  generic -> warp_accumulate_cubic_kernel<T, CN, true, State<CN>>
//   linear, u8 BGR  -> warp_accumulate_u8c3_kernel<AFFINE, 1, 4, true, FastState>: the mean fold's default launch shape
//                      (one wave per row of 64 pixels, four frames in flight)
//   linear, generic -> warp_accumulate_kernel<T, CN, true, State<CN>>
// with (T, CN) from the one ladder (dispatch_depth_cn, warp_body.h). `rows`: the destination rows of the launch — a.dh for
// a whole-image pass, c.band_rows for a store launch (whose states declare in_band: their kernels start at c.y0).
// What a kernel does for a state follows from the state's traits (FoldTraits, warp_body.h), not from this launcher. That
// the fast kernels never run FoldNorm / FoldStoreNorm is a property of the launchers (kernels_local_norm.hip launches the
// generic kernels itself; those states have no add2 / add3k, so naming them here would not compile), not of the traits.
#pragma once
#include "warp_cubic_body.h"

namespace stk {

template <class FastState, template <int> class State>
hipError_t launch_fold(const WarpArgs& a, const ClipArgs& c, int depth, int rows, hipStream_t s) {
    const dim3 grid((a.dw + 63) / 64, (rows + 3) / 4);
    if (a.interp == STK_INTER_CUBIC) {
        if (warp_u8c3_applies(a, depth)) return launch_warp_cubic_u8c3<true, FastState>(a, c, grid, s);
        return launch_warp_cubic<true, State>(a, c, depth, grid, s);
    }
    if (warp_u8c3_applies(a, depth)) {
        if (a.is_affine) warp_accumulate_u8c3_kernel<true, 1, 4, true, FastState><<<grid, 256, 0, s>>>(a, c);
        else warp_accumulate_u8c3_kernel<false, 1, 4, true, FastState><<<grid, 256, 0, s>>>(a, c);
        return hipGetLastError();
    }
    return dispatch_depth_cn(depth, a.cn, [&](auto t, auto ch) {
        constexpr int CN = decltype(ch)::value;
        warp_accumulate_kernel<decltype(t), CN, true, State<CN>><<<grid, 256, 0, s>>>(a, c);
    });
}

}  // namespace stk

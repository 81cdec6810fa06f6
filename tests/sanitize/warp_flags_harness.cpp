// warp_flags_harness.cpp — warp_frame_flags (common.h) on the host: WARPFRAME_SRC_ALIGNED4 must be set exactly for frames
// whose base address AND row stride are multiples of 4. The flag selects the dword-window gathers of the u8 / u16 warp
// kernels, which tell the compiler that their addresses are dword-aligned (__builtin_assume_aligned). On hardware that
// performs unaligned dword loads a wrongly set flag still gathers the right bytes — window start and shift are both taken
// relative to the frame's base — so no comparison of results can see it; the predicate itself is checked here. Also the
// range flag: set for an ordinary homography, clear for one whose W crosses zero inside the destination, never for affine.
#include "hip_stubs.h"

#include <cstdio>

#include "../../libstacker_rs_amd/csrc/common.h"

int main() {
    alignas(16) static unsigned char buf[64];
    const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const float cross[9] = {1, 0, 0, 0, 1, 0, -0.02f, 0, 1};            // W = 1 - 0.02 x changes sign at x = 50
    for (int off = 0; off < 8; off++)
        for (size_t stride : {960u, 961u, 962u, 963u, 964u, 1005u, 1008u, 2010u, 2016u}) {
            const bool want = off % 4 == 0 && stride % 4 == 0;
            for (int affine = 0; affine < 2; affine++) {
                const int f = stk::warp_frame_flags(buf + off, I, stride, 320, 237, affine);
                if (((f & stk::WARPFRAME_SRC_ALIGNED4) != 0) != want) { std::printf("aligned flag: offset %d stride %zu affine %d -> %d\n", off, stride, affine, f); return 1; }
                if (((f & stk::WARPFRAME_DIV_IN_RANGE) != 0) != (affine == 0)) { std::printf("range flag: affine %d -> %d\n", affine, f); return 2; }
            }
            if (stk::warp_frame_flags(buf + off, cross, stride, 320, 237, 0) & stk::WARPFRAME_DIV_IN_RANGE) { std::printf("range flag set for a W that crosses zero\n"); return 3; }
        }
    std::printf("ok\n");
    return 0;
}

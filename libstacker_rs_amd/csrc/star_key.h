// star_key.h — the 16-bit integer key of star detection and star measurement (include/stacker.h, stk_star_deep_params): one
// definition for kernels_star_deep.hip and kernels_star_measure.hip. Device code only.
#pragma once
#include "common.h"
#include "grey.h"

namespace stk {

__device__ __forceinline__ uint32_t key_f32(float gf, float scale) {
    return (uint32_t)(int)fminf(fmaxf(rintf(gf * scale), 0.0f), 65535.0f);     // fmaxf(NaN, 0) = 0
}

// the key of the pixel whose first element is p[0]
template <typename T, int CN>
__device__ __forceinline__ uint32_t deep_key(const T* p, float scale) {
    if constexpr (sizeof(T) == 1) { if constexpr (CN == 1) return p[0]; else return grey_u8(p[0], p[1], p[2]); }
    else if constexpr (sizeof(T) == 2) { if constexpr (CN == 1) return p[0]; else return grey_u16(p[0], p[1], p[2]); }
    else { if constexpr (CN == 1) return key_f32(p[0], scale); else return key_f32(grey_f32(p[0], p[1], p[2]), scale); }
}

}  // namespace stk

// grey.h — cvt_color(BGR2GRAY) on 8-bit pixels (utils.rs:136-142): the one device function every kernel that makes
// an 8-bit grey shares (kernels_prep.hip: grey, grey_blur; kernels_quality.hip: the whole-stack sharpness pass).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace stk {

__device__ __forceinline__ uint8_t grey_u8(unsigned b, unsigned g, unsigned r) {
    return (uint8_t)((b * 3735u + g * 19235u + r * 9798u + (1u << 14)) >> 15);
}

}  // namespace stk

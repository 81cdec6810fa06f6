// grey.h — cvt_color(BGR2GRAY) (utils.rs:136-142): the device functions every kernel that makes a grey shares
// (kernels_prep.hip: grey, grey_blur; kernels_quality.hip: the whole-stack sharpness pass; kernels_star.hip and
// kernels_star_deep.hip: the detection's grey and key).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace stk {

__device__ __forceinline__ uint8_t grey_u8(unsigned b, unsigned g, unsigned r) {
    return (uint8_t)((b * 3735u + g * 19235u + r * 9798u + (1u << 14)) >> 15);
}

// the same on 16-bit pixels (kernels_prep.hip's grey kernels; kernels_star_deep.hip's key)
__device__ __forceinline__ uint16_t grey_u16(unsigned b, unsigned g, unsigned r) {
    return (uint16_t)((b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14);
}
__device__ __forceinline__ float grey_f32(float b, float g, float r) {
    return b * 0.114f + g * 0.587f + r * 0.299f;   // -ffp-contract=off: three roundings, as the oracle
}

}  // namespace stk

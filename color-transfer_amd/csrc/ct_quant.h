// ct_quant.h -- the float32 -> uint8 rule of ct_pack_u8_f32 (pack.hip) for every kernel that writes bytes:
//   q = rint(clamp(x, 0, 1) * 255)
//   - ONE float32 multiplication by 255.0f (the Makefile's -ffp-contract=off keeps it out of an fma; no reciprocal),
//   - round to nearest, ties to even (v_rndne_f32),
//   - NaN, -inf and negatives -> 0;  +inf and values above 1 -> 255.
// Device inline functions only.
#pragma once
#include <hip/hip_runtime.h>

namespace ct {

__device__ __forceinline__ unsigned int quant_u8(float x) {
    // fmaxf(NaN, 0) = 0 (the non-NaN operand); -0.0f * 255 rounds to -0.0f, which converts to 0
    const float c = fminf(fmaxf(x, 0.0f), 1.0f);
    return (unsigned int)__builtin_rintf(c * 255.0f);
}

__device__ __forceinline__ unsigned int pack4(unsigned int a, unsigned int b, unsigned int c, unsigned int d) {
    return a | (b << 8) | (c << 16) | (d << 24);
}

}  // namespace ct

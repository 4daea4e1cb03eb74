// ct_split16.h -- float32 as TWO fp16 pieces (hi + lo, 11 + 11 mantissa bits) with a power-of-two scale, and the three-MFMA
// product of two split operands: the default arithmetic of the hot MFMA kernels (conv_split.hip, conv_ws.hip, conv_wino.hip,
// conv_wino4.hip, linear_ws16.hip, attention16.hip).  Device inline functions and typedefs only: attention16.hip includes this
// file without ct_common.h.  The wave maximum that picks a scale is ct_wave.h's wave_max_nonneg.
#pragma once
#include <hip/hip_runtime.h>
#include "ct_wave.h"

namespace ct {

typedef float f32x16 __attribute__((ext_vector_type(16)));    // one 32x32 MFMA accumulator
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// opaque to the compiler (it otherwise re-derives each half with v_fma_mixlo_f16 when the halves are converted back)
__device__ __forceinline__ unsigned int sp16_cvt_pk(float a, float b) {
    unsigned int r;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// two values at once, packed (x0 in the low half)
__device__ __forceinline__ void sp16_split2x2(float x0, float x1, unsigned int &hw, unsigned int &lw) {
    hw = sp16_cvt_pk(x0, x1);
    const f16x2 h = __builtin_bit_cast(f16x2, hw);
    lw = sp16_cvt_pk(x0 - (float)h.x, x1 - (float)h.y);
}
// eight consecutive floats -> the two 16-byte fp16 fragments (hi, lo)
__device__ __forceinline__ void sp16_split2x8(const float (&x)[8], uint4 &h, uint4 &l) {
    unsigned int hw[4], lw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sp16_split2x2(x[2 * i], x[2 * i + 1], hw[i], lw[i]);
    h = make_uint4(hw[0], hw[1], hw[2], hw[3]); l = make_uint4(lw[0], lw[1], lw[2], lw[3]);
}
// s += A . B with A, B given as (hi, lo) fragments: three v_mfma_f32_32x32x16_f16, small terms first
__device__ __forceinline__ void sp16_mfma3(f32x16 &s, const uint4 (&a)[2], const uint4 (&b)[2]) {
    const f16x8 ah = __builtin_bit_cast(f16x8, a[0]), al = __builtin_bit_cast(f16x8, a[1]);
    const f16x8 bh = __builtin_bit_cast(f16x8, b[0]), bl = __builtin_bit_cast(f16x8, b[1]);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, s, 0, 0, 0);
}
// exponent e with 2^e * mx in [2^11, 2^12); `none` for mx == 0 / denormal (no constraint); 0 for inf / NaN (they propagate)
__device__ __forceinline__ int sp16_scale_exp(float mx, int none) {
    const int fld = (int)(__float_as_uint(mx) >> 23);                  // biased exponent (mx >= 0)
    const int ex = fld == 0 ? none : fld == 255 ? 0 : 138 - fld;       // 12 - (floor(log2 mx) + 1)
    return min(max(ex, -100), 100);
}
__device__ __forceinline__ float sp16_pow2i(int e) { return __uint_as_float((unsigned int)(127 + e) << 23); }   // |e| <= 126

}  // namespace ct

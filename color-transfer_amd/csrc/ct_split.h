// ct_split.h -- device code shared by the MFMA kernels: float32 -> three bf16 pieces (hi + mid + lo) and the six-MFMA product of
// two split operands (conv_split.hip, conv_ws.hip, linear_tokens.hip, attention_tokens.hip), and the epilogue functions
// (activation switch, branch-free GELU) of the convolutions and the token linears.  The two-piece fp16 form is ct_split16.h,
// the wave reductions are ct_wave.h; this file includes both.
#pragma once
#include <hip/hip_runtime.h>
#include "ct_split16.h"      // f32x16, the fp16 two-piece primitives, ct_wave.h

namespace ct {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Activation codes of ConvArgs / GConvArgs.  GEN = false: the DCMCS3DI instantiations, which only know LeakyReLU(0.01) -- the
// full switch in the epilogue costs them 1.5 % (measured r01)
template <bool GEN>
__device__ __forceinline__ float act(float v, int code) {
    if (!GEN) return v > 0.f ? v : 0.01f * v;
    switch (code) {
        case 1: return v > 0.f ? v : 0.01f * v;
        case 2: return v > 0.f ? v : 0.f;
        case 3: return 1.0f / (1.0f + expf(-v));
        case 4: return tanhf(v);
        case 5: return v / (1.0f + expf(-v));        // swish (efficientnet_pytorch MemoryEfficientSwish)
        default: return v;
    }
}

// GELU(v) = v Phi(v) with erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7 absolute, i.e. float32 rounding level of
// the result; branch free: one v_rcp_f32, one v_exp_f32, seven FMAs) instead of the library erff (two branches, both of
// which a wave executes) -- the epilogue of the 1024-wide FFN layer evaluates it 16384 times per workgroup.
__device__ __forceinline__ float gelu_as(float v) {
    const float z = fabsf(v) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(z * z * -1.4426950408889634f);
    const float erfc_half = 0.5f * p * t * e;                       // erfc(z) / 2
    return v > 0.f ? v - v * erfc_half : v * erfc_half;           // v Phi(v), Phi(-z sqrt2) = erfc(z) / 2
}

// x -> (hi, mid, lo) bf16 bit patterns; hi + mid + lo == x up to 2^-24 relative.  NaN stays NaN; an infinity becomes
// (inf, NaN, NaN), i.e. an infinite activation yields NaN outputs where the f32 kernel yields +-inf / NaN.
__device__ __forceinline__ void split3(float x, unsigned int &h, unsigned int &m, unsigned int &l) {
    const __bf16 bh = (__bf16)x;
    const float r1 = x - (float)bh;
    const __bf16 bm = (__bf16)r1;
    const float r2 = r1 - (float)bm;
    const __bf16 bl = (__bf16)r2;
    h = __builtin_bit_cast(unsigned short, bh);
    m = __builtin_bit_cast(unsigned short, bm);
    l = __builtin_bit_cast(unsigned short, bl);
}

// two values at once, packed (x0 in the low half): one v_cvt_pk_bf16_f32 per piece, halves re-expanded by shift / mask
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned int pack_bf16(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ void split3x2(float x0, float x1, unsigned int &hw, unsigned int &mw, unsigned int &lw) {
    hw = pack_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(hw << 16), r1 = x1 - __uint_as_float(hw & 0xffff0000u);
    mw = pack_bf16(r0, r1);
    lw = pack_bf16(r0 - __uint_as_float(mw << 16), r1 - __uint_as_float(mw & 0xffff0000u));
}
// eight consecutive floats -> the three 16-byte bf16 fragments (hi, mid, lo)
__device__ __forceinline__ void split3x8(const float (&x)[8], uint4 &h, uint4 &m, uint4 &l) {
    unsigned int hw[4], mw[4], lw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3x2(x[2 * i], x[2 * i + 1], hw[i], mw[i], lw[i]);
    h = make_uint4(hw[0], hw[1], hw[2], hw[3]); m = make_uint4(mw[0], mw[1], mw[2], mw[3]); l = make_uint4(lw[0], lw[1], lw[2], lw[3]);
}
// s += A . B with A, B given as (hi, mid, lo) fragments: six v_mfma_f32_32x32x16_bf16, small terms first
__device__ __forceinline__ void mfma_split6(f32x16 &s, const uint4 (&a)[3], const uint4 (&b)[3]) {
    const bf16x8 ah = __builtin_bit_cast(bf16x8, a[0]), am = __builtin_bit_cast(bf16x8, a[1]), al = __builtin_bit_cast(bf16x8, a[2]);
    const bf16x8 bh = __builtin_bit_cast(bf16x8, b[0]), bm = __builtin_bit_cast(bf16x8, b[1]), bl = __builtin_bit_cast(bf16x8, b[2]);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, s, 0, 0, 0);
}

}  // namespace ct

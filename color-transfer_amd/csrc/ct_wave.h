// ct_wave.h -- reductions over one wave of 64 lanes: the DPP maximum and sum, the fixed-shape __shfl_down sum tree and the
// __shfl_xor all-reduces.  Device inline functions only (no kernel, no host state): any source may include it, attention16.hip
// included (ct_env.h explains why that file stays clear of ct_common.h).
// A kernel that still writes one of these loops out is one whose compiled code the helper call would have changed.
#pragma once
#include <hip/hip_runtime.h>

namespace ct {

// DPP row operations reduce the 64 lanes in six steps without LDS traffic: shifts by 1, 2, 4, 8 inside the rows of 16 lanes,
// then the row results broadcast into the next rows.
//   0x111 row_shr:1
//   0x112 row_shr:2
//   0x114 row_shr:4
//   0x118 row_shr:8    -> lane 15 of every row holds its row's result
//   0x142 row_bcast:15 into rows 1 and 3 (row mask 0xa)
//   0x143 row_bcast:31 into rows 2 and 3 (row mask 0xc) -> lane 63 holds the wave's result
// max over the wave of a non-negative float (such floats order like their bit patterns); valid in lane 63 only
__device__ __forceinline__ float wave_max_nonneg_lane63(float v) {
    int x = __float_as_int(v);
#define CT_DPP_MAX(ctrl, rmask) x = max(x, __builtin_amdgcn_update_dpp(0, x, ctrl, rmask, 0xf, false))
    CT_DPP_MAX(0x111, 0xf); CT_DPP_MAX(0x112, 0xf); CT_DPP_MAX(0x114, 0xf); CT_DPP_MAX(0x118, 0xf);
    CT_DPP_MAX(0x142, 0xa); CT_DPP_MAX(0x143, 0xc);
#undef CT_DPP_MAX
    return __int_as_float(x);
}
// the same; every lane returns it
__device__ __forceinline__ float wave_max_nonneg(float v) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_max_nonneg_lane63(v)), 63));
}
// float32 sum over the wave, same six steps (a fixed tree): six v_add_f32; the total is returned wave-uniform.  Accuracy: six
// roundings of 6e-8 relative, unbiased.
__device__ __forceinline__ float wave_sum_f32(float v) {
#define CT_DPP_ADD(ctrl, rmask) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rmask, 0xf, true))
    CT_DPP_ADD(0x111, 0xf); CT_DPP_ADD(0x112, 0xf); CT_DPP_ADD(0x114, 0xf); CT_DPP_ADD(0x118, 0xf);
    CT_DPP_ADD(0x142, 0xa); CT_DPP_ADD(0x143, 0xc);
#undef CT_DPP_ADD
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// fixed-shape __shfl_down tree (double, float, unsigned long long): the same summation order on every run; valid in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// NV values at once, in place: one step of the tree for all of them, then the next
template <typename T, int NV>
__device__ __forceinline__ void wave_sum(T (&v)[NV]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] += __shfl_down(v[i], off, 64);
    }
}
// __shfl_xor butterflies: every lane returns the sum / the maximum (fmaxf drops a NaN operand)
template <typename T>
__device__ __forceinline__ T wave_all_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_all_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

}  // namespace ct

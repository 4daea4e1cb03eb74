// ct_minmax.h -- the per-frame min / max of a float32 map through integer atomics: what views.hip and errmaps.hip share.
// A workgroup reduces its lanes (wave shuffles, four waves through LDS), then folds ONE pair into the frame's two keys with
// atomicMin / atomicMax on an order-preserving integer image of the float.  min and max do not depend on the order of their
// operands: the result is deterministic.
#pragma once
#include "ct_common.h"

namespace ct {

// ---- order-preserving integer image of a float32 --------------------------------------------------------------------------------
// a < b as floats  <=>  key(a) < key(b) as unsigned (negative numbers: all bits flipped, others: sign bit set); -0 sorts below +0
__device__ __forceinline__ unsigned int float_key(float f) {
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// min / max of the workgroup's lanes; the result is valid in thread 0.  fminf / fmaxf drop a NaN operand.
__device__ __forceinline__ void block_min_max(float &lo, float &hi, float *lds /* [2][4] */) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off, kWave));
        hi = fmaxf(hi, __shfl_down(hi, off, kWave));
    }
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x >> 6;
    if (lane == 0) { lds[wid] = lo; lds[4 + wid] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(lds[0], lds[1]), fminf(lds[2], lds[3]));
        hi = fmaxf(fmaxf(lds[4], lds[5]), fmaxf(lds[6], lds[7]));
    }
}

// keys[2 b] = key(+inf), keys[2 b + 1] = key(-inf): the neutral elements of the two atomics
static __global__ void minmax_init_kernel(unsigned int *__restrict__ keys, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * n) keys[i] = (i & 1) ? 0x007fffffu : 0xff800000u;
}

}  // namespace ct

// ct_bytes.h -- uint8 frames in 16-byte loads, for every kernel that reads interleaved RGB bytes (linear_u8.hip, idt.hip).
// Frame b of a batch starts at b * 3 * n_pixels bytes, off the 16-byte grid for most sizes: a frame is its first h < 16 pixels
// (3 h = -base mod 16), runs of 16 pixels = 48 bytes = three 16-byte loads, and a tail of < 16 pixels.
// Device inline functions only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ct_quant.h"

namespace ct {

// pixels in front of the first 16-byte boundary that is also a pixel boundary: 3 h = -base (mod 16), 3 * 11 = 1 (mod 16)
__device__ __forceinline__ int head_pixels(uintptr_t base, int64_t n_pixels) {
    const int h = (11 * (int)((16 - (base & 15)) & 15)) & 15;
    return (int64_t)h < n_pixels ? h : (int)n_pixels;
}
__device__ __forceinline__ int head_pixels(const uint8_t *p, int64_t n_pixels) { return head_pixels(reinterpret_cast<uintptr_t>(p), n_pixels); }

__device__ __forceinline__ unsigned int byte_of(const unsigned int (&w)[12], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

__device__ __forceinline__ void load48(const uint8_t *p, unsigned int (&w)[12]) {   // p on the 16-byte grid
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
    const uint4 a = q[0], b = q[1], c = q[2];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
}

__device__ __forceinline__ void load48_bytes(const uint8_t *p, unsigned int (&w)[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) w[i] = pack4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
}

}  // namespace ct

// ct_bytes.h -- uint8 frames in 16-byte loads, for every kernel that reads interleaved RGB bytes (linear_u8.hip, idt.hip), and
// the float64 image that the bytes stand for (idt.hip, regrain.hip).
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

// ---- the image behind the bytes ----------------------------------------------------------------------------------------------
// The bytes of a frame stand for one of two float64 images, chosen per call: entry k of a 256-entry table in LDS is
// (double)((float)k / 255.0f) (input_f32: the float32 tensor a Runner makes of a frame) or (double)k / 255.0 (img_as_float).  A
// kernel instantiated for uint8_t runs the float kernel's statements on the table's values: bitwise the float entry on that image.
template <typename T> struct IsU8 { static constexpr bool v = false; };
template <> struct IsU8<uint8_t> { static constexpr bool v = true; };

// by the first 256 threads of the workgroup (all256: the workgroup has no others, no guard is compiled); the caller's next
// barrier publishes it
__device__ __forceinline__ void fill_u8_table(double *tab, int input_f32, bool all256 = false) {
    const unsigned int k = all256 ? threadIdx.x & 255 : threadIdx.x;
    if (all256 || k < 256) tab[k] = input_f32 ? (double)((float)k / 255.0f) : (double)k / 255.0;
}

// element e of an image of T as float64
template <typename T> __device__ __forceinline__ double ld_u8(const T *p, size_t e, const double *tab) {
    if constexpr (IsU8<T>::v) return tab[p[e]];
    else return p[e];
}

}  // namespace ct

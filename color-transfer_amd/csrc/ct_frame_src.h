// ct_frame_src.h -- where a frame metric reads its pixels: the compile-time frame sources of ssim_tile_kernel, icid_tile_kernel
// (metrics.hip) and fsim_prep_kernel (fsim.hip).  The arithmetic behind a source exists once; a kernel instantiated on another
// source runs the same statements in the same order on the values the source hands out (-ffp-contract=off), so
//   metric<ResultHwcF32, GtHwcU8>(a, b)  is bitwise  metric<PlanarF32, PlanarF32>(clamp(a, 0, 1) as NCHW, float32(b) / 255 as NCHW).
// A source is built per frame from (batch base, frame index, H, W, the workgroup's byte table) and hands out
//   at(c, o)      channel c of pixel o = y * W + x
//   at3(o, v)     the three channels of pixel o (HWC: side by side in memory, one 12-byte / 3-byte run)
// Device inline code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ct {

// entry k = (float)k / 255.0f, IEEE division (no reciprocal): the float32 tensor a loader makes of a byte.  By the first 256
// threads of the workgroup, like fill_u8_table (ct_bytes.h); the caller's next barrier publishes it.
__device__ __forceinline__ void fill_u8_table_f32(float *tab /* LDS [256] */) {
    const unsigned int k = threadIdx.x;
    if (k < 256) tab[k] = (float)k / 255.0f;
}

// torch.clamp(v, 0, 1): a NaN stays a NaN (both comparisons are false), which fminf / fmaxf would drop
__device__ __forceinline__ float clamp01_keep_nan(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// [batch][3][H][W] float32, read as is
struct PlanarF32 {
    typedef float elem;
    static constexpr bool kHwc = false, kTable = false;
    const float *p;
    size_t P;
    __device__ __forceinline__ PlanarF32(const float *base, int img, int H, int W, const float *) : p(base + (size_t)img * 3 * H * W), P((size_t)H * W) {}
    __device__ __forceinline__ float at(int c, size_t o) const { return p[(size_t)c * P + o]; }
    __device__ __forceinline__ void at3(size_t o, float (&v)[3]) const { v[0] = p[o]; v[1] = p[P + o]; v[2] = p[2 * P + o]; }
};

// [batch][H][W][3] float32 (a transfer's result), clamped to [0, 1] as it is read
struct ResultHwcF32 {
    typedef float elem;
    static constexpr bool kHwc = true, kTable = false;
    const float *p;
    __device__ __forceinline__ ResultHwcF32(const float *base, int img, int H, int W, const float *) : p(base + (size_t)img * 3 * H * W) {}
    __device__ __forceinline__ float at(int c, size_t o) const { return clamp01_keep_nan(p[3 * o + c]); }
    __device__ __forceinline__ void at3(size_t o, float (&v)[3]) const {
        const float *q = p + 3 * o;
        const float r = q[0], g = q[1], b = q[2];
        v[0] = clamp01_keep_nan(r); v[1] = clamp01_keep_nan(g); v[2] = clamp01_keep_nan(b);
    }
};

// [batch][H][W][3] uint8 (the ground truth of a frame group): byte k stands for tab[k] = (float)k / 255.0f
struct GtHwcU8 {
    typedef uint8_t elem;
    static constexpr bool kHwc = true, kTable = true;
    const uint8_t *p;
    const float *tab;
    __device__ __forceinline__ GtHwcU8(const uint8_t *base, int img, int H, int W, const float *table) : p(base + (size_t)img * 3 * H * W), tab(table) {}
    __device__ __forceinline__ float at(int c, size_t o) const { return tab[p[3 * o + c]]; }
    __device__ __forceinline__ void at3(size_t o, float (&v)[3]) const {
        const uint8_t *q = p + 3 * o;
        const unsigned int r = q[0], g = q[1], b = q[2];
        v[0] = tab[r]; v[1] = tab[g]; v[2] = tab[b];
    }
};

}  // namespace ct

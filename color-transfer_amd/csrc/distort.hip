// distort.hip -- the deterministic colour distortions of the reference's artificial test set (utils/data.py:12-22,120-125:
// identity + {brightness, contrast, saturation, hue, gamma} x 6 magnitudes applied to the uint8 ground-truth frame), on gfx950.
//
// The reference calls torchvision.transforms.functional.adjust_* on uint8 CHW tensors.  torchvision is third-party and
// absent offline: the arithmetic below restates its tensor backend (torchvision/transforms/_functional_tensor.py: _blend,
// rgb_to_grayscale, adjust_*, _rgb2hsv, _hsv2rgb, convert_image_dtype) operation by operation in float32, including the
// truncating float -> uint8 casts -- "parity unpinned" (oracle/distort.py is the same restatement in torch).
//
// in: uint8 [3][H][W] (what torchvision.io.read_image returns).  out_u8 (optional): the distorted uint8 frame; out_f32
// (optional): that frame / 255 as float32 [3][H][W] -- the `target / 255` the dataset hands to the model
// (utils/data.py:125).  One elementwise sweep; contrast needs the mean of the grey image first (exact integer sum).
#include "ct_common.h"
#include "ct_distort.h"

namespace ct {

__global__ __launch_bounds__(kBlock) void gray_sum_kernel(const uint8_t *__restrict__ in, int64_t n, unsigned long long *__restrict__ sum) {
    __shared__ unsigned long long red[4];
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        s += (unsigned long long)gray_u8((float)in[i], (float)in[n + i], (float)in[2 * n + i]);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum, red[0] + red[1] + red[2] + red[3]);   // integer: order independent, exact
}

__global__ __launch_bounds__(kBlock) void distort_kernel(const uint8_t *__restrict__ in, int64_t n, int kind, float param, float one_minus,
                                                         const unsigned long long *__restrict__ gray_sum, uint8_t *__restrict__ out_u8,
                                                         float *__restrict__ out_f32) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float r = (float)in[i], g = (float)in[n + i], b = (float)in[2 * n + i];
    const float mean = kind == kDistContrast ? gray_mean(gray_sum[0], n) : 0.f;
    distort_pixel(kind, param, one_minus, mean, r, g, b);
    if (out_u8) { out_u8[i] = (uint8_t)r; out_u8[n + i] = (uint8_t)g; out_u8[2 * n + i] = (uint8_t)b; }
    if (out_f32) { out_f32[i] = r / 255.f; out_f32[n + i] = g / 255.f; out_f32[2 * n + i] = b / 255.f; }
}

}  // namespace ct

extern "C" {

// kind: 0 identity, 1 brightness (param = factor), 2 contrast, 3 saturation, 4 hue (param = hue_factor in [-0.5, 0.5]), 5 gamma.
// ws: >= 8 bytes, 8-byte aligned (the integer grey sum of the contrast distortion).
int ct_distort_u8(const uint8_t *in, int height, int width, int kind, double param, uint8_t *out_u8, float *out_f32, void *ws,
                  size_t ws_bytes, void *stream) {
    if (!in || height < 1 || width < 1 || kind < 0 || kind > 5 || (!out_u8 && !out_f32)) return CT_E_BADARG;
    if (kind == ct::kDistHue && !(param >= -0.5 && param <= 0.5)) return CT_E_BADARG;        // torchvision raises ValueError
    if ((kind == ct::kDistBrightness || kind == ct::kDistContrast || kind == ct::kDistSaturation || kind == ct::kDistGamma) && param < 0.0)
        return CT_E_BADARG;
    if (!ws || ws_bytes < 8 || (reinterpret_cast<uintptr_t>(ws) & 7)) return CT_E_WORKSPACE;
    const int64_t n = (int64_t)height * width;
    hipStream_t s = (hipStream_t)stream;
    if (kind == ct::kDistContrast) {
        { const int zr = ct::zero_async(ws, 8, s); if (zr) return zr; }
        const int blocks = (int)((n + ct::kBlock * 8 - 1) / (ct::kBlock * 8));
        hipLaunchKernelGGL(ct::gray_sum_kernel, dim3(blocks < 256 ? blocks : 256), dim3(ct::kBlock), 0, s, in, n, (unsigned long long *)ws);   // one same-address atomic per workgroup: keep them few
        CT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ct::distort_kernel, dim3((unsigned)((n + ct::kBlock - 1) / ct::kBlock)), dim3(ct::kBlock), 0, s, in, n, kind, (float)param,
                       (float)(1.0 - param), (const unsigned long long *)ws, out_u8, out_f32);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"

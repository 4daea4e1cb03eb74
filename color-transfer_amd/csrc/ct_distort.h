// ct_distort.h -- the per-pixel arithmetic of torchvision's uint8 colour adjustments (torchvision/transforms/_functional_tensor.py
// restated, see distort.hip), shared by the whole-frame distortions (distort.hip) and the training / validation augmentation chain
// (augment.hip): both must give the same bits for the same operation.
#pragma once
#include "ct_common.h"

namespace ct {

enum { kDistIdentity = 0, kDistBrightness = 1, kDistContrast = 2, kDistSaturation = 3, kDistHue = 4, kDistGamma = 5, kDistSharpness = 6 };

__device__ __forceinline__ float gray_u8(float r, float g, float b) {           // rgb_to_grayscale(...).to(uint8): truncation
    return truncf(0.2989f * r + 0.587f * g + 0.114f * b);
}
// _blend(...).clamp(0, 255).to(uint8); ratio and 1 - ratio are Python floats (float64) in torchvision, each rounded to
// float32 when it meets the tensor -- 1 - ratio is therefore formed in float64 on the host (one_minus), not as 1.0f - ratio
__device__ __forceinline__ float blend_u8(float a, float b, float ratio, float one_minus) {
    return truncf(fminf(fmaxf(ratio * a + one_minus * b, 0.f), 255.f));
}
__device__ __forceinline__ float to_u8(float x) { return truncf(x * 255.999f); }  // convert_image_dtype(float -> uint8): mul(255 + 1 - 1e-3)

// one pointwise adjustment of a pixel whose channels hold uint8 values; mean: torch.mean of the uint8 grey image in float32 (read
// for contrast only).  Any other kind (identity; sharpness is no pointwise operation) leaves the pixel as it is.
__device__ __forceinline__ void distort_pixel(int kind, float param, float one_minus, float mean, float &r, float &g, float &b) {
    if (kind == kDistBrightness) {
        r = blend_u8(r, 0.f, param, one_minus); g = blend_u8(g, 0.f, param, one_minus); b = blend_u8(b, 0.f, param, one_minus);
    } else if (kind == kDistContrast) {
        r = blend_u8(r, mean, param, one_minus); g = blend_u8(g, mean, param, one_minus); b = blend_u8(b, mean, param, one_minus);
    } else if (kind == kDistSaturation) {
        const float l = gray_u8(r, g, b);
        r = blend_u8(r, l, param, one_minus); g = blend_u8(g, l, param, one_minus); b = blend_u8(b, l, param, one_minus);
    } else if (kind == kDistGamma) {
        r = to_u8(fminf(fmaxf(powf(r / 255.f, param), 0.f), 1.f));
        g = to_u8(fminf(fmaxf(powf(g / 255.f, param), 0.f), 1.f));
        b = to_u8(fminf(fmaxf(powf(b / 255.f, param), 0.f), 1.f));
    } else if (kind == kDistHue) {
        r /= 255.f; g /= 255.f; b /= 255.f;
        // _rgb2hsv
        const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
        const bool eqc = maxc == minc;
        const float cr = maxc - minc;
        const float s = cr / (eqc ? 1.f : maxc);
        const float div = eqc ? 1.f : cr;
        const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
        const float hr = (maxc == r) ? (bc - gc) : 0.f;
        const float hg = ((maxc == g) && (maxc != r)) ? (2.0f + rc - bc) : 0.f;
        const float hb = ((maxc != g) && (maxc != r)) ? (4.0f + gc - rc) : 0.f;
        float h = fmodf((hr + hg + hb) / 6.0f + 1.0f, 1.0f);
        // h = (h + hue_factor) % 1.0  (python / torch remainder: result has the sign of the divisor)
        h = h + param;
        h = h - floorf(h);
        // _hsv2rgb
        const float v = maxc;
        const float h6 = h * 6.0f;
        const float fi = floorf(h6);
        const float f = h6 - fi;
        int idx = (int)fi % 6;
        idx = idx < 0 ? idx + 6 : idx;
        const float p = fminf(fmaxf(v * (1.0f - s), 0.f), 1.f);
        const float q = fminf(fmaxf(v * (1.0f - (s * f)), 0.f), 1.f);
        const float t = fminf(fmaxf(v * (1.0f - (s * (1.0f - f))), 0.f), 1.f);
        // rows of the reference's selection tensors: (v,q,p,p,t,v), (t,v,v,q,p,p), (p,p,t,v,v,q) indexed by idx
        r = to_u8(idx == 0 || idx == 5 ? v : idx == 1 ? q : idx == 4 ? t : p);
        g = to_u8(idx == 1 || idx == 2 ? v : idx == 0 ? t : idx == 3 ? q : p);
        b = to_u8(idx == 3 || idx == 4 ? v : idx == 2 ? t : idx == 5 ? q : p);
    }
}

// the grey-sum to mean step of adjust_contrast: an exact integer sum, divided in float64 and rounded to float32 once
__device__ __forceinline__ float gray_mean(unsigned long long sum, int64_t n) { return (float)((double)sum / (double)n); }

}  // namespace ct

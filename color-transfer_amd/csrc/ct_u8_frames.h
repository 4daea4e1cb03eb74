// ct_u8_frames.h -- what the entries on uint8 frame groups share ("bytes in, bytes out": ct_mk_u8, ct_idt_u8, ct_regrain_u8,
// ct_acg_u8): what their last launch writes, the term of their metric and the rule for their output arguments.  The per-byte
// device helpers (the 16-byte walk, the table of the image behind the bytes) are ct_bytes.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ct_hip.h"

namespace ct {

// What the LAST launch of an entry writes: any of the float64 result, that value rounded once to float32, its bytes by
// ct_quant.h's rule, and per workgroup one float64 partial sum of sq_err over the float32 values, added per thread in pixel order
// and then by block_sum's fixed tree.
struct U8Sinks {
    double *f64;         // [batch][n_pixels][3] or NULL
    float *f32;          // likewise
    uint8_t *u8;         // likewise
    const uint8_t *gt;   // likewise
    double *sq;          // [batch][partials per frame: the entry's], written when gt is given
};

// one term of the metric: (clamp(float32 result, 0, 1) - gt)^2 in float64, gt the float32 k / 255 (IEEE division: the
// reference's .float() / 255).  A NaN result stays NaN (torch.clamp keeps it too).  gt is a callable -- a table lookup or the
// division itself -- so that it is evaluated after the clamp, where every kernel has it: a value argument would move it in front,
// and the compiler then schedules the kernels around it differently.
template <typename G> __device__ __forceinline__ double sq_err(float v, G &&gt) {
    const float c = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    const double d = (double)c - (double)gt();
    return d * d;
}

// the output arguments of an entry: at least one output, gt needs psnr_out, float64 / float32 / psnr_out on their own grids
static inline int check_u8_outputs(const void *gt, const double *out_f64, const float *out_f32, const uint8_t *out_u8, const double *psnr_out) {
    if (!out_f64 && !out_f32 && !out_u8) return CT_E_BADARG;
    if (gt && !psnr_out) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(out_f64) & 7) || (reinterpret_cast<uintptr_t>(out_f32) & 3) || (reinterpret_cast<uintptr_t>(psnr_out) & 7))
        return CT_E_ALIGN;
    return CT_OK;
}

}  // namespace ct

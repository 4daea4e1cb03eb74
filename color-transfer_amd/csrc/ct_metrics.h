// ct_metrics.h -- host-side interface of metrics.hip for the sources whose entries end in a PSNR: the two launches of the
// per-frame PSNR (a kernel can only be launched from the source that defines it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ct {

// float64 partial sums of (a - b)^2 over `batch` frames of n elements: partials[frame][kMaxBlocksPerImage], *n_blocks of
// them written per frame.  Returns CT_OK or a HIP error.
int launch_sqerr_partials(const float *a, const float *b, int64_t n, int batch, double *partials, int *n_blocks, hipStream_t s);

// out[frame] = {mse, PSNR} from the first n_blocks <= stride of partials[frame][stride] (launch_sqerr_partials' or an apply
// sweep's: stride kMaxBlocksPerImage; the regrain's last launch: its own workgroup count), added in a fixed order
int launch_psnr_finish(const double *partials, int n_blocks, int stride, int64_t n, int batch, double *out, hipStream_t s);

}  // namespace ct

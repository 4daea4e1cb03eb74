// losses.hip -- the step losses the reference logs beside its metrics (methods/dmsct.py:118-131: mse_loss and kornia's
// ssim_loss(window_size=11); methods/dcmcs3di.py adds l1_loss), per frame, on gfx950.
//
// kornia.losses.ssim_loss with reduction="mean" is mean(clamp((1 - ssim_map) / 2, 0, 1)) over batch, channels and positions, with the
// per-channel map of kornia.metrics.ssim: the map of the rgbssim view (ct_ssim_map.h, restated from kornia's published source --
// "parity unpinned").  F.l1_loss and F.mse_loss are the means of |a - b| and (a - b)^2.
//
// One pass: a workgroup owns a 64 x 32 tile of one frame and stages it (plus the halo) channel by channel for the SSIM map, so the
// two plain losses read their differences from the staged tile and a and b are read from memory once.  Differences, squares and the
// map are float32 like the reference's torch code; every value is widened to float64 before it is added.  A workgroup leaves
// three float64 partial sums, a finishing kernel adds a frame's partials in a fixed order: deterministic, no atomics.
#include "ct_common.h"
#include "ct_ssim_map.h"

namespace ct {
namespace em {

constexpr int kLossLds = (2 * kSH * kSW + 5 * kSH * kTW) * (int)sizeof(float) + 4 * 3 * (int)sizeof(double);
static_assert(kLossLds <= 80 * 1024 && ((2 * kSH * kSW + 5 * kSH * kTW) * sizeof(float)) % sizeof(double) == 0, "two workgroups per CU; aligned sums");

// grid (tiles_x, tiles_y, batch); partials [batch][tiles_y][tiles_x][3]
__global__ __launch_bounds__(kBlock) void frame_losses_tile_kernel(const float *__restrict__ a, const float *__restrict__ b, int H, int W, int vec,
                                                                   Taps taps, double *__restrict__ partials) {
    extern __shared__ vf4 loss_smem[];                      // 16-byte aligned base
    float *sx = reinterpret_cast<float *>(loss_smem), *sy = sx + kSH * kSW, *hb = sy + kSH * kSW;
    double *red = reinterpret_cast<double *>(hb + 5 * kSH * kTW);
    const int ox = blockIdx.x * kTW, oy = blockIdx.y * kTH;
    const int64_t plane = (int64_t)H * W;
    const int col = threadIdx.x & (kTW - 1), r0 = (threadIdx.x >> 6) * kStrip;
    const bool in_x = ox + col < W;
    double acc[3] = {0.0, 0.0, 0.0};                        // sum |d|, sum d^2, sum of the SSIM loss map
    for (int ch = 0; ch < 3; ++ch) {
        const int64_t off = ((int64_t)blockIdx.z * 3 + ch) * plane;
        stage_plane(a + off, sx, H, W, oy, ox, vec);
        stage_plane(b + off, sy, H, W, oy, ox, vec);
        __syncthreads();                                    // also: the previous channel's column pass has left hb
#pragma unroll
        for (int j = 0; j < kStrip; ++j) {
            if (in_x && oy + r0 + j < H) {
                const int at = (r0 + j + kRad) * kSW + col + kLeft;
                const float d = sx[at] - sy[at];
                acc[0] += (double)fabsf(d);
                acc[1] += (double)(d * d);
            }
        }
        ssim_rows(sx, sy, hb, taps);
        __syncthreads();                                    // the next channel may overwrite sx / sy from here on
        float v[kStrip];
        ssim_columns(hb, taps, r0, col, v);
#pragma unroll
        for (int j = 0; j < kStrip; ++j)
            if (in_x && oy + r0 + j < H) acc[2] += (double)fminf(fmaxf((1.0f - v[j]) / 2.0f, 0.0f), 1.0f);
    }
    block_sum<3>(acc, red);
    if (threadIdx.x == 0) {
        double *p = partials + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3;
        p[0] = acc[0]; p[1] = acc[1]; p[2] = acc[2];
    }
}

// out[frame][q] = (sum of the frame's per_frame partials of quantity q) / count; grid = batch
__global__ __launch_bounds__(kBlock) void frame_losses_finish_kernel(const double *__restrict__ partials, int per_frame, double count,
                                                                     double *__restrict__ out) {
    __shared__ double red[4 * 3];
    const double *p = partials + (size_t)blockIdx.x * per_frame * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < per_frame; i += kBlock) { s[0] += p[3 * i]; s[1] += p[3 * i + 1]; s[2] += p[3 * i + 2]; }
    block_sum<3>(s, red);
    if (threadIdx.x == 0) {
        out[blockIdx.x * 3] = s[0] / count; out[blockIdx.x * 3 + 1] = s[1] / count; out[blockIdx.x * 3 + 2] = s[2] / count;
    }
}

}  // namespace em
}  // namespace ct

extern "C" {

size_t ct_frame_losses_workspace_bytes(int batch, int h, int w) {
    using namespace ct::em;
    if (batch < 1 || h < 1 || w < 1) return 0;
    return (size_t)batch * ((h + kTH - 1) / kTH) * ((w + kTW - 1) / kTW) * 3 * sizeof(double);
}

int ct_frame_losses_f32(const float *a, const float *b, double *out, void *ws, size_t ws_bytes, int batch, int h, int w, void *stream) {
    using namespace ct::em;
    if (!a || !b || !out || batch < 1 || batch > 65535) return CT_E_BADARG;
    if (h <= kRad || w <= kRad) return CT_E_BADARG;          // reflect padding of 5 needs more than 5 pixels
    const dim3 grid((w + kTW - 1) / kTW, (h + kTH - 1) / kTH, batch);
    if (grid.y > 65535u) return CT_E_BADARG;                 // more than two million rows
    if (!ws || ws_bytes < ct_frame_losses_workspace_bytes(batch, h, w) || reinterpret_cast<uintptr_t>(ws) % sizeof(double)) return CT_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) % sizeof(float) || reinterpret_cast<uintptr_t>(out) % sizeof(double))
        return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    static ct::DynLdsAttr attr;
    if (attr.ensure(reinterpret_cast<const void *>(frame_losses_tile_kernel), kLossLds) != hipSuccess) return CT_E_BADARG;
    // every row of every plane starts on 16 bytes when the bases do and the width is a whole number of them
    const int vec = w % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    hipLaunchKernelGGL(frame_losses_tile_kernel, grid, dim3(ct::kBlock), kLossLds, s, a, b, h, w, vec, ssim_taps(), reinterpret_cast<double *>(ws));
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(frame_losses_finish_kernel, dim3(batch), dim3(ct::kBlock), 0, s, reinterpret_cast<const double *>(ws),
                       (int)(grid.x * grid.y), (double)h * w * 3.0, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"

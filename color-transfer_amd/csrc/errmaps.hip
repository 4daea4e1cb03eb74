// errmaps.hip -- the three error maps of the reference's utils/visualizations.py that rest on kornia, on gfx950:
//   ct_view_ssim_map_f32  visualizations.py:55-60  rgbssim: 0.5 - ssim(x, y, window_size=11).mean(dim=1) / 2, min-max scaled
//   ct_view_lab_map_f32   visualizations.py:39-52  labmse / abmse: the channel mean of rgb_to_lab(square(x - y)), min-max scaled
// kornia is third-party and absent offline: kornia.metrics.ssim (11-tap Gaussian of sigma 1.5, separable, reflect padding, C1 =
// 0.01^2, C2 = 0.03^2, eps = 1e-12 on the denominator) and kornia.color.rgb_to_lab (ct_color.h) are restated from their published
// sources -- "parity unpinned" for those two calls; the reference's own lines run with the restatements plugged in
// (tests/golden/make_golden_errmaps.py).
//
// An SSIM value costs two 11-tap passes over five moment maps: it is computed ONCE.  Each producing kernel stores the unscaled
// map into channel 0 of the output and folds its workgroup's min / max into the frame's two keys (ct_minmax.h); one small
// kernel, shared by the three maps, then rewrites channel 0 in place as (m - lo) / (hi - lo) and zeroes channels 1 and 2.  The
// scaling pass reads exactly the floats the reduction saw: every frame spans [0, 1] exactly.  All arithmetic is float32 (the
// Makefile's -ffp-contract=off: every fused product here is an explicit fmaf).
#include "ct_color.h"
#include "ct_common.h"
#include "ct_minmax.h"
#include "ct_ssim_map.h"

namespace ct {
namespace em {

// ---- SSIM map ---------------------------------------------------------------------------------------------------------------------
// One workgroup per 64 x 32 output tile of one frame, the three channels one after the other:
//   stage     the tile of x and y plus the 5-pixel halo, reflect applied to the indices at load time.  The staged columns start 8
//             left of the tile, so that with w % 4 == 0 every run of four is one aligned 16-byte load (80 columns = 20 runs, three
//             unused columns on either side); runs that touch the frame's edge, and every run of a ragged width, go element by
//             element.
//   rows      the horizontal 11-tap pass: the five moments mu1, mu2, E[x^2], E[y^2], E[xy] of 42 rows x 64 columns into LDS; a
//             wave reads 64 consecutive floats per tap (no bank conflict).
//   columns   the vertical pass: a thread owns 8 consecutive rows of one column and walks the 18 moment rows under them once,
//             5 * 18 / 8 = 11.25 LDS reads per output instead of 55; every output adds its taps in ascending order.
// LDS budget: x and y 2 * 42 * 80 * 4 = 26,880 B, the moments 5 * 42 * 64 * 4 = 53,760 B, 32 B for the min / max: 80,672 B, more
// than the 64 KB a static array may have (dynamic LDS, raised once per device), and two workgroups = 8 waves per CU in its
// 160 KB.  A 32 x 32 tile would stay under 64 KB with three workgroups per CU, but loads 1.72 pixels per output pixel instead of
// 1.52 and runs the row pass over 1.31 rows per output row in tiles half as wide for the column pass's 8-row strips.
__global__ __launch_bounds__(kBlock) void ssim_map_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out, int n,
                                                          int H, int W, int vec, Taps taps, unsigned int *__restrict__ keys) {
    extern __shared__ vf4 em_smem[];                        // 16-byte aligned base
    float *sx = reinterpret_cast<float *>(em_smem), *sy = sx + kSH * kSW, *hb = sy + kSH * kSW, *red = hb + 5 * kSH * kTW;
    const int ox = blockIdx.x * kTW, oy = blockIdx.y * kTH;
    const int64_t plane = (int64_t)H * W;
    const int col = threadIdx.x & (kTW - 1), r0 = (threadIdx.x >> 6) * kStrip;
    for (int b = blockIdx.z; b < n; b += gridDim.z) {
        float sum[kStrip];                                  // the channels' SSIM values, added in their order
        for (int ch = 0; ch < 3; ++ch) {
            const int64_t off = ((int64_t)b * 3 + ch) * plane;
            stage_plane(x + off, sx, H, W, oy, ox, vec);
            stage_plane(y + off, sy, H, W, oy, ox, vec);
            __syncthreads();                                // also: the previous channel's column pass has left hb
            ssim_rows(sx, sy, hb, taps);
            __syncthreads();                                // the next channel may overwrite sx / sy from here on
            float v[kStrip];
            ssim_columns(hb, taps, r0, col, v);
#pragma unroll
            for (int j = 0; j < kStrip; ++j) sum[j] = ch == 0 ? v[j] : sum[j] + v[j];
        }
        float lo = __builtin_inff(), hi = -__builtin_inff();
        const int gx = ox + col;
#pragma unroll
        for (int j = 0; j < kStrip; ++j) {
            const int gy = oy + r0 + j;
            if (gy < H && gx < W) {
                const float m = 0.5f - sum[j] / 3.0f / 2.0f;
                out[(int64_t)b * 3 * plane + (int64_t)gy * W + gx] = m;
                lo = fminf(lo, m); hi = fmaxf(hi, m);
            }
        }
        block_min_max(lo, hi, red);
        if (threadIdx.x == 0) {
            atomicMin(keys + 2 * b, float_key(lo));
            atomicMax(keys + 2 * b + 1, float_key(hi));
        }
        __syncthreads();                                    // red is written again for the next frame
    }
}

// ---- Lab maps -----------------------------------------------------------------------------------------------------------------------
// torch's mean over the selected channels adds them in their order: ((L + a) + b) / 3, (a + b) / 2
template <int KIND>
__device__ __forceinline__ float lab_value(float x0, float x1, float x2, float y0, float y1, float y2) {
    const float d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
    float L, A, B;
    rgb_to_lab_f32(d0 * d0, d1 * d1, d2 * d2, L, A, B);
    return KIND == CT_VIEW_LABMSE ? ((L + A) + B) / 3.0f : (A + B) / 2.0f;
}

// blockIdx.y strides over the frames, blockIdx.x over the plane.  vec: whole runs of four pixels through 16-byte loads and one
// 16-byte store, the plane's last plane % 4 pixels (and everything, without vec) one by one.
template <int KIND>
__global__ __launch_bounds__(kBlock) void lab_map_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out, int n,
                                                         int64_t plane, int vec, unsigned int *__restrict__ keys) {
    __shared__ float lds[8];
    const int64_t n_vec = vec ? plane / 4 : 0;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const float *xb = x + (int64_t)b * 3 * plane, *yb = y + (int64_t)b * 3 * plane;
        float *o = out + (int64_t)b * 3 * plane;
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_vec; c += (int64_t)gridDim.x * kBlock) {
            vf4 xv[3], yv[3], m;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                xv[ch] = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(xb + ch * plane) + c);
                yv[ch] = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(yb + ch * plane) + c);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m[k] = lab_value<KIND>(xv[0][k], xv[1][k], xv[2][k], yv[0][k], yv[1][k], yv[2][k]);
                lo = fminf(lo, m[k]); hi = fmaxf(hi, m[k]);
            }
            reinterpret_cast<vf4 *>(o)[c] = m;
        }
        for (int64_t p = 4 * n_vec + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock) {
            const float m = lab_value<KIND>(xb[p], xb[plane + p], xb[2 * plane + p], yb[p], yb[plane + p], yb[2 * plane + p]);
            o[p] = m;
            lo = fminf(lo, m); hi = fmaxf(hi, m);
        }
        block_min_max(lo, hi, lds);
        if (threadIdx.x == 0) {
            atomicMin(keys + 2 * b, float_key(lo));
            atomicMax(keys + 2 * b + 1, float_key(hi));
        }
        __syncthreads();                                    // lds is written again for the next frame
    }
}

// ---- the scaling pass the three maps share ------------------------------------------------------------------------------------------
// channel 0 in place: (m - lo) / (hi - lo); hi == lo: 0 / 0 = NaN, as the reference's division gives.  Channels 1 and 2: zeros.
__global__ __launch_bounds__(kBlock) void scale_in_place_kernel(float *__restrict__ out, int n, int64_t plane, int vec, const unsigned int *__restrict__ keys) {
    const int64_t n_vec = vec ? plane / 4 : 0;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const float lo = key_float(keys[2 * b]), hi = key_float(keys[2 * b + 1]);
        const float range = hi - lo;
        float *o = out + (int64_t)b * 3 * plane;
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_vec; c += (int64_t)gridDim.x * kBlock) {
            vf4 v = reinterpret_cast<const vf4 *>(o)[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (v[k] - lo) / range;
            reinterpret_cast<vf4 *>(o)[c] = v;
            reinterpret_cast<vf4 *>(o + plane)[c] = (vf4)(0.0f);
            reinterpret_cast<vf4 *>(o + 2 * plane)[c] = (vf4)(0.0f);
        }
        for (int64_t p = 4 * n_vec + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock) {
            o[p] = (o[p] - lo) / range;
            o[plane + p] = o[2 * plane + p] = 0.0f;
        }
    }
}

static inline bool on16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what the two entries check alike, before anything is launched
static int check_args(const float *x, const float *y, const float *out, const void *ws, size_t ws_bytes, int b, int h, int w) {
    if (!x || !y || !out || !ws || b < 1 || h < 1 || w < 1 || ws_bytes < ct_view_workspace_bytes(b)) return CT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(ws) % sizeof(unsigned int)) return CT_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) % sizeof(float)) return CT_E_ALIGN;
    return CT_OK;
}

static int scale_in_place(float *out, const unsigned int *keys, int b, int64_t plane, hipStream_t s) {
    const int vec = plane % 4 == 0 && on16(out);
    const int gy = b < 65535 ? b : 65535;
    hipLaunchKernelGGL(scale_in_place_kernel, dim3(blocks_per_image((plane + 3) / 4, gy), gy), dim3(kBlock), 0, s, out, b, plane, vec, keys);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // namespace em
}  // namespace ct

extern "C" {

int ct_view_ssim_map_f32(const float *x, const float *y, float *out, void *ws, size_t ws_bytes, int b, int h, int w, void *stream) {
    using namespace ct::em;
    const int rc = check_args(x, y, out, ws, ws_bytes, b, h, w);
    if (rc) return rc;
    if (h <= kRad || w <= kRad) return CT_E_BADARG;          // reflect padding of 5 needs more than 5 pixels
    const dim3 grid((w + kTW - 1) / kTW, (h + kTH - 1) / kTH, b < 65535 ? b : 65535);
    if (grid.y > 65535u) return CT_E_BADARG;                 // more than two million rows
    hipStream_t s = (hipStream_t)stream;
    static ct::DynLdsAttr attr;
    if (attr.ensure(reinterpret_cast<const void *>(ssim_map_kernel), kSsimLds) != hipSuccess) return CT_E_BADARG;
    const Taps taps = ssim_taps();
    const int64_t plane = (int64_t)h * w;
    // every row of every plane starts on 16 bytes when the bases do and the width is a whole number of them
    const int vec = w % 4 == 0 && on16(x) && on16(y);
    unsigned int *keys = reinterpret_cast<unsigned int *>(ws);
    hipLaunchKernelGGL(ct::minmax_init_kernel, dim3((2 * b + 255) / 256), dim3(256), 0, s, keys, b);
    hipLaunchKernelGGL(ssim_map_kernel, grid, dim3(ct::kBlock), kSsimLds, s, x, y, out, b, h, w, vec, taps, keys);
    CT_CHECK_LAUNCH();
    return scale_in_place(out, keys, b, plane, s);
}

int ct_view_lab_map_f32(const float *x, const float *y, float *out, void *ws, size_t ws_bytes, int b, int h, int w, int kind, void *stream) {
    using namespace ct::em;
    if (kind != CT_VIEW_LABMSE && kind != CT_VIEW_ABMSE) return CT_E_BADARG;
    const int rc = check_args(x, y, out, ws, ws_bytes, b, h, w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t plane = (int64_t)h * w;
    const int vec = plane % 4 == 0 && on16(x) && on16(y) && on16(out);
    unsigned int *keys = reinterpret_cast<unsigned int *>(ws);
    const int gy = b < 65535 ? b : 65535;
    const dim3 grid(ct::blocks_per_image((plane + 3) / 4, gy), gy), block(ct::kBlock);
    hipLaunchKernelGGL(ct::minmax_init_kernel, dim3((2 * b + 255) / 256), dim3(256), 0, s, keys, b);
    if (kind == CT_VIEW_LABMSE) hipLaunchKernelGGL(lab_map_kernel<CT_VIEW_LABMSE>, grid, block, 0, s, x, y, out, b, plane, vec, keys);
    else hipLaunchKernelGGL(lab_map_kernel<CT_VIEW_ABMSE>, grid, block, 0, s, x, y, out, b, plane, vec, keys);
    CT_CHECK_LAUNCH();
    return scale_in_place(out, keys, b, plane, s);
}

}  // extern "C"

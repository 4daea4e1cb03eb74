// views.hip -- the diagnostic views of the reference's image panel (methods/dcmcs3di.py:116-144, methods/dmsct.py:148-184) on gfx950:
//   ct_view_chess_mix_f32     utils/visualizations.py:9-21   chess_mix: a checkerboard of two frames, bitwise a copy
//   ct_view_scaled_plane_f32  utils/visualizations.py:24-36  rgbmse = minmaxscale(mean_c (x - y)^2) in channel 0 (CT_VIEW_RGBMSE),
//                                                           and the same min-max scaling of one plane in three channels (CT_VIEW_GRAY)
//   ct_flow_to_image_u8       utils/flow_viz.py:184-264      flow_to_image: the Middlebury colour code of a flow field, as HWC bytes
// All three are streaming kernels: every input element is read once per pass with 16-byte loads where the frame's rows allow it,
// nothing is reused, LDS holds only the four wave results of a reduction (and the 55-entry colour wheel).  The min-max family and
// the flow image need a per-frame statistic first (min / max of the plane, the largest flow radius): a reduction pass leaves it in
// the caller's workspace -- wave reduce, four waves through LDS, then ONE atomic min / max per workgroup on an order-preserving
// integer image of the float (ct_minmax.h, shared with errmaps.hip) (min and max do not depend on the order of their operands: the result is deterministic) -- and a map
// pass reads it back.  The Makefile's -ffp-contract=off keeps every product and sum below a rounding of its own: the map passes
// recompute exactly the values the reductions saw.
#include "ct_common.h"
#include "ct_minmax.h"

namespace ct {

typedef float vf4 __attribute__((ext_vector_type(4)));

// ---- chess_mix ------------------------------------------------------------------------------------------------------------------
// element e of the flat [planes][H][W] run: row = e / W, block row (row % H) / size, block column (e % W) / size; even sum -> x.
// VEC: W % 4 == 0 and all three bases on 16 bytes, one lane-step is four elements of one row -- one 16-byte load when they share a
// block column (always, when size % 4 == 0), two loads and a per-element choice otherwise.  I: 32-bit indices whenever they fit.
template <typename I, bool VEC>
__global__ __launch_bounds__(kBlock) void chess_mix_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out,
                                                           I n_steps, I height, I width, I size) {
    constexpr I E = VEC ? 4 : 1;
    const I steps_per_row = width / E;
    for (I s = (I)blockIdx.x * kBlock + threadIdx.x; s < n_steps; s += (I)gridDim.x * kBlock) {
        const I row = s / steps_per_row, col = (s - row * steps_per_row) * E;
        const I bi = (row % height) / size, bj = col / size;
        const bool from_x = ((bi + bj) & 1) == 0;
        if constexpr (VEC) {
            const I bj3 = (col + 3) / size;
            const vf4 *px = reinterpret_cast<const vf4 *>(x) + s, *py = reinterpret_cast<const vf4 *>(y) + s;
            vf4 v;
            if (bj3 == bj) {
                v = __builtin_nontemporal_load(from_x ? px : py);
            } else {
                const vf4 a = __builtin_nontemporal_load(px), b = __builtin_nontemporal_load(py);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = (((bi + (col + k) / size) & 1) == 0) ? a[k] : b[k];
            }
            reinterpret_cast<vf4 *>(out)[s] = v;
        } else {
            out[s] = from_x ? x[s] : y[s];
        }
    }
}

// ---- the min-max family ---------------------------------------------------------------------------------------------------------
// torch.square(x - y).mean(dim=1) on a contiguous [B,3,H,W] tensor adds the channels in their order and divides by 3
__device__ __forceinline__ float mse3(float x0, float x1, float x2, float y0, float y1, float y2) {
    const float d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
    return ((d0 * d0 + d1 * d1) + d2 * d2) / 3.0f;
}

// E elements of frame b's plane at p: RGBMSE reads the three channels of x and y, GRAY the one plane of x
template <int KIND, int E>
__device__ __forceinline__ void plane_values(const float *__restrict__ x, const float *__restrict__ y, int b, int64_t plane, int64_t p, float (&m)[E]) {
    typedef float vec_t __attribute__((ext_vector_type(E)));
    if constexpr (KIND == CT_VIEW_GRAY) {
        const vec_t v = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(x + (int64_t)b * plane + p));
#pragma unroll
        for (int k = 0; k < E; ++k) m[k] = v[k];
    } else {
        const float *xb = x + (int64_t)b * 3 * plane + p, *yb = y + (int64_t)b * 3 * plane + p;
        vec_t xv[3], yv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xv[c] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(xb + c * plane));
            yv[c] = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(yb + c * plane));
        }
#pragma unroll
        for (int k = 0; k < E; ++k) m[k] = mse3(xv[0][k], xv[1][k], xv[2][k], yv[0][k], yv[1][k], yv[2][k]);
    }
}
template <int KIND>
__device__ __forceinline__ float plane_value(const float *__restrict__ x, const float *__restrict__ y, int b, int64_t plane, int64_t p) {
    if constexpr (KIND == CT_VIEW_GRAY) return x[(int64_t)b * plane + p];
    const float *xb = x + (int64_t)b * 3 * plane + p, *yb = y + (int64_t)b * 3 * plane + p;
    return mse3(xb[0], xb[plane], xb[2 * plane], yb[0], yb[plane], yb[2 * plane]);
}

// blockIdx.y strides over the frames, blockIdx.x over the plane.  vec: whole runs of four elements through 16-byte loads, the
// plane's last plane % 4 elements (and everything, without vec) one by one.
template <int KIND>
__global__ __launch_bounds__(kBlock) void minmax_reduce_kernel(const float *__restrict__ x, const float *__restrict__ y, int n, int64_t plane, int vec,
                                                               unsigned int *__restrict__ keys) {
    __shared__ float lds[8];
    const int64_t n_vec = vec ? plane / 4 : 0;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_vec; c += (int64_t)gridDim.x * kBlock) {
            float m[4];
            plane_values<KIND, 4>(x, y, b, plane, 4 * c, m);
#pragma unroll
            for (int k = 0; k < 4; ++k) { lo = fminf(lo, m[k]); hi = fmaxf(hi, m[k]); }
        }
        for (int64_t p = 4 * n_vec + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock) {
            const float m = plane_value<KIND>(x, y, b, plane, p);
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

template <int KIND>
__global__ __launch_bounds__(kBlock) void minmax_map_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out, int n,
                                                            int64_t plane, int vec, const unsigned int *__restrict__ keys) {
    const int64_t n_vec = vec ? plane / 4 : 0;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const float lo = key_float(keys[2 * b]), hi = key_float(keys[2 * b + 1]);
        const float range = hi - lo;                        // 0 for a constant frame: 0 / 0 = NaN, as the reference's division gives
        float *o = out + (int64_t)b * 3 * plane;
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_vec; c += (int64_t)gridDim.x * kBlock) {
            float m[4];
            plane_values<KIND, 4>(x, y, b, plane, 4 * c, m);
            vf4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (m[k] - lo) / range;
            const vf4 rest = KIND == CT_VIEW_GRAY ? v : (vf4)(0.0f);
            reinterpret_cast<vf4 *>(o)[c] = v;
            reinterpret_cast<vf4 *>(o + plane)[c] = rest;
            reinterpret_cast<vf4 *>(o + 2 * plane)[c] = rest;
        }
        for (int64_t p = 4 * n_vec + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock) {
            const float v = (plane_value<KIND>(x, y, b, plane, p) - lo) / range;
            o[p] = v;
            o[plane + p] = o[2 * plane + p] = KIND == CT_VIEW_GRAY ? v : 0.0f;
        }
    }
}

// ---- flow_to_image ----------------------------------------------------------------------------------------------------------------
// The 55 colours of the Middlebury wheel from its six segment lengths (flow_viz.py:134-181): within a segment one channel runs
// floor(255 k / n) up or 255 - floor(255 k / n) down (255 k / n is never within 1 / 15 of an integer it does not hit exactly: the
// integer division is numpy's floor of the float64 quotient).
struct Wheel {
    uint8_t c[55][3];
};
constexpr Wheel make_wheel() {
    Wheel w{};
    constexpr int len[6] = {15, 6, 4, 11, 13, 6};          // RY YG GC CB BM MR
    constexpr int full[6] = {0, 1, 1, 2, 2, 0};            // the channel held at 255
    constexpr int ramp[6] = {1, 0, 2, 1, 0, 2};            // the channel that runs: up in segments 0, 2, 4, down in 1, 3, 5
    int col = 0;
    for (int s = 0; s < 6; ++s)
        for (int k = 0; k < len[s]; ++k, ++col) {
            const int v = 255 * k / len[s];
            w.c[col][full[s]] = 255;
            w.c[col][ramp[s]] = (uint8_t)((s & 1) ? 255 - v : v);
        }
    return w;
}
__device__ const Wheel kWheel = make_wheel();
constexpr float kUnknownFlow = 1e7f;                        // UNKNOWN_FLOW_THRESH

// NaN fails both comparisons' complements: it counts as unknown (the reference's own maximum would be NaN for the whole frame)
__device__ __forceinline__ bool flow_known(float u, float v) { return fabsf(u) <= kUnknownFlow && fabsf(v) <= kUnknownFlow; }

// the largest sqrt(u^2 + v^2) (float32, as the reference takes it before it normalises) over a frame's known pixels, as the bits
// of a non-negative float: they order like unsigned integers.  maxbits[b] starts at 0 = the bits of 0.0f (unknown pixels count as
// zero flow, so the maximum is never below 0 and the reference's max(-1, .) never binds).
__global__ __launch_bounds__(kBlock) void flow_maxrad_kernel(const float *__restrict__ flow, int n, int64_t plane, int vec, unsigned int *__restrict__ maxbits) {
    __shared__ float lds[8];
    const int64_t n_vec = vec ? plane / 4 : 0;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const float *u = flow + (int64_t)b * 2 * plane, *v = u + plane;
        float lo = 0.0f, hi = 0.0f;
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_vec; c += (int64_t)gridDim.x * kBlock) {
            const vf4 uu = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(u) + c), vv = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(v) + c);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (flow_known(uu[k], vv[k])) hi = fmaxf(hi, sqrtf(uu[k] * uu[k] + vv[k] * vv[k]));
        }
        for (int64_t p = 4 * n_vec + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock)
            if (flow_known(u[p], v[p])) hi = fmaxf(hi, sqrtf(u[p] * u[p] + v[p] * v[p]));
        block_min_max(lo, hi, lds);
        if (threadIdx.x == 0) atomicMax(maxbits + b, __float_as_uint(hi));
        __syncthreads();
    }
}

// One pixel.  The reference divides the float32 flow by the float64 scalar maxrad + eps, which makes everything after it float64
// under numpy 2's promotion rules (flow_viz.py:256-259 and compute_color); `den` is that scalar.  Returns r | g << 8 | b << 16.
__device__ __forceinline__ unsigned int flow_colour(float uf, float vf, double den, const double *__restrict__ wheel /* LDS [55][3], / 255 */) {
    if (!flow_known(uf, vf)) return 0u;                     // unknown: black
    const double u = (double)uf / den, v = (double)vf / den;
    const double rad = sqrt(u * u + v * v);
    const double a = atan2(-v, -u) / 3.141592653589793;
    const double fk = (a + 1.0) / 2.0 * 54.0 + 1.0;         // in [1, 55]
    int k0 = (int)floor(fk);
    k0 = k0 < 1 ? 1 : (k0 > 55 ? 55 : k0);                  // the table index stays inside whatever atan2 rounds to
    const int k1 = k0 == 55 ? 1 : k0 + 1;
    const double f = fk - (double)k0;
    unsigned int rgb = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double col = (1.0 - f) * wheel[3 * (k0 - 1) + i] + f * wheel[3 * (k1 - 1) + i];
        col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
        const double q = floor(255.0 * col);
        rgb |= (unsigned int)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q)) << (8 * i);
    }
    return rgb;
}

// vec: a lane-step is four pixels -- two 16-byte loads, twelve output bytes as three aligned dwords; otherwise pixel by pixel
__global__ __launch_bounds__(kBlock) void flow_image_kernel(const float *__restrict__ flow, int n, int64_t plane, int vec, const unsigned int *__restrict__ maxbits,
                                                            uint8_t *__restrict__ out) {
    __shared__ double wheel[55 * 3];
    for (int i = threadIdx.x; i < 55 * 3; i += kBlock) wheel[i] = (double)kWheel.c[i / 3][i % 3] / 255.0;
    __syncthreads();
    const int64_t n_vec = vec ? plane / 4 : 0;
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const float *u = flow + (int64_t)b * 2 * plane, *v = u + plane;
        uint8_t *o = out + (int64_t)b * 3 * plane;
        const double den = (double)__uint_as_float(maxbits[b]) + 2.220446049250313e-16;      // maxrad + np.finfo(float).eps
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_vec; c += (int64_t)gridDim.x * kBlock) {
            const vf4 uu = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(u) + c), vv = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(v) + c);
            unsigned int q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = flow_colour(uu[k], vv[k], den, wheel);
            unsigned int *dst = reinterpret_cast<unsigned int *>(o + 12 * c);
            dst[0] = q[0] | (q[1] << 24);
            dst[1] = (q[1] >> 8) | (q[2] << 16);
            dst[2] = (q[2] >> 16) | (q[3] << 8);
        }
        for (int64_t p = 4 * n_vec + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock) {
            const unsigned int q = flow_colour(u[p], v[p], den, wheel);
            o[3 * p] = (uint8_t)q;
            o[3 * p + 1] = (uint8_t)(q >> 8);
            o[3 * p + 2] = (uint8_t)(q >> 16);
        }
    }
}

static inline bool on16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ct

extern "C" {

int ct_view_chess_mix_f32(const float *x, const float *y, float *out, int b, int c, int h, int w, int size, void *stream) {
    if (!x || !y || !out || b < 1 || c < 1 || h < 1 || w < 1 || size < 1) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) % sizeof(float)) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)b * c * h * w;
    const bool vec = w % 4 == 0 && ct::on16(x) && ct::on16(y) && ct::on16(out);
    const int64_t n_steps = vec ? total / 4 : total;
    int64_t blocks = (n_steps + ct::kBlock - 1) / ct::kBlock;
    if (blocks > ct::target_blocks()) blocks = ct::target_blocks();
    const dim3 grid((unsigned)blocks), block(ct::kBlock);
    // 32-bit indices while the strided loop counter itself cannot wrap
    if (n_steps + (int64_t)blocks * ct::kBlock < (int64_t)1 << 32) {
        if (vec) hipLaunchKernelGGL((ct::chess_mix_kernel<uint32_t, true>), grid, block, 0, s, x, y, out, (uint32_t)n_steps, (uint32_t)h, (uint32_t)w, (uint32_t)size);
        else hipLaunchKernelGGL((ct::chess_mix_kernel<uint32_t, false>), grid, block, 0, s, x, y, out, (uint32_t)n_steps, (uint32_t)h, (uint32_t)w, (uint32_t)size);
    } else {
        if (vec) hipLaunchKernelGGL((ct::chess_mix_kernel<int64_t, true>), grid, block, 0, s, x, y, out, n_steps, (int64_t)h, (int64_t)w, (int64_t)size);
        else hipLaunchKernelGGL((ct::chess_mix_kernel<int64_t, false>), grid, block, 0, s, x, y, out, n_steps, (int64_t)h, (int64_t)w, (int64_t)size);
    }
    CT_CHECK_LAUNCH();
    return CT_OK;
}

size_t ct_view_workspace_bytes(int b) { return b < 1 ? 0 : (size_t)b * 2 * sizeof(unsigned int); }

int ct_view_scaled_plane_f32(const float *x, const float *y, float *out, void *ws, size_t ws_bytes, int b, int h, int w, int kind, void *stream) {
    if (!x || !out || b < 1 || h < 1 || w < 1 || (kind != CT_VIEW_RGBMSE && kind != CT_VIEW_GRAY) || (kind == CT_VIEW_RGBMSE && !y)) return CT_E_BADARG;
    if (!ws || ws_bytes < ct_view_workspace_bytes(b) || reinterpret_cast<uintptr_t>(ws) % sizeof(unsigned int)) return CT_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(out)) % sizeof(float)) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t plane = (int64_t)h * w;
    // every plane of every frame starts on 16 bytes when the bases do and the plane is a whole number of them
    const int vec = plane % 4 == 0 && ct::on16(x) && ct::on16(out) && (kind == CT_VIEW_GRAY || ct::on16(y));
    unsigned int *keys = reinterpret_cast<unsigned int *>(ws);
    const int gy = b < 65535 ? b : 65535;
    const dim3 grid(ct::blocks_per_image((plane + 3) / 4, gy), gy), block(ct::kBlock);
    hipLaunchKernelGGL(ct::minmax_init_kernel, dim3((2 * b + 255) / 256), dim3(256), 0, s, keys, b);
    if (kind == CT_VIEW_RGBMSE) {
        hipLaunchKernelGGL(ct::minmax_reduce_kernel<CT_VIEW_RGBMSE>, grid, block, 0, s, x, y, b, plane, vec, keys);
        hipLaunchKernelGGL(ct::minmax_map_kernel<CT_VIEW_RGBMSE>, grid, block, 0, s, x, y, out, b, plane, vec, keys);
    } else {
        hipLaunchKernelGGL(ct::minmax_reduce_kernel<CT_VIEW_GRAY>, grid, block, 0, s, x, y, b, plane, vec, keys);
        hipLaunchKernelGGL(ct::minmax_map_kernel<CT_VIEW_GRAY>, grid, block, 0, s, x, y, out, b, plane, vec, keys);
    }
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_flow_to_image_u8(const float *flow, uint8_t *out_hwc, void *ws, size_t ws_bytes, int b, int h, int w, void *stream) {
    if (!flow || !out_hwc || b < 1 || h < 1 || w < 1) return CT_E_BADARG;
    if (!ws || ws_bytes < ct_view_workspace_bytes(b) || reinterpret_cast<uintptr_t>(ws) % sizeof(unsigned int)) return CT_E_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(flow) % sizeof(float)) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t plane = (int64_t)h * w;
    // four pixels = 12 output bytes: dword stores need the frame's bytes on 4, which plane % 4 == 0 gives every frame of the batch
    const int vec = plane % 4 == 0 && ct::on16(flow) && reinterpret_cast<uintptr_t>(out_hwc) % 4 == 0;
    unsigned int *maxbits = reinterpret_cast<unsigned int *>(ws);
    const int gy = b < 65535 ? b : 65535;
    const dim3 grid(ct::blocks_per_image((plane + 3) / 4, gy), gy), block(ct::kBlock);
    const int rc = ct::zero_async(maxbits, (size_t)b * sizeof(unsigned int), s);
    if (rc) return rc;
    hipLaunchKernelGGL(ct::flow_maxrad_kernel, grid, block, 0, s, flow, b, plane, vec, maxbits);
    hipLaunchKernelGGL(ct::flow_image_kernel, grid, block, 0, s, flow, b, plane, vec, maxbits, out_hwc);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"

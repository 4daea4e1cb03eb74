// gmflow.hip -- the GMFlow / UniMatch matcher's building blocks that are neither convolutions nor token layers, NCHW float32:
//   inorm_*                  InstanceNorm2d (affine=False, eps 1e-5) [+ReLU] [+skip, ReLU] (backbone.py:34-39)
//   eltwise_kernel           gru ops, image normalisation, scaling
//   convex_upsample, bilinear_resize, flow_warp, fb_check   utils.py:137-155, geometry.py
// The rest of the matcher: conv_generic.hip, linear_tokens.hip, attention_tokens.hip, local_corr.hip.
#include "ct_common.h"

namespace ct {

// ReLU that propagates NaN like torch.relu / F.relu (`v > 0 ? v : 0` turns a NaN into 0 and hides it from every isfinite check
// downstream); every other input, -0 included, gives what that form gives
__device__ __forceinline__ float relu_nan(float v) { return v <= 0.f ? 0.f : v; }

// =================================================================================================
// InstanceNorm2d (affine=False, biased variance, eps): one workgroup per (n, c) plane, two passes.
//   mode 0: y = IN(x)          mode 1: y = relu(IN(x))          mode 2: y = relu(skip + relu(IN(x)))   (backbone.py:34-39)
//   mode 3: y = relu(IN(x) + skip')  is not needed: the downsample branch is normalised by its own launch.
// =================================================================================================
__global__ __launch_bounds__(256) void inorm_kernel(const float *__restrict__ x, const float *__restrict__ skip,
                                                    float *__restrict__ y, int plane, float eps, int mode) {
    __shared__ double red[8];
    const size_t base = (size_t)blockIdx.x * plane;
    double s = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < plane; i += 256) {
        const double v = x[base + i];
        s += v;
        ss += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        ss += __shfl_down(ss, off, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid] = s; red[4 + wid] = ss; }
    __syncthreads();
    const double ts = red[0] + red[1] + red[2] + red[3], tss = red[4] + red[5] + red[6] + red[7];
    const double mean = ts / plane;
    double var = tss / plane - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const float fm = (float)mean, rstd = (float)(1.0 / sqrt(var + (double)eps));
    for (int i = threadIdx.x; i < plane; i += 256) {
        float v = (x[base + i] - fm) * rstd;
        if (mode >= 1) v = relu_nan(v);
        if (mode == 2) { v += skip[base + i]; v = relu_nan(v); }
        y[base + i] = v;
    }
}

// Large planes (the 1/2-resolution backbone stage: 128 planes of 115k pixels) cannot fill 256 CUs with one workgroup
// per plane: split every plane over kInormSplit workgroups -- partial sums first (fixed order, no atomics), then each
// workgroup normalises its own chunk.
constexpr int kInormSplit = 16;

__global__ __launch_bounds__(256) void inorm_partial_kernel(const float *__restrict__ x, int plane, double *__restrict__ part) {
    __shared__ double red[8];
    const int chunk = (((plane + kInormSplit - 1) / kInormSplit) + 3) & ~3;
    const int i0 = blockIdx.y * chunk, i1 = (i0 + chunk < plane) ? i0 + chunk : plane;
    const float *xp = x + (size_t)blockIdx.x * plane;
    double s = 0.0, ss = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const double v = xp[i];
        s += v;
        ss += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        ss += __shfl_down(ss, off, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[wid] = s; red[4 + wid] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = part + ((size_t)blockIdx.x * kInormSplit + blockIdx.y) * 2;
        o[0] = red[0] + red[1] + red[2] + red[3];
        o[1] = red[4] + red[5] + red[6] + red[7];
    }
}

__global__ __launch_bounds__(256) void inorm_apply_kernel(const float *__restrict__ x, const float *__restrict__ skip,
                                                          float *__restrict__ y, int plane, float eps, int mode,
                                                          const double *__restrict__ part) {
    const int chunk = (((plane + kInormSplit - 1) / kInormSplit) + 3) & ~3;
    const int i0 = blockIdx.y * chunk, i1 = (i0 + chunk < plane) ? i0 + chunk : plane;
    const double *pp = part + (size_t)blockIdx.x * kInormSplit * 2;
    double ts = 0.0, tss = 0.0;
#pragma unroll
    for (int z = 0; z < kInormSplit; ++z) { ts += pp[2 * z]; tss += pp[2 * z + 1]; }
    const double mean = ts / plane;
    double var = tss / plane - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const float fm = (float)mean, rstd = (float)(1.0 / sqrt(var + (double)eps));
    const size_t base = (size_t)blockIdx.x * plane;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        float v = (x[base + i] - fm) * rstd;
        if (mode >= 1) v = relu_nan(v);
        if (mode == 2) { v += skip[base + i]; v = relu_nan(v); }
        y[base + i] = v;
    }
}

// =================================================================================================
// Elementwise helpers
//   op 0: y = a + b              op 1: y = a * b                  op 2: y = (1 - z) * h + z * q   (a=z, b=h, c=q; gru_blend)
//   op 3: y = (a / 255 - mean[c]) / std[c]   (normalize_img, utils.py:26-34; a: [N,3,H,W], plane given)
//   op 4: y = a * s0             op 5: tanh(a) for channels < split, relu(a) otherwise (refine_proj chunk, unimatch.py:320-323)
// =================================================================================================
__global__ void eltwise_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c,
                               float *__restrict__ y, long long n, int op, int plane, int chans, int split, float s0) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v;
    switch (op) {
        case 0: v = a[i] + b[i]; break;
        case 1: v = a[i] * b[i]; break;
        case 2: v = gru_blend(a[i], b[i], c[i]); break;
        case 3: {
            const int ch = (int)((i / plane) % 3);
            const float mean = ch == 0 ? 0.485f : (ch == 1 ? 0.456f : 0.406f);
            const float sd = ch == 0 ? 0.229f : (ch == 1 ? 0.224f : 0.225f);
            v = (a[i] / 255.0f - mean) / sd;
            break;
        }
        case 4: v = a[i] * s0; break;
        default: {
            const int ch = (int)((i / plane) % chans);
            v = ch < split ? tanhf(a[i]) : relu_nan(a[i]);
        }
    }
    y[i] = v;
}

// =================================================================================================
// Sampling / resampling (NCHW)
// =================================================================================================
// F.interpolate(mode='bilinear', align_corners=True) to (Ho, Wo), times `mul[c]` (mul0 for channel 0, mul1 otherwise)
__global__ void bilinear_resize_kernel(const float *__restrict__ in, float *__restrict__ out, int NC, int C, int H, int W, int Ho,
                                       int Wo, float mul0, float mul1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)NC * Ho * Wo;
    if (i >= total) return;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho);
    const long long nc = i / ((long long)Ho * Wo);
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float fy = sy * yo, fx = sx * xo;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < H - 1 ? y0 : H - 1; x0 = x0 < W - 1 ? x0 : W - 1;
    const int y1 = y0 + (y0 < H - 1), x1 = x0 + (x0 < W - 1);
    const float ly = fy - y0, lx = fx - x0;
    const float *p = in + nc * (long long)H * W;
    const float v = (1.f - ly) * ((1.f - lx) * p[(size_t)y0 * W + x0] + lx * p[(size_t)y0 * W + x1]) +
                    ly * ((1.f - lx) * p[(size_t)y1 * W + x0] + lx * p[(size_t)y1 * W + x1]);
    out[i] = v * (((int)(nc % C) == 0) ? mul0 : mul1);
}

__device__ __forceinline__ float tap_index(float f) { return f < -2.f ? -2.f : (f > 2147483520.f ? 2147483520.f : f); }

// geometry.py:43-75: out = grid_sample(img, (x + flow_x, y + flow_y)), bilinear, zeros padding, align_corners=True
__global__ void flow_warp_kernel(const float *__restrict__ img, const float *__restrict__ flow, float *__restrict__ out, int N, int C,
                                 int H, int W) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long hw = (long long)H * W;
    if (i >= (long long)N * hw) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), n = (int)(i / hw);
    const float sx = (float)x + flow[((size_t)n * 2 + 0) * hw + (size_t)y * W + x];
    const float sy = (float)y + flow[((size_t)n * 2 + 1) * hw + (size_t)y * W + x];
    // bilinear_sample normalises (2 x / (w-1) - 1) and grid_sample maps back ((g + 1) / 2 * (w - 1))
    const float gx = 2.0f * sx / (float)(W - 1) - 1.0f, gy = 2.0f * sy / (float)(H - 1) - 1.0f;
    const float px = ((gx + 1.0f) * 0.5f) * (float)(W - 1), py = ((gy + 1.0f) * 0.5f) * (float)(H - 1);
    const float x0f = floorf(px), y0f = floorf(py);
    // A finite flow beyond +-2^31 has no defined float -> int conversion, and on the saturated INT_MAX the guard of the right-hand
    // tap, compiled as `x0 > -2 && wrapped(x0 + 1) < W`, is TRUE: a load 8 GB past the plane.  Any index outside [-1, W - 1] has no
    // tap, so convert a clamped copy (the weights keep x0f): [-2, 2^31 - 128] converts exactly and x0 + 1 cannot overflow.
    const int x0 = (int)tap_index(x0f), y0 = (int)tap_index(y0f);
    const float wx1 = px - x0f, wy1 = py - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const bool vx0 = x0 >= 0 && x0 < W, vx1 = x0 + 1 >= 0 && x0 + 1 < W, vy0 = y0 >= 0 && y0 < H, vy1 = y0 + 1 >= 0 && y0 + 1 < H;
    for (int c = 0; c < C; ++c) {
        const float *p = img + ((size_t)n * C + c) * hw;
        float v = 0.f;
        if (vy0 && vx0) v += wy0 * wx0 * p[(size_t)y0 * W + x0];
        if (vy0 && vx1) v += wy0 * wx1 * p[(size_t)y0 * W + x0 + 1];
        if (vy1 && vx0) v += wy1 * wx0 * p[(size_t)(y0 + 1) * W + x0];
        if (vy1 && vx1) v += wy1 * wx1 * p[(size_t)(y0 + 1) * W + x0 + 1];
        out[((size_t)n * C + c) * hw + (size_t)y * W + x] = v;
    }
}

// utils.py:137-155: convex upsampling by `f` (mask [B][9*f*f][H][W], flow [B][2][H][W] -> [B][2][fH][fW])
__global__ void convex_upsample_kernel(const float *__restrict__ flow, const float *__restrict__ mask, float *__restrict__ out, int B,
                                       int H, int W, int f) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Ho = H * f, Wo = W * f;
    if (i >= (long long)B * Ho * Wo) return;
    const int xo = (int)(i % Wo), yo = (int)((i / Wo) % Ho), b = (int)(i / ((long long)Ho * Wo));
    const int x = xo / f, y = yo / f, kx = xo % f, ky = yo % f;
    const size_t hw = (size_t)H * W;
    float m[9], mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        m[t] = mask[((size_t)b * 9 * f * f + (size_t)t * f * f + ky * f + kx) * hw + (size_t)y * W + x];
        mx = fmaxf(mx, m[t]);
    }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) { m[t] = expf(m[t] - mx); sum += m[t]; }
    float ox = 0.f, oy = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const float p = m[t] / sum;
            ox += p * (float)f * flow[((size_t)b * 2 + 0) * hw + (size_t)yy * W + xx];
            oy += p * (float)f * flow[((size_t)b * 2 + 1) * hw + (size_t)yy * W + xx];
        }
    }
    out[((size_t)b * 2 + 0) * Ho * Wo + (size_t)yo * Wo + xo] = ox;
    out[((size_t)b * 2 + 1) * Ho * Wo + (size_t)yo * Wo + xo] = oy;
}

// geometry.py:78-99 given the two warped flows: occ = (|a + wa| > alpha (|fwd| + |bwd|) + beta) as 0/1
__global__ void fb_check_kernel(const float *__restrict__ fwd, const float *__restrict__ bwd, const float *__restrict__ wbwd,
                                const float *__restrict__ wfwd, float *__restrict__ focc, float *__restrict__ bocc, int B, int H, int W,
                                float alpha, float beta) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long hw = (long long)H * W;
    if (i >= (long long)B * hw) return;
    const long long b = i / hw, p = i % hw;
    const size_t i0 = (size_t)(b * 2) * hw + p, i1 = i0 + hw;
    const float mag = sqrtf(fwd[i0] * fwd[i0] + fwd[i1] * fwd[i1]) + sqrtf(bwd[i0] * bwd[i0] + bwd[i1] * bwd[i1]);
    const float dfx = fwd[i0] + wbwd[i0], dfy = fwd[i1] + wbwd[i1], dbx = bwd[i0] + wfwd[i0], dby = bwd[i1] + wfwd[i1];
    const float thr = alpha * mag + beta;
    focc[i] = sqrtf(dfx * dfx + dfy * dfy) > thr ? 1.0f : 0.0f;
    bocc[i] = sqrtf(dbx * dbx + dby * dby) > thr ? 1.0f : 0.0f;
}

}  // namespace ct

// -------------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------------
extern "C" {

size_t ct_instance_norm_workspace_bytes(int planes) {
    return planes > 0 ? (size_t)planes * ct::kInormSplit * 2 * sizeof(double) : 0;
}

int ct_instance_norm_f32(const float *x, const float *skip, float *y, int planes, int plane, float eps, int mode, void *ws,
                         size_t ws_bytes, void *stream) {
    if (!x || !y || planes < 0 || plane < 1 || (mode == 2 && !skip)) return CT_E_BADARG;
    if (planes == 0) return CT_OK;
    if (ws && planes < 1024 && plane >= 16384) {   // few, large planes: split them (see inorm_partial_kernel)
        if (ws_bytes < ct_instance_norm_workspace_bytes(planes)) return CT_E_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(ws) & 7) return CT_E_ALIGN;
        dim3 grid(planes, ct::kInormSplit);
        hipLaunchKernelGGL(ct::inorm_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, plane, (double *)ws);
        CT_CHECK_LAUNCH();
        hipLaunchKernelGGL(ct::inorm_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, skip, y, plane, eps, mode,
                           (const double *)ws);
        CT_CHECK_LAUNCH();
        return CT_OK;
    }
    hipLaunchKernelGGL(ct::inorm_kernel, dim3(planes), dim3(256), 0, (hipStream_t)stream, x, skip, y, plane, eps, mode);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_eltwise_f32(const float *a, const float *b, const float *c, float *y, long long n, int op, int plane, int chans, int split,
                   float s0, void *stream) {
    if (!a || !y || n < 0) return CT_E_BADARG;
    if (n == 0) return CT_OK;
    hipLaunchKernelGGL(ct::eltwise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, c, y, n, op,
                       plane > 0 ? plane : 1, chans > 0 ? chans : 1, split, s0);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_bilinear_resize_f32(const float *in, float *out, int n, int c, int h, int w, int ho, int wo, float mul0, float mul1, void *stream) {
    if (!in || !out || n < 0 || c < 1 || h < 1 || w < 1 || ho < 1 || wo < 1) return CT_E_BADARG;
    const long long total = (long long)n * c * ho * wo;
    if (total == 0) return CT_OK;
    hipLaunchKernelGGL(ct::bilinear_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, n * c,
                       c, h, w, ho, wo, mul0, mul1);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_flow_warp_f32(const float *img, const float *flow, float *out, int n, int c, int h, int w, void *stream) {
    if (!img || !flow || !out || n < 0 || c < 1 || h < 2 || w < 2) return CT_E_BADARG;
    const long long total = (long long)n * h * w;
    if (total == 0) return CT_OK;
    hipLaunchKernelGGL(ct::flow_warp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, flow, out, n, c, h, w);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_convex_upsample_f32(const float *flow, const float *mask, float *out, int b, int h, int w, int factor, void *stream) {
    if (!flow || !mask || !out || b < 0 || h < 1 || w < 1 || factor < 1) return CT_E_BADARG;
    const long long total = (long long)b * h * factor * w * factor;
    if (total == 0) return CT_OK;
    hipLaunchKernelGGL(ct::convex_upsample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flow, mask, out, b, h, w, factor);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_fb_check_f32(const float *fwd, const float *bwd, const float *warped_bwd, const float *warped_fwd, float *fwd_occ, float *bwd_occ,
                    int b, int h, int w, float alpha, float beta, void *stream) {
    if (!fwd || !bwd || !warped_bwd || !warped_fwd || !fwd_occ || !bwd_occ || b < 0) return CT_E_BADARG;
    const long long total = (long long)b * h * w;
    if (total == 0) return CT_OK;
    hipLaunchKernelGGL(ct::fb_check_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fwd, bwd, warped_bwd, warped_fwd,
                       fwd_occ, bwd_occ, b, h, w, alpha, beta);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"

// conv_generic.hip -- the GMFlow matcher's Conv2d for any kernel / stride / channel count (backbone.py, reg_refine.py),
// NCHW float32 on the exact-f32 MFMA, and the space-to-depth pass that turns a stride-2 3x3 into a stride-1 2x2 for
// conv_split.hip.  ct_gconv2d_f32 tries conv_direct.hip and conv_exact.hip's LDS-tiled kernels first (same packed weights).
#include "ct_common.h"
#include "ct_conv.h"
#include "ct_split.h"

namespace ct {

// =================================================================================================
// Generic convolution: M = 64 output channels per workgroup, N = 4 rows x 32 columns of output pixels,
// K = (kh*kw) taps x input channels staged through LDS in chunks.
// =================================================================================================
__global__ __launch_bounds__(256, 2) void conv_generic_kernel(GConvArgs a, int tiles_x, int tiles_y) {
    extern __shared__ float tin[];     // [cchunk][TR][TC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int n = blockIdx.z, mt0 = blockIdx.y * 64;           // first output channel of this workgroup
    const int TR = 3 * a.stride + a.KH, TC = 31 * a.stride + a.KW, CS = TR * TC;
    const int oy0 = ty * 4, ox0 = tx * 32;
    const int iy0 = oy0 * a.stride - a.padH, ix0 = ox0 * a.stride - a.padW;
    const size_t iplane = (size_t)a.H * a.W, oplane = (size_t)a.Ho * a.Wo;
    const float *in = a.in + (size_t)n * a.in_bstride;
    const int cin_pairs = (a.cin + 1) >> 1;
    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    for (int c0 = 0; c0 < a.cin; c0 += a.cchunk) {
        const int cc = (a.cin - c0) < a.cchunk ? (a.cin - c0) : a.cchunk;
        const int ccp = (cc + 1) >> 1;
        __syncthreads();
        for (int idx = tid; idx < 2 * ccp * CS; idx += 256) {
            const int c = idx / CS, rem = idx - c * CS;
            const int yy = rem / TC, xx = rem - yy * TC;
            const int gy = iy0 + yy, gx = ix0 + xx;
            float v = 0.f;
            if (c < cc && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = in[(size_t)(c0 + c) * iplane + (size_t)gy * a.W + gx];
            tin[idx] = v;
        }
        __syncthreads();
        for (int tap = 0; tap < a.KH * a.KW; ++tap) {
            const int ky = tap / a.KW, kx = tap - ky * a.KW;
            const float *brow = tin + hl * CS + (wave * a.stride + ky) * TC + nl * a.stride + kx;
            const float *wrow = a.wp + (((size_t)blockIdx.y * a.KH * a.KW + tap) * cin_pairs + (c0 >> 1)) * 128 + hl * 64 + nl;
            for (int p = 0; p < ccp; ++p) {
                const float b = brow[p * 2 * CS];
                const float w0 = wrow[p * 128], w1 = wrow[p * 128 + 32];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, b, acc[1], 0, 0, 0);
            }
        }
    }
    const int oy = oy0 + wave, ox = ox0 + nl;
    if (oy < a.Ho && ox < a.Wo) {
        float *out = a.out + (size_t)n * a.out_bstride + (size_t)oy * a.Wo + ox;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mt0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                if (co < a.cout) {
                    float v = acc[m][r] + (a.bias ? a.bias[co] : 0.f);
                    out[(size_t)co * oplane] = act<true>(v, a.act);
                }
            }
    }
}

// Space-to-depth by 2: out[n][(2 sy + sx) C + c][y][x] = in[n][c][2y + sy][2x + sx] (sub-position major, so the (0, 0) sub-grid --
// what a stride-2 1x1 convolution reads -- is the first C channels).  A stride-2 3x3 "same" convolution is a stride-1 2x2
// convolution over this tensor (block offsets -1 / 0; the (by, sy) pairs (0,1), (1,0), (1,1) are the rows ky = 0, 1, 2 and (0,0)
// carries zero weights), which the MFMA tile kernel computes (conv_split_kernel<2, 2>): backbone.py:14-17,53,67 and the
// stride-2 trident branch (trident_conv.py:64-72) leave the generic kernel.  One thread: 8 input columns -> 4 + 4 outputs.
__global__ __launch_bounds__(256) void space_to_depth2_kernel(const float *__restrict__ in, float *__restrict__ out, int C, int H, int W,
                                                              long long in_bstride, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // over [n][c][input row][W / 8]
    if (i >= total) return;
    const int w8 = W >> 3, ho = H >> 1, wo = W >> 1;
    const int xg = (int)(i % w8);
    long long r = i / w8;
    const int yin = (int)(r % H); r /= H;
    const int c = (int)(r % C);
    const long long n = r / C;
    const float *src = in + n * in_bstride + ((size_t)c * H + yin) * W + 8 * xg;
    const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
    const int sy = yin & 1, y = yin >> 1;
    float *dst = out + ((size_t)(n * 4 + 2 * sy) * C + c) * ho * wo + (size_t)y * wo + 4 * xg;
    *reinterpret_cast<float4 *>(dst) = make_float4(a.x, a.z, b.x, b.z);                       // sx = 0
    *reinterpret_cast<float4 *>(dst + (size_t)C * ho * wo) = make_float4(a.y, a.w, b.y, b.w);   // sx = 1
}

}  // namespace ct

// -------------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------------
extern "C" {

int ct_gconv2d_f32(const float *in, const float *wp, const float *bias, float *out, int n, int cin, int cout, int h, int w,
                   int kh, int kw, int stride, int pad_h, int pad_w, long long in_bstride, long long out_bstride, int act,
                   void *stream) {
    if (!in || !wp || !out || n < 0 || cin < 1 || cout < 1 || h < 1 || w < 1 || kh < 1 || kw < 1 || stride < 1) return CT_E_BADARG;
    if (n == 0) return CT_OK;
    ct::GConvArgs a;
    a.in = in; a.wp = wp; a.bias = bias; a.out = out;
    a.cin = cin; a.cout = cout; a.coutp = 64 * ((cout + 63) / 64);
    a.H = h; a.W = w; a.KH = kh; a.KW = kw; a.stride = stride; a.padH = pad_h; a.padW = pad_w;
    a.Ho = (h + 2 * pad_h - kh) / stride + 1; a.Wo = (w + 2 * pad_w - kw) / stride + 1;
    if (a.Ho < 1 || a.Wo < 1) return CT_E_BADARG;
    a.in_bstride = in_bstride; a.out_bstride = out_bstride; a.act = act;
    {
        const int rc = ct::conv_direct(a, n, (hipStream_t)stream);      // the shapes an implicit-GEMM tile wastes (conv_direct.hip)
        if (rc != 1) return rc;
    }
    if (stride == 1 && pad_h == kh / 2 && pad_w == kw / 2 && (kh & 1) && (kw & 1) && bias) {
        // stride-1 "same" convolution: the LDS-tiled persistent kernel of conv_exact.hip (same weight layout)
        const ct::ConvArgs f = ct::conv_args(in, wp, bias, nullptr, out, cin, cout, h, w, in_bstride, out_bstride, 0, act, 0, a.coutp / 64);
        const int rc = ct::conv_fast(f, n, kh, kw, (hipStream_t)stream);
        if (rc != 1) return rc;
    }
    const int TR = 3 * stride + kh, TC = 31 * stride + kw;
    int cchunk = (48 * 1024) / (TR * TC * 4);
    cchunk &= ~1;
    if (cchunk > 32) cchunk = 32;
    if (cchunk < 2) return CT_E_BADARG;
    a.cchunk = cchunk;
    const size_t lds = (size_t)cchunk * TR * TC * sizeof(float);
    const int tiles_x = (a.Wo + 31) / 32, tiles_y = (a.Ho + 3) / 4;
    dim3 grid(tiles_x * tiles_y, a.coutp / 64, n);
    hipLaunchKernelGGL(ct::conv_generic_kernel, grid, dim3(256), lds, (hipStream_t)stream, a, tiles_x, tiles_y);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// The generic convolution with explicit top / left zero padding and output size (bottom / right padding is whatever the
// output size implies) -- TF-"SAME" static padding of efficientnet_pytorch's stride-2 stem: pad (0, 1).
int ct_gconv2d_pad_f32(const float *in, const float *wp, const float *bias, float *out, int n, int cin, int cout, int h, int w, int kh,
                       int kw, int stride, int pad_top, int pad_left, int out_h, int out_w, long long in_bstride, long long out_bstride,
                       int act, void *stream) {
    if (!in || !wp || !out || n < 0 || cin < 1 || cout < 1 || h < 1 || w < 1 || kh < 1 || kw < 1 || stride < 1 || pad_top < 0 ||
        pad_left < 0 || out_h < 1 || out_w < 1)
        return CT_E_BADARG;
    if ((out_h - 1) * stride - pad_top >= h || (out_w - 1) * stride - pad_left >= w) return CT_E_BADARG;
    if (n == 0) return CT_OK;
    ct::GConvArgs a;
    a.in = in; a.wp = wp; a.bias = bias; a.out = out;
    a.cin = cin; a.cout = cout; a.coutp = 64 * ((cout + 63) / 64);
    a.H = h; a.W = w; a.KH = kh; a.KW = kw; a.stride = stride; a.padH = pad_top; a.padW = pad_left;
    a.Ho = out_h; a.Wo = out_w;
    a.in_bstride = in_bstride; a.out_bstride = out_bstride; a.act = act;
    const int TR = 3 * stride + kh, TC = 31 * stride + kw;
    int cchunk = (48 * 1024) / (TR * TC * 4);
    cchunk &= ~1;
    if (cchunk > 32) cchunk = 32;
    if (cchunk < 2) return CT_E_BADARG;
    a.cchunk = cchunk;
    const size_t lds = (size_t)cchunk * TR * TC * sizeof(float);
    const int tiles_x = (a.Wo + 31) / 32, tiles_y = (a.Ho + 3) / 4;
    hipLaunchKernelGGL(ct::conv_generic_kernel, dim3(tiles_x * tiles_y, a.coutp / 64, n), dim3(256), lds, (hipStream_t)stream, a, tiles_x,
                       tiles_y);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_space_to_depth2_f32(const float *in, float *out, int n, int c, int h, int w, long long in_bstride, void *stream) {
    if (!in || !out || n < 0 || c < 1 || h < 2 || w < 8 || (h & 1) || (w & 7) || (in_bstride & 3)) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) return CT_E_ALIGN;
    if (n == 0) return CT_OK;
    const long long total = (long long)n * c * h * (w >> 3);
    if ((total + 255) / 256 > 0x7fffffffLL) return CT_E_BADARG;
    hipLaunchKernelGGL(ct::space_to_depth2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, c, h, w,
                       in_bstride, total);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"

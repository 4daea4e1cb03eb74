// ct_conv.h -- argument block of the MFMA convolution kernels (conv_exact.hip, conv_split.hip, conv_ws.hip, conv_wino*.hip), shared
// with conv_generic.hip, and the host helpers every launch goes through
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ct_hip.h"

namespace ct {

struct ConvArgs {
    const float *in;
    const float *in2;       // split kernel only: channels >= cin1 come from this tensor (torch.cat on dim 1 without the copy); or NULL
    int cin1;               // channels of `in` when in2 != NULL (a multiple of 16)
    long long in2_bstride;
    const float *wp;
    const float *bias;      // [MT*32], zero padded
    const float *residual;  // nullable, same shape/strides as out
    float *out;
    int cin, cout, H, W;
    long long in_bstride, out_bstride, res_bstride;   // elements between images of a batch
    int act;     // 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 sigmoid, 4 tanh
    int clamp;   // 1 = clamp to [0,1]
    int groups;  // output-channel groups of MT*32 (weights packed group-major); 1 for cout <= 64
    unsigned long long *prof;   // phase stamps of a -DCT_STAMPS build (ct_stamps.h); NULL otherwise
    int n_images = 0;           // conv_ws only (set by its launcher)
    const float *in3 = nullptr;  // split kernel only: channels >= cin2 come from this tensor (a third torch.cat operand); cin2 % 16 == 0
    int cin2 = 0;
    long long in3_bstride = 0;
    int f16 = 0;                // conv_ws only: 1 = two fp16 pieces (weights scaled by 2^w_exp), 0 = three bf16 pieces
    int w_exp = 0;
    int rows_channels = 0;      // split kernel only: > 0 = `out` is a token-rows tensor [N*H, W, rows_channels] and the result goes to its
    int post_op = 0;            // split kernel, F16 form, NCHW output: 1 = result * p1; 2 = (1 - p1) * p2 + p1 * result (the GRU gate of
    const float *p1 = nullptr;  // reg_refine.py:46-55: p1 = z, p2 = h), applied after the activation; p1 / p2 laid out like `out`
    const float *p2 = nullptr;
    int res_pre = 0;            // split kernel only: 1 = `residual` is added BEFORE the activation (a pre-computed partial convolution)
    int rows_c0 = 0;            // channels rows_c0 .. rows_c0 + cout (multiples of 4); no residual / clamp in this mode
    float *sk_ws = nullptr;         // split kernel, F16 form: stream-K scratch (partial tiles, one 64 KiB slot per workgroup), or NULL
    unsigned int *sk_flags = nullptr;   // ... and its flags (one per workgroup; zero between launches)
    unsigned int sk_epoch = 1;      // ... the value a producer of THIS launch publishes (non-zero, new for every launch: a flag left behind
                                    //     by a producer that came too late for its consumer cannot satisfy the next launch's wait)
};

// The fields every entry point fills; the rest keep their defaults (one input tensor, no stamps).
inline ConvArgs conv_args(const float *in, const void *wp, const float *bias, const float *residual, float *out, int cin, int cout, int h,
                          int w, long long in_bstride, long long out_bstride, long long res_bstride, int act, int clamp, int groups) {
    ConvArgs a;
    a.in = in; a.in2 = nullptr; a.cin1 = cin; a.in2_bstride = 0;
    a.wp = reinterpret_cast<const float *>(wp); a.bias = bias; a.residual = residual; a.out = out;
    a.cin = cin; a.cout = cout; a.H = h; a.W = w;
    a.in_bstride = in_bstride; a.out_bstride = out_bstride; a.res_bstride = res_bstride;
    a.act = act; a.clamp = clamp; a.groups = groups; a.prof = nullptr;
    return a;
}

// Argument and alignment checks of the two 16-bit-form 3x3 entries (ct_conv3x3_ws16_f32, ct_conv3x3_wino16_f32): CT_OK or the error
inline int conv3x3_16_check(const float *in, const void *wp16, int w_exp, const float *bias, const float *residual, const float *out, int n,
                            int cin, int cout, int h, int w, long long in_bstride, long long out_bstride, long long res_bstride, int act) {
    if (!in || !wp16 || !bias || !out || n < 0 || cin <= 32 || cin > 64 || cout < 1 || h < 0 || w < 0 || act < 0 || act > 5) return CT_E_BADARG;
    if ((w % 4) || (reinterpret_cast<uintptr_t>(in) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(wp16) & 15) ||
        (in_bstride % 4) || (out_bstride % 4) || (residual && ((reinterpret_cast<uintptr_t>(residual) & 15) || (res_bstride % 4))))
        return CT_E_ALIGN;
    if (w_exp < -100 || w_exp > 100) return CT_E_BADARG;
    return CT_OK;
}

struct GConvArgs {
    const float *in, *wp, *bias;   // wp: [coutp/64][kh*kw][cin_pairs][2][64], coutp = 64*ceil(cout/64); bias padded to coutp (or null)
    float *out;
    int cin, cout, coutp, H, W, Ho, Wo, KH, KW, stride, padH, padW;
    long long in_bstride, out_bstride;
    int act;      // 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 sigmoid, 4 tanh, 5 swish
    int cchunk;   // input channels staged per LDS pass (even)
};

// conv_direct.hip: float32 VALU convolutions for the shapes an implicit-GEMM tile wastes (returns 1 if the shape is not theirs):
//   cout <= 4, kernel 3x3 / 1x1, stride 1, "same" padding (GMFlow's flow head: 256 -> 2), and
//   cin <= 3, kernel <= 7x7, stride 1 or 2 (its 7x7 stem 3 -> 64 and the motion encoder's 7x7 on the 2-channel flow)
int conv_direct(const GConvArgs &a, int N, hipStream_t s);

// conv_exact.hip: stride-1, padding k/2, kernel 3x3 / 1x1 / 1x5 / 5x1, weights packed [group][tap][cin_pair][2][64];
// returns CT_OK / an error, or 1 if (kh, kw) has no LDS-tiled kernel
int conv_fast(const ConvArgs &a, int N, int kh, int kw, hipStream_t s);

// conv_ws.hip: 3x3, 32 < cin <= 64, one input tensor: weights stationary in registers, contraction split across the waves;
// returns CT_OK / an error, or 1 if the geometry is not this kernel's
int conv_ws(const ConvArgs &a, int N, bool gen, hipStream_t s);

// conv_wino.hip / conv_wino4.hip: the same convolution as Winograd F(2x2, 3x3) on two fp16 pieces (weights packed by
// ct_hip.pack_conv_weight_wino16); 1 = not this kernel's geometry
int conv_wino(const ConvArgs &a, int N, hipStream_t s);
int conv_wino4(const ConvArgs &a, int N, hipStream_t s);

// conv_split.hip: sticky status of the current device for ct_device_status (abi.hip): 1 = a stream-K consumer gave up waiting
// for its producer since the last clear, -1 = the device could not be read
int conv_split_read_status(bool clear);

}  // namespace ct

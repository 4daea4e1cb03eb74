"""Host-side weight packers and the named records in which packed operands travel with a weight tensor.  Pure torch: no
library call, no GPU."""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from ._core import CtHipError, _cached_pack


class SplitOperands(NamedTuple):
    """What the split-family convolution kernels read, attached to a packed weight as `_ct_split`"""
    bf16: torch.Tensor                                  # three bf16 pieces (pack_conv_weight_split)
    bias: torch.Tensor                                  # zero-padded to 64 * ceil(cout / 64)
    f16: Optional[Tuple[torch.Tensor, int]] = None      # (two fp16 pieces, w_exp): pack_conv_weight_split16, or None
    wino: Optional[Tuple[torch.Tensor, int]] = None     # (Winograd image, w_exp): pack_conv_weight_wino16, or None


class ConvSource(NamedTuple):
    """The Conv2d parameters a 3x3 packing was made from (`_ct_src`): a stride-2 use builds its space-to-depth form from them"""
    weight: torch.Tensor
    bias: Optional[torch.Tensor]


def _bf16_pieces(w):
    """float32 -> its three bf16 pieces hi / mid / lo as int16 bit patterns [3, *w.shape]"""
    hi = w.to(torch.bfloat16)
    r1 = w - hi.float()
    r1 = torch.where(torch.isfinite(r1), r1, torch.zeros_like(r1))
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo], dim=0).view(torch.int16)


def _fp16_pieces(w):
    """float32 -> (the two fp16 pieces hi / lo of w * 2^w_exp as int16 bit patterns [2, *w.shape], w_exp): w_exp, clamped to
    +-100, puts the largest magnitude into [2^11, 2^12), so both pieces of all but the tiniest elements are normal fp16 numbers"""
    amax = float(w.abs().max())
    w_exp = 0 if not (amax > 0 and amax < float("inf")) else 12 - (int(np.floor(np.log2(amax))) + 1)
    w_exp = max(-100, min(100, w_exp))
    ws = w * (2.0 ** w_exp)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=0).view(torch.int16), w_exp


def _padded(weight, coutp, cinp, dtype=torch.float32):
    cout, cin, kh, kw = weight.shape
    w = torch.zeros((coutp, cinp, kh, kw), dtype=dtype, device=weight.device)
    w[:cout, :cin] = weight.detach().to(dtype)
    return w


def _padded_bias(bias, coutp, cout, device):
    b = torch.zeros(coutp, dtype=torch.float32, device=device)
    if bias is not None:
        b[:cout] = bias.detach().float()
    return b


def pack_conv_weight_split(weight, bias):
    """Conv2d parameters -> ct_conv2d_split_f32 operands: bf16 bit patterns (int16)
    [ceil(cout/64)][ceil(cin/16)][kh*kw][piece hi/mid/lo][m 0..1][k-half 0..1][cout%32][8 channels], and the bias
    zero-padded to 64*ceil(cout/64)."""
    cout, cin, kh, kw = weight.shape
    g, nc = (cout + 63) // 64, (cin + 15) // 16
    pieces = _bf16_pieces(_padded(weight, g * 64, nc * 16))                # [3][coutp][cinp][kh][kw]
    pieces = pieces.reshape(3, g, 2, 32, nc, 2, 8, kh * kw)                # piece, g, m, r, chunk, h, j, tap
    ws = pieces.permute(1, 4, 7, 0, 2, 5, 3, 6).contiguous()               # g, chunk, tap, piece, m, h, r, j
    return ws, _padded_bias(bias, g * 64, cout, weight.device)


def pack_conv_weight_split16(weight):
    """3x3 Conv2d weight (32 < cin <= 64) -> ct_conv3x3_ws16_f32 operand: fp16 bit patterns (int16)
    [ceil(cout/64)][ceil(cin/16)][9][piece hi/lo][m 0..1][k-half 0..1][cout%32][8 channels] of weight * 2^w_exp, and w_exp
    (the largest |weight| lands in [2^11, 2^12): both pieces of all but the tiniest weights are normal fp16 numbers)."""
    cout, cin, kh, kw = weight.shape
    g, nc = (cout + 63) // 64, (cin + 15) // 16
    pieces, w_exp = _fp16_pieces(_padded(weight, g * 64, nc * 16))         # [2][coutp][cinp][kh][kw]
    pieces = pieces.reshape(2, g, 2, 32, nc, 2, 8, kh * kw)                # piece, g, m, r, chunk, h, j, tap
    return pieces.permute(1, 4, 7, 0, 2, 5, 3, 6).contiguous(), w_exp      # g, chunk, tap, piece, m, h, r, j


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def pack_conv_weight_wino16(weight):
    """3x3 Conv2d weight (32 < cin <= 64) -> ct_conv3x3_wino16_f32 operand: the Winograd F(2x2, 3x3) image U = G g G^T (float64,
    rounded once to float32), times 2^w_exp (largest |U| in [2^11, 2^12)), as fp16 hi / lo bit patterns (int16)
    [ceil(cout/64)][16 positions][4 cout blocks][2 cin chunks][piece][64 lanes][8]: lane l of a fragment holds cout 16 mb + l % 16,
    cin 32 kc + 8 (l / 16) + 0..7 (the A operand of v_mfma_f32_16x16x32_f16).  Returns (image, w_exp)."""
    cout, cin, kh, kw = weight.shape
    assert (kh, kw) == (3, 3) and cin <= 64
    g = (cout + 63) // 64
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=weight.device)
    u = torch.einsum("ij,kcjl,ml->kcim", G, _padded(weight, g * 64, 64, torch.float64), G).float()     # [coutp][64][4][4]
    pieces, w_exp = _fp16_pieces(u)                                        # [piece][coutp][64][4][4]
    pieces = pieces.reshape(2, g, 4, 16, 2, 4, 8, 16)                      # piece, g, mb, m, kc, kblk, e, p
    img = pieces.permute(1, 7, 2, 4, 0, 5, 3, 6).contiguous()              # g, p, mb, kc, piece, kblk, m, e  (lane = 16 kblk + m)
    return img.reshape(g, 16, 4, 2, 2, 64, 8), w_exp


def _split_operands(weight, bias):
    """the SplitOperands of a Conv2d: the fp16 image for the tap shapes the tile kernels take in that form, the Winograd image for
    the 3x3 shapes ct_conv3x3_wino16_f32 takes"""
    cout, cin, kh, kw = weight.shape
    w16 = pack_conv_weight_split16(weight) if (kh, kw) in ((3, 3), (1, 1), (1, 5), (5, 1), (2, 2)) else None
    wq = pack_conv_weight_wino16(weight) if (kh, kw) == (3, 3) and 32 < cin <= 64 else None
    return SplitOperands(*pack_conv_weight_split(weight, bias), w16, wq)


def pack_conv_weight(weight, bias):
    """torch Conv2d parameters -> the MFMA A-operand layout of ct_conv2d_f32 (include/ct_hip.h):
    wp[tap][cin_pair][2][32*ceil(cout/32)], bias zero padded."""
    cout, cin, kh, kw = weight.shape
    assert kh == kw and kh in (1, 3)
    coutp = 32 * ((cout + 31) // 32)
    cinp = 2 * ((cin + 1) // 2)
    wp = _padded(weight, coutp, cinp).permute(2, 3, 1, 0).reshape(kh * kw, cinp // 2, 2, coutp).contiguous()
    wp._ct_split = _split_operands(weight, bias)      # operands of the split kernels travel with the packing
    return wp, _padded_bias(bias, coutp, cout, weight.device)


def pack_gconv_weight(weight, bias):
    """Conv2d parameters -> ct_gconv2d_f32 layout: output channels in groups of 64 (zero padded),
    wp[ceil(cout/64)][kh*kw][ceil(cin/2)][2][64]; bias zero padded to 64*ceil(cout/64) (zeros when the conv has none)."""
    cout, cin, kh, kw = weight.shape
    coutp, cinp = 64 * ((cout + 63) // 64), 2 * ((cin + 1) // 2)
    # [g][co64][cin_pair][2][kh][kw] -> [g][kh][kw][cin_pair][2][co64]
    wp = _padded(weight, coutp, cinp).reshape(coutp // 64, 64, cinp // 2, 2, kh, kw).permute(0, 4, 5, 2, 3, 1).contiguous()
    wp = wp.reshape(coutp // 64, kh * kw, cinp // 2, 2, 64)
    if kh * kw <= 9:
        wp._ct_split = _split_operands(weight, bias)
    if (kh, kw) == (3, 3):
        wp._ct_src = ConvSource(weight, bias)         # first stride-2 use: _split_s2d
    return wp, _padded_bias(bias, coutp, cout, weight.device)


def _split_s2d(wp):
    """the 2x2 / 4c form of a 3x3 stride-2 convolution's weight (include/ct_hip.h: ct_space_to_depth2_f32) as SplitOperands, cached
    on the packing (`_ct_split_s2d`) for the current state of the parameters"""
    weight, bias = wp._ct_src

    def pack():
        cout, cin = weight.shape[:2]
        w2 = torch.zeros((cout, 4, cin, 2, 2), dtype=torch.float32, device=weight.device)
        wd = weight.detach().float()
        taps = {0: (0, 1), 1: (1, 0), 2: (1, 1)}           # k -> (block offset index, sub-position): 2 o + k - 1 = 2 (o + b - 1) + s
        for ky, (by, sy) in taps.items():
            for kx, (bx, sx) in taps.items():
                w2[:, 2 * sy + sx, :, by, bx] = wd[:, :, ky, kx]
        return _split_operands(w2.reshape(cout, 4 * cin, 2, 2), bias)
    ver = (weight._version, weight.data_ptr(), None if bias is None else (bias._version, bias.data_ptr()))
    return _cached_pack(wp, "_ct_split_s2d", ver, pack)


def pack_linear_weight_split(weight):
    """nn.Linear weight [N, K] (K % 32 == 0) -> ct_linear_tokens_split_f32's operand: bf16 bit patterns (int16)
    [ceil(N/128)][K/32][piece hi/mid/lo][8-channel group 0..3][feature row 0..127][8 channels], zero rows beyond N."""
    n, k = weight.shape
    nt, nc = (n + 127) // 128, k // 32
    w = torch.zeros((nt * 128, k), dtype=torch.float32, device=weight.device)
    w[:n] = weight.detach().float()
    pieces = _bf16_pieces(w).reshape(3, nt, 128, nc, 4, 8)                 # piece, tile, row, chunk, group, j
    return pieces.permute(1, 3, 0, 4, 2, 5).contiguous()                   # tile, chunk, piece, group, row, j


def pack_linear_weight_ws16(weight):
    """Linear weight [N, K] -> ct_linear_ws16_f32 operand: slices of 256 input channels x 128 output features as fp16 (hi, lo) bit
    patterns (int16) [slice][piece][k step 0..15][lane half 0..1][feature 0..127][8 channels] of weight * 2^w_exp, channel of
    (k step s, half h, j) = 128 h + 8 s + j within the slice; K == 256: N / 128 feature slices, else (N == 128): K / 256 channel
    slices.  Returns (image, w_exp); the largest |weight| lands in [2^11, 2^12)."""
    n, k = weight.shape
    pieces, w_exp = _fp16_pieces(weight.detach().float())                  # [2][N][K]
    if k == 256 and n % 128 == 0:
        img = pieces.reshape(2, n // 128, 128, 2, 16, 8).permute(1, 0, 4, 3, 2, 5)       # slice, piece, s, h, f, j
    elif n == 128 and k % 256 == 0:
        img = pieces.reshape(2, 128, k // 256, 2, 16, 8).permute(2, 0, 4, 3, 1, 5)
    elif k == 128 and n % 128 == 0:                                        # 128-channel slices: channel = 64 h + 8 s + j, s < 8
        img = pieces.reshape(2, n // 128, 128, 2, 8, 8).permute(1, 0, 4, 3, 2, 5)
    else:
        raise CtHipError("pack_linear_weight_ws16: K in (128, 256) with N % 128 == 0, or N == 128 with K % 256 == 0")
    return img.contiguous(), w_exp

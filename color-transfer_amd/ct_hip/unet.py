"""Layers of DMSCT's EfficientNet-B2 / U-Net (csrc/unet.hip)."""
import torch

from ._core import (ACT_NONE, ACT_SWISH, CtHipError, SIGNATURES, _c_int, _c_ll, _c_p, _f32c, _nchw_bstride, _opt, _ptr, _stream, check,
                    lib)

SIGNATURES.update({
    "ct_gconv2d_pad_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 12 + [_c_ll, _c_ll, _c_int, _c_p]),
    "ct_dwconv_tiles": (_c_int, [_c_int, _c_int]),
    "ct_dwconv_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 11 + [_c_p, _c_p]),
    "ct_se_gate_f32": (_c_int, [_c_p, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p]),
    "ct_scale_planes_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_p]),
    "ct_upsample2_concat_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p]),
})


def gconv2d_pad(x, wp, bias, cout, ksize, stride, pad_top_left, out_size, act=ACT_NONE):
    """generic convolution with explicit (top, left) zero padding and output size (TF-"SAME" static padding)"""
    _f32c(x)
    n, cin, h, w = x.shape
    out = torch.empty((n, cout, out_size[0], out_size[1]), dtype=torch.float32, device=x.device)
    check(lib().ct_gconv2d_pad_f32(_ptr(x), _ptr(wp), _opt(bias), _ptr(out), n, cin, cout, h, w, ksize, ksize, stride, pad_top_left[0],
                                   pad_top_left[1], out_size[0], out_size[1], _nchw_bstride(x), _nchw_bstride(out), int(act), _stream()))
    return out


def dwconv(x, weight, bias, ksize, stride, pad_top_left, out_size, act=ACT_SWISH, want_sums=False):
    """depthwise convolution, weight [C, k*k] and bias [C] with the BatchNorm folded in; -> out (, tile sums [N, C, tiles])"""
    _f32c(x, weight, bias)
    n, c, h, w = x.shape
    out = torch.empty((n, c, out_size[0], out_size[1]), dtype=torch.float32, device=x.device)
    sums = None
    if want_sums:
        sums = torch.empty((n, c, lib().ct_dwconv_tiles(out_size[0], out_size[1])), dtype=torch.float32, device=x.device)
    check(lib().ct_dwconv_f32(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), n, c, h, w, ksize, stride, pad_top_left[0], pad_top_left[1],
                              out_size[0], out_size[1], int(act), _opt(sums), _stream()))
    return (out, sums) if want_sums else out


def se_gate(tile_sums, plane, w_reduce, b_reduce, w_expand, b_expand):
    """squeeze-and-excitation gate [N, C] from the tile sums of the depthwise output"""
    _f32c(tile_sums, w_reduce, b_reduce, w_expand, b_expand)
    n, c, tiles = tile_sums.shape
    gate = torch.empty((n, c), dtype=torch.float32, device=tile_sums.device)
    check(lib().ct_se_gate_f32(_ptr(tile_sums), tiles, plane, _ptr(w_reduce), _ptr(b_reduce), _ptr(w_expand), _ptr(b_expand), _ptr(gate),
                               n, c, w_reduce.shape[0], _stream()))
    return gate


def scale_planes_(x, gate):
    """x[n, c] *= gate[n, c] in place"""
    _f32c(x, gate)
    n, c, h, w = x.shape
    check(lib().ct_scale_planes_f32(_ptr(x), _ptr(gate), n * c, h * w, _stream()))
    return x


def upsample2_concat(x, skip=None):
    """cat([nearest-x2(x), skip], dim=1)"""
    _f32c(x, skip)
    n, cx, h, w = x.shape
    cs = 0 if skip is None else skip.shape[1]
    if skip is not None and tuple(skip.shape) != (n, cs, 2 * h, 2 * w):
        raise CtHipError("upsample2_concat: skip must be [N, Cs, 2H, 2W]")
    out = torch.empty((n, cx + cs, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
    check(lib().ct_upsample2_concat_f32(_ptr(x), _opt(skip), _ptr(out), n, cx, cs, h, w, _stream()))
    return out

"""Layers of DMSCT's EfficientNet-B2 / U-Net (csrc/unet.hip).

The kernels index their operands with C, k * k, NSQ and the tile count taken from OTHER arguments, so every wrapper here checks
the operand shapes first and raises CtHipError before anything is allocated or launched: a [C, 9] weight passed with ksize=5 must
never become an out-of-bounds read on the device."""
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


def _want_shape(fn, name, t, shape):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise CtHipError("%s: %s must be %s, got %s" % (fn, name, list(shape), got))


def _want_nchw(fn, x):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise CtHipError("%s: x must be a [N, C, H, W] tensor" % fn)
    return tuple(x.shape)


def gconv2d_pad(x, wp, bias, cout, ksize, stride, pad_top_left, out_size, act=ACT_NONE):
    """generic convolution with explicit (top, left) zero padding and output size (TF-"SAME" static padding).
    wp / bias come from pack_gconv_weight: the packing [ceil(cout/64), k*k, ceil(cin/2), 2, 64] exposes the kernel size exactly
    and the channel counts up to its zero padding (cin to a pair, cout to 64), which is what the kernel reads -- those are checked
    here; a 3x3 packing also carries the Conv2d weight it was made from (`_ct_src`), and then cin and cout are checked exactly.
    For other kernel sizes an odd cin one below the packed pair, or a cout inside the same group of 64, cannot be told apart:
    the kernel then reads the packing's zero rows, never past it."""
    n, cin, h, w = _want_nchw("gconv2d_pad", x)
    cout, ksize = int(cout), int(ksize)
    if cout < 1 or ksize < 1:
        raise CtHipError("gconv2d_pad: cout and ksize must be positive")
    groups = (cout + 63) // 64
    _want_shape("gconv2d_pad", "the packed weight", wp, (groups, ksize * ksize, (cin + 1) // 2, 2, 64))
    if bias is not None:
        _want_shape("gconv2d_pad", "the packed bias", bias, (64 * groups,))
    src = getattr(wp, "_ct_src", None)
    if src is not None and tuple(src.weight.shape[:2]) != (cout, cin):
        raise CtHipError("gconv2d_pad: the weight was packed for %d -> %d channels, the call has %d -> %d"
                         % (src.weight.shape[1], src.weight.shape[0], cin, cout))
    _f32c(x, wp, bias)
    out = torch.empty((n, cout, out_size[0], out_size[1]), dtype=torch.float32, device=x.device)
    check(lib().ct_gconv2d_pad_f32(_ptr(x), _ptr(wp), _opt(bias), _ptr(out), n, cin, cout, h, w, ksize, ksize, stride, pad_top_left[0],
                                   pad_top_left[1], out_size[0], out_size[1], _nchw_bstride(x), _nchw_bstride(out), int(act), _stream()))
    return out


def dwconv(x, weight, bias, ksize, stride, pad_top_left, out_size, act=ACT_SWISH, want_sums=False):
    """depthwise convolution, weight [C, k*k] and bias [C] with the BatchNorm folded in; -> out (, tile sums [N, C, tiles])"""
    n, c, h, w = _want_nchw("dwconv", x)
    if ksize not in (3, 5) or stride not in (1, 2):
        raise CtHipError("dwconv: ksize must be 3 or 5 and stride 1 or 2, got %r and %r" % (ksize, stride))
    _want_shape("dwconv", "weight", weight, (c, ksize * ksize))
    _want_shape("dwconv", "bias", bias, (c,))
    _f32c(x, weight, bias)
    out = torch.empty((n, c, out_size[0], out_size[1]), dtype=torch.float32, device=x.device)
    sums = None
    if want_sums:
        sums = torch.empty((n, c, lib().ct_dwconv_tiles(out_size[0], out_size[1])), dtype=torch.float32, device=x.device)
    check(lib().ct_dwconv_f32(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), n, c, h, w, ksize, stride, pad_top_left[0], pad_top_left[1],
                              out_size[0], out_size[1], int(act), _opt(sums), _stream()))
    return (out, sums) if want_sums else out


def se_gate(tile_sums, plane, w_reduce, b_reduce, w_expand, b_expand):
    """squeeze-and-excitation gate [N, C] from the tile sums [N, C, tiles] of the depthwise output; w_reduce [NSQ, C], b_reduce
    [NSQ], w_expand [C, NSQ], b_expand [C]"""
    if not isinstance(tile_sums, torch.Tensor) or tile_sums.dim() != 3:
        raise CtHipError("se_gate: tile_sums must be [N, C, tiles]")
    n, c, tiles = tile_sums.shape
    if not isinstance(w_reduce, torch.Tensor) or w_reduce.dim() != 2:
        raise CtHipError("se_gate: w_reduce must be [NSQ, C]")
    nsq = w_reduce.shape[0]
    _want_shape("se_gate", "w_reduce", w_reduce, (nsq, c))
    _want_shape("se_gate", "b_reduce", b_reduce, (nsq,))
    _want_shape("se_gate", "w_expand", w_expand, (c, nsq))
    _want_shape("se_gate", "b_expand", b_expand, (c,))
    _f32c(tile_sums, w_reduce, b_reduce, w_expand, b_expand)
    gate = torch.empty((n, c), dtype=torch.float32, device=tile_sums.device)
    check(lib().ct_se_gate_f32(_ptr(tile_sums), tiles, plane, _ptr(w_reduce), _ptr(b_reduce), _ptr(w_expand), _ptr(b_expand), _ptr(gate),
                               n, c, nsq, _stream()))
    return gate


def scale_planes_(x, gate):
    """x[n, c] *= gate[n, c] in place"""
    n, c, h, w = _want_nchw("scale_planes_", x)
    _want_shape("scale_planes_", "gate", gate, (n, c))
    _f32c(x, gate)
    if x.numel() == 0:                                       # an empty tensor has no address to hand to the library
        return x
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

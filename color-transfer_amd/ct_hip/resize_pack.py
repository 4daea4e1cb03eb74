"""Resampling (bicubic, bilinear) and the float32 -> uint8 frame pack."""
import ctypes

import numpy as np
import torch

from ._core import CtHipError, SIGNATURES, _c_f, _c_i64, _c_int, _c_p, _c_sz, _f32c, _ptr, _require_cuda, _stream, check, lib

SIGNATURES.update({
    "ct_pack_u8_f32": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "ct_bicubic_resize_workspace_bytes": (_c_sz, [_c_i64, _c_int, _c_int, _c_int]),
    "ct_bicubic_resize_f32": (_c_int, [_c_p, _c_p, _c_i64, _c_int, _c_int, _c_int, _c_int, ctypes.c_double, ctypes.c_double, _c_int,
                                       _c_p, _c_sz, _c_p]),
    "ct_bilinear_resize_f32": (_c_int, [_c_p, _c_p] + [_c_int] * 6 + [_c_f, _c_f, _c_p]),
})

CT_PACK_HWC, CT_PACK_CHW = 0, 1
PACK_LAYOUTS = {"hwc": CT_PACK_HWC, "chw": CT_PACK_CHW}


def pack_u8(x, layout=None, out=None):
    """Corrected float32 frames -> uint8 [n,H,W,3]: rint(clamp(x, 0, 1) * 255), ties to even, NaN -> 0 (ct_pack_u8_f32; the
    reference's img_as_ubyte(x.clip(0, 1)), utils/postprocess.py:138).  x: [n,3,H,W] ("chw") or [n,H,W,3] ("hwc"), or one
    frame of either as a 3-D tensor.  layout is inferred from the shape and required when both readings fit.  out: an optional
    preallocated uint8 [n,H,W,3] tensor on the same device.  Asynchronous on the current stream; nothing is allocated with out."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise CtHipError("pack_u8 needs a [n,3,H,W] / [n,H,W,3] tensor or one frame of either")
    _require_cuda(x)
    if x.dtype != torch.float32:
        raise CtHipError("pack_u8 needs float32 frames (got %s)" % x.dtype)
    xb = x if x.dim() == 4 else x.unsqueeze(0)
    chw, hwc = xb.shape[1] == 3, xb.shape[3] == 3
    if layout is None:
        if chw == hwc:
            raise CtHipError("pack_u8: %s of shape %s; pass layout='chw' or 'hwc'"
                             % ("both layouts fit a tensor" if chw else "neither layout fits a tensor", tuple(x.shape)))
        layout = "chw" if chw else "hwc"
    if layout not in PACK_LAYOUTS or not (chw if layout == "chw" else hwc):
        raise CtHipError("pack_u8: layout %r does not fit shape %s" % (layout, tuple(x.shape)))
    n = xb.shape[0]
    h, w = (xb.shape[2], xb.shape[3]) if layout == "chw" else (xb.shape[1], xb.shape[2])
    shape = (n, h, w, 3) if x.dim() == 4 else (h, w, 3)               # one frame in, one frame out
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != x.device or tuple(out.shape) not in (shape, (n, h, w, 3)):
            raise CtHipError("pack_u8: out must be a uint8 %s tensor on %s" % (list(shape), x.device))
        _require_cuda(out)
    if x.numel():
        check(lib().ct_pack_u8_f32(_ptr(xb), PACK_LAYOUTS[layout], n, h, w, _ptr(out), _stream()))
    return out


def _pair(v, name, kind):
    """one value for both axes, or an (h, w) pair"""
    vs = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(vs) != 2 or any(isinstance(a, bool) or not isinstance(a, kind) for a in vs):
        raise CtHipError("%s must be one %s or an (h, w) pair of them (got %r)" % (name, "int" if kind == (int,) else "number", v))
    return vs


def resize_geometry(in_hw, size=None, scale_factor=None):
    """The shape rule of torch.nn.functional.interpolate(align_corners=False) for a [.., h, w] input: ((ho, wo), (scale_h, scale_w)).
    With scale_factor the output is floor(in * scale_factor) and the source step per output pixel is 1 / scale_factor (the
    factor itself, not in / out, as torch does without recompute_scale_factor); with size it is in / out.  Exactly one of the two
    is given; each is one number or an (h, w) pair.  The steps are Python floats (float64) and go to the kernel as such.  Pure
    Python: no GPU, no library."""
    if (size is None) == (scale_factor is None):
        raise CtHipError("exactly one of size and scale_factor must be given")
    ins = _pair(in_hw, "in_hw", (int,))
    if min(ins) < 1:
        raise CtHipError("in_hw must be positive (got %r)" % (in_hw,))
    if size is not None:
        outs = _pair(size, "size", (int,))
        if min(outs) < 1:
            raise CtHipError("size must be positive (got %r)" % (size,))
        return (int(outs[0]), int(outs[1])), (ins[0] / outs[0], ins[1] / outs[1])
    fs = tuple(float(f) for f in _pair(scale_factor, "scale_factor", (int, float)))
    if not all(0.0 < f < float("inf") for f in fs):
        raise CtHipError("scale_factor must be positive and finite (got %r)" % (scale_factor,))
    outs = tuple(int(np.floor(float(i * f))) for i, f in zip(ins, fs))
    if min(outs) < 1:
        raise CtHipError("scale_factor %r leaves no pixel of a %d x %d input" % (scale_factor, ins[0], ins[1]))
    return outs, (1.0 / fs[0], 1.0 / fs[1])


def bicubic_resize(x, size=None, scale_factor=None, antialias=False, out=None):
    """torch.nn.functional.interpolate(x, size / scale_factor, mode="bicubic", align_corners=False, antialias=antialias) on a
    float32 [n,c,h,w] device tensor (ct_bicubic_resize_f32, csrc/resize.hip): coordinates and weights in float64, the result not
    clamped.  Exactly one of size and scale_factor (see resize_geometry).  out: an optional preallocated float32 [n,c,ho,wo] tensor
    on the same device.  Asynchronous on the current stream; with antialias a float32 [n,c,h,wo] intermediate is allocated."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise CtHipError("bicubic_resize needs a [n,c,h,w] tensor")
    (ho, wo), (sh, sw) = resize_geometry((x.shape[2], x.shape[3]), size=size, scale_factor=scale_factor)
    _require_cuda(x)
    if x.dtype != torch.float32:
        raise CtHipError("bicubic_resize needs a float32 tensor (got %s)" % x.dtype)
    n, c, h, w = x.shape
    shape = (n, c, ho, wo)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != x.device or tuple(out.shape) != shape:
            raise CtHipError("bicubic_resize: out must be a float32 %s tensor on %s" % (list(shape), x.device))
        _require_cuda(out)
    if n * c:
        tmp = torch.empty((n * c, h, wo), dtype=torch.float32, device=x.device) if antialias else None
        check(lib().ct_bicubic_resize_f32(_ptr(x), _ptr(out), n * c, h, w, ho, wo, sh, sw, 1 if antialias else 0,
                                          _ptr(tmp) if antialias else None, tmp.numel() * 4 if antialias else 0, _stream()))
    return out


def bilinear_resize(x, size, mul0=1.0, mul1=1.0):
    _f32c(x)
    n, c, h, w = x.shape
    out = torch.empty((n, c, size[0], size[1]), dtype=torch.float32, device=x.device)
    check(lib().ct_bilinear_resize_f32(_ptr(x), _ptr(out), n, c, h, w, size[0], size[1], float(mul0), float(mul1), _stream()))
    return out

"""What the entries on uint8 frame groups share (idt_u8, regrain_u8, acg_u8, mk on bytes): the argument rules, raised as CtHipError
before any C call, and the shape of what they return."""
import ctypes

import numpy as np
import torch

from ._core import CtHipError, _as_batch, _ptr, _require_cuda

_NULL = ctypes.c_void_p(0)
_U8_OUT = (torch.uint8, torch.float32, torch.float64)


def _u8_frames(t, name, fn, dtype=torch.uint8):
    """a [H,W,3] / [B,H,W,3] device tensor of `dtype` (the uint8 frames) -> its [B,H,W,3] view; every argument error is raised here"""
    if not isinstance(t, torch.Tensor):
        raise CtHipError("%s: %s must be a tensor, got %s" % (fn, name, type(t).__name__))
    if t.dtype != dtype:
        raise CtHipError("%s: %s must be %s, got %s" % (fn, name, str(dtype).replace("torch.", ""), t.dtype))
    x, _ = _as_batch(t)
    if x.shape[-1] != 3:
        raise CtHipError("%s: %s must be [H,W,3] or [B,H,W,3], got %s" % (fn, name, tuple(t.shape)))
    if x.numel() == 0:
        raise CtHipError("%s: %s is empty %s" % (fn, name, tuple(t.shape)))
    _require_cuda(x)
    return x


def _u8_outputs(x, out, out_dtype, fn):
    """the `out` / `out_dtype` rule of the uint8 entries -> (the tensors as given, {dtype: tensor})"""
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    if out is None:
        if out_dtype not in _U8_OUT:
            raise CtHipError("%s writes uint8, float32 or float64, not %s (out_dtype)" % (fn, out_dtype))
        outs = [torch.empty(x.shape, dtype=out_dtype, device=x.device)]
    slots = {}
    for o in outs:
        if not isinstance(o, torch.Tensor) or o.dtype not in _U8_OUT:
            raise CtHipError("%s: out takes uint8, float32 or float64 tensors, got %s" % (fn, getattr(o, "dtype", type(o).__name__)))
        _require_cuda(o)
        if o.device != x.device:
            raise CtHipError("%s: out is on %s, the input on %s" % (fn, o.device, x.device))
        if o.numel() != x.numel():
            raise CtHipError("%s: out has %d elements, the target %d" % (fn, o.numel(), x.numel()))
        if o.dtype in slots:
            raise CtHipError("%s: two outputs (out) of dtype %s" % (fn, o.dtype))
        slots[o.dtype] = o
    if not slots:
        raise CtHipError("%s needs at least one output (out)" % fn)
    return outs, slots


def _u8_metric(x, gt, psnr_out, fn):
    """the gt / psnr_out rule of the uint8 entries -> (the [B,H,W,3] view of gt, psnr_out), or (None, None) without gt"""
    if gt is None:
        if psnr_out is not None:
            raise CtHipError("%s: psnr_out without gt" % fn)
        return None, None
    g = _u8_frames(gt, "gt", fn)
    if g.shape != x.shape or g.device != x.device:
        raise CtHipError("%s: gt must be uint8 frames of the target's shape and device, got %s on %s" % (fn, tuple(g.shape), g.device))
    B = x.shape[0]
    if psnr_out is None:
        psnr_out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    if not isinstance(psnr_out, torch.Tensor):
        raise CtHipError("%s: psnr_out must be a tensor" % fn)
    _require_cuda(psnr_out)
    if psnr_out.dtype != torch.float64 or psnr_out.numel() < 2 * B or psnr_out.device != x.device:
        raise CtHipError("%s: psnr_out must be float64 with >= 2*B elements on the input's device" % fn)
    return g, psnr_out


def _u8_rotations(rotations, B, fn):
    rot = rotations.detach().cpu().numpy() if isinstance(rotations, torch.Tensor) else np.asarray(rotations)
    if rot.ndim not in (3, 4) or rot.shape[-2:] != (3, 3) or rot.shape[-3] < 1 or (rot.ndim == 4 and rot.shape[0] != B):
        raise CtHipError("%s: rotations must be [n_iter,3,3] or [B,n_iter,3,3] with n_iter >= 1, got %s" % (fn, tuple(rot.shape)))
    return rot


def _u8_pair(target, reference, fn):
    """target and reference frames of one device and batch size -> their [B,H,W,3] views"""
    x, r = _u8_frames(target, "target", fn), _u8_frames(reference, "reference", fn)
    if x.device != r.device:
        raise CtHipError("%s: target on %s, reference on %s" % (fn, x.device, r.device))
    if x.shape[0] != r.shape[0]:
        raise CtHipError("%s needs target/reference of one batch size, got %d and %d" % (fn, x.shape[0], r.shape[0]))
    return x, r


def _u8_bins(bins, fn):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= 1024:
        raise CtHipError("%s: bins must be an integer in 1..1024, got %r" % (fn, bins))
    return int(bins)


def _out_ptrs(slots, shape, a, b):
    """the float64 / float32 / uint8 output pointers of frames [a, b) of the call, NULL where a dtype is not asked for"""
    return [(_ptr(slots[d].view(shape)[a:b]) if d in slots else _NULL) for d in (torch.float64, torch.float32, torch.uint8)]


def _result(target, out, outs, g, psnr_out, *more):
    """out in the target's shape (a tuple where a sequence was given), then psnr_out with gt, then whatever else the entry returns"""
    res = tuple(o.view(tuple(target.shape)) for o in outs)
    ret = (res if isinstance(out, (tuple, list)) else res[0],) + ((psnr_out,) if g is not None else ()) + more
    return ret if len(ret) > 1 else ret[0]

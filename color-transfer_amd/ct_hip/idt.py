"""Iterative distribution transfer (csrc/idt.hip)."""
import ctypes

import numpy as np
import torch

from ._core import (CT_WS_IDT, CtHipError, SIGNATURES, _as_batch, _c_i64, _c_int, _c_p, _c_sz, _ptr, _require_cuda, _stream, _suffix,
                    _upload_small, check, lib, workspace)

SIGNATURES.update({
    "ct_idt_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "ct_idt_f32": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz,
                            _c_p, _c_p]),
    "ct_idt_f64": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz,
                            _c_p, _c_p]),
    "ct_idt_u8_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_i64, _c_int]),
    "ct_idt_u8": (_c_int, [_c_p, _c_i64, _c_p, _c_i64, _c_p, _c_int, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p,
                           _c_p, _c_p, _c_sz, _c_p, _c_p]),
})


class IdtDebug(ctypes.Structure):
    """struct ct_idt_debug (include/ct_hip.h)"""
    _fields_ = [("hist", _c_p), ("lut", _c_p), ("par", _c_p), ("binidx", _c_p)]


def _upload_rotations(rotations, B, device):
    """[n_iter,3,3] (shared by the batch) or [B,n_iter,3,3] -> (device [2][B][n_iter][9]: the matrices and their inverses, n_iter)"""
    rot = np.asarray(rotations.cpu().numpy() if isinstance(rotations, torch.Tensor) else rotations, dtype=np.float64)
    if rot.ndim == 3:
        rot = np.broadcast_to(rot, (B,) + rot.shape)
    n_iter = rot.shape[1]
    rinv = np.linalg.inv(rot)                       # host 3x3 inverses (the reference LU-solves, iterative.py:55)
    return _upload_small(np.ascontiguousarray(np.stack([rot, rinv]).reshape(2, B, n_iter, 9)), device), n_iter


def _debug_probes(B, n_iter, bins, n_t, device):
    dbg_t = {"hist": torch.zeros((B, n_iter, 2, 3, bins), dtype=torch.int32, device=device),
             "lut": torch.zeros((B, n_iter, 3, bins, 2), dtype=torch.float64, device=device),
             "par": torch.zeros((B, n_iter, 3, 4), dtype=torch.float64, device=device),
             "binidx": torch.zeros((B, n_iter, 3, n_t), dtype=torch.int16, device=device)}
    st = IdtDebug(dbg_t["hist"].data_ptr(), dbg_t["lut"].data_ptr(), dbg_t["par"].data_ptr(), dbg_t["binidx"].data_ptr())
    return dbg_t, st


def idt(target, reference, rotations, bins=255, round_dr_f32=None, out=None, debug=False):
    """methods.iterative.iterative_distribution_transfer on device tensors (methods/iterative.py:8-59).

    target [H,W,3] or [B,H,W,3], reference likewise (its H x W may differ), float32 or float64 (same
    dtype); rotations: float64 numpy/tensor [n_iter,3,3] (shared by the batch) or [B,n_iter,3,3].
    Returns the float64 result (and a dict of device probe tensors when debug=True)."""
    x, _ = _as_batch(target)
    r, _ = _as_batch(reference)
    _require_cuda(x, r)
    if x.dtype != r.dtype or x.shape[0] != r.shape[0]:
        raise CtHipError("idt needs target/reference of one dtype and batch size")
    B, n_t, n_r = x.shape[0], x.shape[1] * x.shape[2], r.shape[1] * r.shape[2]
    both, n_iter = _upload_rotations(rotations, B, x.device)
    if round_dr_f32 is None:
        round_dr_f32 = x.dtype == torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    need = lib().ct_idt_workspace_bytes(B, n_iter, bins)
    if need == 0:
        raise CtHipError("idt: unsupported bins=%d / n_iter=%d" % (bins, n_iter))
    ws = workspace(CT_WS_IDT, 0, B, x.device, need=need)
    dbg_t, dbg_p = {}, ctypes.c_void_p(0)
    if debug:
        dbg_t, st = _debug_probes(B, n_iter, bins, n_t, x.device)
        dbg_p = ctypes.cast(ctypes.pointer(st), ctypes.c_void_p)
    fn = getattr(lib(), "ct_idt_" + _suffix(x))
    check(fn(_ptr(x), n_t, _ptr(r), n_r, B, _ptr(both[0]), _ptr(both[1]), n_iter, bins, int(bool(round_dr_f32)),
             _ptr(out), _ptr(ws), ws.numel(), dbg_p, _stream()))
    out = out.view(target.shape)
    return (out, dbg_t) if debug else out


_U8_OUT = (torch.uint8, torch.float32, torch.float64)


def _u8_frames(t, name, fn="idt_u8", dtype=torch.uint8):
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


def idt_u8(target, reference, rotations, bins=255, input_f32=True, round_dr_f32=None, out_dtype=torch.uint8, out=None, gt=None,
           psnr_out=None, debug=False):
    """Iterative distribution transfer on uint8 frames, B pairs per call, no host sync (ct_idt_u8).

    target, reference: uint8 device tensors [H,W,3] or [B,H,W,3] (the reference's H x W may differ); rotations as for idt().
    input_f32: the bytes stand for float32(k) / 255 (what a Runner feeds to idt()), else for k / 255.0; round_dr_f32 defaults to
    it.  The result is bitwise idt() on that image: float64 (out_dtype torch.float64), rounded once to float32, or the bytes
    ct_hip.pack_u8 makes of the float32 value (the default).  out: a tensor to write instead of a fresh one, or a sequence of up
    to three of distinct dtypes (all are written, the tuple is returned).  With gt (uint8 frames of the target's shape) the call
    also fills psnr_out, float64 [B, 2] = (mse, PSNR) of the clamped float32 result.
    Returns out, (out, psnr_out) with gt, and the dict of probe tensors as a last item with debug=True."""
    x, r = _u8_frames(target, "target"), _u8_frames(reference, "reference")
    if x.device != r.device:
        raise CtHipError("idt_u8: target on %s, reference on %s" % (x.device, r.device))
    if x.shape[0] != r.shape[0]:
        raise CtHipError("idt_u8 needs target/reference of one batch size, got %d and %d" % (x.shape[0], r.shape[0]))
    B, n_t, n_r = x.shape[0], x.shape[1] * x.shape[2], r.shape[1] * r.shape[2]
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= 1024:
        raise CtHipError("idt_u8: bins must be an integer in 1..1024, got %r" % (bins,))
    rot = _u8_rotations(rotations, B, "idt_u8")
    if round_dr_f32 is None:
        round_dr_f32 = input_f32
    outs, slots = _u8_outputs(x, out, out_dtype, "idt_u8")
    null = ctypes.c_void_p(0)
    g, psnr_out = _u8_metric(x, gt, psnr_out, "idt_u8")
    both, n_iter = _upload_rotations(rot, B, x.device)
    need = lib().ct_idt_u8_workspace_bytes(B, n_iter, bins, n_t, 0 if torch.float64 in slots else 1)
    if need == 0:
        raise CtHipError("idt_u8: unsupported bins=%d / n_iter=%d" % (bins, n_iter))
    ws = workspace(CT_WS_IDT, 0, B, x.device, need=need)
    dbg_t, dbg_p = {}, null
    if debug:
        dbg_t, st = _debug_probes(B, n_iter, bins, n_t, x.device)
        dbg_p = ctypes.cast(ctypes.pointer(st), ctypes.c_void_p)
    p = [(_ptr(slots[d]) if d in slots else null) for d in (torch.float64, torch.float32, torch.uint8)]
    check(lib().ct_idt_u8(_ptr(x), n_t, _ptr(r), n_r, _ptr(g) if g is not None else null, B, _ptr(both[0]), _ptr(both[1]), n_iter,
                          int(bins), int(bool(input_f32)), int(bool(round_dr_f32)), p[0], p[1], p[2],
                          _ptr(psnr_out) if g is not None else null, _ptr(ws), ws.numel(), dbg_p, _stream()))
    res = tuple(o.view(tuple(target.shape)) for o in outs)
    ret = (res if isinstance(out, (tuple, list)) else res[0],)
    if g is not None:
        ret += (psnr_out,)
    if debug:
        ret += (dbg_t,)
    return ret if len(ret) > 1 else ret[0]

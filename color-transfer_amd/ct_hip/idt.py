"""Iterative distribution transfer (csrc/idt.hip)."""
import ctypes

import numpy as np
import torch

from ._core import (CT_WS_IDT, CtHipError, SIGNATURES, _as_batch, _c_i64, _c_int, _c_p, _c_sz, _ptr, _require_cuda, _stream, _suffix,
                    _upload_small, check, lib, workspace)
from ._u8 import _NULL, _out_ptrs, _result, _u8_bins, _u8_metric, _u8_outputs, _u8_pair, _u8_rotations

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
    fn = "idt_u8"
    x, r = _u8_pair(target, reference, fn)
    B, n_t, n_r = x.shape[0], x.shape[1] * x.shape[2], r.shape[1] * r.shape[2]
    bins = _u8_bins(bins, fn)
    rot = _u8_rotations(rotations, B, fn)
    if round_dr_f32 is None:
        round_dr_f32 = input_f32
    outs, slots = _u8_outputs(x, out, out_dtype, fn)
    g, psnr_out = _u8_metric(x, gt, psnr_out, fn)
    both, n_iter = _upload_rotations(rot, B, x.device)
    need = lib().ct_idt_u8_workspace_bytes(B, n_iter, bins, n_t, 0 if torch.float64 in slots else 1)
    if need == 0:
        raise CtHipError("idt_u8: unsupported bins=%d / n_iter=%d" % (bins, n_iter))
    ws = workspace(CT_WS_IDT, 0, B, x.device, need=need)
    dbg_t, dbg_p = {}, _NULL
    if debug:
        dbg_t, st = _debug_probes(B, n_iter, bins, n_t, x.device)
        dbg_p = ctypes.cast(ctypes.pointer(st), ctypes.c_void_p)
    p = _out_ptrs(slots, x.shape, 0, B)
    check(lib().ct_idt_u8(_ptr(x), n_t, _ptr(r), n_r, _ptr(g) if g is not None else _NULL, B, _ptr(both[0]), _ptr(both[1]), n_iter,
                          bins, int(bool(input_f32)), int(bool(round_dr_f32)), p[0], p[1], p[2],
                          _ptr(psnr_out) if g is not None else _NULL, _ptr(ws), ws.numel(), dbg_p, _stream()))
    return _result(target, out, outs, g, psnr_out, *((dbg_t,) if debug else ()))

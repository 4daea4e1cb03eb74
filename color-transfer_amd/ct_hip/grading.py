"""Automated colour grading on uint8 frame groups: the batched regrain (ct_regrain_u8) and IDT + regrain in one entry (ct_acg_u8),
csrc/regrain.hip."""
import ctypes

import numpy as np
import torch

from ._core import (CT_WS_IDT, CtHipError, SIGNATURES, _c_i64, _c_int, _c_p, _c_sz, _ptr, _stream, check, lib,
                    workspace)
from ._u8 import _NULL, _out_ptrs, _result, _u8_bins, _u8_frames, _u8_metric, _u8_outputs, _u8_pair, _u8_rotations
from .idt import _upload_rotations

SIGNATURES.update({
    "ct_regrain_u8_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int]),
    "ct_regrain_u8": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_sz, _c_p]),
    "ct_acg_u8_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "ct_acg_u8": (_c_int, [_c_p, _c_p, _c_i64, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_int, _c_p, _c_p,
                           _c_p, _c_p, _c_p, _c_sz, _c_p]),
})

NBITS = (4, 16, 32, 64, 64, 64)                  # the reference's default (methods/iterative.py:62)


def _nbits(nbits, fn):
    try:
        nb = [int(v) for v in nbits]
    except (TypeError, ValueError):
        raise CtHipError("%s: nbits must be a sequence of 1..8 sweep counts, got %r" % (fn, nbits))
    if not 1 <= len(nb) <= 8 or any(v < 0 for v in nb):
        raise CtHipError("%s: nbits needs 1..8 non-negative entries, got %r" % (fn, tuple(nbits)))
    return nb


def _splits(B, frames_per_call, fn):
    if frames_per_call is None:
        return [(0, B)]
    if isinstance(frames_per_call, bool) or not isinstance(frames_per_call, (int, np.integer)) or frames_per_call < 1:
        raise CtHipError("%s: frames_per_call must be a positive integer or None, got %r" % (fn, frames_per_call))
    return [(a, min(a + int(frames_per_call), B)) for a in range(0, B, int(frames_per_call))]


def regrain_u8(img_in_u8, img_col, nbits=NBITS, input_f32=True, out_dtype=torch.float64, out=None, gt=None, psnr_out=None,
               frames_per_call=None):
    """`_regrain` (methods/iterative.py:62-117) of B frames in the launches of one, the original target as bytes (ct_regrain_u8).

    img_in_u8: uint8 device tensor [H,W,3] or [B,H,W,3]; img_col: float64 of that shape (the IDT result).  input_f32: the bytes
    stand for float32(k) / 255, else for k / 255.0.  The float64 result (the default out_dtype) is bitwise ct_hip.regrain on that
    image, frame by frame; float32 is it rounded once, uint8 what ct_hip.pack_u8 makes of the float32 value.  out, gt, psnr_out
    and the return value as for ct_hip.idt_u8; frames_per_call as for acg_u8."""
    fn = "regrain_u8"
    x = _u8_frames(img_in_u8, "img_in_u8", fn)
    c = _u8_frames(img_col, "img_col", fn, torch.float64)
    if c.shape != x.shape or c.device != x.device:
        raise CtHipError("%s: img_col must have the shape and device of img_in_u8, got %s on %s" % (fn, tuple(c.shape), c.device))
    nb = _nbits(nbits, fn)
    outs, slots = _u8_outputs(x, out, out_dtype, fn)
    g, psnr_out = _u8_metric(x, gt, psnr_out, fn)
    B, h, w = x.shape[0], x.shape[1], x.shape[2]
    arr = (ctypes.c_int * len(nb))(*nb)
    for a, b in _splits(B, frames_per_call, fn):
        need = lib().ct_regrain_u8_workspace_bytes(b - a, h, w, len(nb))
        if need == 0:
            raise CtHipError("%s: unsupported batch / frame size %s" % (fn, tuple(x.shape)))
        ws = workspace(CT_WS_IDT, 0, b - a, x.device, need=need)
        p = _out_ptrs(slots, x.shape, a, b)
        check(lib().ct_regrain_u8(_ptr(x[a:b]), _ptr(c[a:b]), b - a, h, w, int(bool(input_f32)), ctypes.cast(arr, ctypes.c_void_p), len(nb),
                                  p[0], p[1], p[2], _ptr(g[a:b]) if g is not None else _NULL,
                                  _ptr(psnr_out.view(-1)[2 * a:]) if g is not None else _NULL, _ptr(ws), ws.numel(), _stream()))
    return _result(img_in_u8, out, outs, g, psnr_out)


def acg_u8(target, reference, rotations, bins=255, nbits=NBITS, input_f32=True, out_dtype=torch.uint8, out=None, gt=None, psnr_out=None,
           frames_per_call=None):
    """Automated colour grading (IDT, then regrain; methods/iterative.py:118-138) on uint8 frames, B pairs per call, no host sync
    (ct_acg_u8).

    target, reference: uint8 device tensors [H,W,3] or [B,H,W,3] (the reference's H x W may differ); rotations as for idt().
    input_f32: the bytes stand for float32(k) / 255 (what a Runner feeds to automated_color_grading_cuda), else for k / 255.0.
    The result is bitwise ct_hip.regrain(that image, ct_hip.idt_u8(..., out_dtype=torch.float64)) frame by frame: float64, rounded
    once to float32, or the bytes ct_hip.pack_u8 makes of the float32 value (the default).  out, gt, psnr_out and the return value
    as for ct_hip.idt_u8.  frames_per_call: the group goes through in sub-batches of that many frames, which bounds the workspace
    (at 1080p the float64 pyramid takes ~360 MB per frame); the result does not depend on it."""
    fn = "acg_u8"
    x, r = _u8_pair(target, reference, fn)
    B, h, w, n_r = x.shape[0], x.shape[1], x.shape[2], r.shape[1] * r.shape[2]
    bins = _u8_bins(bins, fn)
    rot = _u8_rotations(rotations, B, fn)
    nb = _nbits(nbits, fn)
    outs, slots = _u8_outputs(x, out, out_dtype, fn)
    g, psnr_out = _u8_metric(x, gt, psnr_out, fn)
    splits = _splits(B, frames_per_call, fn)
    both, n_iter = _upload_rotations(rot, B, x.device)
    arr = (ctypes.c_int * len(nb))(*nb)
    for a, b in splits:
        need = lib().ct_acg_u8_workspace_bytes(b - a, h, w, n_iter, bins, len(nb))
        if need == 0:
            raise CtHipError("%s: unsupported bins=%d / n_iter=%d / frame size %s" % (fn, bins, n_iter, tuple(x.shape)))
        ws = workspace(CT_WS_IDT, 0, b - a, x.device, need=need)
        p = _out_ptrs(slots, x.shape, a, b)
        check(lib().ct_acg_u8(_ptr(x[a:b]), _ptr(r[a:b]), n_r, _ptr(g[a:b]) if g is not None else _NULL, b - a, h, w, _ptr(both[0][a:b]),
                              _ptr(both[1][a:b]), n_iter, bins, int(bool(input_f32)), ctypes.cast(arr, ctypes.c_void_p), len(nb),
                              p[0], p[1], p[2], _ptr(psnr_out.view(-1)[2 * a:]) if g is not None else _NULL, _ptr(ws), ws.numel(), _stream()))
    return _result(target, out, outs, g, psnr_out)

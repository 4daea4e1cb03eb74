"""Perspective warp of uint8 frames: the flip, the crop to bbox, cv2.warpPerspective and the second crop of the reference's
dataset postprocessing (utils/postprocess.py:97, 127-136; csrc/warp.hip)."""
import numpy as np
import torch

from ._core import CtHipError, SIGNATURES, _as_batch, _c_int, _c_p, _ptr, _require_cuda, _stream, _upload_small, check, lib

SIGNATURES.update({
    "ct_warp_perspective_u8": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_int, _c_int, _c_int, _c_int,
                                        _c_int, _c_p, _c_int, _c_p]),
})

CT_WARP_AUTO, CT_WARP_STAGED, CT_WARP_GLOBAL = 0, 1, 2
WARP_PATHS = {None: CT_WARP_AUTO, "auto": CT_WARP_AUTO, "staged": CT_WARP_STAGED, "global": CT_WARP_GLOBAL}
WARP_MAX_SIDE = 32767


def invert3x3(m):
    """cv2.invert of a 3 x 3 float64 matrix (DECOMP_LU takes the closed form for 3 x 3): d = 1 / det, every entry cofactor * d;
    a zero determinant gives the all-zero matrix."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError("invert3x3 needs a 3 x 3 matrix, got %s" % (m.shape,))
    (a, b, c), (d, e, f), (g, h, i) = m.tolist()
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    if det == 0.0:
        return np.zeros((3, 3), dtype=np.float64)
    t = 1.0 / det
    return np.array([[(e * i - f * h) * t, (c * h - b * i) * t, (b * f - c * e) * t],
                     [(f * g - d * i) * t, (a * i - c * g) * t, (c * d - a * f) * t],
                     [(d * h - e * g) * t, (b * g - a * h) * t, (a * e - b * d) * t]], dtype=np.float64)


def _rect(value, name, default):
    if value is None:
        return default
    try:
        rect = tuple(value)
        ok = len(rect) == 4 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in rect)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("%s must be four ints (x, y, w, h), got %r" % (name, value))
    return tuple(int(v) for v in rect)


def warp_maps(matrices, batch, inverse_map=False):
    """host [3,3] or [B,3,3] -> (float64 [1 or B, 9] destination -> source matrices, shared flag); ValueError for anything else"""
    m = np.asarray(matrices, dtype=np.float64)
    if m.shape != (3, 3) and m.shape != (batch, 3, 3):
        raise ValueError("matrices must be [3,3] or [%d,3,3], got %s" % (batch, m.shape))
    if not np.isfinite(m).all():
        raise ValueError("matrices hold non-finite entries")
    shared = m.ndim == 2
    m = m.reshape(-1, 3, 3)
    if not inverse_map:
        m = np.stack([invert3x3(k) for k in m])
    return np.ascontiguousarray(m.reshape(-1, 9)), shared


def warp_perspective(frames_u8, matrices, crop=None, flip_x=False, window=None, inverse_map=False, out=None, path=None):
    """cv2.warpPerspective(src, M, (crop_w, crop_h)) with INTER_LINEAR and a constant 0 border on uint8 [H,W,3] / [B,H,W,3] device
    frames, OpenCV's fixed-point rule restated (include/ct_hip.h: ct_warp_perspective_u8; parity unpinned).
    src = the crop (x, y, w, h) of the frame (default: all of it) -- with flip_x of the frame mirrored left-right, cv2.flip(., 1);
    a tap outside the crop is 0.  matrices: host [3,3] (all frames) or [B,3,3]; as cv2 takes them, source -> destination, inverted
    here in float64 like cv2.invert (invert3x3), or with inverse_map=True (cv2.WARP_INVERSE_MAP) destination -> source as they are.
    window (x, y, w, h): the part of the crop_w x crop_h destination that is computed and returned (default: all of it).
    path: None / "auto" / "global" (taps from memory, the default) or "staged" (a tile's source rows through LDS): the same bytes.
    Non-finite matrix entries, a crop outside the frame or a window outside the destination: ValueError.  Asynchronous on the
    current stream; the matrices go up through the binding's ring of pinned slots."""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (3, 4) or frames_u8.shape[-1] != 3:
        raise ValueError("warp_perspective needs a uint8 [H,W,3] or [B,H,W,3] tensor")
    x, batched = _as_batch(frames_u8)
    b, h, w, _ = x.shape
    if b < 1 or h < 1 or w < 1:
        raise ValueError("warp_perspective: empty frames of shape %s" % (tuple(frames_u8.shape),))
    if path not in WARP_PATHS:
        raise ValueError("path %r: one of auto, staged, global" % (path,))
    cx, cy, cw, ch = _rect(crop, "crop", (0, 0, w, h))
    if cw < 1 or ch < 1 or cx < 0 or cy < 0 or cx + cw > w or cy + ch > h:
        raise ValueError("crop %r is not inside the %d x %d frame" % ((cx, cy, cw, ch), w, h))
    if cw > WARP_MAX_SIDE or ch > WARP_MAX_SIDE:
        raise ValueError("crop %r: sides up to %d (the 16-bit source coordinates of the rule)" % ((cx, cy, cw, ch), WARP_MAX_SIDE))
    ox, oy, ow, oh = _rect(window, "window", (0, 0, cw, ch))
    if ow < 1 or oh < 1 or ox < 0 or oy < 0 or ox + ow > cw or oy + oh > ch:
        raise ValueError("window %r is not inside the %d x %d destination" % ((ox, oy, ow, oh), cw, ch))
    maps, shared = warp_maps(matrices, b, inverse_map)
    _require_cuda(x)
    if out is None:
        out = torch.empty((b, oh, ow, 3), dtype=torch.uint8, device=x.device)
    else:
        _require_cuda(out)
        if out.dtype != torch.uint8 or out.device != x.device or out.numel() != b * oh * ow * 3:
            raise CtHipError("out must hold uint8 [%d,%d,%d,3] on %s" % (b, oh, ow, x.device))
    dev_maps = _upload_small(maps, x.device)
    check(lib().ct_warp_perspective_u8(_ptr(x), b, h, w, 1 if flip_x else 0, cx, cy, cw, ch, _ptr(dev_maps), 1 if shared else 0, ox, oy, ow, oh,
                                       _ptr(out), WARP_PATHS[path], _stream()))
    return out.view((b, oh, ow, 3) if batched else (oh, ow, 3))

"""8-bit Y'CbCr 4:2:0 (packed I420 frames) <-> RGB bytes on the device (csrc/yuv.hip; the rule: include/ct_hip.h)."""
import torch

from ._core import CtHipError, SIGNATURES, _c_i64, _c_int, _c_p, _check_device, _ptr, _require_cuda, _stream, check, lib

SIGNATURES.update({
    "ct_yuv420_to_rgb_u8": (_c_int, [_c_p, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p]),
    "ct_rgb_to_yuv420_u8": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_i64, _c_p]),
})

YUV_MATRICES = {"bt601": 0, "bt709": 1}
YUV_RANGES = {"limited": 0, "full": 1}
YUV_SITINGS = {"center": 0, "left": 1}


def yuv420_frame_bytes(h, w):
    """bytes of one packed I420 frame: the Y plane and two chroma planes of ceil(h / 2) x ceil(w / 2)"""
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, int) or not isinstance(w, int) or h < 1 or w < 1:
        raise CtHipError("yuv420_frame_bytes needs a positive integer height and width (got %r, %r)" % (h, w))
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def _enums(who, matrix, range, siting):
    for name, value, table in (("matrix", matrix, YUV_MATRICES), ("range", range, YUV_RANGES), ("siting", siting, YUV_SITINGS)):
        if value not in table:
            raise CtHipError("%s: %s must be one of %s (got %r)" % (who, name, sorted(table), value))
    return YUV_MATRICES[matrix], YUV_RANGES[range], YUV_SITINGS[siting]


def _frames_2d(who, t, fb, what):
    """a uint8 device tensor [n, >= fb] (or one frame [fb]) whose bytes are dense along the last dimension -> ([n, fb] view)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (1, 2):
        raise CtHipError("%s: %s must be a uint8 [n, %d] or [%d] tensor" % (who, what, fb, fb))
    if not t.is_cuda:
        raise CtHipError("ct_hip needs device tensors (got %s); no CPU path exists" % t.device)
    _check_device(t)
    tb = t if t.dim() == 2 else t.unsqueeze(0)
    if tb.shape[1] != fb:
        raise CtHipError("%s: %s has %d bytes per frame, the frame size needs %d" % (who, what, tb.shape[1], fb))
    if tb.stride(1) != 1 or (tb.shape[0] > 1 and tb.stride(0) < fb):
        raise CtHipError("%s: %s needs a last-dimension stride of 1 and a row stride of at least %d bytes" % (who, what, fb))
    return tb


def yuv420_to_rgb(yuv_u8, height, width, matrix="bt709", range="limited", siting="center", out=None):
    """Packed I420 frames -> uint8 [n,H,W,3] (ct_yuv420_to_rgb_u8): yuv_u8 is a uint8 device tensor [n, frame_bytes] or
    [frame_bytes], last-dimension stride 1, row stride >= frame_bytes = yuv420_frame_bytes(height, width) (a slice of wider rows
    is fine, and so is any base address).  The bytes are the exact rule of include/ct_hip.h.  out: an optional preallocated uint8
    [n,H,W,3] tensor on the same device.  Asynchronous on the current stream; nothing is allocated with out.  No CPU path."""
    m, r, s = _enums("yuv420_to_rgb", matrix, range, siting)
    fb = yuv420_frame_bytes(height, width)
    yb = _frames_2d("yuv420_to_rgb", yuv_u8, fb, "yuv_u8")
    n = yb.shape[0]
    shape = (n, height, width, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=yb.device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != yb.device or tuple(out.shape) != shape:
            raise CtHipError("yuv420_to_rgb: out must be a uint8 %s tensor on %s" % (list(shape), yb.device))
        _require_cuda(out)
    if n:
        check(lib().ct_yuv420_to_rgb_u8(_ptr(yb), yb.stride(0) if n > 1 else fb, n, height, width, m, r, s, _ptr(out), _stream()))
    return out


def rgb_to_yuv420(frames, matrix="bt709", range="limited", siting="center", out=None):
    """uint8 [n,H,W,3] frames -> packed I420 frames, uint8 [n, frame_bytes] (ct_rgb_to_yuv420_u8).  float32 frames ([n,3,H,W] or
    [n,H,W,3]) go through pack_u8 first: the result is by definition the YUV of the bytes pack_u8 makes of them.  out: an optional
    uint8 [n, frame_bytes] device tensor, last-dimension stride 1 and row stride >= frame_bytes.  Asynchronous on the current
    stream; nothing is allocated with out and uint8 frames.  No CPU path."""
    m, r, s = _enums("rgb_to_yuv420", matrix, range, siting)
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise CtHipError("rgb_to_yuv420 needs uint8 [n,H,W,3] frames, or float32 frames in either layout")
    if frames.dtype == torch.float32:
        from .resize_pack import pack_u8
        frames = pack_u8(frames)
    if frames.dtype != torch.uint8 or frames.shape[3] != 3:
        raise CtHipError("rgb_to_yuv420 needs uint8 [n,H,W,3] frames, or float32 frames in either layout (got %s %s)"
                         % (frames.dtype, tuple(frames.shape)))
    _require_cuda(frames)
    n, h, w, _ = frames.shape
    if h < 1 or w < 1:
        raise CtHipError("rgb_to_yuv420: empty frames %s" % (tuple(frames.shape),))
    fb = yuv420_frame_bytes(h, w)
    if out is None:
        out = torch.empty((n, fb), dtype=torch.uint8, device=frames.device)
        ob = out
    else:
        ob = _frames_2d("rgb_to_yuv420", out, fb, "out")
        if ob.shape[0] != n or ob.device != frames.device:
            raise CtHipError("rgb_to_yuv420: out must hold %d frames of %d bytes on %s" % (n, fb, frames.device))
    if n:
        check(lib().ct_rgb_to_yuv420_u8(_ptr(frames), n, h, w, m, r, s, _ptr(ob), ob.stride(0) if n > 1 else fb, _stream()))
    return out

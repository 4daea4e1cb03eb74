"""Per-frame metrics (PSNR, SSIM, FSIM with its FFT, iCID), the uint8 distortions and the regrain step."""
import ctypes

import torch

from ._core import (CT_WS_LAB_STATS, CtHipError, SIGNATURES, _c_i64, _c_int, _c_p, _c_sz, _check_device, _lock, _ptr, _require_cuda,
                    _stream, check, lib, workspace)

SIGNATURES.update({
    "ct_frame_psnr_f32": (_c_int, [_c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_distort_u8": (_c_int, [_c_p, _c_int, _c_int, _c_int, ctypes.c_double, _c_p, _c_p, _c_p, _c_sz, _c_p]),
    "ct_regrain_workspace_bytes": (_c_sz, [_c_int, _c_int]),
    "ct_regrain_f64": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_p, _c_int, _c_p, _c_sz, _c_p]),
    "ct_metric_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "ct_frame_ssim_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_icid_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_fft2d_c2c_f32": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_fsim_pooled_size": (_c_int, [_c_int, _c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "ct_fsim_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "ct_fsim_stage_offsets": (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_sz)]),
    "ct_fsim_setup_f32": (_c_int, [_c_int, _c_int, _c_p, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_fsim_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_ssim_hwc_u8": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_icid_hwc_u8": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_fsim_hwc_u8": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_sz, _c_p]),
    "ct_icid_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int, _c_int]),
    "ct_frame_icid_opt_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_icid_opt_hwc_u8": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p, _c_p, _c_sz, _c_p]),
})


def frame_psnr(a, b):
    """Per-frame (mse, PSNR) of two float32 batches [B, ...] with data range 1 -> float64 [B, 2] (methods/__init__.py:32)."""
    _require_cuda(a, b)
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise CtHipError("frame_psnr needs two float32 tensors of one shape")
    B = a.shape[0]
    n = a.numel() // max(B, 1)
    out = torch.empty((B, 2), dtype=torch.float64, device=a.device)
    if B == 0:
        return out
    ws = workspace(CT_WS_LAB_STATS, n, B, a.device)
    check(lib().ct_frame_psnr_f32(_ptr(a), _ptr(b), n, B, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


DISTORTIONS = {"identity": 0, "brightness": 1, "contrast": 2, "saturation": 3, "hue": 4, "gamma": 5}


def distort_u8(img, kind, param, want_u8=False):
    """torchvision.transforms.functional.adjust_<kind>(img, param) on a uint8 [3,H,W] device tensor (utils/data.py:12-22).
    Returns the distorted frame / 255 as float32 [3,H,W] (and the uint8 frame when want_u8)."""
    if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[0] != 3 or not img.is_contiguous():
        raise CtHipError("distort_u8 needs a contiguous uint8 [3,H,W] device tensor")
    _check_device(img)
    h, w = img.shape[1], img.shape[2]
    out_f = torch.empty((3, h, w), dtype=torch.float32, device=img.device)
    out_u = torch.empty_like(img) if want_u8 else None
    ws = workspace(CT_WS_LAB_STATS, 0, 1, img.device, need=64)
    rc = lib().ct_distort_u8(_ptr(img), h, w, DISTORTIONS[kind] if isinstance(kind, str) else int(kind), float(param),
                             _ptr(out_u) if want_u8 else ctypes.c_void_p(0), _ptr(out_f), _ptr(ws), ws.numel(), _stream())
    if rc == -1:
        raise ValueError("distortion %r: parameter %r out of range" % (kind, param))      # torchvision raises ValueError too
    check(rc)
    return (out_f, out_u) if want_u8 else out_f


def regrain(img_in, img_col, nbits=(4, 16, 32, 64, 64, 64), out=None):
    """`_regrain(img_arr_in, img_arr_col, nbits)` of methods/iterative.py:62-117 on device tensors [H,W,3] (any float dtype;
    computed in float64).  Returns float64 [H,W,3]."""
    _require_cuda(img_in, img_col)
    if img_in.dim() != 3 or img_in.shape[2] != 3 or img_in.shape != img_col.shape:
        raise CtHipError("regrain needs two [H,W,3] tensors of one shape")
    if len(nbits) < 1 or len(nbits) > 8:
        raise CtHipError("regrain: nbits needs 1..8 entries")
    a, b = img_in.double().contiguous(), img_col.double().contiguous()
    h, w = a.shape[0], a.shape[1]
    if out is None:
        out = torch.empty_like(a)
    ws = workspace(CT_WS_LAB_STATS, 0, 1, a.device, need=lib().ct_regrain_workspace_bytes(h, w))
    nb = (ctypes.c_int * len(nbits))(*[int(v) for v in nbits])
    check(lib().ct_regrain_f64(_ptr(a), _ptr(b), _ptr(out), h, w, ctypes.cast(nb, ctypes.c_void_p), len(nbits), _ptr(ws), ws.numel(),
                               _stream()))
    return out


def _frame_metric(name, a, b):
    _require_cuda(a, b)
    if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise CtHipError("%s needs two float32 [B,3,H,W] tensors of one shape" % name)
    B, _, h, w = a.shape
    out = torch.empty((B,), dtype=torch.float64, device=a.device)
    if B == 0:                                     # an empty tensor has a null data pointer, which the library refuses
        return out
    ws = workspace(CT_WS_LAB_STATS, 0, B, a.device, need=lib().ct_metric_workspace_bytes(h, w, B))
    check(getattr(lib(), name)(_ptr(a), _ptr(b), h, w, B, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def frame_ssim(a, b):
    """Per-frame piq.ssim(a, b) (defaults, data range 1) of float32 [B,3,H,W] batches -> float64 [B] (methods/__init__.py:33)."""
    return _frame_metric("ct_frame_ssim_f32", a, b)


ICID_INTENTS = {"perceptual": 0, "hue-preserving": 1, "chromatic": 2}              # CT_ICID_* of include/ct_hip.h


def icid_intent(intent):
    """CT_ICID_* of an intent name; anything else raises the reference's ValueError (utils/icid.py:49).  Touches no device."""
    if not isinstance(intent, str) or intent not in ICID_INTENTS:
        raise ValueError("Intent should be either 'perceptual', 'hue-preserving', or 'chromatic'")
    return ICID_INTENTS[intent]


def _frame_icid_opt(name, a, b, B, h, w, intent, omit_maps67, downsampling):
    """the iCID entry with options `name` on B frames of h x w, with the workspace of its map grid"""
    out = torch.empty((B,), dtype=torch.float64, device=a.device)
    if B == 0:
        return out
    down = 1 if downsampling else 0
    ws = workspace(CT_WS_LAB_STATS, 0, B, a.device, need=lib().ct_icid_workspace_bytes(h, w, B, down))
    check(getattr(lib(), name)(_ptr(a), _ptr(b), h, w, B, intent, 1 if omit_maps67 else 0, down, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def frame_icid(a, b, intent="perceptual", omit_maps67=False, downsampling=True):
    """Per-frame utils.icid.icid(a, b, intent, omit_maps67, downsampling) of float32 [B,3,H,W] batches -> float64 [B]
    (methods/__init__.py:35; the arguments of utils/icid.py:28-34).  The defaults call ct_frame_icid_f32, anything else
    ct_frame_icid_opt_f32: downsampling=False takes the maps at the frames' own size.  An unknown intent raises the reference's
    ValueError before any device call."""
    code = icid_intent(intent)
    if code == 0 and not omit_maps67 and downsampling:
        return _frame_metric("ct_frame_icid_f32", a, b)
    _require_cuda(a, b)
    if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise CtHipError("ct_frame_icid_opt_f32 needs two float32 [B,3,H,W] tensors of one shape")
    return _frame_icid_opt("ct_frame_icid_opt_f32", a, b, a.shape[0], a.shape[2], a.shape[3], code, omit_maps67, downsampling)

_fsim_tables = {}                                  # (device, h, w) -> (filters [16, hp*wp] float32, consts [4, 3] float64)
CT_WS_FSIM = -7


def fft2d_(x, inverse=False):
    """In-place batched 2-D DFT of a complex64 tensor [..., H, W] (csrc/fft2d.hip; the transform inside frame_fsim): torch.fft.fft2,
    or -- inverse=True -- torch.fft.ifft2 without its 1 / (H W)."""
    if not x.is_cuda or x.dtype != torch.complex64 or not x.is_contiguous() or x.dim() < 2:
        raise CtHipError("fft2d_ needs a contiguous complex64 device tensor [..., H, W]")
    _check_device(x)
    h, w = x.shape[-2], x.shape[-1]
    planes = x.numel() // (h * w) if h * w else 0
    check(lib().ct_fft2d_c2c_f32(_ptr(x), h, w, planes, 1 if inverse else 0, _stream()))
    return x


def _fsim_ws(device, batch, h, w):
    need = lib().ct_fsim_workspace_bytes(batch, h, w)
    if need == 0:
        raise CtHipError("fsim: frames of %dx%d are too small (pooled size < 2)" % (h, w))
    ws = workspace(CT_WS_FSIM, 0, batch, device, need=need + 256)
    off = (-ws.data_ptr()) % 256
    return ws[off:off + need]


def _frame_fsim(name, a, b, B, h, w):
    """the FSIM entry `name` on B frames of h x w; the filter bank of a frame size is built on the device at first use and cached,
    one cache for the planar and the HWC entry"""
    out = torch.empty((B,), dtype=torch.float64, device=a.device)
    if B == 0:
        return out
    ws = _fsim_ws(a.device, B, h, w)
    key = (str(a.device), h, w)
    with _lock:
        tab = _fsim_tables.get(key)
    if tab is None:
        hp, wp = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().ct_fsim_pooled_size(h, w, ctypes.byref(hp), ctypes.byref(wp)))
        filters = torch.empty((16, hp.value * wp.value), dtype=torch.float32, device=a.device)
        consts = torch.empty((4, 3), dtype=torch.float64, device=a.device)
        check(lib().ct_fsim_setup_f32(h, w, _ptr(filters), _ptr(consts), _ptr(ws), ws.numel(), _stream()))
        tab = (filters, consts)
        with _lock:
            _fsim_tables[key] = tab
    check(getattr(lib(), name)(_ptr(a), _ptr(b), _ptr(out), B, h, w, _ptr(tab[0]), _ptr(tab[1]), _ptr(ws), ws.numel(), _stream()))
    return out


def frame_fsim(a, b):
    """Per-frame piq.fsim(a, b) (chromatic, piq defaults, data range 1) of float32 [B,3,H,W] batches -> float64 [B]
    (methods/__init__.py:34).  The filter bank of a frame size is built on the device at first use and cached."""
    _require_cuda(a, b)
    if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise CtHipError("ct_frame_fsim_f32 needs two float32 [B,3,H,W] tensors of one shape")
    return _frame_fsim("ct_frame_fsim_f32", a, b, a.shape[0], a.shape[2], a.shape[3])


def _check_hwc(name, result, gt_u8):
    """a frame group's own buffers: float32 [B,H,W,3] (unclamped result) and uint8 [B,H,W,3] (ground truth), one device, contiguous;
    a view with a storage offset (a slice of a larger group) is fine -> (B, H, W)"""
    if not (torch.is_tensor(result) and torch.is_tensor(gt_u8)):
        raise CtHipError("%s needs two tensors" % name)
    if (result.dtype != torch.float32 or gt_u8.dtype != torch.uint8 or result.dim() != 4 or result.shape[3] != 3
            or result.shape != gt_u8.shape):
        raise CtHipError("%s needs a float32 [B,H,W,3] result and a uint8 [B,H,W,3] ground truth of one shape (got %s %s and %s %s)"
                         % (name, result.dtype, tuple(result.shape), gt_u8.dtype, tuple(gt_u8.shape)))
    if not (result.is_contiguous() and gt_u8.is_contiguous()):
        raise CtHipError("%s needs contiguous tensors" % name)
    if not (result.is_cuda and gt_u8.is_cuda) or result.device != gt_u8.device:
        raise CtHipError("%s needs both tensors on one GPU" % name)
    _check_device(result)
    return result.shape[0], result.shape[1], result.shape[2]


def _frame_metric_hwc(name, result, gt_u8):
    B, h, w = _check_hwc(name, result, gt_u8)
    out = torch.empty((B,), dtype=torch.float64, device=result.device)
    if B == 0:
        return out
    ws = workspace(CT_WS_LAB_STATS, 0, B, result.device, need=lib().ct_metric_workspace_bytes(h, w, B))
    check(getattr(lib(), name)(_ptr(result), _ptr(gt_u8), h, w, B, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def frame_ssim_hwc(result, gt_u8):
    """frame_ssim read from a frame group's own buffers: result float32 [B,H,W,3] (clamped to [0, 1] as it is read, a NaN stays),
    gt_u8 uint8 [B,H,W,3] (k -> float32(k) / 255) -> float64 [B]; bitwise frame_ssim(result.clamp(0, 1) as NCHW, gt_u8.float() / 255
    as NCHW), without those passes."""
    return _frame_metric_hwc("ct_frame_ssim_hwc_u8", result, gt_u8)


def frame_icid_hwc(result, gt_u8, intent="perceptual", omit_maps67=False, downsampling=True):
    """frame_icid, with its options, read from a frame group's own buffers (see frame_ssim_hwc) -> float64 [B]; the defaults call
    ct_frame_icid_hwc_u8, anything else ct_frame_icid_opt_hwc_u8"""
    code = icid_intent(intent)
    if code == 0 and not omit_maps67 and downsampling:
        return _frame_metric_hwc("ct_frame_icid_hwc_u8", result, gt_u8)
    B, h, w = _check_hwc("ct_frame_icid_opt_hwc_u8", result, gt_u8)
    return _frame_icid_opt("ct_frame_icid_opt_hwc_u8", result, gt_u8, B, h, w, code, omit_maps67, downsampling)


def frame_fsim_hwc(result, gt_u8):
    """frame_fsim read from a frame group's own buffers (see frame_ssim_hwc) -> float64 [B]; the filter bank cache is frame_fsim's"""
    B, h, w = _check_hwc("ct_frame_fsim_hwc_u8", result, gt_u8)
    return _frame_fsim("ct_frame_fsim_hwc_u8", result, gt_u8, B, h, w)


def _fsim_stages(a, b):
    """frame_fsim(a, b) and clones of what it leaves in its workspace (tests read the stages behind the weighted mean): a dict
    with "score" [B] float64 and float32 tensors with image index 2 * pair + (0: a, 1: b) -- "iq" [2B, 2, hp, wp], "grad" and
    "pc" [2B, hp, wp], "thr" [2B, 4]."""
    out = frame_fsim(a, b)
    B, _, h, w = a.shape
    if B == 0:
        raise CtHipError("_fsim_stages needs at least one pair")
    hp, wp = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().ct_fsim_pooled_size(h, w, ctypes.byref(hp), ctypes.byref(wp)))
    hp, wp = hp.value, wp.value
    off = (_c_sz * 4)()
    check(lib().ct_fsim_stage_offsets(B, h, w, off))
    ws = _fsim_ws(a.device, B, h, w)                 # the same (device, stream) buffer and alignment frame_fsim just used

    def region(o, *shape):
        n = 1
        for v in shape:
            n *= v
        return ws[o:o + 4 * n].view(torch.float32).view(*shape).clone()
    return {"score": out, "iq": region(off[0], 2 * B, 2, hp, wp), "grad": region(off[1], 2 * B, hp, wp),
            "pc": region(off[2], 2 * B, hp, wp), "thr": region(off[3], 2 * B, 4)}

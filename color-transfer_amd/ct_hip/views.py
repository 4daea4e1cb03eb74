"""Diagnostic views: the checkerboard mix, the min-max scaled error / disparity planes, the SSIM and Lab error maps and the Middlebury
flow colouring of the reference's image panel (utils/visualizations.py, utils/flow_viz.py; csrc/views.hip, csrc/errmaps.hip)."""
import torch

from ._core import CtHipError, SIGNATURES, _c_int, _c_p, _c_sz, _f32c, _ptr, _stream, check, lib

SIGNATURES.update({
    "ct_view_chess_mix_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_view_workspace_bytes": (_c_sz, [_c_int]),
    "ct_view_scaled_plane_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_flow_to_image_u8": (_c_int, [_c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_p]),
    "ct_view_ssim_map_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_p]),
    "ct_view_lab_map_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_int, _c_p]),
})

CT_VIEW_RGBMSE, CT_VIEW_GRAY, CT_VIEW_LABMSE, CT_VIEW_ABMSE = 0, 1, 2, 3


def _nchw(x, name, channels=None):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or (channels is not None and x.shape[1] != channels):
        raise CtHipError("%s needs a [B,%s,H,W] tensor" % (name, "C" if channels is None else channels))
    _f32c(x)
    if not x.numel():
        raise CtHipError("%s: empty tensor of shape %s" % (name, tuple(x.shape)))


def _stats(b, device):
    """the per-frame statistics of one call: a few bytes, private to it (allocated here, like every result of this module)"""
    need = lib().ct_view_workspace_bytes(b)
    return torch.empty(need, dtype=torch.uint8, device=device), need


def chess_mix(x, y, size=25):
    """utils/visualizations.py:9-21 on float32 [B,C,H,W] device tensors: block (i, j) of size x size pixels from x when i + j is even,
    else from y; ragged last blocks.  Bitwise a copy (ct_view_chess_mix_f32).  Asynchronous on the current stream."""
    _nchw(x, "chess_mix")
    _nchw(y, "chess_mix")
    if x.shape != y.shape or x.device != y.device:
        raise CtHipError("chess_mix: x of shape %s on %s, y of shape %s on %s" % (tuple(x.shape), x.device, tuple(y.shape), y.device))
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:
        raise CtHipError("chess_mix: size must be a positive int (got %r)" % (size,))
    out = torch.empty_like(x)
    b, c, h, w = x.shape
    check(lib().ct_view_chess_mix_f32(_ptr(x), _ptr(y), _ptr(out), b, c, h, w, size, _stream()))
    return out


def _pair(x, y, name):
    """the checks the error maps share: two float32 [B,3,H,W] device tensors of one shape on one device"""
    _nchw(x, name, 3)
    _nchw(y, name, 3)
    if x.shape != y.shape or x.device != y.device:
        raise CtHipError("%s: x of shape %s on %s, y of shape %s on %s" % (name, tuple(x.shape), x.device, tuple(y.shape), y.device))


def rgbmse_view(x, y):
    """utils/visualizations.py:31-36 (rgbmse) on float32 [B,3,H,W] device tensors: channel 0 = the per-pixel mean over the channels
    of (x - y)^2, min-max scaled with the frame's own extremes; channels 1, 2 = 0.  A frame without any error is NaN (0 / 0, as in
    the reference; pack_u8 shows it black).  Deterministic; asynchronous on the current stream (ct_view_scaled_plane_f32)."""
    _pair(x, y, "rgbmse_view")
    b, _, h, w = x.shape
    out = torch.empty_like(x)
    ws, need = _stats(b, x.device)
    check(lib().ct_view_scaled_plane_f32(_ptr(x), _ptr(y), _ptr(out), _ptr(ws), need, b, h, w, CT_VIEW_RGBMSE, _stream()))
    return out


def rgbssim_view(x, y):
    """utils/visualizations.py:55-60 (rgbssim) on float32 [B,3,H,W] device tensors: channel 0 = 0.5 - ssim(x, y, window_size=11)
    .mean(dim=1) / 2, min-max scaled with the frame's own extremes; channels 1, 2 = 0.  kornia.metrics.ssim is restated from its
    published source (11-tap Gaussian of sigma 1.5, separable, reflect padding; parity unpinned).  Frames need more than 5 pixels
    either way.  Deterministic; asynchronous on the current stream (ct_view_ssim_map_f32)."""
    _pair(x, y, "rgbssim_view")
    b, _, h, w = x.shape
    if h < 6 or w < 6:
        raise CtHipError("rgbssim_view: the reflect padding of 5 needs frames of more than 5 pixels either way (got %d x %d)" % (h, w))
    out = torch.empty_like(x)
    ws, need = _stats(b, x.device)
    check(lib().ct_view_ssim_map_f32(_ptr(x), _ptr(y), _ptr(out), _ptr(ws), need, b, h, w, _stream()))
    return out


def _lab_view(x, y, name, kind):
    _pair(x, y, name)
    b, _, h, w = x.shape
    out = torch.empty_like(x)
    ws, need = _stats(b, x.device)
    check(lib().ct_view_lab_map_f32(_ptr(x), _ptr(y), _ptr(out), _ptr(ws), need, b, h, w, kind, _stream()))
    return out


def labmse_view(x, y):
    """utils/visualizations.py:39-44 (labmse) on float32 [B,3,H,W] device tensors: channel 0 = the mean of L, a, b of
    rgb_to_lab((x - y)^2), min-max scaled with the frame's own extremes; channels 1, 2 = 0.  kornia.color.rgb_to_lab is restated
    from its published source (parity unpinned).  Identical frames are NaN (a constant map: 0 / 0, as in the reference).
    Deterministic; asynchronous on the current stream (ct_view_lab_map_f32)."""
    return _lab_view(x, y, "labmse_view", CT_VIEW_LABMSE)


def abmse_view(x, y):
    """utils/visualizations.py:47-52 (abmse): labmse_view with the mean of a and b only."""
    return _lab_view(x, y, "abmse_view", CT_VIEW_ABMSE)


def gray_view(x):
    """One plane [B,1,H,W] (a disparity) -> [B,3,H,W]: (x - min) / (max - min) of each frame in all three channels, the way the
    reference's logger shows a one-channel image.  A constant frame is NaN.  Same kernel and rules as rgbmse_view."""
    _nchw(x, "gray_view", 1)
    b, _, h, w = x.shape
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=x.device)
    ws, need = _stats(b, x.device)
    check(lib().ct_view_scaled_plane_f32(_ptr(x), None, _ptr(out), _ptr(ws), need, b, h, w, CT_VIEW_GRAY, _stream()))
    return out


def flow_to_image(flow):
    """utils/flow_viz.py:229-264 (flow_to_image, the Middlebury colour code) on a float32 [B,2,H,W] device tensor -> uint8 [B,H,W,3],
    every frame normalised by its own largest radius (ct_flow_to_image_u8).  Pixels with |u| or |v| > 1e7 are unknown: black, and
    not part of the maximum; NaN pixels likewise (the reference's own maximum does not survive a NaN).  An all-zero flow is white.
    The input is not modified (the reference zeroes the unknown pixels of its argument in place)."""
    _nchw(flow, "flow_to_image", 2)
    b, _, h, w = flow.shape
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=flow.device)
    ws, need = _stats(b, flow.device)
    check(lib().ct_flow_to_image_u8(_ptr(flow), _ptr(out), _ptr(ws), need, b, h, w, _stream()))
    return out

"""Training / validation samples (crop, flips and the chain of colour adjustments of the reference's ArtificialTrainValDataset;
csrc/augment.hip) and the step losses (L1, MSE and kornia's SSIM loss; csrc/losses.hip)."""
import numpy as np
import torch

from ._core import CtHipError, SIGNATURES, _c_int, _c_p, _c_sz, _check_device, _f32c, _opt, _ptr, _stream, _upload_small, check, lib
from .metrics import DISTORTIONS

SIGNATURES.update({
    "ct_augment_workspace_bytes": (_c_sz, [_c_int]),
    "ct_augment_u8": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p, _c_p, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p, _c_sz, _c_p]),
    "ct_frame_losses_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "ct_frame_losses_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_p]),
})

AUGMENT_MAX_OPS = 6
AUGMENT_KINDS = dict(DISTORTIONS, sharpness=6)
# include/ct_hip.h: ct_augment_sample, 144 bytes
AUGMENT_SAMPLE = np.dtype({"names": ["top", "left", "swap_hflip", "vflip", "n_ops", "kind", "reserved", "param", "one_minus"],
                           "formats": ["<i4", "<i4", "<i4", "<i4", "<i4", ("<i4", AUGMENT_MAX_OPS), "<i4", ("<f8", AUGMENT_MAX_OPS),
                                       ("<f8", AUGMENT_MAX_OPS)],
                           "offsets": [0, 4, 8, 12, 16, 20, 44, 48, 96], "itemsize": 144})


def augment_table(params):
    """A sequence of per-sample dicts {top, left, swap_hflip, vflip, ops: [(kind, param), ...]} (kind: a name of AUGMENT_KINDS or its
    number) -> the ct_augment_sample records the library reads; 1 - param is formed here, in float64.  More than six operations
    cannot be stored: ValueError."""
    table = np.zeros(len(params), dtype=AUGMENT_SAMPLE)
    for rec, p in zip(table, params):
        ops = list(p.get("ops", ()))
        if len(ops) > AUGMENT_MAX_OPS:
            raise ValueError("augment_u8: a chain has at most %d operations (got %d)" % (AUGMENT_MAX_OPS, len(ops)))
        rec["top"], rec["left"], rec["swap_hflip"], rec["vflip"], rec["n_ops"] = int(p["top"]), int(p["left"]), int(p["swap_hflip"]), int(p["vflip"]), len(ops)
        for k, (kind, value) in enumerate(ops):
            rec["kind"][k] = AUGMENT_KINDS[kind] if isinstance(kind, str) else int(kind)
            rec["param"][k] = float(value)
            rec["one_minus"][k] = 1.0 - float(value)
    return table


def augment_u8(gt, ref, params, crop_size, want_u8=False):
    """One batch of the reference's ArtificialTrainValDataset samples (utils/data.py:65-84) from n source pairs of one size.
    gt, ref: uint8 [n,3,H,W] device tensors (what read_image returns, stacked); params: n dicts as for augment_table (utils.data's
    sample_params draws them); crop_size: (crop_h, crop_w).  Returns {"gt", "reference", "target"}: float32 [n,3,crop_h,crop_w] =
    the cropped / flipped views and the distorted gt, each / 255 (and "target_u8" when want_u8).  A parameter out of range is a
    ValueError, as torchvision raises.  Asynchronous on the current stream; deterministic."""
    for t in (gt, ref):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[1] != 3 or not t.is_contiguous():
            raise CtHipError("augment_u8 needs contiguous uint8 [n,3,H,W] device tensors")
        _check_device(t)
    if gt.shape != ref.shape or gt.device != ref.device:
        raise CtHipError("augment_u8: gt of shape %s on %s, ref of shape %s on %s" % (tuple(gt.shape), gt.device, tuple(ref.shape), ref.device))
    n, _, h, w = gt.shape
    if len(params) != n:
        raise CtHipError("augment_u8: %d source pairs but %d parameter records" % (n, len(params)))
    ch, cw = int(crop_size[0]), int(crop_size[1])
    table = params if isinstance(params, np.ndarray) and params.dtype == AUGMENT_SAMPLE else augment_table(params)
    table = np.ascontiguousarray(table)
    out = {k: torch.empty((n, 3, max(ch, 0), max(cw, 0)), dtype=torch.float32, device=gt.device) for k in ("gt", "reference", "target")}
    if want_u8:
        out["target_u8"] = torch.empty((n, 3, max(ch, 0), max(cw, 0)), dtype=torch.uint8, device=gt.device)
    table_dev = _upload_small(table.view(np.int64), gt.device)       # 8-byte aligned records
    need = lib().ct_augment_workspace_bytes(n)
    ws = torch.empty(need // 8, dtype=torch.int64, device=gt.device)                  # private to this call: the grey sums
    rc = lib().ct_augment_u8(_ptr(gt), _ptr(ref), n, h, w, table.ctypes.data, _ptr(table_dev), ch, cw, _ptr(out["gt"]), _ptr(out["reference"]),
                             _ptr(out["target"]), _opt(out.get("target_u8")), _ptr(ws), ws.numel() * 8, _stream())
    if rc == -1:
        raise ValueError("augment_u8: a crop of %dx%d that leaves the %dx%d source, an unknown operation or a parameter out of range" % (ch, cw, h, w))
    check(rc)
    return out


def frame_losses(a, b):
    """The step losses of the reference (methods/dmsct.py:118-131, methods/dcmcs3di.py) for a result a and a ground truth b, float32
    [B,3,H,W] device tensors of one shape.  Returns (batch, per_frame): per_frame float64 [B,3] = each frame's F.l1_loss, F.mse_loss and
    kornia.losses.ssim_loss(window_size=11) (restated, parity unpinned); batch float64 [3] = the reference's batch values (one mean
    over B, C, H, W), the mean of the per-frame values.  Frames need more than 5 pixels either way.  Deterministic; asynchronous."""
    _f32c(a, b)
    if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3 or a.device != b.device or not a.numel():
        raise CtHipError("frame_losses needs two float32 [B,3,H,W] tensors of one shape")
    n, _, h, w = a.shape
    if h < 6 or w < 6:
        raise CtHipError("frame_losses: the reflect padding of 5 needs frames of more than 5 pixels either way (got %d x %d)" % (h, w))
    out = torch.empty((n, 3), dtype=torch.float64, device=a.device)
    need = lib().ct_frame_losses_workspace_bytes(n, h, w)
    ws = torch.empty(need // 8, dtype=torch.float64, device=a.device)
    check(lib().ct_frame_losses_f32(_ptr(a), _ptr(b), _ptr(out), _ptr(ws), need, n, h, w, _stream()))
    return out.mean(dim=0), out

"""Sums of the parallax-attention losses over materialised attention maps (pasmnet/losses.py; csrc/pam_losses.hip)."""
import torch

from ._core import CtHipError, SIGNATURES, _c_i64, _c_int, _c_p, _c_sz, _f32c, _opt, _ptr, _stream, check, lib
from .disparity import _mask_f32

SIGNATURES.update({
    "ct_pam_losses_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "ct_pam_cycle_l1_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_p]),
    "ct_pam_map_sweep_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_int, _c_int, _c_p]),
    "ct_masked_l1_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_sz, _c_int, _c_i64, _c_i64, _c_i64, _c_p]),
})

PAM_SWEEP_MAX_W = 1024


def _maps(name, *atts):
    """[B,H,W,W] float32 contiguous device maps of one shape -> (b, h, w)"""
    for t in atts:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise CtHipError("%s runs on the GPU only (no CPU fallback)" % name)
        if t.dim() != 4 or t.shape[2] != t.shape[3] or t.shape != atts[0].shape or not t.numel():
            raise CtHipError("%s needs attention maps of one shape [B,H,W,W], got %s" % (name, tuple(t.shape)))
    _f32c(*atts)
    return tuple(atts[0].shape[:3])


def _workspace(b, h, w, device):
    need = lib().ct_pam_losses_workspace_bytes(b, h, w)
    return torch.empty(need // 8, dtype=torch.float64, device=device), need       # private to the call


def pam_cycle_l1(att_a, att_b, mask):
    """loss_pam_cycle's sums for the cycle map att_a @ att_b WITHOUT building it: att_a, att_b float32 [B,H,W,W], mask bool or 0/1
    float [B,1,H,W].  Returns (num, count), float64 [B] device tensors: num[b] = sum_h sum_i mask[h][i] sum_k |(A_h B_h)[i][k] -
    delta_ik| (the product on the exact-f32 MFMA), count[b] = sum mask.  The reference's value is num.sum() / count.sum() (NaN for a
    count of zero).  Deterministic; asynchronous."""
    b, h, w = _maps("pam_cycle_l1", att_a, att_b)
    mask = _mask_f32(mask, (b, 1, h, w), "pam_cycle_l1")
    out = torch.empty((b, 2), dtype=torch.float64, device=att_a.device)
    ws, need = _workspace(b, h, w, att_a.device)
    check(lib().ct_pam_cycle_l1_f32(_ptr(att_a), _ptr(att_b), _ptr(mask), _ptr(out), _ptr(ws), need, b, h, w, _stream()))
    return out[:, 0], out[:, 1]


def pam_map_sweep(att, src=None, dst=None, mask=None):
    """One pass over att float32 [B,H,W,W] (W <= 1024).  Returns a dict of per-image float64 [B] tensors (on the device, but for the
    two analytic counts, which are host tensors):
        vertical, vertical_count      sum |att[h] - att[h+1]| and (H-1) W W                       loss_pam_smoothness, first term
        diagonal, diagonal_count      sum |att[:, i, j] - att[:, i+1, j+1]| and H (W-1) (W-1)      loss_pam_smoothness, second term
        photometric                   sum_c mask |dst - warp(src, att)|        (None without src, dst [B,3,H,W] float32 and mask)
        identity                      sum mask sum_j |att - I|                 (None without mask): loss_pam_cycle of a cycle map
        mask_sum                      sum mask                                 (None without mask)
    mask: bool or 0/1 float [B,1,H,W].  The reference divides the batch sums: x.sum() / count.sum(), 0 / 0 = NaN included.
    Deterministic; asynchronous."""
    b, h, w = _maps("pam_map_sweep", att)
    if w > PAM_SWEEP_MAX_W:
        raise CtHipError("pam_map_sweep: maps of up to %d columns (got %d)" % (PAM_SWEEP_MAX_W, w))
    if (src is None) != (dst is None) or (src is not None and mask is None):
        raise CtHipError("pam_map_sweep: the photometric term needs src, dst and mask together")
    if src is not None:
        for t in (src, dst):
            if not torch.is_tensor(t) or tuple(t.shape) != (b, 3, h, w):
                raise CtHipError("pam_map_sweep: src and dst must be [B,3,H,W] images of the maps' size")
        _f32c(src, dst)
    if mask is not None:
        mask = _mask_f32(mask, (b, 1, h, w), "pam_map_sweep")
    out = torch.empty((b, 5), dtype=torch.float64, device=att.device)
    ws, need = _workspace(b, h, w, att.device)
    check(lib().ct_pam_map_sweep_f32(_ptr(att), _opt(src), _opt(dst), _opt(mask), _ptr(out), _ptr(ws), need, b, h, w, _stream()))
    counts = torch.tensor([(h - 1) * w * w, h * (w - 1) * (w - 1)], dtype=torch.float64).expand(b, 2)     # per image, like the sums
    return dict(vertical=out[:, 0], vertical_count=counts[:, 0], diagonal=out[:, 1], diagonal_count=counts[:, 1],
                photometric=out[:, 2] if src is not None else None, identity=out[:, 3] if mask is not None else None,
                mask_sum=out[:, 4] if mask is not None else None)


def masked_l1_sums(x, y, mask):
    """The sums of the reference's masked_l1_loss for the two layouts it is called with: x, y float32 [B,3,H,W] with mask [B,1,H,W],
    or x, y float32 [B,H,W,W'] with mask [B,H,W,1] (bool or 0/1 float).  Returns (sum |x - y| * mask, sum mask), float64 [B]."""
    for t in (x, y, mask):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise CtHipError("masked_l1_sums runs on the GPU only (no CPU fallback)")
    if x.dim() != 4 or x.shape != y.shape or mask.dim() != 4 or not x.numel():
        raise CtHipError("masked_l1_sums needs x, y of one 4-d shape and a 4-d mask")
    _f32c(x, y)
    n = x.shape[0]
    if mask.shape[1] == 1 and tuple(mask.shape) == (n, 1) + tuple(x.shape[2:]):
        a, p, b = x.shape[1], x.shape[2] * x.shape[3], 1
    elif mask.shape[3] == 1 and tuple(mask.shape) == tuple(x.shape[:3]) + (1,):
        a, p, b = 1, x.shape[1] * x.shape[2], x.shape[3]
    else:
        raise CtHipError("masked_l1_sums: mask %s does not broadcast over x %s as [B,1,H,W] or [B,H,W,1]" % (tuple(mask.shape), tuple(x.shape)))
    mask = _mask_f32(mask, mask.shape, "masked_l1_sums")
    out = torch.empty((n, 2), dtype=torch.float64, device=x.device)
    ws = torch.empty(n * 64, dtype=torch.float64, device=x.device)
    check(lib().ct_masked_l1_f32(_ptr(x), _ptr(y), _ptr(mask), _ptr(out), _ptr(ws), ws.numel() * 8, n, a, p, b, _stream()))
    return out[:, 0], out[:, 1]

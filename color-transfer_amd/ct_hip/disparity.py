"""Disparity of the parallax attention (pasmnet/utils.py:55-105; csrc/disparity.hip)."""
import torch

from ._core import CtHipError, SIGNATURES, _c_f, _c_int, _c_p, _check_device, _f32c, _ptr, _stream, check, lib

SIGNATURES.update({
    "ct_attention_rows64_disp_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_f, _c_p]),
    "ct_pam_disp_fill_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p]),
    "ct_pam_regress_disp_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p]),
})


def attention_rows64_index(qt, kt, b, h, w):
    """disp_ini [B,1,H,W] = i - sum_j softmax_j(q_i.k_j / 64) j from token rows qt, kt [B*H, W, 64] (the index-only streaming pass)"""
    for t in (qt, kt):
        if t.shape != (b * h, w, 64):
            raise CtHipError("attention_rows64_index needs [B*H, W, 64] token rows")
    _f32c(qt, kt)
    disp_ini = torch.empty((b, 1, h, w), dtype=torch.float32, device=qt.device)
    check(lib().ct_attention_rows64_disp_f32(_ptr(qt), _ptr(kt), _c_p(0), _c_p(0), _ptr(disp_ini), b * h, w, 1.0 / 64, _stream()))
    return disp_ini


def _mask_f32(valid, shape, name):
    if not torch.is_tensor(valid) or not valid.is_cuda:
        raise CtHipError("%s: the mask must be a CUDA tensor (no CPU path)" % name)
    _check_device(valid)
    if tuple(valid.shape) != tuple(shape):
        raise CtHipError("%s: mask of shape %s, expected %s" % (name, tuple(valid.shape), tuple(shape)))
    return valid.to(torch.float32).contiguous()


def pam_disp_fill(disp_ini, valid):
    """The occlusion fill of regress_disp (utils.py:85-105) on disp_ini [B,1,H,W]: valid pixels keep disp_ini, an invalid pixel k
    steps right of a valid one gets its value divided k times by float32 (1 + 1e-4), the hole at a row's start likewise from the
    row's first valid pixel, a row without valid pixels 0.  valid: bool or 0/1 float [B,1,H,W]."""
    _f32c(disp_ini)
    if disp_ini.dim() != 4 or disp_ini.shape[1] != 1:
        raise CtHipError("pam_disp_fill needs disp_ini of shape [B,1,H,W]")
    valid = _mask_f32(valid, disp_ini.shape, "pam_disp_fill")
    b, _, h, w = disp_ini.shape
    out = torch.empty_like(disp_ini)
    check(lib().ct_pam_disp_fill_f32(_ptr(disp_ini), _ptr(valid), _ptr(out), b, h, w, _stream()))
    return out


def regress_disp(att, valid):
    """pasmnet/utils.py:55-105 on the GPU: att [B,H,W,W] float32 (rows need not sum to 1), valid bool or 0/1 float [B,1,H,W]
    -> disp [B,1,H,W] float32.  One pass over att (i - sum_j att_ij j, fixed order), then the row fill of pam_disp_fill."""
    if not torch.is_tensor(att) or not att.is_cuda:
        raise CtHipError("regress_disp runs on the GPU only (no CPU fallback)")
    if att.dim() != 4 or att.shape[2] != att.shape[3]:
        raise CtHipError("regress_disp needs att of shape [B,H,W,W]")
    att = att.to(torch.float32).contiguous()
    _f32c(att)
    b, h, w, _ = att.shape
    valid = _mask_f32(valid, (b, 1, h, w), "regress_disp")
    out = torch.empty((b, 1, h, w), dtype=torch.float32, device=att.device)
    check(lib().ct_pam_regress_disp_f32(_ptr(att), _ptr(valid), _ptr(out), b, h, w, _stream()))
    return out

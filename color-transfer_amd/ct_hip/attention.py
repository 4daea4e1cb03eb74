"""Attention (csrc/pam.hip, attention_tokens.hip, attention16.hip): DCMCS3DI's parallax attention (dense and
streaming, token rows) and GMFlow's token / window attention."""
import ctypes

import torch

from ._core import (CtHipError, SIGNATURES, _c_f, _c_int, _c_ll, _c_p, _c_sz, _check_device, _f32c, _nchw_bstride, _opt, _ptr, _stream,
                    check, lib, workspace)

SIGNATURES.update({
    "ct_pam_workspace_bytes": (_c_sz, [_c_int, _c_int, _c_int]),
    "ct_pam_attend_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_pam_valid_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_sz, _c_p]),
    "ct_attention_workspace_bytes": (ctypes.c_size_t, [_c_int, _c_int, _c_int, _c_int]),
    "ct_attention_tokens_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_f, _c_int, _c_p,
                                         ctypes.c_size_t, ctypes.c_longlong, _c_p]),
    "ct_nchw_to_rows_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_ll, _c_int, _c_int, _c_p]),
    "ct_rows_to_nchw_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_ll, _c_int, _c_int, _c_p]),
    "ct_attention_rows64_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_f, _c_p]),
    "ct_attention_colsum64_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_f, _c_p]),
})


def pam_attend(q, k, v, rgb, want_att=False):
    """softmax(q.k/c) @ [v | rgb] per image row (pasmnet/attention.py:39-41, utils.py:30,123-125)."""
    for t in (q, k, v, rgb):
        if t.is_cuda:
            _check_device(t)
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise CtHipError("pam_attend needs contiguous float32 CUDA tensors")
    n, c, h, w = q.shape
    cv = v.shape[1]
    out_v = torch.empty_like(v)
    out_rgb = torch.empty_like(rgb)
    att = torch.empty((n, h, w, w), dtype=torch.float32, device=q.device) if want_att else None
    check(lib().ct_pam_attend_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(rgb), _ptr(out_v), _ptr(out_rgb),
                                  _ptr(att) if att is not None else _c_p(0), n, c, cv, h, w, _stream()))
    return out_v, out_rgb, att


def pam_valid(q, k, want_att=False):
    """valid mask (as 0/1 float [n,1,h,w]) + pre-threshold column sums of softmax(q.k/c) (utils.py:31,34-35)."""
    for t in (q, k):
        if t.is_cuda:
            _check_device(t)
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise CtHipError("pam_valid needs contiguous float32 CUDA tensors")
    n, c, h, w = q.shape
    valid = torch.empty((n, 1, h, w), dtype=torch.float32, device=q.device)
    colsum = torch.empty((n, 1, h, w), dtype=torch.float32, device=q.device)
    att = torch.empty((n, h, w, w), dtype=torch.float32, device=q.device) if want_att else None
    need = lib().ct_pam_workspace_bytes(n, h, w)
    ws = workspace(-1, 0, 0, q.device, need=need)
    check(lib().ct_pam_valid_f32(_ptr(q), _ptr(k), _ptr(valid), _ptr(colsum), _ptr(att) if att is not None else _c_p(0),
                                 n, c, h, w, _ptr(ws), ws.numel(), _stream()))
    return valid, colsum, att


def attention_tokens(q, k, v, region=None, scale=None, rowmap=None, nsplit=None, kv_shift=0):
    """q,k [B,L,128], v [B,L,128] or [B,L,2]; region int32 [B,L] or None -> [B,L,cv].
    With rowmap (int32 [B', L']): B' x L' attention problems whose token (b, i) is row rowmap[b, i] of the flattened
    q / k / v / out -- window partitions without copies; the result has v's shape.  kv_shift (with rowmap): keys / values are
    read kv_shift rows further (mod the row count) than the queries: cross attention to the other half of the batch."""
    _f32c(q, k, v)
    c, cv = q.shape[-1], v.shape[-1]
    for t in (region, rowmap):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise CtHipError("region / rowmap must be contiguous int32")
    if rowmap is not None:
        b, l = rowmap.shape
        if region is not None and tuple(region.shape) != (b, l):
            raise CtHipError("region and rowmap must have the same shape")
        if b * l != q.numel() // c or b * l != v.numel() // cv or k.shape != q.shape:
            raise CtHipError("rowmap must be a permutation of the token rows")
        out = torch.empty_like(v)
    else:
        b, l, _ = q.shape
        out = torch.empty((b, l, cv), dtype=torch.float32, device=q.device)
    if nsplit is None:
        # key split so that ~2 workgroups per CU exist (global matching at 1/8 resolution launches only 56 otherwise)
        wgs = b * ((l + 127) // 128)
        nsplit = 1 if wgs >= 384 else max(1, min(8, 512 // max(wgs, 1), (l + 255) // 256))
    ws, need = None, 0
    if nsplit > 1:
        need = lib().ct_attention_workspace_bytes(b, l, cv, nsplit)
        ws = workspace(-2, 0, 0, q.device, need=need)
    check(lib().ct_attention_tokens_f32(_ptr(q), _ptr(k), _ptr(v), _opt(region), _opt(rowmap), _ptr(out), b, l, cv,
                                        float(scale if scale is not None else c ** -0.5), nsplit, _opt(ws), need, int(kv_shift), _stream()))
    return out


def nchw_to_tokens(x):
    """[B,C,H,W] -> channels-last tokens [B, H*W, C] (transformer.py:238-239's flatten + permute) through the LDS-tiled transpose"""
    _f32c(x)
    b, c, h, w = x.shape
    out = torch.empty((b, h * w, c), dtype=torch.float32, device=x.device)
    check(lib().ct_nchw_to_rows_f32(_ptr(x), _ptr(out), b, c, h, w, c * h * w, c, 0, _stream()))
    return out


def tokens_to_nchw(t, h, w):
    """tokens [B, H*W, C] -> [B,C,H,W]"""
    _f32c(t)
    b, l, c = t.shape
    if l != h * w:
        raise CtHipError("tokens_to_nchw: %d tokens are not %d x %d" % (l, h, w))
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=t.device)
    check(lib().ct_rows_to_nchw_f32(_ptr(t), _ptr(out), b, c, h, w, c * h * w, c, 0, _stream()))
    return out


def pam_streaming(q, k, v, rgb, q_other, k_other, want_disp=False):
    """DCMCS3DI's parallax attention through the streaming kernels (any width):
    q,k [B,64,H,W] = Q(left), K(right); v [B,64,H,W], rgb [B,3,H,W]; q_other,k_other = Q(right), K(left).
    Returns (fea_warped [B,64,H,W], warped_rgb [B,3,H,W], valid [B,1,H,W] 0/1, colsum [B,1,H,W]), and with want_disp the
    unfilled disparity disp_ini [B,1,H,W] = i - E[j] under the same attention as a fifth element (pam_streaming_rows)."""
    _f32c(q, k, v, rgb, q_other, k_other)
    b, c, h, w = q.shape
    if c != 64 or v.shape[1] != 64:
        raise CtHipError("pam_streaming is built for 64 channels")
    vt = torch.empty((b * h, w, 96), dtype=torch.float32, device=q.device)
    nchw_to_rows(v, vt, 0)
    return pam_streaming_rows(nchw_to_rows(q), nchw_to_rows(k), vt, rgb, nchw_to_rows(q_other), nchw_to_rows(k_other),
                              want_disp=want_disp)


def nchw_to_rows(t, out=None, c0=0):
    """[B,C,H,W] -> channels c0.. of a [B*H, W, C'] token-rows tensor (data movement only)"""
    b, ct, h, w = t.shape
    if out is None:
        out = torch.empty((b * h, w, ct), dtype=torch.float32, device=t.device)
    check(lib().ct_nchw_to_rows_f32(_ptr(t), _ptr(out), b, ct, h, w, _nchw_bstride(t), out.shape[2], c0, _stream()))
    return out


def pam_streaming_rows(qt, kt, vt, rgb, qo, ko, want_disp=False):
    """pam_streaming on token rows: qt, kt, qo, ko [B*H, W, 64] (contiguous; views of a larger rows tensor along dim 0 are fine);
    vt [B*H, W, 96] with the value in channels 0..63 -- channels 64..95 are filled here (rgb [B,3,H,W] + zero padding).
    want_disp: the attend pass also accumulates the expected matching column (ct_attention_rows64_disp_f32, same `out` bit for
    bit) and disp_ini [B,1,H,W] is returned as a fifth element."""
    b, _, h, w = rgb.shape
    for t in (qt, kt, qo, ko):
        if t.shape != (b * h, w, 64) or not t.is_contiguous() or t.dtype != torch.float32 or not t.is_cuda:
            raise CtHipError("pam_streaming_rows needs contiguous float32 [B*H, W, 64] CUDA tensors")
    if vt.shape != (b * h, w, 96) or not vt.is_contiguous() or vt.dtype != torch.float32:
        raise CtHipError("pam_streaming_rows needs a contiguous float32 [B*H, W, 96] value tensor")
    _f32c(rgb)
    scale = 1.0 / 64                                  # the reference scales by 1/c, not 1/sqrt(c) (attention.py:41)

    def nchw(t, ct, c0):                              # [B*H, W, C'] tokens -> [B,ct,H,W] from channels c0..c0+ct
        out = torch.empty((b, ct, h, w), dtype=torch.float32, device=t.device)
        check(lib().ct_rows_to_nchw_f32(_ptr(t), _ptr(out), b, ct, h, w, ct * h * w, t.shape[2], c0, _stream()))
        return out
    vt[:, :, 67:] = 0.0                               # the 29 padding channels of the 96-channel value
    nchw_to_rows(rgb, vt, 64)
    out = torch.empty((b * h, w, 96), dtype=torch.float32, device=qt.device)
    if want_disp:
        disp_ini = torch.empty((b, 1, h, w), dtype=torch.float32, device=qt.device)
        check(lib().ct_attention_rows64_disp_f32(_ptr(qt), _ptr(kt), _ptr(vt), _ptr(out), _ptr(disp_ini), b * h, w, scale, _stream()))
    else:
        check(lib().ct_attention_rows64_f32(_ptr(qt), _ptr(kt), _ptr(vt), _ptr(out), _c_p(0), b * h, w, scale, _stream()))
    fea = nchw(out, 64, 0)
    wrgb = nchw(out, 3, 64)
    valid, colsum = pam_valid_rows(qo, ko, b, h, w)
    if want_disp:
        return fea, wrgb, valid, colsum, disp_ini
    return fea, wrgb, valid, colsum


def pam_valid_rows(qo, ko, b, h, w):
    """valid mask of the left view from the streaming kernels: qo = Q(right), ko = K(left) as token rows [B*H, W, 64].
    Returns (valid [B,1,H,W] 0/1, colsum [B,1,H,W])."""
    scale = 1.0 / 64
    stats = torch.empty((b * h, w, 2), dtype=torch.float32, device=qo.device)
    check(lib().ct_attention_rows64_f32(_ptr(qo), _ptr(ko), _c_p(0), _c_p(0), _ptr(stats), b * h, w, scale, _stream()))
    colsum = torch.empty((b * h, w), dtype=torch.float32, device=qo.device)
    check(lib().ct_attention_colsum64_f32(_ptr(qo), _ptr(ko), _ptr(stats), _ptr(colsum), b * h, w, scale, _stream()))
    colsum = colsum.view(b, 1, h, w)
    valid = (colsum > 0.1).float()                    # threshold only (utils.py:34); the sums come from the kernel
    return valid, colsum

"""GMFlow building blocks that are neither convolutions nor token layers (csrc/gmflow.hip, local_corr.hip): instance norm,
elementwise steps, local correlation, warping, convex upsampling, the forward-backward check."""
import ctypes

import torch

from ._core import SIGNATURES, _c_f, _c_int, _c_ll, _c_p, _f32c, _opt, _ptr, _stream, check, lib, workspace

SIGNATURES.update({
    "ct_instance_norm_workspace_bytes": (ctypes.c_size_t, [_c_int]),
    "ct_instance_norm_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_f, _c_int, _c_p, ctypes.c_size_t, _c_p]),
    "ct_eltwise_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_ll, _c_int, _c_int, _c_int, _c_int, _c_f, _c_p]),
    "ct_local_corr_softmax_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_local_corr_flow_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_local_attn_prop_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_flow_warp_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_convex_upsample_f32": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_fb_check_f32": (_c_int, [_c_p] * 6 + [_c_int, _c_int, _c_int, _c_f, _c_f, _c_p]),
})


def instance_norm(x, mode=0, skip=None, eps=1e-5):
    _f32c(x, skip)
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    need = lib().ct_instance_norm_workspace_bytes(n * c)
    ws = workspace(-3, 0, 0, x.device, need=need)
    check(lib().ct_instance_norm_f32(_ptr(x), _opt(skip), _ptr(y), n * c, h * w, eps, mode, _ptr(ws), need, _stream()))
    return y


def eltwise(op, a, b=None, c=None, plane=1, chans=1, split=0, s0=1.0):
    _f32c(a, b, c)
    y = torch.empty_like(a)
    check(lib().ct_eltwise_f32(_ptr(a), _opt(b), _opt(c), _ptr(y), a.numel(), op, plane, chans, split, float(s0), _stream()))
    return y


def local_corr_softmax(f0, f1, h, w, radius):
    _f32c(f0, f1)
    b = f0.shape[0]
    flow = torch.empty((b, 2, h, w), dtype=torch.float32, device=f0.device)
    check(lib().ct_local_corr_softmax_f32(_ptr(f0), _ptr(f1), _ptr(flow), b, h, w, radius, _stream()))
    return flow


def local_corr_flow(f0, f1, flow, radius):
    _f32c(f0, f1, flow)
    b, _, h, w = flow.shape
    corr = torch.empty((b, (2 * radius + 1) ** 2, h, w), dtype=torch.float32, device=f0.device)
    check(lib().ct_local_corr_flow_f32(_ptr(f0), _ptr(f1), _ptr(flow), _ptr(corr), b, h, w, radius, _stream()))
    return corr


def local_attn_prop(q, k, flow, radius):
    _f32c(q, k, flow)
    b, _, h, w = flow.shape
    out = torch.empty_like(flow)
    check(lib().ct_local_attn_prop_f32(_ptr(q), _ptr(k), _ptr(flow), _ptr(out), b, h, w, radius, _stream()))
    return out


def flow_warp(img, flow):
    _f32c(img, flow)
    n, c, h, w = img.shape
    out = torch.empty_like(img)
    check(lib().ct_flow_warp_f32(_ptr(img), _ptr(flow), _ptr(out), n, c, h, w, _stream()))
    return out


def convex_upsample(flow, mask, factor):
    _f32c(flow, mask)
    b, _, h, w = flow.shape
    out = torch.empty((b, 2, h * factor, w * factor), dtype=torch.float32, device=flow.device)
    check(lib().ct_convex_upsample_f32(_ptr(flow), _ptr(mask), _ptr(out), b, h, w, factor, _stream()))
    return out


def fb_check(fwd, bwd, alpha=0.01, beta=0.5):
    """forward_backward_consistency_check (geometry.py:78-99) -> (fwd_occ, bwd_occ) [B,H,W] as 0/1 floats"""
    _f32c(fwd, bwd)
    b, _, h, w = fwd.shape
    wb, wf = flow_warp(bwd, fwd), flow_warp(fwd, bwd)
    fo = torch.empty((b, h, w), dtype=torch.float32, device=fwd.device)
    bo = torch.empty_like(fo)
    check(lib().ct_fb_check_f32(_ptr(fwd), _ptr(bwd), _ptr(wb), _ptr(wf), _ptr(fo), _ptr(bo), b, h, w, alpha, beta, _stream()))
    return fo, bo

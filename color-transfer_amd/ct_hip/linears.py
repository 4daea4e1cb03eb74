"""nn.Linear on channels-last tokens and LayerNorm(128) (csrc/linear_tokens.hip, linear_ws16.hip): the exact,
three-piece bf16 and weight-stationary fp16 kernels."""
import os

import torch

from ._core import ACT_GELU, ACT_NONE, CtHipError, SIGNATURES, _c_int, _c_ll, _c_p, _cached_pack, _f32c, _opt, _ptr, _stream, check, lib
from .conv import conv_mode
from .packing import pack_linear_weight_split, pack_linear_weight_ws16

SIGNATURES.update({
    "ct_linear_tokens_f32": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_ll, _c_int, _c_int, _c_int, _c_p]),
    "ct_linear_tokens_split_f32": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_ll, _c_int, _c_int, _c_int, _c_p]),
    "ct_layernorm128_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_ll, _c_int, _c_p]),
    "ct_linear_ws16_f32": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_int, _c_p, _c_p, _c_ll, _c_int, _c_int, _c_int, _c_p, _c_p, _c_p, _c_p]),
})


def _packed_linear(weight):
    ver = (weight._version, weight.data_ptr(), str(weight.device))
    return _cached_pack(weight, "_ct_lin_split", ver, lambda: pack_linear_weight_split(weight))


def _packed_linear_ws16(weight):
    ver = (weight._version, weight.data_ptr(), str(weight.device))
    return _cached_pack(weight, "_ct_lin_ws16", ver, lambda: pack_linear_weight_ws16(weight))


_lin_ws16 = os.environ.get("CT_HIP_LINEAR_WS16", "1") != "0"


def linear_tokens_multi(x, weights, biases=None, mode=None):
    """[linear_tokens(x, w, b) for w, b in zip(weights, biases)] for up to four 128 -> 128 layers reading the SAME tokens (the q / k /
    v projections of a transformer layer, transformer.py:26-31): one launch of ct_linear_ws16_f32 whose feature slices share the
    tokens through L2 and write one result slab each.  Falls back to separate calls where that kernel does not apply."""
    biases = list(biases) if biases is not None else [None] * len(weights)
    k = x.shape[-1]
    t = x.numel() // k
    ok = ((mode or conv_mode()) == "split" and _lin_ws16 and k == 128 and 1 <= len(weights) <= 4 and t >= 4096 and
          all(tuple(w.shape) == (128, 128) for w in weights) and (all(b is None for b in biases) or all(b is not None for b in biases)))
    if not ok:
        return [linear_tokens(x, w, b, mode=mode) for w, b in zip(weights, biases)]
    _f32c(x, *weights, *biases)
    ver = tuple((w._version, w.data_ptr()) for w in weights) + (str(x.device),)
    img, w_exp = _cached_pack(weights[0], "_ct_lin_ws16_multi", ver,
                              lambda: pack_linear_weight_ws16(torch.cat([w.detach() for w in weights], dim=0)))
    bias = torch.cat([b.detach().float() for b in biases]) if biases[0] is not None else None
    out = torch.empty((len(weights),) + tuple(x.shape[:-1]) + (128,), dtype=torch.float32, device=x.device)
    check(lib().ct_linear_ws16_f32(_ptr(x), _c_p(0), 128, _ptr(img), int(w_exp), _opt(bias), _ptr(out), t, 128, 128 * len(weights), 0,
                                   _c_p(0), _c_p(0), _c_p(0), _stream()))
    return [out[i] for i in range(len(weights))]


def linear_layernorm128(x, weight, bias, gamma, beta, residual=None, mode=None):
    """[residual +] LayerNorm_128(linear(x, weight, bias)) for a 128 -> 128 layer (the merge projection with norm1 and the skip,
    transformer.py:120-127,139-147): one launch of ct_linear_ws16_f32 where that kernel applies, else the two kernels"""
    t = x.numel() // x.shape[-1]
    if ((mode or conv_mode()) == "split" and _lin_ws16 and tuple(weight.shape) == (128, 128) and x.shape[-1] == 128 and t >= 4096):
        _f32c(x, weight, bias, gamma, beta, residual)
        img, w_exp = _packed_linear_ws16(weight)
        out = torch.empty_like(x)
        check(lib().ct_linear_ws16_f32(_ptr(x), _c_p(0), 128, _ptr(img), int(w_exp), _opt(bias), _ptr(out), t, 128, 128, 0,
                                       _ptr(gamma), _ptr(beta), _opt(residual), _stream()))
        return out
    return layernorm128(linear_tokens(x, weight, bias, mode=mode), gamma, beta, residual=residual)


def set_linear_ws16(on):
    """True (default): the FFN-shaped linears (K = 256 -> N % 128 = 0; K % 256 = 0 -> N = 128 as partial slabs) run in
    ct_linear_ws16_f32 (weight slice resident in LDS, two fp16 pieces); False: everything in ct_linear_tokens_split_f32"""
    global _lin_ws16
    _lin_ws16 = bool(on)


def linear_tokens(x, weight, bias=None, act=ACT_NONE, x2=None, mode=None, partials=False):
    """x [..., K1] channels-last tokens (optionally concatenated with x2 [..., K2] on the fly), weight [N, K1+K2]
    (PyTorch layout) -> [..., N].  mode (default: conv_mode()): "split" = 16-bit matrix pipe, float32-grade (K % 32 == 0; the
    pre-split weight is cached on the weight tensor); "exact" = v_mfma_f32_32x32x2_f32.
    partials=True: the result may come back as [P, ..., N] slabs whose sum over P is the result (K-sliced ct_linear_ws16_f32;
    layernorm128 adds them on its way in) -- the caller must accept either shape (P == 1 slab otherwise)."""
    _f32c(x, weight, bias, x2)
    k1, n = x.shape[-1], weight.shape[0]
    k = k1 + (x2.shape[-1] if x2 is not None else 0)
    if weight.shape[1] != k or (x2 is not None and x2.shape[:-1] != x.shape[:-1]):
        raise CtHipError("linear_tokens: shape mismatch")
    t = x.numel() // k1
    if (mode or conv_mode()) == "split" and _lin_ws16 and act in (ACT_NONE, ACT_GELU) and t >= 4096:
        nsl = k == 256 and n % 128 == 0 and n // 128 in (1, 2, 4, 8) and (k1 == 128 if x2 is not None else True)
        ksl = (not nsl) and partials and n == 128 and k % 256 == 0 and k // 256 in (2, 4, 8) and x2 is None and act == ACT_NONE
        if nsl or ksl:
            img, w_exp = _packed_linear_ws16(weight)
            shape = ((k // 256,) if ksl else ()) + tuple(x.shape[:-1]) + (n,)
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
            check(lib().ct_linear_ws16_f32(_ptr(x), _opt(x2), k1, _ptr(img), int(w_exp), _opt(bias), _ptr(out), t, k, n, int(act),
                                           _c_p(0), _c_p(0), _c_p(0), _stream()))
            return out
    out = torch.empty(x.shape[:-1] + (n,), dtype=torch.float32, device=x.device)
    if (mode or conv_mode()) == "split" and k % 32 == 0:
        check(lib().ct_linear_tokens_split_f32(_ptr(x), _opt(x2), k1, _ptr(_packed_linear(weight)), _opt(bias), _ptr(out), t, k, n,
                                               int(act), _stream()))
    else:
        check(lib().ct_linear_tokens_f32(_ptr(x), _opt(x2), k1, _ptr(weight), _opt(bias), _ptr(out), t, k, n, int(act), _stream()))
    return out


def layernorm128(x, gamma, beta, residual=None, partials=1):
    """LayerNorm(128) (+ residual) of x [..., 128]; partials = P > 1: x is [P, ..., 128] and the input is the sum of its P slabs
    (added in slab order: the K-sliced linear's partial results)"""
    _f32c(x, gamma, beta, residual)
    if x.shape[-1] != 128:
        raise CtHipError("layernorm128: last dim must be 128")
    partials = int(partials)
    if partials < 1 or (partials > 1 and x.shape[0] != partials):
        raise CtHipError("layernorm128: x must be [partials, ..., 128]")
    out = torch.empty(x.shape[1:] if partials > 1 else x.shape, dtype=torch.float32, device=x.device)
    check(lib().ct_layernorm128_f32(_ptr(x), _ptr(gamma), _ptr(beta), _opt(residual), _ptr(out), out.numel() // 128, partials, _stream()))
    return out

"""Convolutions (csrc/conv_exact.hip, conv_split.hip, conv_ws.hip, conv_wino*.hip, conv1x1_rows.hip, conv_generic.hip): the arithmetic
switches, ONE dispatch (_conv_entry) and the three front doors conv2d, conv2d_rows and gconv2d."""
import os

import torch

from ._core import (ACT_NONE, CtHipError, SIGNATURES, _c_int, _c_ll, _c_p, _c_sz, _check_device, _lock, _nchw_bstride, _opt, _ptr,
                    _stream, check, lib)
from .gmflow import eltwise
from .packing import SplitOperands, _split_s2d

SIGNATURES.update({
    "ct_conv2d_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_ll, _c_ll,
                               _c_ll, _c_int, _c_int, _c_p]),
    "ct_conv2d_split_f32": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_int,
                                     _c_int, _c_int, _c_ll, _c_ll, _c_ll, _c_ll, _c_ll, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p,
                                     _c_p, _c_p, _c_ll, _c_p]),
    "ct_conv_split_scratch_bytes": (_c_sz, []),
    "ct_gconv2d_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 10 + [_c_ll, _c_ll, _c_int, _c_p]),
    "ct_conv2d_split_rows_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 7 + [_c_ll, _c_int, _c_int, _c_int, _c_int, _c_int, _c_p]),
    "ct_conv3x3_ws16_f32": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_p, _c_p] + [_c_int] * 5 + [_c_ll, _c_ll, _c_ll, _c_int, _c_int, _c_p]),
    "ct_conv3x3_wino16_f32": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_p, _c_p] + [_c_int] * 5 + [_c_ll, _c_ll, _c_ll, _c_int, _c_int, _c_p]),
    "ct_set_conv_wino_form": (_c_int, [_c_int]),
    "ct_conv1x1_rows_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 5 + [_c_ll, _c_int, _c_int, _c_int, _c_p]),
    "ct_space_to_depth2_f32": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_ll, _c_p]),
})

# ---- convolution arithmetic --------------------------------------------------------------------------------------
# "split": float32 operands as three bf16 pieces, six bf16 MFMAs per product (csrc/conv_split.hip; float32-grade
#          accuracy, 2.67x the matrix rate).  "exact": v_mfma_f32_32x32x2_f32, bitwise an fmaf chain (csrc/conv_exact.hip).
# Geometries the split kernel does not cover (stride 2, 7x7, W % 4 != 0, unaligned views) always run "exact".
_conv_mode = os.environ.get("CT_HIP_CONV", "split")
# split mode: two fp16 pieces / three MFMAs per product (power-of-two scales per layer and per staged tile / row) instead of three
# bf16 pieces / six MFMAs, in the weight-stationary kernel (csrc/conv_ws.hip) and the tile kernel (csrc/conv_split.hip);
# CT_HIP_CONV_WS16=0 switches back to the bf16 form
_ws16 = os.environ.get("CT_HIP_CONV_WS16", "1") != "0"
_wino = os.environ.get("CT_HIP_CONV_WINO", "1") not in ("0", "")
_stream_k = True


def set_conv_mode(mode):
    global _conv_mode
    if mode not in ("split", "exact"):
        raise ValueError("conv mode must be 'split' or 'exact'")
    _conv_mode = mode


def conv_mode():
    return _conv_mode


def set_conv_ws16(on):
    global _ws16
    _ws16 = bool(on)


def conv_ws16():
    return _ws16


def set_conv_wino(on):
    """True (default; env CT_HIP_CONV_WINO=0 turns it off): the 3x3 convolutions that ct_conv3x3_ws16_f32 would take run as
    Winograd F(2x2, 3x3) (ct_conv3x3_wino16_f32: 2.25x fewer matrix instructions, float32-grade); False: the direct kernel."""
    global _wino
    _wino = bool(on)


def conv_wino():
    return _wino


def set_conv_wino_form(form):
    """Which Winograd kernel ct_conv3x3_wino16_f32 launches (include/ct_hip.h: ct_set_conv_wino_form): 0 = the four-wave pipelined
    kernel of round 6 (csrc/conv_wino4.hip, default), 1 = the eight-wave kernel of round 5 (csrc/conv_wino.hip)."""
    check(lib().ct_set_conv_wino_form(int(form)))


def set_conv_stream_k(on):
    """False: the tile convolution gets no scratch, i.e. every workgroup computes whole (tile, 64-channel) units (include/ct_hip.h:
    ct_conv2d_split_f32, scratch == NULL); True (default): badly quantised launches share units between neighbouring workgroups."""
    global _stream_k
    _stream_k = bool(on)


# ---- dispatch: which entry takes a convolution -------------------------------------------------------------------
def _aligned(t):
    """16-byte aligned, batch stride a multiple of four floats: what the vector loads / stores of the split kernels need"""
    return t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0


def _split_ok(x, out, residual, kh, kw, stride, ph, pw):
    """the geometries of the split family: split mode, stride 1, "same" padding, one of four tap shapes, W % 4 == 0, aligned tensors"""
    return (_conv_mode == "split" and stride == 1 and (kh, kw) in ((3, 3), (1, 1), (1, 5), (5, 1)) and (ph, pw) == (kh // 2, kw // 2) and
            x.shape[3] % 4 == 0 and all(t is None or _aligned(t) for t in (x, out, residual)))


def _ws16_ok(x, ops, kh, kw):
    """the layers of the weight-stationary kernels (direct and Winograd): 3x3, 32 < cin <= 64, fp16 form"""
    return _ws16 and (kh, kw) == (3, 3) and 32 < x.shape[1] <= 64 and ops.f16 is not None


def _split_entry(x, ops, kh, kw, x2=None, res_pre=False, post=None):
    """Which kernel of the split family takes a convolution whose geometry the family covers: "wino16" / "ws16" (one input, the
    residual after the activation, no post-op), else the tile kernel "split"."""
    if x2 is None and not res_pre and not (post is not None and post[0]) and _ws16_ok(x, ops, kh, kw):
        # Winograd: 32-bit byte offsets over 64 output planes; larger frames take the direct kernel
        return "wino16" if _wino and ops.wino is not None and x.shape[2] * x.shape[3] * 256 < (1 << 32) else "ws16"
    return "split"


def _conv_entry(x, out, residual, kh, kw, ops, x2=None, x3=None, res_pre=False, post=None, stride=1, padding=None, rows=False):
    """THE decision which library entry takes a convolution of x (with x2 / x3 following it channel-wise) under the current
    switches (conv_mode, conv_ws16, conv_wino): "wino16" (ct_conv3x3_wino16_f32), "ws16" (ct_conv3x3_ws16_f32), "split"
    (ct_conv2d_split_f32), "rows" (rows=True: ct_conv2d_split_rows_f32, the only split kernel with a token-rows output), or
    "exact": the caller's float32 kernel (after materialising the concatenation), or whatever it does without the split family.
    ops: the weight's SplitOperands or None; out / residual may be None (not made yet / absent); padding None = "same".
    Reads shapes, strides and addresses only; argument validation stays with the callers."""
    ph, pw = (kh // 2, kw // 2) if padding is None else padding
    if ops is None or not _split_ok(x, out, residual, kh, kw, stride, ph, pw):
        return "exact"
    if x2 is not None:                               # channel offsets of the further inputs in units of 16, aligned like x
        c1 = x.shape[1]
        if c1 % 16 or (x3 is not None and (c1 + x2.shape[1]) % 16) or not all(t is None or _aligned(t) for t in (x2, x3)):
            return "exact"
    return "rows" if rows else _split_entry(x, ops, kh, kw, x2, res_pre, post)


def _tile_weights(ops):
    """(image, w_exp, f16 flag) for the tile kernels: the two-piece fp16 image (default) replaces the three-piece bf16 one"""
    if _ws16 and ops.f16 is not None:
        return ops.f16 + (1,)
    return ops.bf16, 0, 0


# ---- stream-K scratch of the tile kernel ---------------------------------------------------------------------------
_sk_cache = {}                                   # (device index, stream) -> zero-initialised stream-K scratch of ct_conv2d_split_f32


def conv_stream_k_state(device=None):
    """(nonzero flag words, consumers that gave up) of the current stream's stream-K scratch -- both 0 between launches; None
    before the first launch on this stream."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    buf = _sk_cache.get((device.index, torch.cuda.current_stream(device).cuda_stream))
    if buf is None:
        return None
    words = buf[:4096].view(torch.int32)
    return int(words[:1000].ne(0).sum()), int(words[1000])


def _conv_scratch(device):
    """The stream-K scratch of the tile convolution for the current stream (include/ct_hip.h: all zero before its first use, then
    owned by the launches of one stream, which leave its flag words zero again).  None while the stream is being captured and
    no scratch exists for it yet: an allocation made inside a capture belongs to that graph's private pool (its zero fill is a
    node of that graph only), so a later graph on the same capture stream would share memory the allocator may already have
    handed out again -- such launches run without stream-K instead (every workgroup computes whole units, same results)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    need = lib().ct_conv_split_scratch_bytes()      # outside the lock: lib() takes it on first use
    with _lock:
        buf = _sk_cache.get(key)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                return None
            buf = torch.zeros(need, dtype=torch.uint8, device=device)
            _sk_cache[key] = buf
    return buf


def conv_scratch_prepare(device=None, stream=None):
    """Create the stream-K scratch of `stream` (default: the current one) OUTSIDE any capture, e.g. for the stream a
    torch.cuda.graph() block is about to capture on, so that the captured convolutions keep stream-K."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    if stream is None:
        return _conv_scratch(device)
    with torch.cuda.stream(stream):
        return _conv_scratch(device)


# ---- launchers and front doors -----------------------------------------------------------------------------------
def _conv_split(x, split, cout, kh, kw, act, residual, clamp, out, x2=None, x3=None, res_pre=False, post=None, entry=None):
    """Launch a split-family kernel.  split: SplitOperands, or a plain (bf16 pieces, bias) pair; entry: what _conv_entry chose
    ("wino16" / "ws16" / "split"), or None for a caller that vouches for the geometry itself and leaves the kernel to _split_entry."""
    ops = SplitOperands(*split)
    if entry is None:
        entry = _split_entry(x, ops, kh, kw, x2, res_pre, post)
    n, cin1, h, w = x.shape
    cin2 = cin1 + (x2.shape[1] if x2 is not None else 0)
    cin = cin2 + (x3.shape[1] if x3 is not None else 0)
    rs = _nchw_bstride(residual) if residual is not None else 0
    ws, w_exp, f16 = _tile_weights(ops)
    post_op, p1, p2 = (0, None, None) if post is None else post
    if post_op and not f16:
        raise CtHipError("a fused post-op needs the fp16 form of the split kernel")
    if entry != "split":
        fn, (ws, w_exp) = (lib().ct_conv3x3_wino16_f32, ops.wino) if entry == "wino16" else (lib().ct_conv3x3_ws16_f32, ops.f16)
        check(fn(_ptr(x), _ptr(ws), int(w_exp), _ptr(ops.bias), _opt(residual), _ptr(out), n, cin, cout, h, w,
                 _nchw_bstride(x), _nchw_bstride(out), rs, int(act), int(bool(clamp)), _stream()))
        return out
    scratch = _conv_scratch(x.device) if (f16 and _stream_k) else None
    check(lib().ct_conv2d_split_f32(_ptr(x), _opt(x2), cin1, _opt(x3), cin2, _ptr(ws), _ptr(ops.bias), _opt(residual), _ptr(out), n, cin,
                                    cout, h, w, kh, kw, _nchw_bstride(x), _nchw_bstride(x2) if x2 is not None else 0,
                                    _nchw_bstride(x3) if x3 is not None else 0, _nchw_bstride(out), rs, int(act), int(bool(clamp)),
                                    int(bool(res_pre)), f16, int(w_exp), int(post_op), _opt(p1), _opt(p2), _opt(scratch),
                                    scratch.numel() if scratch is not None else 0, _stream()))
    return out


def conv2d(x, wp, bias, cout, ksize, act=0, residual=None, clamp=False, out=None, x2=None, x3=None):
    """Conv2d(ksize, padding=ksize//2) + bias [+ LeakyReLU(0.01)] [+ residual] [clamp 0..1], float32 NCHW.
    x2 / x3: further input tensors whose channels follow x's -- torch.cat([x, x2, x3], 1) without the copy when the split kernel
    takes the convolution (channel counts of x and x + x2 multiples of 16); otherwise the concatenation is materialised here."""
    ops = getattr(wp, "_ct_split", None)
    if x2 is not None:
        if out is None:
            out = torch.empty((x.shape[0], cout, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
        dense = all(t is None or (t.is_cuda and t.dtype == torch.float32 and t[0].is_contiguous()) for t in (x2, x3))
        entry = _conv_entry(x, out, residual, ksize, ksize, ops if dense else None, x2=x2, x3=x3)
        if entry != "exact":
            return _conv_split(x, ops, cout, ksize, ksize, act, residual, clamp, out, x2=x2, x3=x3, entry=entry)
        x = torch.cat([t for t in (x, x2, x3) if t is not None], dim=1)
    if x.is_cuda:
        _check_device(x)
    if not x.is_cuda or x.dtype != torch.float32:
        raise CtHipError("conv2d needs float32 CUDA tensors (no CPU path)")
    n, cin, h, w = x.shape
    if out is None:
        out = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    entry = _conv_entry(x, out, residual, ksize, ksize, ops)
    if entry != "exact":
        return _conv_split(x, ops, cout, ksize, ksize, act, residual, clamp, out, entry=entry)
    rs = _nchw_bstride(residual) if residual is not None else 0
    check(lib().ct_conv2d_f32(_ptr(x), _ptr(wp), _ptr(bias), _opt(residual), _ptr(out), n, cin, cout, h, w, ksize, _nchw_bstride(x),
                              _nchw_bstride(out), rs, int(act), int(bool(clamp)), _stream()))
    return out


def conv2d_rows(x, wp, bias, cout, ksize, act=0, out=None, c0=0, channels=None, raw=None):
    """conv2d whose result is written as token rows: out[n*H + y, x, c0 + co] of a [N*H, W, channels] tensor (the layout the
    streaming attention reads), so the NCHW tensor and its transpose are never made.  Returns None when the split kernel cannot
    take the convolution (exact mode, W % 4): the caller then runs conv2d + the transpose.
    raw = (Conv2d weight, bias or None): with it a 1x1 convolution of 64 input channels takes the streaming float32 kernel
    ct_conv1x1_rows_f32 (csrc/conv1x1_rows.hip) in every convolution mode."""
    n, cin, h, w = x.shape

    def rows_out(out, channels):
        channels = int(channels if channels is not None else (out.shape[2] if out is not None else cout))
        if out is None:
            out = torch.empty((n * h, w, channels), dtype=torch.float32, device=x.device)
        if (out.shape != (n * h, w, channels) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != x.device or
                channels % 4 or c0 % 4 or cout % 4 or c0 + cout > channels):
            raise CtHipError("conv2d_rows: out must be a contiguous float32 [N*H, W, channels] tensor, channels / c0 / cout multiples of 4")
        return out, channels
    # raw 1x1: taken ahead of the dispatch, in every convolution mode (raw itself is not validated here)
    if (raw is not None and ksize == 1 and cin == 64 and cout <= 64 and cout % 4 == 0 and x.is_cuda and x.dtype == torch.float32 and
            x.stride(3) == 1 and x.stride(2) == w and x.stride(1) == h * w and act <= 4):
        _check_device(x)
        out, channels = rows_out(out, channels)
        wt = raw[0].detach().reshape(cout, 64).contiguous().float()
        bs = raw[1].detach().contiguous().float() if raw[1] is not None else torch.zeros(cout, dtype=torch.float32, device=x.device)
        check(lib().ct_conv1x1_rows_f32(_ptr(x), _ptr(wt), _ptr(bs), _ptr(out), n, cin, cout, h, w, _nchw_bstride(x), channels, int(c0),
                                        int(act), _stream()))
        return out
    ops = getattr(wp, "_ct_split", None)
    if not x.is_cuda or x.dtype != torch.float32 or _conv_entry(x, None, None, ksize, ksize, ops, rows=True) != "rows":
        return None
    _check_device(x)
    out, channels = rows_out(out, channels)
    ws, w_exp, f16 = _tile_weights(ops)
    check(lib().ct_conv2d_split_rows_f32(_ptr(x), _ptr(ws), _ptr(ops.bias), _ptr(out), n, cin, cout, h, w, ksize, ksize,
                                         _nchw_bstride(x), channels, int(c0), int(act), f16, int(w_exp), _stream()))
    return out


def space_to_depth2(x):
    """[n, c, h, w] -> [n, 4c, h/2, w/2], channel (2 sy + sx) c + ch = x[:, ch, sy::2, sx::2] (ct_space_to_depth2_f32).
    No cache here (round 4 kept the last image keyed on the tensor's identity and `_version`: inference tensors have no version
    counter, and writers that go through raw pointers -- this library's own out= entries -- do not bump it): a caller whose two
    stride-2 convolutions read one input makes the image once and hands it to both (gconv2d(..., s2d=...))."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or not x[0].is_contiguous():
        raise CtHipError("space_to_depth2 needs a float32 CUDA tensor [n, c, h, w] with dense images (no CPU path)")
    _check_device(x)
    n, c, h, w = x.shape
    out = torch.empty((n, 4 * c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    check(lib().ct_space_to_depth2_f32(_ptr(x), _ptr(out), n, c, h, w, _nchw_bstride(x), _stream()))
    return out


def s2d_ok(x):
    """True when a stride-2 3x3 'same' / 1x1 convolution of x can take the tile kernel over space_to_depth2(x) (fp16 form)"""
    return (_conv_mode == "split" and _ws16 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[2] % 2 == 0 and
            x.shape[3] % 8 == 0 and _aligned(x) and x[0].is_contiguous())


def gconv2d(x, wp, bias, cout, ksize, stride=1, padding=0, act=ACT_NONE, out=None, x2=None, residual=None, addend=None, post=None, s2d=None):
    """s2d: space_to_depth2(x) made by the caller (stride-2 convolutions that share their input); x2: optional second input tensor whose channels follow x's (torch.cat([x, x2], 1) without the copy when the
    split-bf16 kernel takes the convolution; otherwise the concatenation is materialised here).  residual: added to the
    result (act must be ACT_NONE: MBConvBlock's identity skip).  addend: a tensor of the output's shape added BEFORE the
    activation (a pre-computed part of the convolution); split kernel only -- CtHipError otherwise.  post (with addend, fp16 form):
    (1, p1, None) = the activated result times p1; (2, z, h) = (1 - z) * h + z * result -- the GRU's two elementwise steps."""
    kh, kw = (ksize, ksize) if isinstance(ksize, int) else ksize
    pad = (padding, padding) if isinstance(padding, int) else padding
    if residual is not None and (act != ACT_NONE or x2 is not None or addend is not None):
        raise CtHipError("gconv2d: a residual needs act=ACT_NONE, a single input and no addend")
    ops = getattr(wp, "_ct_split", None) if bias is not None else None     # every split kernel adds its (padded) bias
    if addend is not None:
        if out is None:
            out = torch.empty((x.shape[0], cout, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
        entry = "exact"
        if addend.shape == out.shape and addend.dtype == torch.float32:
            entry = _conv_entry(x, out, addend, kh, kw, ops, x2=x2, res_pre=True, post=post, stride=stride, padding=pad)
        if entry == "exact":
            raise CtHipError("gconv2d: an addend needs the split kernel (conv mode 'split', stride 1, 'same' padding, W % 4 == 0)")
        if post is not None:
            if not _ws16 or any(t is not None and (t.shape != out.shape or not t.is_contiguous() or t.dtype != torch.float32) for t in post[1:]):
                raise CtHipError("gconv2d: post-op operands must be contiguous float32 tensors of the output's shape (fp16 form only)")
            if not out.is_contiguous():
                raise CtHipError("gconv2d: a post-op needs a contiguous output")
        return _conv_split(x, ops, cout, kh, kw, act, addend, False, out, x2=x2, res_pre=True, post=post, entry=entry)
    if x2 is not None:
        # no out yet: a fresh one is aligned like a fresh x
        entry = _conv_entry(x, out if out is not None else x, None, kh, kw, ops, x2=x2, stride=stride, padding=pad)
        if entry != "exact":
            if out is None:
                out = torch.empty((x.shape[0], cout, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
            return _conv_split(x, ops, cout, kh, kw, act, None, False, out, x2=x2, entry=entry)
        x = torch.cat([x, x2], dim=1)
    n, cin, h, w = x.shape
    ho, wo = (h + 2 * pad[0] - kh) // stride + 1, (w + 2 * pad[1] - kw) // stride + 1
    if out is None:
        out = torch.empty((n, cout, ho, wo), dtype=torch.float32, device=x.device)
    # stride 2, 3x3 "same" or 1x1: the MFMA tile kernel over the space-to-depth image of x (fp16 form)
    geom = (kh, kw, pad[0], pad[1])
    if (stride == 2 and ops is not None and residual is None and cout > 4 and s2d_ok(x) and _aligned(out) and
            ((geom == (3, 3, 1, 1) and hasattr(wp, "_ct_src")) or geom == (1, 1, 0, 0))):
        if s2d is None:
            s2d = space_to_depth2(x)
        elif s2d.shape != (n, 4 * cin, h // 2, w // 2) or s2d.dtype != torch.float32 or not s2d.is_contiguous():
            raise CtHipError("gconv2d: s2d must be space_to_depth2(x)")
        if kh == 1:
            return _conv_split(s2d[:, :cin], ops, cout, 1, 1, act, None, False, out, entry="split")
        return _conv_split(s2d, _split_s2d(wp), cout, 2, 2, act, None, False, out, entry="split")
    # cout <= 4 (the flow head's 256 -> 2): ct_gconv2d_f32's direct kernel instead of a 64-output-channel tile
    entry = _conv_entry(x, out, residual, kh, kw, ops if (cout > 4 or residual is not None) else None, stride=stride, padding=pad)
    if entry != "exact":
        return _conv_split(x, ops, cout, kh, kw, act, residual, False, out, entry=entry)
    check(lib().ct_gconv2d_f32(_ptr(x), _ptr(wp), _opt(bias), _ptr(out), n, cin, cout, h, w, kh, kw, stride, pad[0], pad[1],
                               _nchw_bstride(x), _nchw_bstride(out), int(act), _stream()))
    if residual is not None:
        return eltwise(0, out, residual)
    return out

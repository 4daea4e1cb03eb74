"""Reinhard / MK / Xiao: Lab and RGB statistics, the affine maps, the fused and persistent Reinhard entries, the Lab mode."""
import ctypes

import numpy as np
import torch

from ._core import (CT_LAB_STATS_STRIDE, CT_RGB_STATS_STRIDE, CT_WS_LAB_STATS, CT_WS_MK_U8, CT_WS_REINHARD, CT_WS_REINHARD_PERSIST,
                    CT_WS_REINHARD_PSNR, CT_WS_RGB_MEANCOV, CtHipError, SIGNATURES, _as_batch, _c_i64, _c_int, _c_p,
                    _c_sz, _ptr, _require_cuda, _stream, _suffix, _upload_small, check, lib, workspace)
from ._u8 import _u8_metric

SIGNATURES.update({
    "ct_profile_events": (None, [_c_p, _c_p, _c_p, _c_p]),
    "ct_set_lab_mode": (_c_int, [_c_int]),
    "ct_get_lab_mode": (_c_int, []),
    "ct_set_lab_mode_thread": (_c_int, [_c_int]),
    "ct_set_reinhard_pipeline": (_c_int, [_c_int, _c_int]),
    "ct_set_reinhard_pipeline_thread": (_c_int, [_c_int, _c_int]),
    "ct_get_reinhard_pipeline": (_c_int, [_c_p, _c_p]),
    "ct_reinhard_pipeline_chunk": (_c_int, [_c_i64, _c_int]),
    "ct_lab_stats_f32": (_c_int, [_c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_lab_stats_f64": (_c_int, [_c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_reinhard_apply_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_reinhard_apply_f64": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_reinhard_lab_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_reinhard_f32": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_reinhard_f64": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_reinhard_psnr_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_reinhard_persist_supported": (_c_int, [_c_i64]),
    "ct_reinhard_takes_persist": (_c_int, [_c_i64]),
    "ct_reinhard_persist_f32": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_reinhard_psnr_u8": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_rgb_meancov_f32": (_c_int, [_c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_rgb_meancov_f64": (_c_int, [_c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_mk_f32_f32": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_int, _c_p, _c_sz, _c_p]),
    "ct_mk_f32_f64": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_int, _c_p, _c_sz, _c_p]),
    "ct_mk_f64_f64": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_int, _c_p, _c_sz, _c_p]),
    "ct_mk_coef_f64": (_c_int, [_c_p, _c_p, _c_int, _c_int, _c_p, _c_p]),
    "ct_affine3x3_f32_f64": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_affine3x3_f64_f64": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_affine3x3_f32_f32": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_rgb_meancov_u8": (_c_int, [_c_p, _c_i64, _c_int, _c_p, _c_p, _c_sz, _c_p]),
    "ct_affine3x3_u8_f32": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_affine3x3_u8_u8": (_c_int, [_c_p, _c_p, _c_p, _c_i64, _c_int, _c_p]),
    "ct_mk_u8": (_c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_int, _c_int, _c_p, _c_sz, _c_p]),
})

CT_LAB_TABLE, CT_LAB_EXACT = 0, 1


def set_lab_mode(mode, thread=False):
    """Lab arithmetic of the float32 Reinhard entries: "table" (default; LDS look-up tables, Lab within ~5e-7 of the
    float64 path) or "exact" (float64 with hardware seeds).  Process-wide default (ct_set_lab_mode), or -- thread=True -- an
    override for the calling thread only (ct_set_lab_mode_thread; mode None removes it)."""
    if thread and mode is None:
        check(lib().ct_set_lab_mode_thread(-1))
        return
    code = {"table": CT_LAB_TABLE, "exact": CT_LAB_EXACT}.get(mode)
    if code is None:
        raise ValueError("lab mode must be 'table' or 'exact', got %r" % (mode,))
    check(lib().ct_set_lab_mode_thread(code) if thread else lib().ct_set_lab_mode(code))


def lab_mode():
    return "exact" if lib().ct_get_lab_mode() == CT_LAB_EXACT else "table"


CT_PIPE_T_NT, CT_PIPE_T_PLAIN = 0, 1


def set_reinhard_pipeline(chunk_pairs, t_policy=-1, thread=False):
    """The float32 Reinhard sweeps over chunks of pairs on the caller's stream and a library-owned one (include/ct_hip.h: ct_set_reinhard_pipeline).
    chunk_pairs: -1 the built-in plan, 0 off, > 0 forced at any frame size and batch; t_policy: "nt" / "plain" (or the codes; -1 =
    the built-in choice) for the target tiles of a chunk's statistics sweep.  Process-wide, or -- thread=True -- for the calling
    thread only (chunk_pairs None removes that override)."""
    if thread and chunk_pairs is None:
        check(lib().ct_set_reinhard_pipeline_thread(-2, -1))
        return
    code = {"nt": CT_PIPE_T_NT, "plain": CT_PIPE_T_PLAIN}.get(t_policy, t_policy)
    if code not in (-1, CT_PIPE_T_NT, CT_PIPE_T_PLAIN):
        raise ValueError("target-load policy must be 'nt', 'plain' or -1, got %r" % (t_policy,))
    fn = lib().ct_set_reinhard_pipeline_thread if thread else lib().ct_set_reinhard_pipeline
    check(fn(int(chunk_pairs), code))


def reinhard_pipeline():
    """(chunk_pairs, t_policy code) the calling thread's next reinhard() / reinhard_psnr() call reads"""
    c, p = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().ct_get_reinhard_pipeline(ctypes.byref(c), ctypes.byref(p)))
    return c.value, p.value


def reinhard_pipeline_chunk(n_pixels, batch):
    """Pairs per chunk the current setting gives float32 frames of n_pixels in a call of `batch` pairs (0 = the whole-batch launches)"""
    return int(lib().ct_reinhard_pipeline_chunk(int(n_pixels), int(batch)))


def profile_events(events):
    """events: None (off) or four torch.cuda.Event(enable_timing=True) that have been recorded once (so that their
    hipEvent_t exists); the library re-records them around moments_kernel / reinhard_apply_kernel."""
    if events is None:
        lib().ct_profile_events(None, None, None, None)
    else:
        lib().ct_profile_events(*[ctypes.c_void_p(e.cuda_event) for e in events])


def lab_stats(img):
    """rgb2lab + mean/std (population) per image: returns float64 [B, 8] = mean[3], std[3], n, 0.
    Replaces methods/linear.py:25-26,33-36."""
    x, _ = _as_batch(img)
    _require_cuda(x)
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    stats = torch.empty((B, CT_LAB_STATS_STRIDE), dtype=torch.float64, device=x.device)
    ws = workspace(CT_WS_LAB_STATS, n, B, x.device)
    fn = getattr(lib(), "ct_lab_stats_" + _suffix(x))
    check(fn(_ptr(x), n, B, _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return stats


def _suffix_u8(t):
    """_suffix for the entries that also read or write bytes (rgb_meancov, affine3x3)"""
    return "u8" if t.dtype == torch.uint8 else _suffix(t)


def rgb_meancov(img):
    """np.mean + np.cov (ddof 1) per image: float64 [B, 16] = mean[3], cov[9], n, 0,0,0.
    Replaces methods/linear.py:64-67,103-106.  A uint8 image stands for k / 255; its record comes from exact integer sums
    (ct_rgb_meancov_u8: independent of the summation order and of the batch, exactly 0 for a constant frame)."""
    x, _ = _as_batch(img)
    _require_cuda(x)
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    stats = torch.empty((B, CT_RGB_STATS_STRIDE), dtype=torch.float64, device=x.device)
    ws = workspace(CT_WS_RGB_MEANCOV, n, B, x.device)
    fn = getattr(lib(), "ct_rgb_meancov_" + _suffix_u8(x))
    check(fn(_ptr(x), n, B, _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    return stats


def reinhard_apply(target, stats_t, stats_r, out=None, to_lab=False):
    """Affine map in Lab + lab2rgb (methods/linear.py:38-40); stats stay on the device."""
    x, _ = _as_batch(target)
    _require_cuda(x, stats_t, stats_r)
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    if out is None:
        out = torch.empty_like(x)
    if to_lab:
        if x.dtype != torch.float32:
            raise CtHipError("the Lab probe exists for float32 only")
        fn = lib().ct_reinhard_lab_f32
    else:
        fn = getattr(lib(), "ct_reinhard_apply_" + _suffix(x))
    check(fn(_ptr(x), _ptr(stats_t), _ptr(stats_r), _ptr(out), n, B, _stream()))
    return out.view(target.shape)


def reinhard(target, reference, out=None, stats_out=None):
    """methods.linear.color_transfer_between_images on device tensors, B pairs per call
    (same H x W for target and reference).  One stats sweep over all 2B images, a finishing
    kernel, one apply sweep; no host synchronisation."""
    x, _ = _as_batch(target)
    r, _ = _as_batch(reference)
    _require_cuda(x, r)
    if x.shape != r.shape or x.dtype != r.dtype:
        raise CtHipError("fused reinhard needs equal shapes/dtypes; use lab_stats + reinhard_apply otherwise")
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    if out is None:
        out = torch.empty_like(x)
    ws = workspace(CT_WS_REINHARD, n, B, x.device)
    fn = getattr(lib(), "ct_reinhard_" + _suffix(x))
    if stats_out is not None:
        _require_cuda(stats_out)
        if stats_out.dtype != torch.float64 or stats_out.numel() < 2 * B * CT_LAB_STATS_STRIDE:
            raise CtHipError("stats_out must be float64 with >= 2*B*8 elements")
    sp = _ptr(stats_out) if stats_out is not None else ctypes.c_void_p(0)
    check(fn(_ptr(x), _ptr(r), _ptr(out), n, B, sp, _ptr(ws), ws.numel(), _stream()))
    return out.view(target.shape)


def reinhard_psnr(target, reference, gt, out=None, psnr_out=None, stats_out=None):
    """color_transfer_between_images for B float32 pairs + the per-frame PSNR of the result against `gt` (same layout as the
    images), as Runner.test_step computes it (methods/__init__.py:30-32).  Returns (out, psnr float64 [B, 2] = mse, PSNR).
    stats_out: float64, >= 2*B*8 elements, receives the Lab records (targets, then references) like reinhard()'s."""
    x, _ = _as_batch(target)
    r, _ = _as_batch(reference)
    g, _ = _as_batch(gt)
    _require_cuda(x, r, g)
    if not (x.shape == r.shape == g.shape) or not (x.dtype == r.dtype == g.dtype == torch.float32):
        raise CtHipError("reinhard_psnr needs three float32 tensors of one shape")
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    if out is None:
        out = torch.empty_like(x)
    if psnr_out is None:
        psnr_out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    if stats_out is not None:
        _require_cuda(stats_out)
        if stats_out.dtype != torch.float64 or stats_out.numel() < 2 * B * CT_LAB_STATS_STRIDE:
            raise CtHipError("stats_out must be float64 with >= 2*B*8 elements")
    sp = _ptr(stats_out) if stats_out is not None else ctypes.c_void_p(0)
    ws = workspace(CT_WS_REINHARD_PSNR, n, B, x.device)
    check(lib().ct_reinhard_psnr_f32(_ptr(x), _ptr(r), _ptr(g), _ptr(out), _ptr(psnr_out), n, B, sp, _ptr(ws), ws.numel(), _stream()))
    return out.view(target.shape), psnr_out


def reinhard_persist_supported(n_pixels):
    """True when frames of n_pixels can take the one-launch Reinhard kernel on this device (csrc/reinhard_persist.hip)."""
    return bool(lib().ct_reinhard_persist_supported(int(n_pixels)))


def reinhard_takes_persist(n_pixels):
    """True when reinhard() / reinhard_psnr() run float32 frames of n_pixels as the persistent launch (current Lab mode)."""
    return bool(lib().ct_reinhard_takes_persist(int(n_pixels)))


def reinhard_persist(target, reference, gt=None, out=None, psnr_out=None, stats_out=None, verify=False):
    """color_transfer_between_images (methods/linear.py:8-42) for B pairs as ONE persistent launch, optionally with the
    per-frame PSNR against `gt`.  float32 frames in [0,1] or uint8 frames (the reference's `.float() / 255`, utils/data.py:84);
    the result is float32.  Returns out, or (out, psnr [B, 2]) with gt.  verify=True synchronises and raises if a workgroup of
    the grid never became resident (results NaN)."""
    x, _ = _as_batch(target)
    r, _ = _as_batch(reference)
    ts = [x, r]
    g = None
    if gt is not None:
        g, _ = _as_batch(gt)
        ts.append(g)
    _require_cuda(*ts)
    if any(t.shape != x.shape or t.dtype != x.dtype for t in ts) or x.dtype not in (torch.float32, torch.uint8):
        raise CtHipError("reinhard_persist needs float32 or uint8 tensors of one shape")
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    if not reinhard_persist_supported(n):
        raise CtHipError("frames of %d pixels do not fit the persistent Reinhard launch on this device" % n)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if g is not None and psnr_out is None:
        psnr_out = torch.empty((B, 2), dtype=torch.float64, device=x.device)
    if stats_out is not None:
        _require_cuda(stats_out)
        if stats_out.dtype != torch.float64 or stats_out.numel() < 2 * B * CT_LAB_STATS_STRIDE:
            raise CtHipError("stats_out must be float64 with >= 2*B*8 elements")
    ws = workspace(CT_WS_REINHARD_PERSIST, n, B, x.device)
    null = ctypes.c_void_p(0)
    if x.dtype == torch.uint8:
        fn = lib().ct_reinhard_psnr_u8
    else:
        fn = lib().ct_reinhard_persist_f32
    check(fn(_ptr(x), _ptr(r), _ptr(g) if g is not None else null, _ptr(out), _ptr(psnr_out) if g is not None else null, n, B,
                          _ptr(stats_out) if stats_out is not None else null, _ptr(ws), ws.numel(), _stream()))
    if verify:
        torch.cuda.synchronize()
        if int(ws[:4].view(torch.int32)[0].item()) != 0:
            raise CtHipError("persistent Reinhard launch: a workgroup of the grid never became resident (results are NaN)")
    o = out.view(tuple(target.shape))
    return (o, psnr_out) if g is not None else o


def _check_out(out, x, family):
    """An `out` the caller passes is written as x.numel() elements from its first one: anything else is an error here, not an
    out-of-bounds store.  Returns the entry's name."""
    if out.device != x.device:
        raise CtHipError("out is on %s, the input on %s" % (out.device, x.device))
    if not out.is_contiguous():
        raise CtHipError("out must be contiguous")
    if out.numel() != x.numel():
        raise CtHipError("out has %d elements, the input %d" % (out.numel(), x.numel()))
    name = "ct_%s_%s_%s" % (family, _suffix_u8(x), _suffix_u8(out))
    if name not in SIGNATURES:
        raise CtHipError("no kernel for %s" % name)
    return name


def _check_records(t, batch, what):
    """float64 [>= batch, 16] records (rgb_meancov statistics, affine3x3 coefficients), contiguous, on the current device"""
    _require_cuda(t)
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != CT_RGB_STATS_STRIDE or t.shape[0] < batch:
        raise CtHipError("%s must be float64 [B >= %d, %d], got %s %s" % (what, batch, CT_RGB_STATS_STRIDE, t.dtype, tuple(t.shape)))


def mk(target, reference, decomposition="MK", out_dtype=None, out=None, gt=None, psnr_out=None):
    """methods.linear.monge_kantorovitch_color_transfer on device tensors, B pairs per call, no host sync (ct_mk_*).
    out_dtype: float64 by default.  uint8 frames (the image is k / 255; ct_mk_u8): out_dtype float32 (default, unclipped) or uint8
    (ct_hip.pack_u8's rule on the float32 result); with gt (uint8 frames of the same shape) the call also fills psnr_out, float64
    [B, 2] = (mse, PSNR) of the clamped float32 result, and returns (out, psnr_out), like reinhard_persist."""
    x, _ = _as_batch(target)
    r, _ = _as_batch(reference)
    _require_cuda(x, r)
    if x.shape != r.shape or x.dtype != r.dtype:
        raise CtHipError("fused mk needs equal shapes/dtypes")
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    mode = {"MK": 0, "sqrt": 1, "cholesky": 2}[decomposition]
    if x.dtype == torch.uint8:
        return _mk_u8(target, x, r, B, n, mode, out_dtype, out, gt, psnr_out)
    if gt is not None or psnr_out is not None:
        raise CtHipError("mk computes the PSNR for uint8 frames only (gt / psnr_out with %s frames)" % x.dtype)
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or torch.float64, device=x.device)
    name = _check_out(out, x, "mk")
    ws = workspace(CT_WS_REINHARD, n, B, x.device)
    check(getattr(lib(), name)(_ptr(x), _ptr(r), _ptr(out), n, B, mode, _ptr(ws), ws.numel(), _stream()))
    return out.view(target.shape)


def _mk_u8(target, x, r, B, n, mode, out_dtype, out, gt, psnr_out):
    """mk() for uint8 frames: every argument error is raised here, before the C call"""
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or torch.float32, device=x.device)
    _require_cuda(out)
    if out.device != x.device:
        raise CtHipError("out is on %s, the input on %s" % (out.device, x.device))
    if out.numel() != x.numel():
        raise CtHipError("out has %d elements, the input %d" % (out.numel(), x.numel()))
    if out.dtype not in (torch.float32, torch.uint8):
        raise CtHipError("mk on uint8 frames writes float32 or uint8, not %s" % out.dtype)
    null = ctypes.c_void_p(0)
    g, psnr_out = _u8_metric(x, gt, psnr_out, "mk")
    ws = workspace(CT_WS_MK_U8, n, B, x.device)
    f32, u8 = (_ptr(out), null) if out.dtype == torch.float32 else (null, _ptr(out))
    check(lib().ct_mk_u8(_ptr(x), _ptr(r), _ptr(g) if g is not None else null, f32, u8, _ptr(psnr_out) if g is not None else null,
                         n, B, mode, _ptr(ws), ws.numel(), _stream()))
    o = out.view(tuple(target.shape))
    return (o, psnr_out) if g is not None else o


def upload_records(records, device):
    """Host float64 [B, 16] records (affine3x3 coefficients made on the host) -> a device tensor without a blocking copy: through
    the binding's ring of pinned slots, asynchronously on the current stream."""
    records = np.ascontiguousarray(records, dtype=np.float64)
    if records.ndim != 2 or records.shape[1] != CT_RGB_STATS_STRIDE:
        raise CtHipError("records must be [B, %d], got %s" % (CT_RGB_STATS_STRIDE, records.shape))
    return _upload_small(records, device)


def mk_coef(stats_t, stats_r, decomposition="MK"):
    """On-device 3x3 algebra of MK (methods/linear.py:108-118): rgb_meancov records -> affine3x3 coefficient records."""
    mode = {"MK": 0, "sqrt": 1, "cholesky": 2}[decomposition]
    _check_records(stats_t, 0, "stats_t")
    b = stats_t.shape[0]
    _check_records(stats_r, b, "stats_r")
    if stats_r.shape[0] != b:
        raise CtHipError("stats_t holds %d records, stats_r %d" % (b, stats_r.shape[0]))
    coef = torch.empty((b, 16), dtype=torch.float64, device=stats_t.device)
    check(lib().ct_mk_coef_f64(_ptr(stats_t), _ptr(stats_r), mode, b, _ptr(coef), _stream()))
    return coef


def affine3x3(img, coef, out_dtype=None, out=None):
    """out = (x - mu_t) @ A + mu_r per image; coef float64 [B,16] = A[9], mu_t[3], mu_r[3], 0.
    Replaces methods/linear.py:80,122.  out_dtype: float64 by default; for a uint8 image (x = k / 255) float32 (default) or
    uint8 (ct_hip.pack_u8's rule on the float32 result)."""
    x, _ = _as_batch(img)
    _require_cuda(x)
    B, n = x.shape[0], x.shape[1] * x.shape[2]
    _check_records(coef, B, "coef")
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or (torch.float32 if x.dtype == torch.uint8 else torch.float64), device=x.device)
    name = _check_out(out, x, "affine3x3")
    check(getattr(lib(), name)(_ptr(x), _ptr(coef), _ptr(out), n, B, _stream()))
    return out.view(img.shape)

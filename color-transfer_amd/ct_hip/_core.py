"""Library loading and what every kernel-family module of the binding shares: the signature table, the ctypes shorthands,
the pointer / stream / argument-check helpers, the workspace and upload caches.

PyTorch is used here only as the device allocator / stream provider: every function
takes CUDA (= HIP on ROCm) tensors, passes raw device pointers and the current HIP stream
to the library and returns without synchronising.

There is NO CPU fallback: importing works anywhere (so that `-m "not gpu"` tests can
check the exported symbols), but the first compute call without the library or without a
GPU raises.
"""
import ctypes
import os
import threading
from typing import NamedTuple

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CT_HIP_LIB") or os.path.join(_HERE, "libct_hip.so")   # CT_HIP_LIB: tuning builds only

CT_ABI_VERSION = 9            # include/ct_hip.h: CT_ABI_VERSION; lib() refuses any other library
CT_LAB_STATS_STRIDE = 8
CT_RGB_STATS_STRIDE = 16
CT_WS_LAB_STATS, CT_WS_RGB_MEANCOV, CT_WS_REINHARD, CT_WS_IDT, CT_WS_REINHARD_PSNR, CT_WS_REINHARD_PERSIST = 0, 1, 2, 3, 4, 5
CT_WS_MK_U8 = 6

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_p = ctypes.c_void_p
_c_sz = ctypes.c_size_t
_c_ll = ctypes.c_longlong
_c_f = ctypes.c_float

ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_SWISH, ACT_GELU = 0, 1, 2, 3, 4, 5, 6

# name -> (restype, argtypes); ONE table, filled by every module of the package as it is imported (ct_hip/__init__.py imports
# them all before anything can call lib()), so tests can check it against include/ct_hip.h
SIGNATURES = {
    "ct_abi_version": (_c_int, []),
    "ct_error_string": (ctypes.c_char_p, [_c_int]),
    "ct_workspace_bytes": (_c_sz, [_c_int, _c_i64, _c_int]),
    "ct_device_status": (_c_int, [_c_int]),
}

_lib = None
_lock = threading.RLock()          # re-entrant: lib() takes it on first use, possibly under a caller that already holds it


class CtHipError(RuntimeError):
    pass


def lib():
    """Load libct_hip.so (once). Raises loudly when it is missing -- there is no fallback."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise CtHipError(
                        "HIP library %s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C color-transfer_amd/csrc`; this package has no CPU fallback" % LIB_PATH)
                handle = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(handle, name)  # AttributeError = ABI mismatch, also loud
                    fn.restype = res
                    fn.argtypes = args
                got = handle.ct_abi_version()
                if got != CT_ABI_VERSION:            # a stale build (or CT_HIP_LIB) would misread every changed argument list
                    raise CtHipError("%s reports ABI version %d, this binding needs %d: rebuild with `make -C color-transfer_amd/csrc`"
                                     % (LIB_PATH, got, CT_ABI_VERSION))
                _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise CtHipError("libct_hip: %s (code %d)" % (lib().ct_error_string(rc).decode(), rc))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_device(t):
    """Kernels launch on the CURRENT device's stream: a tensor that lives elsewhere would be touched from the wrong
    context.  One process drives one GPU here, so this is an error, not a device switch."""
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise CtHipError("tensor on %s but the current device is cuda:%d; call torch.cuda.set_device(%d) first"
                         % (t.device, torch.cuda.current_device(), t.device.index))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _require_cuda(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise CtHipError("ct_hip needs device tensors (got %s); no CPU path exists" % t.device)
        if not t.is_contiguous():
            raise CtHipError("ct_hip needs contiguous HWC tensors")
        _check_device(t)


_ws_cache = {}


def workspace(kind, n_pixels, n_images, device, need=None):
    """Per-(device, stream) scratch buffer, grown on demand (never shrinks)."""
    if need is None:
        need = lib().ct_workspace_bytes(kind, n_pixels, n_images)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _lock:
        buf = _ws_cache.get(key)
        if buf is None or buf.numel() < need:
            buf = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=device)
            _ws_cache[key] = buf
    return buf


_upload_rings = {}                               # device index -> [pinned uint8 [slots, bytes], events, next slot]
_UPLOAD_SLOTS, _UPLOAD_BYTES = 32, 1 << 14


def _upload_small(arr, device):
    """A small host array -> device tensor WITHOUT a blocking copy: staged through a ring of pinned slots and copied
    asynchronously on the current stream (a pageable `.to(device)` is a synchronous hipMemcpy: it would drain the stream on
    every call and serialise the host with the GPU)."""
    arr = np.ascontiguousarray(arr)
    if arr.nbytes > _UPLOAD_BYTES:
        return torch.from_numpy(arr).to(device)
    with _lock:
        ring = _upload_rings.get(device.index)
        if ring is None:
            ring = [torch.empty((_UPLOAD_SLOTS, _UPLOAD_BYTES), dtype=torch.uint8).pin_memory(), [None] * _UPLOAD_SLOTS, 0]
            _upload_rings[device.index] = ring
        slot = ring[2]
        ring[2] = (slot + 1) % _UPLOAD_SLOTS
    if ring[1][slot] is not None:
        ring[1][slot].synchronize()                # the copy that last used this slot (32 calls ago) has long finished
    host = ring[0][slot, :arr.nbytes].view(torch.from_numpy(arr).dtype).view(arr.shape)
    host.copy_(torch.from_numpy(arr))
    dev = torch.empty(arr.shape, dtype=host.dtype, device=device)
    dev.copy_(host, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    ring[1][slot] = ev
    return dev


def _as_batch(img):
    """[H,W,3] or [B,H,W,3] -> ([B,H,W,3] view, had_batch_dim)."""
    if img.dim() == 3:
        return img.unsqueeze(0), False
    if img.dim() == 4:
        return img, True
    raise CtHipError("expected [H,W,3] or [B,H,W,3], got %s" % (tuple(img.shape),))


def _suffix(t):
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == torch.float64:
        return "f64"
    raise CtHipError("unsupported dtype %s (float32/float64 only)" % t.dtype)


def device_status(clear=False, sync=True):
    """Sticky status bits of the current device (include/ct_hip.h: ct_device_status): 0 = all well; bit 0 = a persistent Reinhard
    launch gave up a bounded spin (its frames and PSNR records are NaN), bit 1 = a stream-K convolution gave up.  For loops that
    never synchronise per call: check once at the end (utils/sharding.gather_frame_metrics does)."""
    if sync:
        torch.cuda.synchronize()
    v = lib().ct_device_status(1 if clear else 0)
    if v < 0:
        raise CtHipError("ct_device_status: the device could not be read")
    return v


def _f32c(*ts):
    for t in ts:
        if t is None:
            continue
        if t.is_cuda:
            _check_device(t)
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise CtHipError("needs contiguous float32 CUDA tensors (no CPU path)")


def _opt(t):
    return _ptr(t) if t is not None else _c_p(0)


def _nchw_bstride(t):
    n, c, h, w = t.shape
    if t.stride(3) != 1 or t.stride(2) != w or t.stride(1) != h * w:
        raise CtHipError("conv2d needs NCHW tensors with dense planes (channel slices are fine)")
    return t.stride(0)


class Packed(NamedTuple):
    """a packed operand cached on the tensor it was made from, with the state of that tensor it is valid for"""
    version: tuple
    operand: object


def _cached_pack(owner, attr, version, pack):
    """owner.<attr>.operand, re-made by pack() when the cached one is missing or belongs to another `version`"""
    hit = getattr(owner, attr, None)
    if hit is None or hit.version != version:
        hit = Packed(version, pack())
        setattr(owner, attr, hit)
    return hit.operand

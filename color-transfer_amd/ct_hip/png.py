"""PNG serialisation on the device: filtered rows -> deflate streams (csrc/png.hip), and back: zlib streams -> filtered rows -> planar
frames (csrc/png_decode.hip).  The container around them is utils/png.py."""
import numpy as np
import torch

from ._core import CtHipError, SIGNATURES, _c_int, _c_ll, _c_p, _ptr, _require_cuda, _stream, check as _check_rc, lib

SIGNATURES.update({
    "ct_png_slot_capacity": (_c_ll, [_c_int, _c_int, _c_int]),
    "ct_png_deflate_u8": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_ll, _c_p, _c_p, _c_p]),
    "ct_png_inflate_u8": (_c_int, [_c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "ct_png_unfilter_u8": (_c_int, [_c_p, _c_p, _c_p, _c_int, _c_p, _c_p, _c_p, _c_p]),
})

PNG_ROWS_PER_CHUNK = 16
PNG_MAX_WIDTH = 8192                    # include/ct_hip.h: CT_PNG_MAX_WIDTH
# include/ct_hip.h: CT_INFLATE_*
INFLATE_STATUS = ("ok", "bad zlib header", "reserved block type", "stored block: LEN != ~NLEN", "code lengths over-subscribed",
                  "code lengths incomplete", "repeat symbol without a previous length or past HLIT + HDIST", "invalid symbol",
                  "distance beyond the start of the output", "input exhausted", "output larger than its slot",
                  "output smaller than expected", "Adler-32 mismatch", "filter type above 4", "sizes do not fit the dimensions")


def png_geometry(height, width, rows_per_chunk=PNG_ROWS_PER_CHUNK):
    """(chunks per frame, capacity of a chunk's slot in bytes) of png_deflate for frames of height x width.  The capacity is
    F + 5 ceil(F / 65535) + 5 with F = min(rows_per_chunk, height) * (3 width + 1): what the chunk takes as stored blocks plus an
    empty one; no chunk is larger.  Pure Python: no GPU, no library."""
    for name, v in (("height", height), ("width", width), ("rows_per_chunk", rows_per_chunk)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise CtHipError("png_geometry: %s must be a positive int (got %r)" % (name, v))
    rows = min(rows_per_chunk, height)
    filtered = rows * (3 * width + 1)
    return (height + rows - 1) // rows, filtered + 5 * ((filtered + 65534) // 65535) + 5


def png_deflate(frames_u8, rows_per_chunk=PNG_ROWS_PER_CHUNK, out=None):
    """uint8 [n,H,W,3] device frames -> (streams, sizes, adler): every frame cut into chunks of rows_per_chunk rows, every chunk
    PNG-filtered (one filter per row, minimum sum of absolute values) and deflated with a Huffman code of its own, or stored when
    that is not smaller (ct_png_deflate_u8).  streams: uint8 [n, chunks, capacity], chunk c of frame f is streams[f, c, :sizes[f, c]];
    sizes: int32 [n, chunks]; adler: int32 [n, chunks, 2], the Adler-32 halves (s1, s2, both below 65521) of each chunk's filtered
    bytes.  utils.png.assemble makes the file from them.
    out: an optional (streams, sizes, adler) triple of preallocated tensors of these shapes on the same device (uint8, int32, int32).
    The bytes of a frame depend on that frame alone.  Asynchronous on the current stream; nothing is allocated with out."""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise CtHipError("png_deflate needs a uint8 [n,H,W,3] tensor")
    _require_cuda(frames_u8)
    if frames_u8.dtype != torch.uint8:
        raise CtHipError("png_deflate needs uint8 frames (got %s)" % frames_u8.dtype)
    if isinstance(rows_per_chunk, bool) or not isinstance(rows_per_chunk, int) or rows_per_chunk < 1:
        raise CtHipError("png_deflate: rows_per_chunk must be a positive int (got %r)" % (rows_per_chunk,))
    n, h, w, _ = frames_u8.shape
    if not frames_u8.numel():
        raise CtHipError("png_deflate: empty tensor of shape %s" % (tuple(frames_u8.shape),))
    chunks, cap = png_geometry(h, w, rows_per_chunk)
    shapes = ((n, chunks, cap), (n, chunks), (n, chunks, 2))
    dtypes = (torch.uint8, torch.int32, torch.int32)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=frames_u8.device) for s, d in zip(shapes, dtypes))
    else:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise CtHipError("png_deflate: out must be a (streams, sizes, adler) triple")
        for t, s, d, name in zip(out, shapes, dtypes, ("streams", "sizes", "adler")):
            if not isinstance(t, torch.Tensor) or t.dtype != d or t.device != frames_u8.device or tuple(t.shape) != s:
                raise CtHipError("png_deflate: out's %s must be a %s %s tensor on %s" % (name, d, list(s), frames_u8.device))
            _require_cuda(t)
    streams, sizes, adler = out
    _check_rc(lib().ct_png_deflate_u8(_ptr(frames_u8), n, h, w, rows_per_chunk, _ptr(streams), cap, _ptr(sizes), _ptr(adler), _stream()))
    return streams, sizes, adler


def _status_name(code):
    return INFLATE_STATUS[code] if 0 <= code < len(INFLATE_STATUS) else "status %d" % code


def _raise_on_status(what, status):
    """one synchronisation: the status of every stream read back; the first that is not 0 raises"""
    codes = status.cpu().tolist()
    for i, code in enumerate(codes):
        if code:
            raise CtHipError("%s: stream %d: %s (status %d)" % (what, i, _status_name(code), code))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def _upload_bytes(parts, device):
    """host byte strings / 1-D uint8 host tensors -> one device uint8 tensor, through one pinned buffer and one copy"""
    total = sum(len(p) for p in parts)
    host = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
    view, at = host.numpy(), 0
    for p in parts:
        n = len(p)
        view[at:at + n] = p.numpy() if isinstance(p, torch.Tensor) else np.frombuffer(p, dtype=np.uint8)
        at += n
    return host.to(device, non_blocking=True)          # the pinned block is not reused before the copy has been made (torch's host allocator)


def _gather_streams(what, streams):
    """-> (device uint8 buffer, int64 host offsets [n + 1] or device offsets tensor, n)"""
    if isinstance(streams, tuple) and len(streams) == 2 and isinstance(streams[0], torch.Tensor):
        buf, offsets = streams
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
            raise CtHipError("%s: the offsets of a device buffer are an int64 [n + 1] device tensor" % what)
        if buf.dtype != torch.uint8 or buf.dim() != 1:
            raise CtHipError("%s needs a 1-D uint8 buffer (got %s %s)" % (what, buf.dtype, tuple(buf.shape)))
        _require_cuda(buf, offsets)
        return buf, offsets, offsets.numel() - 1
    if not isinstance(streams, (list, tuple)) or not streams:
        raise CtHipError("%s needs a non-empty list of byte strings, or (device uint8 buffer, int64 offsets)" % what)
    if all(isinstance(s, torch.Tensor) for s in streams):
        for s in streams:
            if s.dtype != torch.uint8 or s.dim() != 1:
                raise CtHipError("%s needs 1-D uint8 tensors (got %s %s)" % (what, s.dtype, tuple(s.shape)))
        if all(s.is_cuda for s in streams):
            _require_cuda(*streams)
            return torch.cat(list(streams)), _offsets([s.numel() for s in streams]), len(streams)
        if any(s.is_cuda for s in streams):
            raise CtHipError("%s: streams on the host and on the device in one call" % what)
    elif not all(isinstance(s, (bytes, bytearray, memoryview)) for s in streams):
        raise CtHipError("%s needs byte strings or 1-D uint8 tensors (got %s)" % (what, sorted({type(s).__name__ for s in streams})))
    if not torch.cuda.is_available():
        raise CtHipError("ct_hip needs a GPU: no CPU path exists")
    device = torch.device("cuda", torch.cuda.current_device())
    return _upload_bytes(streams, device), _offsets([len(s) for s in streams]), len(streams)


def _device_i64(arr, device):
    return arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64)).to(device)


def inflate(streams, sizes, check=True, out=None):
    """zlib streams -> their bytes, on the device (ct_png_inflate_u8: one wave per stream).  streams: a list of byte strings (or of
    1-D uint8 tensors, all on the host or all on the device), or (device uint8 buffer, int64 [n + 1] device offsets).  sizes: what
    each stream must inflate to, exactly.  out: an optional 1-D uint8 device buffer of at least sum(sizes) bytes.
    Returns (buffer, status): stream i at buffer[sum(sizes[:i]) : sum(sizes[:i + 1])], status int32 [n] on the device
    (ct_hip.INFLATE_STATUS names the values).  check=True reads the status back (one synchronisation) and raises CtHipError naming
    the first stream that failed; check=False stays asynchronous.  The Adler-32 of every stream is compared on the device."""
    buf, status, _ = _inflate("inflate", streams, sizes, out)
    if check:
        _raise_on_status("inflate", status)
    return buf, status


def _inflate(what, streams, sizes, out=None):
    src, src_off, n = _gather_streams(what, streams)
    sizes = [int(s) for s in sizes]
    if len(sizes) != n or any(s < 0 or s > 0x7fffffff for s in sizes):
        raise CtHipError("%s: %d streams need %d sizes in [0, 2^31) (got %r)" % (what, n, n, sizes[:8]))
    device = src.device
    dst_off_host = _offsets(sizes)
    total = int(dst_off_host[-1])
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < total:
            raise CtHipError("%s: out must be a 1-D uint8 device tensor of at least %d bytes" % (what, total))
        _require_cuda(out)
    src_off = _device_i64(src_off, device)
    dst_off = _device_i64(dst_off_host, device)
    status = torch.empty(n, dtype=torch.int32, device=device)
    adler = torch.empty(n, dtype=torch.int32, device=device)
    _check_rc(lib().ct_png_inflate_u8(_ptr(src), _ptr(src_off), n, _ptr(out), _ptr(dst_off), _ptr(status), _ptr(adler), _stream()))
    return out, status, dst_off


def png_decode(files, check=True):
    """PNG files -> uint8 [3,H,W] device tensors, inflated and unfiltered on the device (ct_png_inflate_u8 + ct_png_unfilter_u8, two
    launches for the whole list).  files: a list whose items are a file's bytes (parsed by utils.png.parse) or (payload, height,
    width) with the zlib payload of the IDAT chunks as bytes or a 1-D uint8 tensor (all on the host or all on the device).  Only
    what utils.png.device_decodable accepts: 8 bits, colour type 2, no interlace, at most PNG_MAX_WIDTH wide.  The results are views
    of one buffer; files of one size come back as the slices of one [n,3,H,W] tensor.
    check=True: one synchronisation, CtHipError naming the first file that failed and why; check=False: (frames, status) with the
    int32 [n] status on the device, asynchronous."""
    if not isinstance(files, (list, tuple)) or not files:
        raise CtHipError("png_decode needs a non-empty list of PNG files (bytes) or (payload, height, width) triples")
    payloads, dims = [], []
    for i, f in enumerate(files):
        if isinstance(f, (bytes, bytearray, memoryview)):
            from utils import png
            try:
                info = png.parse(f)
            except ValueError as e:
                raise CtHipError("png_decode: file %d: %s" % (i, e))
            if not png.device_decodable(info):
                raise CtHipError("png_decode: file %d is %d-bit, colour type %d, interlace %d: only 8-bit RGB without interlace is "
                                 "decoded on the device" % (i, info.bit_depth, info.colour_type, info.interlace))
            f = (info.payload, info.height, info.width)
        if not isinstance(f, (tuple, list)) or len(f) != 3:
            raise CtHipError("png_decode: item %d is neither a file's bytes nor (payload, height, width)" % i)
        h, w = int(f[1]), int(f[2])
        if h < 1 or w < 1 or w > PNG_MAX_WIDTH or h * (1 + 3 * w) > 0x7fffffff:
            raise CtHipError("png_decode: item %d: %d x %d is outside 1 <= width <= %d, height (1 + 3 width) < 2^31" % (i, h, w, PNG_MAX_WIDTH))
        payloads.append(f[0])
        dims.append((h, w))
    filtered, status, filt_off = _inflate("png_decode", payloads, [h * (1 + 3 * w) for h, w in dims])
    device = filtered.device
    n = len(dims)
    out_off_host = _offsets([3 * h * w for h, w in dims])
    meta = np.concatenate([out_off_host, np.asarray(dims, dtype=np.int32).reshape(-1).view(np.int64)])     # one upload: offsets, then (h, w) pairs
    meta_dev = torch.from_numpy(meta).to(device)
    out_off, dims_dev = meta_dev[:n + 1], meta_dev[n + 1:].view(torch.int32)
    out = torch.empty(int(out_off_host[-1]), dtype=torch.uint8, device=device)
    _check_rc(lib().ct_png_unfilter_u8(_ptr(filtered), _ptr(filt_off), _ptr(dims_dev), n, _ptr(out), _ptr(out_off), _ptr(status), _stream()))
    if len(set(dims)) == 1:
        frames = list(out.view(n, 3, dims[0][0], dims[0][1]).unbind(0))
    else:
        frames = [out[int(out_off_host[i]):int(out_off_host[i + 1])].view(3, h, w) for i, (h, w) in enumerate(dims)]
    if check:
        _raise_on_status("png_decode", status)
        return frames
    return frames, status

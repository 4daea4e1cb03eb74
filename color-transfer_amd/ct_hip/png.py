"""PNG serialisation on the device: filtered rows -> deflate streams (csrc/png.hip).  The container around them is utils/png.py."""
import torch

from ._core import CtHipError, SIGNATURES, _c_int, _c_ll, _c_p, _ptr, _require_cuda, _stream, check, lib

SIGNATURES.update({
    "ct_png_slot_capacity": (_c_ll, [_c_int, _c_int, _c_int]),
    "ct_png_deflate_u8": (_c_int, [_c_p, _c_int, _c_int, _c_int, _c_int, _c_p, _c_ll, _c_p, _c_p, _c_p]),
})

PNG_ROWS_PER_CHUNK = 16


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
    check(lib().ct_png_deflate_u8(_ptr(frames_u8), n, h, w, rows_per_chunk, _ptr(streams), cap, _ptr(sizes), _ptr(adler), _stream()))
    return streams, sizes, adler

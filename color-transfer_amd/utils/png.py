"""The host half of a PNG file: the container around deflate streams that were made elsewhere (ct_hip.png_deflate on the device).

A PNG file is a signature and a list of chunks `length, type, data, CRC-32(type + data)` (PNG specification, section 5).  The image
data is ONE zlib stream (RFC 1950: two header bytes, deflate blocks, the Adler-32 of the uncompressed bytes) of the filtered rows.
The device delivers that stream in pieces that each end on a byte boundary and contain no final block, with the Adler-32 of each
piece's own bytes; what is left for the host is arithmetic on a few numbers and one `zlib.crc32` over the compressed bytes (which
releases the GIL, so the writer's threads run it in parallel).  `parse` is the same container read: the chunks checked, the IDAT
payload handed on as it is for ct_hip.png_decode to inflate and unfilter on the device.  Pure Python, `zlib` and `struct` only."""
import struct
import zlib
from collections import namedtuple

ADLER_MOD = 65521
SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x01"               # deflate, 32 KB window, no preset dictionary, fastest level (a hint only); 0x7801 % 31 == 0
FINAL_EMPTY_BLOCK = b"\x01\x00\x00\xff\xff"     # BFINAL = 1, stored, LEN = 0


def adler32_combine(a, b, len_b):
    """Adler-32 of X + Y from a = adler32(X), b = adler32(Y) and len_b = len(Y).  With s1 = 1 + sum(bytes) and s2 = the sum of
    the running s1 (both mod 65521): s1(XY) = s1(X) + s1(Y) - 1, and Y's running sums each start s1(X) - 1 higher than they do
    from the initial value 1, which adds len_b * (s1(X) - 1) to s2."""
    a1, a2 = a & 0xffff, (a >> 16) & 0xffff
    b1, b2 = b & 0xffff, (b >> 16) & 0xffff
    s1 = (a1 + b1 - 1) % ADLER_MOD
    s2 = (a2 + b2 + (len_b % ADLER_MOD) * (a1 - 1)) % ADLER_MOD
    return (s2 << 16) | s1


def png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def assemble(height, width, chunks, adler_parts):
    """An 8-bit RGB PNG file of height x width from the deflate streams of its row chunks.  chunks: the byte strings of one frame in
    order, each a run of non-final deflate blocks that ends on a byte boundary; together they inflate to the height * (1 + 3 width)
    filtered bytes.  adler_parts: per chunk (s1, s2, n_bytes): the Adler-32 halves of the chunk's filtered bytes and their number.
    The file: signature, IHDR (8 bits, colour type 2, no interlace), one IDAT = zlib header + chunks + an empty final block +
    the combined Adler-32, IEND."""
    chunks = list(chunks)
    adler_parts = list(adler_parts)
    if len(chunks) != len(adler_parts):
        raise ValueError("%d chunks but %d Adler-32 parts" % (len(chunks), len(adler_parts)))
    adler, total = 1, 0
    for s1, s2, n_bytes in adler_parts:
        adler = adler32_combine(adler, (int(s2) << 16) | int(s1), int(n_bytes))
        total += int(n_bytes)
    if total != height * (1 + 3 * width):
        raise ValueError("the chunks hold %d filtered bytes, a %d x %d RGB frame has %d" % (total, height, width, height * (1 + 3 * width)))
    idat = b"".join([ZLIB_HEADER] + [bytes(c) for c in chunks] + [FINAL_EMPTY_BLOCK, struct.pack(">I", adler)])
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)
    return SIGNATURE + png_chunk(b"IHDR", ihdr) + png_chunk(b"IDAT", idat) + png_chunk(b"IEND", b"")


def chunk_rows(height, rows_per_chunk):
    """the number of rows of each chunk of a frame: rows_per_chunk (at most the height), the last one what is left"""
    rows = min(int(rows_per_chunk), int(height))
    return [min(rows, height - r) for r in range(0, height, rows)]


PngInfo = namedtuple("PngInfo", "height width bit_depth colour_type interlace payload")


def parse(data):
    """The container of a PNG file: PngInfo(height, width, bit_depth, colour_type, interlace, payload), payload = the data of
    every IDAT chunk concatenated = ONE zlib stream of the filtered rows (not inflated here).  Checked: the signature, every chunk's
    CRC-32, IHDR first, IEND present; a ValueError names what is wrong.  Ancillary chunks are skipped (their CRC is still checked)."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG file: bad signature %r" % data[:8])
    at, first, ihdr, idat, ended = 8, True, None, [], False
    while at < len(data):
        if at + 8 > len(data):
            raise ValueError("truncated PNG file: a chunk header at byte %d of %d" % (at, len(data)))
        length, kind = struct.unpack(">I4s", data[at:at + 8])
        end = at + 12 + length
        if end > len(data):
            raise ValueError("truncated PNG file: chunk %r at byte %d needs %d bytes, %d are left" % (kind, at, 12 + length, len(data) - at))
        body = data[at + 8:at + 8 + length]
        crc, = struct.unpack(">I", data[end - 4:end])
        if zlib.crc32(body, zlib.crc32(kind)) != crc:
            raise ValueError("chunk %r at byte %d: CRC-32 mismatch" % (kind, at))
        if first and kind != b"IHDR":
            raise ValueError("the first chunk is %r, not IHDR" % kind)
        first = False
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise ValueError("a second IHDR chunk" if ihdr is not None else "IHDR of %d bytes, not 13" % length)
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        at = end
    if ihdr is None:
        raise ValueError("truncated PNG file: no IHDR chunk")
    if not ended:
        raise ValueError("truncated PNG file: no IEND chunk")
    width, height, depth, colour, _, _, interlace = ihdr
    return PngInfo(height, width, depth, colour, interlace, b"".join(idat))


def device_decodable(info):
    """what ct_hip.png_decode takes: 8 bits per sample, colour type 2 (RGB), not interlaced"""
    return info.bit_depth == 8 and info.colour_type == 2 and info.interlace == 0 and info.height >= 1 and info.width >= 1

"""The host half of a PNG file: the container around deflate streams that were made elsewhere (ct_hip.png_deflate on the device).

A PNG file is a signature and a list of chunks `length, type, data, CRC-32(type + data)` (PNG specification, section 5).  The image
data is ONE zlib stream (RFC 1950: two header bytes, deflate blocks, the Adler-32 of the uncompressed bytes) of the filtered rows.
The device delivers that stream in pieces that each end on a byte boundary and contain no final block, with the Adler-32 of each
piece's own bytes; what is left for the host is arithmetic on a few numbers and one `zlib.crc32` over the compressed bytes (which
releases the GIL, so the writer's threads run it in parallel).  Pure Python, `zlib` and `struct` only."""
import struct
import zlib

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

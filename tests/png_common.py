"""Shared by tests/test_png_host.py and tests/test_png_gpu.py: reading a PNG file apart with `struct` and `zlib` alone, and the PNG
row filters 0 and 2 done by hand.  Not a test module."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def png_chunks(data):
    """[(type, payload)] of a PNG file; the CRC-32 of every chunk is checked"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        payload = data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + payload), kind
        out.append((kind, payload))
        at += 12 + n
    assert at == len(data)
    return out


def idat_of(data):
    kinds = [k for k, _ in png_chunks(data)]
    assert kinds == [b"IHDR", b"IDAT", b"IEND"], kinds
    return png_chunks(data)[1][1]


def decode(data):
    """the file's pixels through PIL (which checks the chunk CRCs; zlib inside it checks the Adler-32)"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == "RGB"
        im.load()
        return np.asarray(im).copy()


def filter_rows(frame, types):
    """frame uint8 [H,W,3], types: one of 0 (None) / 2 (Up) per row -> the filtered bytes H * (1 + 3 W), as PNG defines them"""
    h = frame.shape[0]
    rows = frame.reshape(h, -1)
    out = bytearray()
    for r in range(h):
        t = types[r]
        assert t in (0, 2)
        above = rows[r - 1] if r else np.zeros_like(rows[0])
        out.append(t)
        out += (rows[r] if t == 0 else (rows[r].astype(np.int16) - above).astype(np.uint8)).tobytes()
    return bytes(out)


def adler_halves(data):
    a = zlib.adler32(data)
    return a & 0xffff, a >> 16

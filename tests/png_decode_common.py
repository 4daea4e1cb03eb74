"""Shared by tests/test_png_decode_host.py and tests/test_png_decode_gpu.py: the five PNG row filters by hand, a fixed-Huffman bit
writer, a reader of dynamic block headers (the tests assert their own premise with it), the corpus of streams both sides decode, and
the stand-alone host program around csrc/ct_inflate.h.  The oracles are zlib and PIL.  Not a test module."""
import io
import os
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "color-transfer_amd", "csrc")
# include/ct_hip.h: CT_INFLATE_*
(OK, BAD_HEADER, BLOCK_TYPE, STORED_LEN, OVERSUBSCRIBED, INCOMPLETE, REPEAT, INVALID_SYMBOL, DISTANCE, INPUT_EXHAUSTED, TOO_LARGE, TOO_SMALL,
 ADLER, FILTER, DIMS) = range(15)


# ---- row filters ------------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    """numpy int arrays -> the predictor, ties in the order a, b, c"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(frame, types):
    """frame uint8 [H,W,3], types: one of 0 .. 4 per row -> the filtered bytes H * (1 + 3 W) as the PNG specification defines them
    (a type above 4 is written as it is, with the bytes of type 0: for the status tests)"""
    h = frame.shape[0]
    rows = frame.reshape(h, -1).astype(np.int32)
    zero = np.zeros_like(rows[0])
    out = bytearray()
    for r in range(h):
        t = int(types[r])
        x = rows[r]
        a = np.concatenate([zero[:3], x[:-3]])
        b = rows[r - 1] if r else zero
        c = np.concatenate([zero[:3], b[:-3]])
        pred = {0: zero, 1: a, 2: b, 3: (a + b) >> 1, 4: paeth(a, b, c)}.get(t, zero)
        out.append(t)
        out += ((x - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def png_file(height, width, payload, idat_split=None):
    """an 8-bit RGB PNG file around a zlib payload (one IDAT, or cut at the byte positions of idat_split)"""
    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    cuts = [0] + list(idat_split or []) + [len(payload)]
    idats = b"".join(chunk(b"IDAT", payload[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:]))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)) + idats + chunk(b"IEND", b"")


def pil_decode(data):
    """uint8 [3,H,W] of a file through PIL, like utils.data.read_image"""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB")).transpose(2, 0, 1))


def pil_encode(frame_hwc, level=6, mode="RGB"):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame_hwc, mode).save(buf, format="PNG", compress_level=level)
    return buf.getvalue()


def chunk_kinds(data):
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        out.append(kind)
        at += 12 + n
    return out


# ---- a fixed-Huffman block, written by hand -----------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    """RFC 1951 bit order: values LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):
        self.bits(int(format(value, "0%db" % count)[::-1], 2), count)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def fixed_symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, distance):
        ls = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
        self.fixed_symbol(257 + ls)
        self.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(i for i in range(30) if DIST_BASE[i] <= distance)
        self.code(ds, 5)
        self.bits(distance - DIST_BASE[ds], DIST_EXTRA[ds])


def zlib_wrap(deflate, raw):
    return b"\x78\x01" + bytes(deflate) + struct.pack(">I", zlib.adler32(raw))


def fixed_block_stream(literals, matches, final=True):
    """zlib stream of ONE fixed block: the literals, then the (length, distance) matches, then end of block -> (stream, its bytes)"""
    w = BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    raw = bytearray(literals)
    for b in literals:
        w.fixed_symbol(b)
    for length, distance in matches:
        w.fixed_match(length, distance)
        for _ in range(length):
            raw.append(raw[-distance])
    w.fixed_symbol(256)
    w.align()
    return zlib_wrap(w.out, bytes(raw)), bytes(raw)


# ---- a reader of the first block's header -----------------------------------------------------------------------------------------
class BitReader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def bits(self, count):
        v = 0
        for k in range(count):
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << k
            self.at += 1
        return v


def canonical(lens):
    """{(length, code): symbol}"""
    code, out = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[(l, code)] = s
                code += 1
        code <<= 1
    return out


def first_block(stream):
    """the first deflate block of a zlib stream: {"type", and for type 2: "lit_lens", "dist_lens", "repeats" (which of 16 / 17 / 18 occur),
    "longest" (the longest literal / length code)}"""
    r = BitReader(stream[2:])
    r.bits(1)
    info = {"type": r.bits(2)}
    if info["type"] != 2:
        return info
    hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = r.bits(3)
    table = canonical(cl)
    lens, repeats = [], set()
    while len(lens) < hlit + hdist:
        l, code = 0, 0
        while (l, code) not in table:
            code = (code << 1) | r.bits(1)
            l += 1
            assert l <= 7
        s = table[(l, code)]
        if s < 16:
            lens.append(s)
        else:
            repeats.add(s)
            lens += [lens[-1]] * (3 + r.bits(2)) if s == 16 else [0] * ((3 + r.bits(3)) if s == 17 else (11 + r.bits(7)))
    assert len(lens) == hlit + hdist
    info.update(lit_lens=lens[:hlit], dist_lens=lens[hlit:], repeats=repeats, longest=max(lens[:hlit]))
    return info


# ---- the frames and streams of the tests --------------------------------------------------------------------------------------------
def structured_frame(h, w, seed=0):
    """smooth ramps + a little noise, uint8 [H,W,3]: compressible, every filter type has something to do"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [40 + 3 * x + 2 * y, 200 - 2 * x + y, 20 + x * y // 3]
    return ((np.stack(planes, axis=-1) + rng.integers(0, 3, (h, w, 3))) % 256).astype(np.uint8)


def noise_frame(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def fibonacci_frame():
    """tests/test_png_gpu.py's frame restated: 144 x 66 pixels whose 28 656 filtered bytes take 21 values with the counts 1, 1, 2, 3,
    5 ... 10946, shuffled, so that filter 0 wins on every row and an unlimited Huffman code would be 20 bits deep"""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 28656 == 144 * (1 + 3 * 66)
    values = [0] + [v for k in range(1, 11) for v in (k, 256 - k)]
    counts = dict(zip(values, sorted(fib, reverse=True)))
    counts[0] -= 144
    pixels = np.concatenate([np.full(c, v, dtype=np.uint8) for v, c in counts.items()])
    np.random.default_rng(21).shuffle(pixels)
    return pixels.reshape(144, 66, 3)


def power_of_two_frame():
    """7 x 1560 pixels whose 32 767 filtered bytes take 15 values with the counts 1, 2, 4 ... 16384, shuffled (filter 0 wins on every
    row, as in the Fibonacci frame): with end-of-block the Huffman code is 15 bits deep and needs no limiting, so this project's
    encoder emits 15-bit literal codes for it.  (The Fibonacci frame does not: ct_png.h's length limiter turns its 20-bit-deep code
    into one of 2 .. 11 bits that costs the same, two symbols per length.)"""
    counts = [2 ** k for k in range(15)]
    assert sum(counts) == 32767 == 7 * (1 + 3 * 1560)
    values = [0] + [v for k in range(1, 8) for v in (k, 256 - k)]
    by_value = dict(zip(values, sorted(counts, reverse=True)))
    by_value[0] -= 7
    pixels = np.concatenate([np.full(c, v, dtype=np.uint8) for v, c in by_value.items()])
    np.random.default_rng(22).shuffle(pixels)
    return pixels.reshape(7, 1560, 3)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return co.compress(raw) + co.flush()


def repeat_symbols_raw():
    """bytes whose level-6 header needs all three repeat symbols: long runs of unused literals (18), short ones (17) and runs of
    equal lengths (16); first_block() confirms it in the tests"""
    rng = np.random.default_rng(5)
    vals = np.concatenate([np.arange(0, 40), np.arange(44, 48), np.arange(200, 256)]).astype(np.uint8)
    return rng.choice(vals, 6000).tobytes()


def fifteen_bit_stream():
    """literals 0 .. 15 with the code lengths 1, 2, ... 14, 15, 15 minus end-of-block's share: a complete code whose longest codes have
    15 bits, sent with a code-length code of 4 bits each and no repeat symbols; every literal occurs once"""
    lens = [0] * 257
    for i in range(14):
        lens[i] = i + 1                                     # 1 .. 14 bits
    lens[14], lens[256] = 15, 15                            # the last two share the last slot: the Kraft sum is exactly 1
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(15, 4)          # final, dynamic, HLIT = 257, HDIST = 1, HCLEN = 19
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]:
        w.bits(4 if s < 16 else 0, 3)                       # the code-length code: 16 codes of 4 bits, symbol L is L
    for l in lens + [0]:                                    # 257 literal / length lengths and one distance length of 0
        w.code(l, 4)
    codes = {s: (l, c) for (l, c), s in canonical(lens).items()}
    raw = bytes(list(range(15)) * 3)
    for b in raw:
        w.code(codes[b][1], codes[b][0])
    w.code(codes[256][1], codes[256][0])
    w.align()
    return zlib_wrap(w.out, raw), raw


_corpus = None


def valid_streams():
    """{name: (zlib stream, its bytes)}: every valid stream the GPU tests inflate; the host program decodes them all as well"""
    global _corpus
    if _corpus is not None:
        return _corpus
    out = {}
    frame = structured_frame(23, 37, 1)
    raw = filter_rows(frame, [r % 5 for r in range(23)])
    for name, level, strategy in (("level0", 0, zlib.Z_DEFAULT_STRATEGY), ("level1", 1, zlib.Z_DEFAULT_STRATEGY), ("level6", 6, zlib.Z_DEFAULT_STRATEGY),
                                  ("level9", 9, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY),
                                  ("rle", 6, zlib.Z_RLE)):
        out[name] = (deflate(raw, level, strategy), raw)
    big = np.random.default_rng(2).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    out["stored_two_blocks"] = (deflate(big, 0), big)
    co = zlib.compressobj(6)
    out["full_flush"] = (co.compress(raw[:1000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[1000:]) + co.flush(), raw)
    lits = np.random.default_rng(3).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    out["match_geometry"] = fixed_block_stream(lits, [(258, 32768), (3, 1), (258, 1), (10, 3)])
    rep = repeat_symbols_raw()
    out["repeat_symbols"] = (deflate(rep, 6), rep)
    out["fifteen_bits"] = fifteen_bit_stream()
    _corpus = out
    return out


def small_streams():
    """three streams of at most 600 bytes -- stored, fixed, dynamic -- for the truncation and bit-flip sweep"""
    raw = filter_rows(structured_frame(5, 9, 4), [0, 1, 2, 3, 4])
    dyn_raw = (raw * 6)[:700]
    out = {"stored": (deflate(raw, 0), raw), "fixed": (deflate(raw, 6, zlib.Z_FIXED), raw), "dynamic": (deflate(dyn_raw, 6), dyn_raw)}
    for s, _ in out.values():
        assert len(s) <= 600
    return out


def status_cases():
    """{name: (stream, slot size, expected status)} of the malformed streams; the host program decodes them before the GPU does"""
    good, raw = valid_streams()["level6"]
    w = BitWriter()
    w.bits(1, 1), w.bits(1, 2), w.fixed_symbol(65), w.fixed_match(3, 2), w.fixed_symbol(256), w.align()
    too_far = zlib_wrap(w.out, b"AAAA")
    stored = b"\x78\x01\x01\x04\x00\xfb\xfe" + b"abcd" + struct.pack(">I", zlib.adler32(b"abcd"))       # NLEN is not ~LEN
    return {
        "truncated": (good[:-1], len(raw), INPUT_EXHAUSTED),
        "adler": (good[:-1] + bytes([good[-1] ^ 1]), len(raw), ADLER),
        "distance": (too_far, 4, DISTANCE),
        "block_type": (b"\x78\x01\x07" + b"\x00" * 8, 4, BLOCK_TYPE),
        "stored_len": (stored, 4, STORED_LEN),
        "slot_small": (good, len(raw) - 1, TOO_LARGE),
        "slot_large": (good, len(raw) + 1, TOO_SMALL),
    }


# ---- the stand-alone host program around ct_inflate.h ---------------------------------------------------------------------------------
HOST_MAIN = r"""
// cases.bin: u32 count, then per case u32 expected size, u32 length, the stream.  results.bin: per case i32 status, u32 n, n bytes
// (n = expected size when the status is 0, else 0).  Every stream and every slot is a heap block of exactly its size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ct_inflate.h"
static unsigned rd32(FILE *f) { unsigned v = 0; if (fread(&v, 4, 1, f) != 1) { fprintf(stderr, "short read\n"); exit(2); } return v; }
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const unsigned count = rd32(in);
    ct::InflateTables *tables = new ct::InflateTables;
    for (unsigned c = 0; c < count; ++c) {
        const unsigned expect = rd32(in), len = rd32(in);
        unsigned char *src = (unsigned char *)malloc(len ? len : 1), *dst = (unsigned char *)malloc(expect ? expect : 1);
        if (len && fread(src, 1, len, in) != len) return 2;
        memset(tables, 0xEE, sizeof *tables);
        ct::InflateArraySource source{src, (long long)len};
        ct::InflateArraySink sink{dst, 0u};
        const int status = ct::inflate(source, (long long)len, sink, expect, *tables);
        const unsigned n = status == 0 ? expect : 0u;
        fwrite(&status, 4, 1, out);
        fwrite(&n, 4, 1, out);
        if (n) fwrite(dst, 1, n, out);
        free(src);
        free(dst);
    }
    delete tables;
    fclose(in);
    fclose(out);
    printf("%u cases\n", count);
    return 0;
}
"""


def build_host_program(directory, sanitize=True):
    """compile HOST_MAIN against csrc/ct_inflate.h with the host compiler (AddressSanitizer + UBSan) -> path of the program"""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(str(directory), "inflate_main.cpp")
    exe = os.path.join(str(directory), "inflate_main")
    with open(src, "w") as fh:
        fh.write(HOST_MAIN)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall"] + flags + ["-I", CSRC, src, "-o", exe]
    # the sanitizer runtimes linked statically where the compiler has them: the program then runs whatever else the loader preloads
    if not sanitize or subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return exe


def run_host_program(exe, cases, directory):
    """cases: [(stream, expected size)] -> [(status, bytes or None)]; the program runs ONCE, as its own process, and must exit 0 with
    nothing on stderr (a sanitizer report goes there)"""
    import subprocess
    cases = list(cases)
    cin, cout = os.path.join(str(directory), "cases.bin"), os.path.join(str(directory), "results.bin")
    with open(cin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for stream, expect in cases:
            fh.write(struct.pack("<II", expect, len(stream)) + bytes(stream))
    done = subprocess.run([exe, cin, cout], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0 and not done.stderr.strip(), (done.returncode, done.stderr[-2000:])
    data, at, out = open(cout, "rb").read(), 0, []
    for _ in cases:
        status, n = struct.unpack("<iI", data[at:at + 8])
        out.append((status, data[at + 8:at + 8 + n] if status == 0 else None))
        at += 8 + n
    assert at == len(data)
    return out


def zlib_says(stream):
    """zlib's bytes of the stream, or None where it refuses it"""
    try:
        return zlib.decompress(bytes(stream))
    except zlib.error:
        return None

"""The YUV4MPEG2 (Y4M) container, 8-bit 4:2:0 progressive only: a text header, then per frame a `FRAME` line and the raw planes
(Y, Cb, Cr: a packed I420 frame, what ct_hip.yuv420_to_rgb reads and ct_hip.rgb_to_yuv420 writes).  It is the stand-in for
cv2.VideoCapture (the reference's utils/postprocess.py:78-103) that needs no library: `ffmpeg -i left.mp4 -f yuv4mpegpipe left.y4m`
makes one, and every encoder takes one.  Pure Python: no GPU, no torch.

    YUV4MPEG2 W1920 H1080 F25:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\\n
    FRAME\\n <W*H + 2*ceil(W/2)*ceil(H/2) bytes> FRAME\\n ...

Chroma tags: `C420jpeg`, plain `C420` and no `C` tag mean chroma sited at the centre of its 2x2 luma block ("center");
`C420mpeg2` means horizontally co-sited with the even luma column ("left").  Everything else (4:2:2, 4:4:4, mono, more than 8
bits, `C420paldv`, interlaced streams) is refused with a message that names the tag."""
import os
from typing import NamedTuple, Optional

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME"
SITING_OF_TAG = {None: "center", "420": "center", "420jpeg": "center", "420mpeg2": "left"}
TAG_OF_SITING = {"center": "420jpeg", "left": "420mpeg2"}
RANGES = ("limited", "full")
MAX_HEADER = 4096                      # a header line longer than this is not a Y4M header


class Y4MError(ValueError):
    pass


class Header(NamedTuple):
    width: int
    height: int
    fps: str                           # "num:den" as written ("25:1"); "0:0" = unknown
    aspect: str                        # "num:den"; "0:0" = unknown
    interlacing: str                   # "p"
    chroma: Optional[str]              # the C tag without its letter ("420jpeg"), None when the stream has none
    color_range: Optional[str]         # "limited" / "full" from XCOLORRANGE, None without the extension
    header_len: int                    # bytes up to and including the newline

    @property
    def siting(self):
        return SITING_OF_TAG[self.chroma]

    @property
    def frame_bytes(self):
        return frame_bytes(self.width, self.height)


def frame_bytes(width, height):
    return width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2)


def _ratio(tag, value):
    parts = value.split(":")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise Y4MError("Y4M header: tag %r is not a ratio num:den" % (tag + value))
    return "%d:%d" % (int(parts[0]), int(parts[1]))


def parse_header(data):
    """the first bytes of a file (at least the header line) -> Header"""
    data = bytes(data[:MAX_HEADER])
    end = data.find(b"\n")
    if not data.startswith(MAGIC + b" ") or end < 0:
        raise Y4MError("not a Y4M stream: it does not start with a `YUV4MPEG2 ...` line of at most %d bytes" % MAX_HEADER)
    try:
        tags = data[len(MAGIC):end].decode("ascii").split()
    except UnicodeDecodeError:
        raise Y4MError("Y4M header: not ASCII")
    width = height = None
    fps, aspect, inter, chroma, crange = "0:0", "0:0", "p", None, None
    for t in tags:
        key, value = t[0], t[1:]
        if key in "WH":
            if not value.isdigit() or int(value) < 1:
                raise Y4MError("Y4M header: tag %r is not a positive size" % t)
            if key == "W":
                width = int(value)
            else:
                height = int(value)
        elif key == "F":
            fps = _ratio(key, value)
        elif key == "A":
            aspect = _ratio(key, value)
        elif key == "I":
            if value != "p":
                raise Y4MError("Y4M header: tag %r: only progressive streams (Ip) are taken, no interlaced material" % t)
            inter = value
        elif key == "C":
            if value not in SITING_OF_TAG:
                raise Y4MError("Y4M header: tag %r: only 8-bit 4:2:0 is taken (C420jpeg, C420mpeg2, C420)" % t)
            chroma = value
        elif key == "X":
            if value.startswith("COLORRANGE="):
                r = value[len("COLORRANGE="):].lower()
                if r not in RANGES:
                    raise Y4MError("Y4M header: tag %r: XCOLORRANGE is LIMITED or FULL" % t)
                crange = r
        else:
            raise Y4MError("Y4M header: unknown tag %r" % t)
    if width is None or height is None:
        raise Y4MError("Y4M header: no %s tag" % ("W" if width is None else "H"))
    return Header(width, height, fps, aspect, inter, chroma, crange, end + 1)


def header(width, height, fps="25:1", aspect="1:1", siting="center", range="limited"):
    """the header line of a stream this package writes, as bytes"""
    if isinstance(width, bool) or isinstance(height, bool) or not isinstance(width, int) or not isinstance(height, int) or width < 1 or height < 1:
        raise Y4MError("Y4M header: width and height must be positive integers (got %r, %r)" % (width, height))
    if siting not in TAG_OF_SITING:
        raise Y4MError("Y4M header: siting %r: one of %s" % (siting, ", ".join(sorted(TAG_OF_SITING))))
    if range not in RANGES:
        raise Y4MError("Y4M header: range %r: one of %s" % (range, ", ".join(RANGES)))
    fps, aspect = _ratio("F", str(fps)), _ratio("A", str(aspect))
    return ("YUV4MPEG2 W%d H%d F%s Ip A%s C%s XCOLORRANGE=%s\n" % (width, height, fps, aspect, TAG_OF_SITING[siting], range.upper())).encode("ascii")


def read_header(path):
    with open(path, "rb") as fh:
        return parse_header(fh.read(MAX_HEADER))


def frame_offsets(file):
    """(Header, [offset of every frame's first plane byte]) of a Y4M file (a path or a binary file object).  When the file's size is
    the header plus a whole number of (6 + frame_bytes) and every FRAME line is the bare 6 bytes where the arithmetic puts it, the
    offsets are computed; otherwise the file is scanned FRAME line by FRAME line (a line may carry parameters).  A truncated last
    frame, or bytes that are no FRAME line where one is due, raise Y4MError."""
    if isinstance(file, (str, bytes, os.PathLike)):
        with open(file, "rb") as fh:
            return frame_offsets(fh)
    fh = file
    fh.seek(0)
    hdr = parse_header(fh.read(MAX_HEADER))
    size = fh.seek(0, os.SEEK_END)
    fb, bare = hdr.frame_bytes, len(FRAME) + 1
    body = size - hdr.header_len

    def line_at(pos, n=MAX_HEADER):
        fh.seek(pos)
        return fh.read(n)

    if body % (bare + fb) == 0:
        n = body // (bare + fb)
        # every FRAME line is bare exactly when each sits where the arithmetic puts it: 6 bytes read per frame, no plane touched
        if all(line_at(hdr.header_len + i * (bare + fb), bare) == FRAME + b"\n" for i in range(n)):
            return hdr, [hdr.header_len + i * (bare + fb) + bare for i in range(n)]
    offsets, pos = [], hdr.header_len
    while pos < size:
        line = line_at(pos)
        end = line.find(b"\n")
        if not line.startswith(FRAME) or end < 0 or (end > len(FRAME) and line[len(FRAME):len(FRAME) + 1] != b" "):
            raise Y4MError("Y4M stream: no FRAME line at byte %d (frame %d)" % (pos, len(offsets)))
        start = pos + end + 1
        if start + fb > size:
            raise Y4MError("Y4M stream: frame %d is truncated (%d of %d bytes)" % (len(offsets), size - start, fb))
        offsets.append(start)
        pos = start + fb
    return hdr, offsets

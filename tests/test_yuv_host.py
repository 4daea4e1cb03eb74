"""Host half of the Y'CbCr 4:2:0 path (no GPU): the int64 oracle of tests/yuv_common.py against the rule's own statement in exact
fractions and against PIL, its round-trip pin, the Y4M container (utils/y4m.py), and the argument checks of the writer, the command
line and the header."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import yuv_common as yc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against the statement ---------------------------------------------------------------------------------------
def _bilinear16(plane, y, x, siting):
    """chroma at luma (y, x) by the siting, straight from the sample positions: 16 times the bilinear value, as a Fraction"""
    ch, cw = plane.shape
    py = (Fraction(y) - Fraction(1, 2)) / 2                     # chroma row i sits at luma 2i + 1/2
    px = (Fraction(x) - Fraction(1, 2)) / 2 if siting == "center" else Fraction(x, 2)        # column j at 2j + 1/2, or at 2j
    iy, ix = py.numerator // py.denominator, px.numerator // px.denominator                 # floor
    fy, fx = py - iy, px - ix

    def at(i, j):
        return int(plane[min(max(i, 0), ch - 1), min(max(j, 0), cw - 1)])
    v = ((1 - fy) * ((1 - fx) * at(iy, ix) + fx * at(iy, ix + 1)) + fy * ((1 - fx) * at(iy + 1, ix) + fx * at(iy + 1, ix + 1)))
    return 16 * v


@pytest.mark.parametrize("matrix,range_,siting", yc.CONFIGS)
def test_oracle_equals_the_rule_in_fractions(matrix, range_, siting):
    """a few thousand random samples per configuration, both directions, odd sizes included"""
    rng = np.random.default_rng(100 + yc.CONFIGS.index((matrix, range_, siting)))
    for h, w, n in ((5, 7, 60), (4, 6, 40), (1, 1, 20), (3, 2, 20)):
        yuv = yc.random_yuv(rng, n, h, w)
        got = yc.decode_oracle(yuv, h, w, matrix, range_, siting)
        ys, cbs, crs = yc.planes(yuv, h, w)
        for f in range(n):
            for y in range(h):
                for x in range(w):
                    cb16, cr16 = _bilinear16(cbs[f], y, x, siting), _bilinear16(crs[f], y, x, siting)
                    assert cb16.denominator == 1 and cr16.denominator == 1            # an exact count of sixteenths
                    want = yc.decode_fraction(int(ys[f, y, x]), int(cb16), int(cr16), matrix, range_)
                    assert tuple(got[f, y, x]) == want, (f, y, x)
        rgb = yc.random_rgb(rng, n, h, w)
        enc = yc.encode_oracle(rgb, matrix, range_, siting)
        ey, ecb, ecr = yc.planes(enc, h, w)
        for f in range(n):
            for y in range(h):
                for x in range(w):
                    assert ey[f, y, x] == yc.encode_luma_fraction(*map(int, rgb[f, y, x]), matrix, range_)
            for i in range((h + 1) // 2):
                for j in range((w + 1) // 2):
                    rows = [min(2 * i, h - 1), min(2 * i + 1, h - 1)]
                    if siting == "center":
                        taps = [(min(2 * j, w - 1), 1), (min(2 * j + 1, w - 1), 1)]
                    else:
                        taps = [(min(max(2 * j - 1, 0), w - 1), 1), (min(2 * j, w - 1), 2), (min(2 * j + 1, w - 1), 1)]
                    tw = sum(t for _, t in taps) * 2
                    mean = [Fraction(sum(t * int(rgb[f, r, c, k]) for r in rows for c, t in taps), tw) for k in range(3)]
                    assert (ecb[f, i, j], ecr[f, i, j]) == yc.encode_chroma_fraction(*mean, matrix, range_), (f, i, j)


def test_full_range_bt601_encode_is_within_one_code_of_pil():
    """the one independent anchor present offline: Image.convert("YCbCr") is full-range BT.601 in 16-bit fixed point and truncates;
    on constant colours the rule is within 1 code of it on all 2^24"""
    from PIL import Image
    worst, equal = 0, 0
    for r0 in range(0, 256, 16):
        blocks, colours = yc.colour_cube_blocks(r0, r0 + 16)
        del blocks
        flat = colours.reshape(-1, 3)
        pil = np.asarray(Image.fromarray(flat.reshape(-1, 256, 3)).convert("YCbCr")).reshape(-1, 3).astype(np.int64)
        ours = yc.encode_oracle(flat.reshape(-1, 1, 1, 3), "bt601", "full", "center").astype(np.int64)
        worst = max(worst, int(np.abs(ours - pil).max()))
        equal += int((ours == pil).all(axis=1).sum())
    print("PIL anchor: worst |difference| %d code, %.1f %% of the colours equal in all three planes" % (worst, 100.0 * equal / 2 ** 24))
    assert worst <= 1


ROUND_TRIP_WORST = {"limited": 2, "full": 1}           # from the oracle itself, every matrix and siting


@pytest.mark.parametrize("matrix,range_,siting", yc.CONFIGS)
def test_round_trip_of_constant_frames_is_pinned(matrix, range_, siting):
    """decode(encode(constant frame)) on the 18^3 grid of colours in steps of 15: the worst error is the quantisation of the range
    (219 / 224 steps for 255), a regression pin"""
    g = np.arange(0, 256, 15, dtype=np.uint8)
    col = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 1, 1, 3)
    frames = np.ascontiguousarray(np.broadcast_to(col, (col.shape[0], 2, 2, 3)))
    back = yc.decode_oracle(yc.encode_oracle(frames, matrix, range_, siting), 2, 2, matrix, range_, siting)
    assert int(np.abs(back.astype(np.int64) - frames).max()) == ROUND_TRIP_WORST[range_]


# ---- the container -------------------------------------------------------------------------------------------------------------------
def test_y4m_header_round_trip():
    from utils import y4m
    for w, h, fps, aspect, siting, rng_ in ((1920, 1080, "25:1", "1:1", "center", "limited"), (31, 17, "30000:1001", "16:15", "left", "full"),
                                            (1, 1, "0:0", "0:0", "center", "full")):
        head = y4m.header(w, h, fps, aspect, siting, rng_)
        assert head.startswith(b"YUV4MPEG2 ") and head.endswith(b"\n") and head.count(b"\n") == 1
        p = y4m.parse_header(head + b"FRAME\n....")
        assert (p.width, p.height, p.fps, p.aspect, p.interlacing, p.siting, p.color_range, p.header_len) == \
               (w, h, fps, aspect, "p", siting, rng_, len(head))
        assert p.frame_bytes == yc.frame_bytes(h, w) == w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    # what other writers leave out: no I, no C, no X; plain C420; an unknown X extension is skipped
    p = y4m.parse_header(b"YUV4MPEG2 W4 H2\n")
    assert (p.width, p.height, p.fps, p.aspect, p.chroma, p.siting, p.color_range) == (4, 2, "0:0", "0:0", None, "center", None)
    assert y4m.parse_header(b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C420 XYSCSS=420JPEG\n").siting == "center"
    assert y4m.parse_header(b"YUV4MPEG2 W4 H2 C420mpeg2 XCOLORRANGE=FULL\n")[5:7] == ("420mpeg2", "full")
    for bad in ((0, 2, "25:1", "1:1", "center", "limited"), (2, 2, "25", "1:1", "center", "limited"), (2, 2, "25:1", "1:1", "top", "limited"),
                (2, 2, "25:1", "1:1", "center", "tv")):
        with pytest.raises(y4m.Y4MError):
            y4m.header(*bad)


@pytest.mark.parametrize("tag", ["C422", "C444", "C420p10", "C420p12", "C422p10", "C444p16", "Cmono", "Cmono16", "C420paldv", "C411", "C444alpha",
                                 "It", "Ib", "Im", "I?"])
def test_y4m_refuses_what_it_does_not_take(tag):
    from utils import y4m
    with pytest.raises(y4m.Y4MError) as e:
        y4m.parse_header(("YUV4MPEG2 W8 H8 F25:1 %s A1:1\n" % tag).encode())
    assert repr(tag) in str(e.value)                              # the message names the tag


def test_y4m_refuses_broken_headers():
    from utils import y4m
    for data in (b"", b"YUV4MPEG W8 H8\n", b"YUV4MPEG2 W8 H8", b"YUV4MPEG2 W8\n", b"YUV4MPEG2 H8\n", b"YUV4MPEG2 W0 H8\n", b"YUV4MPEG2 W8 H8 F25\n",
                 b"YUV4MPEG2 W8 H8 Q1\n", b"YUV4MPEG2 W8 H8 XCOLORRANGE=TV\n", b"RIFF....AVI LIST"):
        with pytest.raises(y4m.Y4MError):
            y4m.parse_header(data)


@pytest.mark.parametrize("w,h", [(8, 6), (5, 3), (1, 1), (31, 17)])
def test_y4m_frame_offsets_computed_scanned_and_truncated(tmp_path, w, h):
    from utils import y4m
    rng = np.random.default_rng(w * 100 + h)
    frames = yc.random_yuv(rng, 4, h, w)
    fb = yc.frame_bytes(h, w)
    bare = tmp_path / "bare.y4m"
    yc.write_y4m(bare, frames, w, h)
    head, offs = y4m.frame_offsets(str(bare))
    assert (head.width, head.height, head.frame_bytes) == (w, h, fb)
    assert offs == [head.header_len + 6 + i * (6 + fb) for i in range(4)]
    data = bare.read_bytes()
    assert all(data[o:o + fb] == frames[i].tobytes() for i, o in enumerate(offs))
    # FRAME lines with parameters: scanned
    par = tmp_path / "par.y4m"
    yc.write_y4m(par, frames, w, h, tag="C420mpeg2", extra="XCOLORRANGE=FULL", frame_params=" Ip XFOO=1")
    head2, offs2 = y4m.frame_offsets(str(par))
    assert (head2.siting, head2.color_range) == ("left", "full")
    line = len(b"FRAME Ip XFOO=1\n")
    assert offs2 == [head2.header_len + line + i * (line + fb) for i in range(4)]
    data2 = par.read_bytes()
    assert all(data2[o:o + fb] == frames[i].tobytes() for i, o in enumerate(offs2))
    # only ONE line with parameters, of a length that keeps the total on the bare grid when frame data is dropped: still scanned right
    mixed = tmp_path / "mixed.y4m"
    with open(mixed, "wb") as f:
        f.write(data[:head.header_len] + b"FRAME Ip\n" + frames[0].tobytes() + b"FRAME\n" + frames[1].tobytes())
    assert y4m.frame_offsets(str(mixed))[1] == [head.header_len + 9, head.header_len + 9 + fb + 6]
    # a truncated last frame, and garbage where a FRAME line is due
    cut = tmp_path / "cut.y4m"
    cut.write_bytes(data[:-1])
    with pytest.raises(y4m.Y4MError) as e:
        y4m.frame_offsets(str(cut))
    assert "truncated" in str(e.value) and "frame 3" in str(e.value)
    junk = tmp_path / "junk.y4m"
    junk.write_bytes(data[:offs[1] + fb] + b"FRAMED\n" + b"\0" * fb)
    with pytest.raises(y4m.Y4MError):
        y4m.frame_offsets(str(junk))
    # a header alone is an empty video
    empty = tmp_path / "empty.y4m"
    empty.write_bytes(data[:head.header_len])
    assert y4m.frame_offsets(str(empty))[1] == []


# ---- the writer, the command line, the header ---------------------------------------------------------------------------------------
def test_frame_writer_y4m_argument_errors(tmp_path):
    from utils import y4m
    from utils.writer import FORMATS, FrameWriter, truncate_y4m, y4m_options
    assert "y4m" in FORMATS
    with pytest.raises(ValueError) as e:
        FrameWriter(tmp_path, fmt="y4m")
    assert "n_frames" in str(e.value)
    for bad in ({"matrix": "bt2020"}, {"range": "tv"}, {"siting": "top"}, {"fps": "25"}, {"aspect": "x:y"}, {"bitrate": 1}):
        with pytest.raises(ValueError):
            FrameWriter(tmp_path, fmt="y4m", n_frames=3, y4m=bad)
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, fmt="png", y4m={"fps": "25:1"})                      # the options belong to the format
    assert y4m_options(None) == {"fps": "25:1", "aspect": "1:1", "matrix": "bt709", "range": "limited", "siting": "center"}
    assert y4m_options({"fps": None, "siting": "left"})["siting"] == "left"         # None = the default
    with FrameWriter(tmp_path, fmt="y4m", n_frames=3, y4m={"fps": "30000:1001"}) as w:
        with pytest.raises(ValueError) as e:
            w.submit([0], torch.zeros((1, 4, 6, 3), dtype=torch.uint8))              # host tensors have no device to convert on
        assert "device" in str(e.value)
        with pytest.raises(ValueError) as e:
            w.submit([0], torch.zeros((1, 4, 6, 3), dtype=torch.uint8), suffix="chess")
        assert "one file" in str(e.value)
        with pytest.raises(ValueError):
            w.submit([3], torch.zeros((1, 4, 6, 3), dtype=torch.uint8))
    n = truncate_y4m(tmp_path / "o", 4, 6, {"fps": "30000:1001", "siting": "left", "range": "full"})
    data = (tmp_path / "o" / "frames.y4m").read_bytes()
    head = y4m.parse_header(data)
    assert len(data) == n == head.header_len
    assert (head.width, head.height, head.fps, head.siting, head.color_range) == (6, 4, "30000:1001", "left", "full")


CFG = """
model:
  class_path: tests.cli_stub.StubRunner
data:
  class_path: utils.data.DataModule
  init_args:
    n_frames: 3
    height: 8
    width: 12
"""


def test_cli_refuses_y4m_on_the_cpu_before_the_first_frame(tmp_path, monkeypatch):
    from utils import cli
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    out = tmp_path / "o"
    with pytest.raises(SystemExit) as e:
        cli.main(["predict", "--config", str(cfg), "--output", str(out), "--format", "y4m"])
    assert "y4m" in str(e.value) and "GPU" in str(e.value) and not out.exists()
    with pytest.raises(SystemExit) as e:
        cli.main(["predict", "--config", str(cfg), "--output", str(out), "--format", "jpeg"])
    assert "jpeg" in str(e.value) and "y4m" in str(e.value)                     # the list of formats names the new one
    for extra in (["--data.y4m_target", str(tmp_path / "t.y4m"), "--data.y4m_reference", str(tmp_path / "r.y4m")], ["--data.synthetic", "video_yuv"]):
        for cmd in (["test"], ["predict", "--output", str(out), "--format", "npy"]):
            with pytest.raises(SystemExit) as e:
                cli.main(cmd[:1] + ["--config", str(cfg)] + cmd[1:] + extra)
            assert "GPU" in str(e.value) and not out.exists()
    with pytest.raises(SystemExit) as e:
        cli.main(["predict", "--config", str(cfg), "--output", str(out), "--format", "y4m", "--views", "chess"])
    assert "y4m" in str(e.value)
    # a ratio on the command line stays text (YAML 1.1 would read 25:1 as a sexagesimal 1501)
    parsed = cli._parse(["predict", "--writer.y4m_fps", "25:1", "--writer.depth", "2"])[0]
    assert parsed["writer"] == {"y4m_fps": "25:1", "depth": 2}
    # the default formats still run on the CPU as before
    assert cli.main(["predict", "--config", str(cfg), "--output", str(out), "--format", "npy"]) == 3


def test_header_declares_the_entries_under_abi_9():
    import ct_hip
    src = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ct_yuv420_to_rgb_u8\s*\(\s*const uint8_t \*yuv, int64_t frame_stride, int n, int height, int width, int matrix, "
                     r"int range, int siting,\s*uint8_t \*out_rgb, void \*stream\)", code)
    assert re.search(r"\bint\s+ct_rgb_to_yuv420_u8\s*\(\s*const uint8_t \*rgb, int n, int height, int width, int matrix, int range, int siting, "
                     r"uint8_t \*out_yuv,\s*int64_t frame_stride, void \*stream\)", code)
    for name, value in (("CT_YUV_BT601", 0), ("CT_YUV_BT709", 1), ("CT_YUV_LIMITED", 0), ("CT_YUV_FULL", 1), ("CT_YUV_SITING_CENTER", 0),
                        ("CT_YUV_SITING_LEFT", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), code)
    assert (ct_hip.YUV_MATRICES, ct_hip.YUV_RANGES, ct_hip.YUV_SITINGS) == ({"bt601": 0, "bt709": 1}, {"limited": 0, "full": 1}, {"center": 0, "left": 1})
    assert re.search(r"#define CT_ABI_VERSION 9\b", code) and ct_hip.CT_ABI_VERSION == 9
    assert {"ct_yuv420_to_rgb_u8", "ct_rgb_to_yuv420_u8"} <= set(ct_hip.SIGNATURES)
    assert len(ct_hip.SIGNATURES["ct_yuv420_to_rgb_u8"][1]) == 10 and len(ct_hip.SIGNATURES["ct_rgb_to_yuv420_u8"][1]) == 10
    lib = ct_hip.lib()
    assert lib.ct_abi_version() == 9
    # argument errors come back before anything touches a device
    assert lib.ct_yuv420_to_rgb_u8(None, 6, 1, 2, 2, 1, 0, 0, None, None) == -1
    one = ct_hip._core._c_p(16)
    for args in ((6, 0, 2, 2, 1, 0, 0), (6, 1, 0, 2, 1, 0, 0), (5, 1, 2, 2, 1, 0, 0), (6, 1, 2, 2, 2, 0, 0), (6, 1, 2, 2, 1, 2, 0), (6, 1, 2, 2, 1, 0, 2),
                 (2 ** 40, 1, 32768, 32768, 1, 0, 0)):
        assert lib.ct_yuv420_to_rgb_u8(one, args[0], *args[1:], one, None) == -1, args
        assert lib.ct_rgb_to_yuv420_u8(one, *args[1:], one, args[0], None) == -1, args
    assert ct_hip.yuv420_frame_bytes(1080, 1920) == 3110400 and ct_hip.yuv420_frame_bytes(3, 5) == 15 + 2 * 6
    for bad in ((0, 4), (4, -1), (2.0, 2), (True, 2)):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.yuv420_frame_bytes(*bad)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.yuv420_to_rgb(torch.zeros(6, dtype=torch.uint8), 2, 2)               # a host tensor: there is no CPU path
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.rgb_to_yuv420(torch.zeros((1, 2, 2, 3), dtype=torch.uint8))
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.yuv420_to_rgb(torch.zeros(6, dtype=torch.uint8), 2, 2, matrix="bt2020")

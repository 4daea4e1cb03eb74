"""The host side of the device PNG decoder: utils.png.parse, csrc/ct_inflate.h as a stand-alone program under AddressSanitizer and
UBSan (its own process: nothing is loaded into Python), and the option plumbing.  zlib and PIL are the oracles; every comparison is
bitwise.  The sweep over every truncation and every single-bit flip of three small streams is what stands between malformed bytes
and the GPU: the core that the kernel runs is the core that runs here."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

from tests import png_decode_common as C

ROOT = C.ROOT
PKG = os.path.join(ROOT, "color-transfer_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


# ---- parse ------------------------------------------------------------------------------------------------------------------------
def test_parse_accepts_pil_files():
    from utils import png
    for frame, min_idats in ((C.structured_frame(40, 48), 1), (C.noise_frame(300, 200), 2)):
        data = C.pil_encode(frame)
        info = png.parse(data)
        assert (info.height, info.width, info.bit_depth, info.colour_type, info.interlace) == (frame.shape[0], frame.shape[1], 8, 2, 0)
        assert C.chunk_kinds(data).count(b"IDAT") >= min_idats
        assert png.device_decodable(info)
        raw = zlib.decompress(info.payload)
        assert len(raw) == frame.shape[0] * (1 + 3 * frame.shape[1])


def test_parse_refuses_broken_files():
    from utils import png
    data = C.pil_encode(C.structured_frame(40, 48))
    with pytest.raises(ValueError, match="signature"):
        png.parse(b"\x88" + data[1:])
    at = data.index(b"IDAT") + 10
    with pytest.raises(ValueError, match="CRC"):
        png.parse(data[:at] + bytes([data[at] ^ 0x40]) + data[at + 1:])
    with pytest.raises(ValueError, match="truncated"):
        png.parse(data[:len(data) // 2])
    with pytest.raises(ValueError, match="IEND"):
        png.parse(data[:-12])
    with pytest.raises(ValueError, match="IHDR"):
        png.parse(data[:8] + data[8 + 25:])


def test_other_formats_parse_but_are_not_device_decodable():
    from utils import png
    rng = np.random.default_rng(0)
    from PIL import Image
    import io
    files = {"L": C.pil_encode(rng.integers(0, 256, (9, 11), dtype=np.uint8), mode="L"),
             "RGBA": C.pil_encode(rng.integers(0, 256, (9, 11, 4), dtype=np.uint8), mode="RGBA")}
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (9, 11), dtype=np.uint8), "L").convert("P").save(buf, format="PNG")
    files["P"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 65536, (9, 11)).astype(np.uint16)).save(buf, format="PNG")
    files["16"] = buf.getvalue()
    rgb = C.pil_encode(C.structured_frame(9, 11))
    ihdr = bytearray(rgb[16:29])
    ihdr[12] = 1
    files["interlaced"] = rgb[:16] + bytes(ihdr) + struct.pack(">I", zlib.crc32(b"IHDR" + bytes(ihdr))) + rgb[33:]
    for name, data in files.items():
        info = png.parse(data)
        assert (info.height, info.width) == (9, 11), name
        assert not png.device_decodable(info), name
    assert png.parse(files["16"]).bit_depth == 16 and png.parse(files["interlaced"]).interlace == 1
    assert png.device_decodable(png.parse(rgb))


# ---- ct_inflate.h on the CPU --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_host")
    return C.build_host_program(d), d


def test_premises_of_the_corpus():
    s = C.valid_streams()
    assert [C.first_block(s[k][0])["type"] for k in ("level0", "level1", "level6", "level9", "fixed", "huffman_only", "rle")] == [0, 2, 2, 2, 1, 2, 2]
    assert len(s["stored_two_blocks"][1]) == 70000 and len(s["stored_two_blocks"][0]) == 70000 + 2 * 5 + 6
    assert b"\x00\x00\xff\xff" in s["full_flush"][0]
    stream, raw = s["match_geometry"]
    assert len(raw) == 33297 and zlib.decompress(stream) == raw
    assert C.first_block(s["repeat_symbols"][0])["repeats"] == {16, 17, 18}
    for name, (stream, raw) in s.items():
        assert zlib.decompress(stream) == raw, name
    small = C.small_streams()
    assert [C.first_block(small[k][0])["type"] for k in ("stored", "fixed", "dynamic")] == [0, 1, 2]


def test_valid_streams_match_zlib(host_program):
    exe, d = host_program
    s = C.valid_streams()
    names = sorted(s)
    got = C.run_host_program(exe, [(s[k][0], len(s[k][1])) for k in names], d)
    for name, (status, out) in zip(names, got):
        assert status == C.OK and out == s[name][1], (name, status)


def test_fifteen_bit_codes_on_the_host(host_program):
    """a dynamic header written by hand with code lengths 1 .. 15: the slow path above the primary table"""
    exe, d = host_program
    stream, raw = C.fifteen_bit_stream()
    assert C.first_block(stream)["longest"] == 15 and zlib.decompress(stream) == raw
    (status, out), = C.run_host_program(exe, [(stream, len(raw))], d)
    assert status == C.OK and out == raw


def test_status_cases_on_the_host(host_program):
    exe, d = host_program
    cases = C.status_cases()
    names = sorted(cases)
    got = C.run_host_program(exe, [(cases[k][0], cases[k][1]) for k in names], d)
    for name, (status, _) in zip(names, got):
        assert status == cases[name][2], (name, status)
    assert C.zlib_says(cases["distance"][0]) is None


def test_every_truncation_and_bit_flip(host_program):
    """the program exits 0 with some status and no sanitizer report; where the status is ok, zlib gives the same bytes"""
    exe, d = host_program
    for name, (stream, raw) in C.small_streams().items():
        inputs = [stream[:n] for n in range(len(stream))]
        for bit in range(8 * len(stream)):
            b = bytearray(stream)
            b[bit >> 3] ^= 1 << (bit & 7)
            inputs.append(bytes(b))
        got = C.run_host_program(exe, [(s, len(raw)) for s in inputs], d)
        n_ok = 0
        for s, (status, out) in zip(inputs, got):
            assert 0 <= status <= C.ADLER
            if status == C.OK:
                n_ok += 1
                assert C.zlib_says(s) == out, (name, len(s))
        assert all(status != C.OK for status, _ in got[:len(stream)]), "a truncated stream was accepted"
        print("%s: %d inputs, %d accepted (zlib agrees on each)" % (name, len(inputs), n_ok))
    # slots of every other size: too small and too large are statuses, never writes outside the slot
    stream, raw = C.small_streams()["dynamic"]
    got = C.run_host_program(exe, [(stream, n) for n in range(len(raw) + 3)], d)
    assert [st for st, _ in got] == [C.TOO_LARGE] * len(raw) + [C.OK, C.TOO_SMALL, C.TOO_SMALL]


# ---- option plumbing ----------------------------------------------------------------------------------------------------------------
def test_data_module_refuses_an_unknown_decoder():
    from utils.data import DataModule
    with pytest.raises(ValueError, match="png_decoder"):
        DataModule(png_decoder="bogus")
    assert DataModule().png_decoder == "host" and DataModule(png_decoder="device", decode_ahead=4).decode_ahead == 4


def test_cli_refuses_the_device_decoder_on_the_cpu(monkeypatch):
    from utils import cli
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    cfg = os.path.join(PKG, "configs", "others.yaml")
    for sub in ("test", "predict"):
        extra = ["--output", "unused"] if sub == "predict" else []
        with pytest.raises(SystemExit, match="--data.png_decoder device needs a GPU"):
            cli.main([sub, "--config", cfg, "--data.png_decoder", "device"] + extra)
    with pytest.raises(SystemExit, match="one of host, device"):
        cli.main(["test", "--config", cfg, "--data.png_decoder", "gpu"])


def test_binding_exports():
    import ct_hip
    assert ct_hip.CT_ABI_VERSION == 9
    for name in ("ct_png_inflate_u8", "ct_png_unfilter_u8"):
        assert name in ct_hip._core.SIGNATURES
    assert len(ct_hip.INFLATE_STATUS) == 15 and callable(ct_hip.inflate) and callable(ct_hip.png_decode)
    for bad in (None, [], [1], "x"):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.png_decode(bad)

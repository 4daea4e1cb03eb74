"""The host half of the device PNG encoder, without a GPU: utils.png (the Adler-32 combination and the container) fed with deflate
streams that zlib makes in the form the kernel emits -- Huffman only, every chunk closed by Z_SYNC_FLUSH (an empty stored block on a
byte boundary, no final block) -- on rows filtered by hand; FrameWriter's `png_encoder` option on host tensors; and the refusal of
`--writer.png_encoder device` under CT_CLI_DEVICE=cpu.  The kernel itself is tests/test_png_gpu.py."""
import os
import threading
import zlib

import numpy as np
import pytest
import torch

from tests.png_common import adler_halves, decode, filter_rows, idat_of
from tests.test_predict_host import CFG


@pytest.mark.parametrize("n,cut", [(0, 0), (1, 0), (1, 1), (10, 3), (5552, 5552), (5553, 1), (20000, 5553), (70000, 65521), (70000, 3),
                                    (200000, 65522), (200000, 0), (200000, 200000)])
def test_adler32_combine_against_zlib(n, cut):
    from utils.png import adler32_combine
    data = np.random.default_rng(n + cut).integers(0, 256, n, dtype=np.uint8).tobytes()
    x, y = data[:cut], data[cut:]
    assert adler32_combine(zlib.adler32(x), zlib.adler32(y), len(y)) == zlib.adler32(data)


def test_adler32_combine_worst_case_sums():
    """all bytes 255: the sums wrap 65521 as often as they can"""
    from utils.png import adler32_combine
    data = b"\xff" * 150000
    for cut in (1, 5552, 65521, 70001, 149999):
        assert adler32_combine(zlib.adler32(data[:cut]), zlib.adler32(data[cut:]), len(data) - cut) == zlib.adler32(data)
    a = 1                                                   # many pieces, folded left to right as assemble does
    for i in range(0, len(data), 7001):
        a = adler32_combine(a, zlib.adler32(data[i:i + 7001]), len(data[i:i + 7001]))
    assert a == zlib.adler32(data)


def _zlib_chunks(filtered, bounds):
    """the filtered bytes cut at `bounds`, each piece deflated Huffman-only and closed by Z_SYNC_FLUSH: the form the kernel emits"""
    co = zlib.compressobj(level=6, method=zlib.DEFLATED, wbits=-15, memLevel=9, strategy=zlib.Z_HUFFMAN_ONLY)
    chunks, parts = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        piece = filtered[lo:hi]
        chunks.append(co.compress(piece) + co.flush(zlib.Z_SYNC_FLUSH))
        assert chunks[-1].endswith(b"\x00\x00\xff\xff")
        parts.append(adler_halves(piece) + (len(piece),))
    return chunks, parts


@pytest.mark.parametrize("h,w,rows_per_chunk", [(1, 1, 16), (7, 13, 16), (32, 20, 8), (23, 37, 8), (40, 9, 1)])
def test_assemble_decodes_bit_for_bit(h, w, rows_per_chunk):
    from utils import png
    rng = np.random.default_rng(h * 100 + w)
    frame = (rng.integers(0, 256, (h, w, 3)) // 16 * 16 + np.arange(h)[:, None, None]).astype(np.uint8)
    types = [0 if r % 3 == 0 else 2 for r in range(h)]
    filtered = filter_rows(frame, types)
    rows = png.chunk_rows(h, rows_per_chunk)
    assert sum(rows) == h and all(0 < r <= rows_per_chunk for r in rows) and (h % rows_per_chunk == 0 or h < rows_per_chunk or rows[-1] < rows_per_chunk)
    bounds = np.concatenate([[0], np.cumsum(rows) * (1 + 3 * w)]).tolist()
    chunks, parts = _zlib_chunks(filtered, bounds)
    data = png.assemble(h, w, chunks, parts)
    assert np.array_equal(decode(data), frame)
    idat = idat_of(data)
    assert zlib.decompress(idat) == filtered                # zlib checks the combined Adler-32
    assert idat[-9:-4] == b"\x01\x00\x00\xff\xff" and data[:8] == png.SIGNATURE and data[-12:] == png.png_chunk(b"IEND", b"")
    with pytest.raises(ValueError):
        png.assemble(h, w, chunks, parts[:-1])
    with pytest.raises(ValueError):
        png.assemble(h + 1, w, chunks, parts)


def test_assemble_refuses_nothing_silently():
    """a wrong Adler-32 part gives a file that decoders refuse: the check is theirs, assemble only combines"""
    from utils import png
    frame = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    filtered = filter_rows(frame, [0, 2, 2, 0])
    chunks, parts = _zlib_chunks(filtered, [0, 32, 64])
    good = png.assemble(4, 5, chunks, parts)
    assert np.array_equal(decode(good), frame)
    bad = png.assemble(4, 5, chunks, [parts[0], (parts[1][0] ^ 1, parts[1][1], parts[1][2])])
    with pytest.raises(zlib.error):
        zlib.decompress(idat_of(bad))


def _frames(n, h, w, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def test_writer_png_encoder_option(tmp_path):
    import inspect
    from utils.writer import FrameWriter
    assert inspect.signature(FrameWriter.__init__).parameters["png_encoder"].default == "host"
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, fmt="png", png_encoder="bogus")
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, fmt="npy", png_encoder="bogus")
    assert not [t for t in threading.enumerate() if t.name.startswith("FrameWriter")]      # a refused writer starts no thread
    frames = _frames(3, 12, 20)
    for enc in ("host", "device"):                          # host tensors: the PIL path under both
        with FrameWriter(tmp_path / enc, fmt="png", png_encoder=enc) as w:
            assert w.png_encoder == enc
            assert w.submit([0, 1, 2], frames) is None
            w.submit([5], frames[:1], suffix="chess")
    names = sorted(os.listdir(tmp_path / "host"))
    assert names == ["000000.png", "000001.png", "000002.png", "000005.chess.png"] == sorted(os.listdir(tmp_path / "device"))
    for name in names:
        assert (tmp_path / "host" / name).read_bytes() == (tmp_path / "device" / name).read_bytes()
    with FrameWriter(tmp_path / "npy", fmt="npy", png_encoder="device") as w:               # other formats ignore the option
        w.submit([0], frames[:1])
    assert np.array_equal(np.load(tmp_path / "npy" / "000000.npy"), frames[0].numpy())


def test_cli_refuses_the_device_encoder_on_cpu(tmp_path, monkeypatch):
    from utils import cli
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    with pytest.raises(SystemExit) as e:
        cli.main(["predict", "--config", str(cfg), "--output", str(tmp_path / "o"), "--writer.png_encoder", "device"])
    assert "png_encoder device" in str(e.value) and "CT_CLI_DEVICE=cpu" in str(e.value)
    assert not os.path.exists(tmp_path / "o")               # before the first frame: nothing was made
    with pytest.raises(SystemExit) as e:
        cli.main(["predict", "--config", str(cfg), "--output", str(tmp_path / "o"), "--writer.png_encoder", "gpu"])
    assert "png_encoder" in str(e.value) and "host, device" in str(e.value)
    assert cli.main(["predict", "--config", str(cfg), "--output", str(tmp_path / "o"), "--writer.png_encoder", "host"]) == 7
    assert sorted(os.listdir(tmp_path / "o")) == ["%06d.png" % i for i in range(7)]


def test_png_geometry_is_the_stored_bound():
    import ct_hip
    assert ct_hip.png_geometry(1080, 1920) == (68, 16 * 5761 + 5 * 2 + 5)
    assert ct_hip.png_geometry(1, 1) == (1, 4 + 5 + 5)
    assert ct_hip.png_geometry(23, 37, 8) == (3, 8 * 112 + 5 + 5)
    assert ct_hip.png_geometry(5, 7, 100) == (1, 5 * 22 + 5 + 5)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.png_geometry(4, 4, 0)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.png_deflate(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))            # a host tensor: no CPU path

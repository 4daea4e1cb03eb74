"""ct_png_deflate_u8 (csrc/png.hip) and the device PNG encoder of FrameWriter / `utils.cli predict` on the GPU.

Two decoders that had no part in writing the encoder judge every file: PIL (pixels bit for bit; it checks the chunk CRCs) and zlib
(the filtered bytes, the Adler-32).  Around them: every slot is filled with a sentinel before the launch and must be untouched beyond
its size, every size is at most the slot's capacity, the Adler-32 parts combine to zlib's, and a frame's bytes do not depend on the
batch it is encoded in.

Compression (the gradient and the Fibonacci frame): the decompressed filtered bytes are deflated again chunk by chunk by zlib with
Z_HUFFMAN_ONLY (memLevel 9: one block per chunk up to 32 767 bytes, like the kernel).  Both emit one optimal-or-nearly-so Huffman
code per chunk; they differ in the header -- the kernel sends 1106 fixed bits (csrc/png.hip: 17 + 19 * 3 + 258 * 4, no repeat symbols),
zlib a run-length coded one -- and in how lengths above 15 bits are shortened.  A device chunk may exceed zlib's by those 1106 bits
(whole bytes: 139) plus PAYLOAD_MARGIN of zlib's size."""
import os
import zlib

import numpy as np
import pytest

from tests.png_common import decode, idat_of

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")
SENTINEL = 0xA5
HEADER_BYTES = (17 + 19 * 3 + 258 * 4 + 7) // 8
PAYLOAD_MARGIN = 0.0            # the worst ratio over these cases is 0.9976, below 1: rounded up to the next 0.5 % it leaves none


def encode(frames, rows_per_chunk=16):
    """frames: numpy uint8 [n,H,W,3] -> (files, streams, sizes, filtered bytes per frame); checks 1 - 4 of every frame on the way"""
    import ct_hip
    from utils import png
    n, h, w, _ = frames.shape
    chunks, cap = ct_hip.png_geometry(h, w, rows_per_chunk)
    dev = torch.from_numpy(frames).cuda()
    out = (torch.full((n, chunks, cap), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((n, chunks), -1, dtype=torch.int32, device="cuda"),
           torch.full((n, chunks, 2), -1, dtype=torch.int32, device="cuda"))
    got = ct_hip.png_deflate(dev, rows_per_chunk, out=out)
    assert all(a is b for a, b in zip(got, out))
    streams, sizes, adler = (t.cpu().numpy() for t in out)
    assert sizes.min() >= 1 and sizes.max() <= cap, (sizes.min(), sizes.max(), cap)
    rows = png.chunk_rows(h, rows_per_chunk)
    assert len(rows) == chunks
    files, filtered = [], []
    for f in range(n):
        for c in range(chunks):
            assert (streams[f, c, sizes[f, c]:] == SENTINEL).all(), "frame %d chunk %d wrote past its size" % (f, c)
        parts = [(int(adler[f, c, 0]), int(adler[f, c, 1]), rows[c] * (1 + 3 * w)) for c in range(chunks)]
        data = png.assemble(h, w, [streams[f, c, :sizes[f, c]].tobytes() for c in range(chunks)], parts)
        assert np.array_equal(decode(data), frames[f]), "frame %d does not decode to its pixels" % f
        raw = zlib.decompress(idat_of(data))
        assert len(raw) == h * (1 + 3 * w)
        types = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)[:, 0]
        assert types.max() <= 4
        a, at = 1, 0
        for s1, s2, nb in parts:
            assert ((s2 << 16) | s1) == zlib.adler32(raw[at:at + nb])
            a = png.adler32_combine(a, (s2 << 16) | s1, nb)
            at += nb
        assert a == zlib.adler32(raw)
        files.append(data)
        filtered.append(raw)
    return files, streams, sizes, filtered


def huffman_only_sizes(raw, bounds):
    co = zlib.compressobj(level=6, method=zlib.DEFLATED, wbits=-15, memLevel=9, strategy=zlib.Z_HUFFMAN_ONLY)
    return [len(co.compress(raw[lo:hi]) + co.flush(zlib.Z_SYNC_FLUSH)) for lo, hi in zip(bounds[:-1], bounds[1:])]


def check_compression(name, raw, sizes, h, w, rows_per_chunk):
    from utils import png
    bounds = np.concatenate([[0], np.cumsum(png.chunk_rows(h, rows_per_chunk)) * (1 + 3 * w)]).tolist()
    ref = huffman_only_sizes(raw, bounds)
    worst = 0.0
    for c, (mine, theirs) in enumerate(zip(sizes.tolist(), ref)):
        ratio = (mine - HEADER_BYTES) / theirs
        worst = max(worst, ratio)
        print("%s chunk %d: device %d bytes, zlib Z_HUFFMAN_ONLY %d, (device - %d) / zlib = %.4f" % (name, c, mine, theirs, HEADER_BYTES, ratio))
    print("%s: worst payload ratio %.4f" % (name, worst))
    for mine, theirs in zip(sizes.tolist(), ref):
        assert mine <= theirs + HEADER_BYTES + PAYLOAD_MARGIN * theirs, (name, mine, theirs)


def random_frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("n,h,w,rpc", [(1, 1, 1, 16), (1, 1, 37, 16), (1, 23, 37, 8), (1, 16, 1920, 16)])
def test_shapes_decode_bit_for_bit(n, h, w, rpc):
    rng = np.random.default_rng(h * 1000 + w)
    # a few grey levels on a vertical ramp: compressible, so the Huffman form is what these shapes run (1x1 is smaller stored)
    frames = (rng.integers(0, 4, (n, h, w, 3)) * 7 + np.arange(h)[None, :, None, None] * 3).astype(np.uint8)
    _, _, sizes, _ = encode(frames, rpc)
    import ct_hip
    _, cap = ct_hip.png_geometry(h, w, rpc)
    if h * w > 400:
        assert sizes.max() < cap - 10 - 100, "the Huffman form was expected here"


def test_frame_bytes_do_not_depend_on_the_batch():
    frames = (random_frames(3, 23, 37, 5) // 32 * 32).astype(np.uint8)
    _, streams, sizes, _ = encode(frames, 8)
    for f in range(3):
        _, s1, z1, _ = encode(frames[f:f + 1], 8)
        assert np.array_equal(z1[0], sizes[f]) and np.array_equal(s1[0], streams[f])


def test_unaligned_slots_and_views():
    """a capacity that is no multiple of 4 puts most slots off the dword grid (23x37x8: 906 bytes); and a streams view at an odd base"""
    import ct_hip
    frames = (random_frames(2, 23, 37, 6) // 64 * 64).astype(np.uint8)
    _, streams, sizes, _ = encode(frames, 8)
    chunks, cap = ct_hip.png_geometry(23, 37, 8)
    assert cap % 4 != 0
    flat = torch.full((1 + 2 * chunks * cap,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = (flat[1:].view(2, chunks, cap), torch.empty((2, chunks), dtype=torch.int32, device="cuda"), torch.empty((2, chunks, 2), dtype=torch.int32, device="cuda"))
    ct_hip.png_deflate(torch.from_numpy(frames).cuda(), 8, out=out)
    assert int(flat[0]) == SENTINEL and np.array_equal(out[1].cpu().numpy(), sizes)
    got = out[0].cpu().numpy()
    for f in range(2):
        for c in range(chunks):
            assert np.array_equal(got[f, c, :sizes[f, c]], streams[f, c, :sizes[f, c]]) and (got[f, c, sizes[f, c]:] == SENTINEL).all()


def test_constant_frame_one_literal():
    """all zeros: filter 0 everywhere, one used literal and end-of-block, one bit each"""
    frames = np.zeros((1, 40, 50, 3), dtype=np.uint8)
    _, _, sizes, filtered = encode(frames, 16)
    assert set(filtered[0]) == {0}
    # 1106 header bits + one bit per byte and end-of-block + 3, then 00 00 FF FF
    assert sizes.tolist() == [[(1106 + rows * 151 + 1 + 3 + 7) // 8 + 4 for rows in (16, 16, 8)]]
    grey = np.full((1, 20, 30, 3), 200, dtype=np.uint8)     # any other constant: Sub / Up leave zeros after the first pixel
    _, _, _, filtered = encode(grey, 16)
    assert sorted(set(filtered[0])) == [0, 1, 2, 200]


def test_random_bytes_are_stored_within_the_capacity():
    import ct_hip
    frames = random_frames(1, 48, 1500, 9)                   # 16 rows x 4501 bytes = 72 016 per chunk: two stored blocks each
    _, streams, sizes, _ = encode(frames, 16)
    _, cap = ct_hip.png_geometry(48, 1500, 16)
    assert cap == 72016 + 10 + 5
    assert sizes.tolist() == [[72016 + 10] * 3]
    assert streams[0, 0, 0] == 0 and streams[0, 0, 1:5].tolist() == [0xFF, 0xFF, 0, 0] and streams[0, 0, 65540] == 0
    small = random_frames(2, 9, 11, 10)
    encode(small, 4)


def fibonacci_frame():
    """144 rows of 66 pixels = one chunk of 28 656 filtered bytes whose 21 symbols have the counts 1, 1, 2, 3, 5, ... 10946 (an
    unlimited Huffman code would be 20 bits deep).  The counts go to the byte values 0, 1, 255, 2, 254, ... in descending order and
    the bytes are shuffled: the minimum-sum rule then keeps filter 0 on every row (differences of independent draws are larger),
    whose 144 filter-type bytes are part of the count of 0.  The test checks the histogram on the decompressed bytes."""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) == 28656 == 144 * (1 + 3 * 66)
    values = [0] + [v for k in range(1, 11) for v in (k, 256 - k)]
    counts = dict(zip(values, sorted(fib, reverse=True)))
    counts[0] -= 144
    pixels = np.concatenate([np.full(c, v, dtype=np.uint8) for v, c in counts.items()])
    np.random.default_rng(21).shuffle(pixels)
    return pixels.reshape(1, 144, 66, 3), sorted(fib)


def gradient_frame():
    y, x = np.mgrid[0:64, 0:160]
    planes = [np.round(40 + 1.1 * x + 0.6 * y + 6 * np.sin(x / 17.0) * np.cos(y / 13.0)), np.round(200 - 0.9 * x + 0.4 * y),
              np.round(20 + 0.02 * x * y + 0.7 * x)]
    return (np.stack(planes, axis=-1) % 256).astype(np.uint8)[None]


def test_fibonacci_frequencies_need_the_length_limit():
    frames, fib = fibonacci_frame()
    _, _, sizes, filtered = encode(frames, 144)
    raw = np.frombuffer(filtered[0], dtype=np.uint8)
    hist = np.bincount(raw, minlength=256)
    assert sorted(hist[hist > 0].tolist()) == fib, "the filtered bytes lost the Fibonacci skew"
    assert sizes.shape == (1, 1) and sizes[0, 0] < 28656
    check_compression("fibonacci", filtered[0], sizes[0], 144, 66, 144)


def test_gradient_compresses():
    frames = gradient_frame()
    files, _, sizes, filtered = encode(frames, 16)
    types = np.frombuffer(filtered[0], dtype=np.uint8).reshape(64, 481)[:, 0]
    print("gradient filter types:", np.bincount(types, minlength=5).tolist())
    assert (types != 0).all()                               # Sub, Up, Average or Paeth on every row
    stored = 64 * 481 + 5 * 4
    print("gradient: %d bytes of streams, %d stored, file %d" % (sizes.sum(), stored, len(files[0])))
    assert sizes.sum() < stored and len(files[0]) < stored
    check_compression("gradient", filtered[0], sizes[0], 64, 160, 16)


def test_interface():
    import ct_hip
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    streams, sizes, adler = ct_hip.png_deflate(x)
    assert tuple(streams.shape) == (2, 1, ct_hip.png_geometry(8, 8)[1]) and sizes.dtype == torch.int32 and tuple(adler.shape) == (2, 1, 2)
    for bad in (x.cpu(), x.float(), x.permute(0, 2, 1, 3)[:, :, ::2], x[..., :2], x[0]):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.png_deflate(bad)
    for rpc in (0, -1, 1.5, True):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.png_deflate(x, rpc)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.png_deflate(x, 2000)                         # above the kernel's 1024 rows per chunk: a bad return code
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.png_deflate(x, out=(streams[:, :, :-1], sizes, adler))
    lib = ct_hip.lib()
    cap = ct_hip.png_geometry(8, 8)[1]
    args = (x.data_ptr(), 2, 8, 8, 16, streams.data_ptr())
    assert lib.ct_png_slot_capacity(8, 8, 16) == cap and lib.ct_png_slot_capacity(8, 8, 1025) == 0
    assert lib.ct_png_deflate_u8(*args, cap - 1, sizes.data_ptr(), adler.data_ptr(), None) == -2
    assert lib.ct_png_deflate_u8(*args, cap, None, adler.data_ptr(), None) == -1
    assert lib.ct_png_deflate_u8(*args, cap, sizes.data_ptr() + 1, adler.data_ptr(), None) == -3


def test_frame_writer_device_encoder(tmp_path):
    """device frames through the ring: more groups than slots, a shape that grows, suffixes, the event"""
    from utils.writer import FrameWriter
    g = torch.Generator().manual_seed(0)
    small = (torch.randint(0, 256, (6, 20, 32, 3), dtype=torch.uint8, generator=g) // 32) * 32
    big = torch.randint(0, 256, (4, 40, 48, 3), dtype=torch.uint8, generator=g)
    with FrameWriter(tmp_path, fmt="png", depth=2, workers=2, png_encoder="device") as w:
        for c in range(3):
            ev = w.submit([2 * c, 2 * c + 1], small[2 * c:2 * c + 2].cuda())
            assert isinstance(ev, torch.cuda.Event)
        for c in range(2):
            w.submit([6 + 2 * c, 7 + 2 * c], big[2 * c:2 * c + 2].cuda())
        w.submit([0], small[5:6].cuda(), suffix="chess")
        w.submit([1], small[4:5], suffix="chess")            # a host tensor: the PIL path
    assert sorted(os.listdir(tmp_path)) == sorted(["%06d.png" % i for i in range(10)] + ["000000.chess.png", "000001.chess.png"])
    for i in range(10):
        data = (tmp_path / ("%06d.png" % i)).read_bytes()
        assert np.array_equal(decode(data), (small[i] if i < 6 else big[i - 6]).numpy())
        assert zlib.decompress(idat_of(data))               # one IDAT: the device encoder's file, not PIL's
    assert np.array_equal(decode((tmp_path / "000000.chess.png").read_bytes()), small[5].numpy())
    assert np.array_equal(decode((tmp_path / "000001.chess.png").read_bytes()), small[4].numpy())


def test_predict_with_the_device_encoder(tmp_path):
    from utils import cli
    args = ["predict", "--config", os.path.join(CFG, "others.yaml"), "--data.n_frames", "4", "--data.height", "270", "--data.width", "480"]
    assert cli.main(args + ["--output", str(tmp_path / "npy"), "--format", "npy", "--views", "corrected,chess"]) == 4
    assert cli.main(args + ["--output", str(tmp_path / "png"), "--writer.png_encoder", "device"]) == 4
    assert cli.main(args + ["--output", str(tmp_path / "views"), "--views", "corrected,chess", "--writer.png_encoder", "device"]) == 4
    assert sorted(os.listdir(tmp_path / "png")) == ["%06d.png" % f for f in range(4)]
    assert sorted(os.listdir(tmp_path / "views")) == sorted(n[:-3] + "png" for n in os.listdir(tmp_path / "npy"))
    assert len(os.listdir(tmp_path / "views")) == 12
    for name in os.listdir(tmp_path / "npy"):
        want = np.load(tmp_path / "npy" / name)
        data = (tmp_path / "views" / (name[:-3] + "png")).read_bytes()
        assert want.shape == (270, 480, 3) and np.array_equal(decode(data), want), name
        assert len(zlib.decompress(idat_of(data))) == 270 * (1 + 3 * 480)
    for f in range(4):
        assert (tmp_path / "png" / ("%06d.png" % f)).read_bytes() == (tmp_path / "views" / ("%06d.png" % f)).read_bytes()


def test_predict_grouped_video_with_the_device_encoder(tmp_path):
    """grouped uint8 video: one encode launch per group of 8 (11 frames: the last group ragged), against the npy run"""
    from utils import cli
    args = ["predict", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr", "--data.data_dir", "null", "--data.synthetic", "video_u8",
            "--data.n_frames", "11", "--data.height", "135", "--data.width", "240"]
    timing = {}
    assert cli.main(args + ["--output", str(tmp_path / "npy"), "--format", "npy"]) == 11
    assert cli.main(args + ["--output", str(tmp_path / "png"), "--writer.png_encoder", "device"], timing=timing) == 11
    assert timing["grouped"] is True and timing["frames_per_call"] == 8
    for f in range(11):
        assert np.array_equal(decode((tmp_path / "png" / ("%06d.png" % f)).read_bytes()), np.load(tmp_path / "npy" / ("%06d.npy" % f)))

"""ct_png_inflate_u8 / ct_png_unfilter_u8 (csrc/png_decode.hip), ct_hip.inflate / png_decode and the png_decoder="device" data path
on the GPU.  The oracles are zlib.decompress and PIL's decoder; every comparison is bitwise.  The shapes are the smallest at which
each mechanism can go wrong; the tests assert their own premise (block types, code lengths, repeat symbols, IDAT counts, which
Paeth predictor wins) before they trust a case.  Every malformed stream that runs here has passed the sanitizer build of the same
core on the CPU (tests/test_png_decode_host.py)."""
import os
import zlib

import numpy as np
import pytest

from tests import png_decode_common as C

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(C.ROOT, "color-transfer_amd", "configs")
GUARD = 0xA5
GUARD_BYTES = 64


def inflate_guarded(streams, sizes):
    """one ct_hip.inflate call (check=False) with an empty pseudo-stream and a GUARD_BYTES slot after every real one, the whole output
    prefilled with 0xA5 -> (bytes of every real slot, status of the real streams); the guards must be intact and their streams
    'input exhausted'"""
    import ct_hip
    all_streams, all_sizes = [], []
    for s, n in zip(streams, sizes):
        all_streams += [bytes(s), b""]
        all_sizes += [n, GUARD_BYTES]
    out = torch.full((sum(all_sizes),), GUARD, dtype=torch.uint8, device="cuda")
    buf, status = ct_hip.inflate(all_streams, all_sizes, check=False, out=out)
    assert buf is out
    host, status = out.cpu().numpy(), status.cpu().numpy()
    slots, at = [], 0
    for k, n in enumerate(all_sizes):
        if k % 2:
            assert (host[at:at + n] == GUARD).all(), "the guard after stream %d was written" % (k // 2)
            assert status[k] == C.INPUT_EXHAUSTED
        else:
            slots.append(host[at:at + n].tobytes())
        at += n
    return slots, status[0::2].tolist()


def test_block_types_match_geometry_and_long_codes():
    """items 1 - 3 of the corpus in ONE call: stored / fixed / dynamic first blocks, two stored blocks across 65 535, a full flush in
    the middle, the hand-written fixed block (length 258, distance 32 768, D = 1, D < L), repeat symbols 16 / 17 / 18, 15-bit codes"""
    s = C.valid_streams()
    assert [C.first_block(s[k][0])["type"] for k in ("level0", "level1", "level6", "level9", "fixed", "huffman_only", "rle")] == [0, 2, 2, 2, 1, 2, 2]
    assert len(s["match_geometry"][1]) == 33297 and zlib.decompress(s["match_geometry"][0]) == s["match_geometry"][1]
    assert C.first_block(s["repeat_symbols"][0])["repeats"] == {16, 17, 18}
    assert C.first_block(s["fifteen_bits"][0])["longest"] == 15
    names = sorted(s)
    slots, status = inflate_guarded([s[k][0] for k in names], [len(s[k][1]) for k in names])
    assert status == [0] * len(names), dict(zip(names, status))
    for name, got in zip(names, slots):
        assert got == s[name][1] == zlib.decompress(s[name][0]), name


def roundtrip_through_the_device_encoder(frame, rows_per_chunk):
    import ct_hip
    from utils import png
    h, w, _ = frame.shape
    streams, sizes, adler = (t.cpu().numpy() for t in ct_hip.png_deflate(torch.from_numpy(frame[None]).cuda(), rows_per_chunk))
    assert sizes.shape == (1, 1)
    data = png.assemble(h, w, [streams[0, 0, :sizes[0, 0]].tobytes()], [(int(adler[0, 0, 0]), int(adler[0, 0, 1]), h * (1 + 3 * w))])
    block = C.first_block(png.parse(data).payload)
    print("%d x %d through png_deflate: block type %d, longest literal code %d bits" % (h, w, block["type"], block.get("longest", 0)))
    got, = ct_hip.png_decode([data])
    assert np.array_equal(got.cpu().numpy(), frame.transpose(2, 0, 1)) and np.array_equal(C.pil_decode(data), frame.transpose(2, 0, 1))
    return block


def test_frames_of_the_device_encoder_with_long_codes():
    """this project's own encoder, decoded back on the device.  The Fibonacci-count frame of tests/test_png_gpu.py: its code was
    expected to reach 15 bits, but ct_png.h's length limiter gives it 2 .. 11 bits (measured on an MI355X and with ct_png.h on the
    CPU; the two codes cost the same), so what it holds is codes longer than the 10-bit primary table.  The 15-bit premise is kept
    by the power-of-two-count frame (and by the hand-written header `fifteen_bits` of the corpus): asserted before the case counts."""
    block = roundtrip_through_the_device_encoder(C.fibonacci_frame(), 144)
    assert block["type"] == 2 and block["longest"] > 10
    block = roundtrip_through_the_device_encoder(C.power_of_two_frame(), 7)
    assert block["type"] == 2 and block["longest"] == 15


def paeth_frame(h, w):
    """noise, so that each of the three Paeth predictors wins somewhere, with flat patches, where they tie"""
    f = C.noise_frame(h, w, 7)
    f[2:6, 3:9] = 77
    return f


def test_filters_against_pil():
    """all five types cycling from row 0, each type alone on every row (rows 0 and 1 differ in their edge rule), one to three bands
    of 64 rows, one pixel, one row, one column, a 1920-pixel row: ONE decode call for all of them"""
    import ct_hip
    cases = [("cycle", C.structured_frame(23, 37, 1), [r % 5 for r in range(23)])]
    cases += [("type%d" % t, C.structured_frame(23, 37, 2 + t) if t < 4 else paeth_frame(23, 37), [t] * 23) for t in range(5)]
    for h, w in ((1, 1), (1, 37), (37, 1), (65, 5), (129, 3), (16, 1920)):
        cases.append(("%dx%d" % (h, w), C.noise_frame(h, w, h + w) if h * w < 2000 else C.structured_frame(h, w, 3), [(r + 1) % 5 for r in range(h)]))
    # the premise of the Paeth case, counted in numpy: a, b and c each win somewhere, and there are ties
    f = paeth_frame(23, 37).astype(np.int32)
    a, b, c = f[1:, :-1], f[:-1, 1:], f[:-1, :-1]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    wins_a, wins_b = (pa <= pb) & (pa <= pc), ~((pa <= pb) & (pa <= pc)) & (pb <= pc)
    assert wins_a.sum() > 0 and wins_b.sum() > 0 and (~wins_a & ~wins_b).sum() > 0
    assert ((pa == pb) & (a != b)).sum() > 0 and ((pb == pc) & (b != c)).sum() > 0
    files = []
    for name, frame, types in cases:
        raw = C.filter_rows(frame, types)
        assert sorted(set(np.frombuffer(raw, np.uint8).reshape(frame.shape[0], -1)[:, 0].tolist())) == sorted(set(types))
        files.append(C.png_file(frame.shape[0], frame.shape[1], zlib.compress(raw, 6)))
    got = ct_hip.png_decode(files)
    for (name, frame, _), data, g in zip(cases, files, got):
        want = C.pil_decode(data)
        assert np.array_equal(want, frame.transpose(2, 0, 1)), "the hand-made filter of %s is wrong" % name
        assert g.dtype == torch.uint8 and tuple(g.shape) == want.shape and np.array_equal(g.cpu().numpy(), want), name


def test_whole_files_written_by_pil():
    import ct_hip
    from utils import png
    frame = C.structured_frame(40, 48)
    files = [C.pil_encode(frame, level) for level in (1, 6, 9)]
    for data in files:
        raw = zlib.decompress(png.parse(data).payload)
        print("PIL's filter types:", sorted(set(np.frombuffer(raw, np.uint8).reshape(40, -1)[:, 0].tolist())))
    got = ct_hip.png_decode(files)
    assert got[0].data_ptr() + 3 * 40 * 48 == got[1].data_ptr()           # equal sizes: the slices of one [n,3,H,W] tensor
    for data, g in zip(files, got):
        assert np.array_equal(g.cpu().numpy(), C.pil_decode(data))
    noise = C.pil_encode(C.noise_frame(300, 200))
    assert C.chunk_kinds(noise).count(b"IDAT") >= 2
    both = ct_hip.png_decode([noise, files[1]])                            # mixed sizes in one call
    assert np.array_equal(both[0].cpu().numpy(), C.pil_decode(noise)) and np.array_equal(both[1].cpu().numpy(), C.pil_decode(files[1]))


def test_batch_of_65_streams():
    """65 streams of mixed sizes in one call = each alone; odd byte offsets; the guards; repeated calls are bitwise equal"""
    import ct_hip
    rng = np.random.default_rng(11)
    raws, streams = [], []
    for k in range(65):
        n = int(rng.integers(1, 6000))
        raw = (rng.integers(0, 256, n, dtype=np.uint8) // (1 + k % 7) * (1 + k % 5)).astype(np.uint8).tobytes()
        raws.append(raw)
        streams.append(C.deflate(raw, (0, 1, 6, 9)[k % 4], zlib.Z_FIXED if k % 9 == 4 else zlib.Z_DEFAULT_STRATEGY))
    starts = np.cumsum([0] + [len(s) for s in streams])[:-1]
    assert (starts % 2 == 1).any() and (starts % 4 != 0).any()
    sizes = [len(r) for r in raws]
    slots, status = inflate_guarded(streams, sizes)
    assert status == [0] * 65
    for k in range(65):
        assert slots[k] == raws[k], k
    again, _ = inflate_guarded(streams, sizes)
    assert again == slots
    total, _ = ct_hip.inflate(streams, sizes)                   # no guards: the slots back to back, many off the 4-byte grid
    assert total.cpu().numpy().tobytes() == b"".join(raws)
    for k in range(0, 65, 8):
        alone, _ = ct_hip.inflate([streams[k]], [sizes[k]])
        assert alone.cpu().numpy().tobytes() == raws[k], k
    buf = torch.from_numpy(np.frombuffer(b"\x00" + b"".join(streams), dtype=np.uint8).copy()).cuda()      # every stream one byte further on
    offsets = torch.from_numpy(np.concatenate([[1], 1 + np.cumsum([len(s) for s in streams])]).astype(np.int64)).cuda()
    shifted, _ = ct_hip.inflate((buf, offsets), sizes)
    assert torch.equal(shifted, total)


def test_statuses_beside_valid_streams():
    """each malformed stream between two valid ones: its status lands on its index, the neighbours decode, the guards are intact"""
    s = C.valid_streams()
    (va, ra), (vb, rb) = s["level6"], s["fixed"]
    cases = C.status_cases()
    for name in sorted(cases):
        stream, size, want = cases[name]
        slots, status = inflate_guarded([va, stream, vb], [len(ra), size, len(rb)])
        assert status == [0, want, 0], (name, status)
        assert slots[0] == ra and slots[2] == rb, name


def test_check_raises_naming_the_index():
    import ct_hip
    s = C.valid_streams()
    (va, ra), (vb, rb) = s["level6"], s["fixed"]
    stream, size, want = C.status_cases()["adler"]
    with pytest.raises(ct_hip.CtHipError, match=r"stream 1: Adler-32 mismatch \(status %d\)" % want):
        ct_hip.inflate([va, stream, vb], [len(ra), size, len(rb)])
    # a filter-type byte of 5 in the middle file
    frame = C.structured_frame(9, 11)
    good = C.png_file(9, 11, zlib.compress(C.filter_rows(frame, [r % 5 for r in range(9)])))
    bad = C.png_file(9, 11, zlib.compress(C.filter_rows(frame, [0, 1, 5, 2, 3, 4, 0, 1, 2])))
    frames, status = ct_hip.png_decode([good, bad, good], check=False)
    assert status.cpu().tolist() == [0, C.FILTER, 0]
    assert np.array_equal(frames[0].cpu().numpy(), C.pil_decode(good)) and np.array_equal(frames[2].cpu().numpy(), C.pil_decode(good))
    with pytest.raises(ct_hip.CtHipError, match="stream 1: filter type above 4"):
        ct_hip.png_decode([good, bad, good])


def test_interface():
    import ct_hip
    lib = ct_hip.lib()
    assert lib.ct_abi_version() == 9
    stream, raw = C.valid_streams()["level6"]
    src = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    off = torch.tensor([0, len(stream), 0], dtype=torch.int64, device="cuda")
    doff = torch.tensor([0, len(raw), 0], dtype=torch.int64, device="cuda")
    dst = torch.empty(len(raw), dtype=torch.uint8, device="cuda")
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    adler = torch.zeros(2, dtype=torch.int32, device="cuda")
    dims = torch.tensor([1, 1], dtype=torch.int32, device="cuda")
    p = [t.data_ptr() for t in (src, off, dst, doff, status, adler)]
    assert lib.ct_png_inflate_u8(p[0], p[1], 1, p[2], p[3], p[4], p[5], None) == 0
    torch.cuda.synchronize()
    assert status[0].item() == 0 and adler[0].item() & 0xffffffff == zlib.adler32(raw) and dst.cpu().numpy().tobytes() == raw
    for k in range(6):
        args = list(p)
        args[k] = None
        assert lib.ct_png_inflate_u8(args[0], args[1], 1, args[2], args[3], args[4], args[5], None) == -1
    assert lib.ct_png_inflate_u8(p[0], p[1], -1, p[2], p[3], p[4], p[5], None) == -1
    assert lib.ct_png_inflate_u8(p[0], p[1] + 4, 1, p[2], p[3], p[4], p[5], None) == -3
    assert lib.ct_png_inflate_u8(p[0], p[1], 1, p[2], p[3] + 4, p[4], p[5], None) == -3
    assert lib.ct_png_inflate_u8(p[0], p[1], 1, p[2], p[3], p[4] + 2, p[5], None) == -3
    u = [p[2], p[3], dims.data_ptr(), p[2], p[3], p[4]]
    for k in range(6):
        args = list(u)
        args[k] = None
        assert lib.ct_png_unfilter_u8(args[0], args[1], args[2], 1, args[3], args[4], args[5], None) == -1
    assert lib.ct_png_unfilter_u8(u[0], u[1], u[2], 0, u[3], u[4], u[5], None) == -1
    assert lib.ct_png_unfilter_u8(u[0], u[1] + 4, u[2], 1, u[3], u[4], u[5], None) == -3
    for bad in ([stream.decode("latin1")], [src.cpu(), src], (src.float(), off), (src, off.int()), (src.cpu(), off)):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.inflate(bad, [len(raw)] * (2 if isinstance(bad, list) and len(bad) == 2 else 1))
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.inflate([stream], [len(raw), 3])
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.png_decode([C.pil_encode(np.zeros((4, 4), dtype=np.uint8), mode="L")])      # not device-decodable: no quiet fallback here


# ---- the data path ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    """the reference's layout, written by PIL; one file is RGBA and one greyscale (decoded by PIL, mixed in)"""
    from PIL import Image
    root = tmp_path_factory.mktemp("dataset")
    (root / "Test").mkdir()
    (root / "Real-World Test" / "a").mkdir(parents=True)
    for k, name in enumerate(("a_L", "a_R", "b_L", "b_R")):
        frame = C.structured_frame(40, 56, 20 + k)
        if name == "b_R":
            Image.fromarray(np.dstack([frame, np.full((40, 56), 255, np.uint8)]), "RGBA").save(root / "Test" / (name + ".png"))
        else:
            Image.fromarray(frame).save(root / "Test" / (name + ".png"))
    for k, name in enumerate(("s_L", "s_LD", "s_R")):
        frame = C.structured_frame(33, 47, 30 + k)
        if name == "s_R":
            Image.fromarray(frame[:, :, 0], "L").save(root / "Real-World Test" / "a" / (name + ".png"))
        else:
            Image.fromarray(frame).save(root / "Real-World Test" / "a" / (name + ".png"))
    return root


def same(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]) for k in a)


def test_datasets_device_equals_host(data_dir):
    from utils.data import ArtificialTestDataset, ArtificialTrainValDataset, BatchLoader, Encoded, RealWorldTestDataset, prefetch, prefetch_decoded
    device = torch.device("cuda", 0)
    host, dev = ArtificialTestDataset(data_dir / "Test"), ArtificialTestDataset(data_dir / "Test", png_decoder="device")
    frames, extra = dev.host_frames(40)
    assert isinstance(extra, Encoded) and frames["gt"].dim() == 1 and extra.dims == {"gt": (40, 56)} and frames["reference"].shape == (3, 40, 56)
    want = [host[i] for i in range(len(host))]
    assert len(dev) == 62
    for i in range(0, 62, 3):
        assert same(dev[i], want[i]), i
    for ahead in (1, 3, 16):
        got = list(prefetch_decoded(dev, range(62), device, ahead=ahead))
        assert [i for i, _ in got] == list(range(62))
        assert all(same(s, want[i]) for i, s in got), ahead
    assert all(same(s, want[i]) for i, s in prefetch(dev, [0, 33, 61], device))          # the unchanged prefetcher decodes in finish
    rw_host, rw_dev = RealWorldTestDataset(data_dir / "Real-World Test"), RealWorldTestDataset(data_dir / "Real-World Test", png_decoder="device")
    assert len(rw_dev) == 1 and same(rw_dev[0], rw_host[0])
    (i, s), = prefetch_decoded(rw_dev, [0], device)
    assert i == 0 and same(s, rw_host[0])
    # the validation set: the same draws, a batch decoded by one call
    tv = [ArtificialTrainValDataset(data_dir / "Test", (16, 24), 2, png_decoder=d) for d in ("host", "device")]
    batches = []
    for ds in tv:
        np.random.seed(3)
        torch.manual_seed(3)
        batches.append(list(BatchLoader(ds, 4).batches(range(4), device)))
    for (ids_h, b_h), (ids_d, b_d) in zip(*batches):
        assert ids_h == ids_d and same(b_h, b_d)


def test_cli_metric_table_is_bitwise_equal(data_dir):
    from utils import cli
    args = ["test", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr", "--data.data_dir", str(data_dir)]
    host = cli.main(args)
    dev = cli.main(args + ["--data.png_decoder", "device", "--data.decode_ahead", "5"])
    assert host.shape == (62, 4) and np.array_equal(host.cpu().numpy(), dev.cpu().numpy(), equal_nan=True)
    assert np.isfinite(host.cpu().numpy()[:, 0]).all()

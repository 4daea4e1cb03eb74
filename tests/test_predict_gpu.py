"""ct_pack_u8_f32 (csrc/pack.hip) and `utils.cli predict` on the GPU.  Every comparison is BITWISE.

The oracle of the pack rule is numpy: np.rint(np.clip(np.nan_to_num(x, nan=0), 0, 1).astype(float32) * float32(255)) -- ONE float32
multiplication, round to nearest with ties to even, NaN / -inf / negatives -> 0, +inf / above 1 -> 255 -- which is what
skimage.util.img_as_ubyte does to a float32 image (the reference's utils/postprocess.py:138; skimage is absent here, so parity with
the real function is unpinned and the rule is cited from its source).  The tie set (tests/test_predict_host.py) tells that rule from
round-half-up (130 of its 2 295 values differ) and from rounding the exact, fma-style product (128 differ)."""
import os

import numpy as np
import pytest

from tests.test_predict_host import oracle_u8, tie_set

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")


def _both_layouts(x_hwc):
    """x_hwc: numpy float32 [n,H,W,3] -> pack_u8 of it in both layouts against the oracle"""
    import ct_hip
    want = oracle_u8(x_hwc)
    hwc = torch.from_numpy(x_hwc).cuda()
    got = ct_hip.pack_u8(hwc, "hwc")
    assert got.dtype == torch.uint8 and tuple(got.shape) == x_hwc.shape
    bad = int((got.cpu().numpy() != want).sum())
    print("hwc %s: %d of %d bytes differ" % (x_hwc.shape, bad, want.size))
    assert bad == 0
    chw = hwc.permute(0, 3, 1, 2).contiguous()
    got = ct_hip.pack_u8(chw, "chw")
    assert tuple(got.shape) == x_hwc.shape
    bad = int((got.cpu().numpy() != want).sum())
    print("chw %s: %d of %d bytes differ" % (x_hwc.shape, bad, want.size))
    assert bad == 0


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 5, 7), (1, 33, 50), (3, 270, 480), (1, 1080, 1920)])
def test_pack_random_frames_bitwise(n, h, w):
    rng = np.random.default_rng(h * 10007 + w)
    x = (rng.random((n, h, w, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)      # some of it outside [0, 1]
    _both_layouts(x)


@pytest.mark.parametrize("h,w,offset", [(33, 50, 0), (33, 50, 7), (33, 50, 33 * 50 * 3 - 2303), (5, 7, 0), (64, 96, 4099), (31, 37, 1001)])
def test_pack_tie_set_bitwise(h, w, offset):
    """the tie set at several offsets of a frame: in the vector body, across its 16-element runs, in the element-wise tail (33x50x3 =
    4950 = 309 * 16 + 6; 31x37 planes are off the 16-byte grid, so CHW takes the per-pixel path there) and, for frames smaller than the
    set, wrapped around in pieces"""
    ties = tie_set()
    flat = np.full(h * w * 3, 0.25, dtype=np.float32)
    m = min(len(ties), len(flat) - offset)
    flat[offset:offset + m] = ties[:m]
    x = flat.reshape(1, h, w, 3)
    _both_layouts(x)
    if m < len(ties):                                   # the rest of the set, from the start of a second frame
        rest = ties[m:]
        for start in range(0, len(rest), len(flat)):
            piece = rest[start:start + len(flat)]
            flat = np.full(h * w * 3, 0.75, dtype=np.float32)
            flat[:len(piece)] = piece
            _both_layouts(flat.reshape(1, h, w, 3))


def test_pack_whole_tie_set_in_one_frame_all_alignments():
    """all 2 303 values in one frame at 16 consecutive offsets: every value meets every position of a 16-element run"""
    ties = tie_set()
    frames = []
    for offset in range(16):
        flat = np.full(40 * 24 * 3, 0.5, dtype=np.float32)
        flat[offset:offset + len(ties)] = ties
        frames.append(flat.reshape(40, 24, 3))
    _both_layouts(np.stack(frames))


def test_pack_misaligned_bases_take_the_fallback():
    """bases that are element-aligned but off the 16-byte grid (views into a larger buffer) are no error"""
    import ct_hip
    rng = np.random.default_rng(5)
    x = rng.random(3 + 2 * 16 * 24 * 3, dtype=np.float32)
    dev = torch.from_numpy(x).cuda()
    for shift in (1, 2, 3):
        v = dev[shift:shift + 2 * 16 * 24 * 3]
        want = oracle_u8(x[shift:shift + 2 * 16 * 24 * 3])
        assert np.array_equal(ct_hip.pack_u8(v.view(2, 16, 24, 3), "hwc").cpu().numpy(), want.reshape(2, 16, 24, 3))
        want_chw = want.reshape(2, 3, 16, 24).transpose(0, 2, 3, 1)
        assert np.array_equal(ct_hip.pack_u8(v.view(2, 3, 16, 24), "chw").cpu().numpy(), want_chw)
        out = torch.zeros(1 + 2 * 16 * 24 * 3, dtype=torch.uint8, device="cuda")          # an odd OUTPUT base
        ct_hip.pack_u8(dev[:2 * 16 * 24 * 3].view(2, 16, 24, 3), "hwc", out=out[1:].view(2, 16, 24, 3))
        assert np.array_equal(out[1:].cpu().numpy(), oracle_u8(x[:2 * 16 * 24 * 3])) and int(out[0]) == 0


def test_pack_interface():
    import ct_hip
    x = torch.rand(2, 3, 20, 28, device="cuda")
    out = torch.empty(2, 20, 28, 3, dtype=torch.uint8, device="cuda")
    ptr = out.data_ptr()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = ct_hip.pack_u8(x, out=out)                                                # layout inferred: chw
    assert got is out and out.data_ptr() == ptr and torch.cuda.memory_allocated() == before
    assert np.array_equal(out.cpu().numpy(), oracle_u8(x.permute(0, 2, 3, 1).cpu().numpy()))
    one = ct_hip.pack_u8(x[0].permute(1, 2, 0).contiguous())                        # one frame, hwc inferred
    assert tuple(one.shape) == (20, 28, 3) and torch.equal(one, out[0])
    assert torch.equal(ct_hip.pack_u8(x[1]), out[1])                                # one frame, chw inferred
    amb = torch.rand(3, 3, 5, 3, device="cuda")
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.pack_u8(amb)
    assert np.array_equal(ct_hip.pack_u8(amb, "hwc").cpu().numpy(), oracle_u8(amb.cpu().numpy()))
    assert np.array_equal(ct_hip.pack_u8(amb, "chw").cpu().numpy(), oracle_u8(amb.permute(0, 2, 3, 1).cpu().numpy()))
    for bad in (x.cpu(), x.double(), x.permute(0, 1, 3, 2), torch.rand(2, 4, 20, 28, device="cuda"), torch.rand(20, 28, device="cuda")):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pack_u8(bad)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.pack_u8(x, "hwc")                                                    # a layout that does not fit the shape
    for bad_out in (torch.empty(2, 20, 28, 3, dtype=torch.uint8), torch.empty(2, 20, 28, 3, device="cuda"),
                    torch.empty(2, 28, 20, 3, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pack_u8(x, out=bad_out)
    lib = ct_hip.lib()
    p = x.data_ptr()
    assert lib.ct_pack_u8_f32(p, 2, 1, 4, 4, out.data_ptr(), None) == -1            # unknown layout
    assert lib.ct_pack_u8_f32(p, 0, 0, 4, 4, out.data_ptr(), None) == -1 and lib.ct_pack_u8_f32(p, 0, 1, 4, 0, out.data_ptr(), None) == -1
    assert lib.ct_pack_u8_f32(None, 0, 1, 4, 4, out.data_ptr(), None) == -1 and lib.ct_pack_u8_f32(p, 0, 1, 4, 4, None, None) == -1
    assert lib.ct_pack_u8_f32(p + 2, 0, 1, 4, 4, out.data_ptr(), None) == -3        # CT_E_ALIGN


def test_frame_writer_downloads_device_frames(tmp_path):
    """the ring on a real stream: device frames, more groups than slots, a shape that grows, the events it hands back"""
    from utils.writer import FrameWriter
    g = torch.Generator().manual_seed(0)
    small = torch.randint(0, 256, (6, 20, 32, 3), dtype=torch.uint8, generator=g)
    big = torch.randint(0, 256, (4, 40, 48, 3), dtype=torch.uint8, generator=g)
    with FrameWriter(tmp_path, fmt="npy", depth=2, workers=2) as w:
        for c in range(3):
            ev = w.submit([2 * c, 2 * c + 1], small[2 * c:2 * c + 2].cuda())
            assert isinstance(ev, torch.cuda.Event)
        for c in range(2):
            w.submit([6 + 2 * c, 7 + 2 * c], big[2 * c:2 * c + 2].cuda())
    for i in range(6):
        assert np.array_equal(np.load(tmp_path / ("%06d.npy" % i)), small[i].numpy())
    for i in range(4):
        assert np.array_equal(np.load(tmp_path / ("%06d.npy" % (6 + i))), big[i].numpy())


def _npy_frames(d, n):
    assert sorted(f for f in os.listdir(d) if f.endswith(".npy")) == ["%06d.npy" % i for i in range(n)]
    return [np.load(os.path.join(d, "%06d.npy" % i)) for i in range(n)]


def test_predict_reinhard_npy_raw_png(tmp_path, capsys):
    import ct_hip
    from methods import Runner
    from utils import cli
    from utils.data import SyntheticStereoFrames
    args = ["--config", os.path.join(CFG, "others.yaml"), "--data.n_frames", "9", "--data.height", "64", "--data.width", "96"]
    n = cli.main(["predict"] + args + ["--output", str(tmp_path / "npy"), "--format", "npy"])
    assert n == 9
    out = capsys.readouterr().out
    assert "wrote 9 frames to %s (npy, 1 GPU)" % (tmp_path / "npy") in out
    got = _npy_frames(tmp_path / "npy", 9)
    fr, model = SyntheticStereoFrames(9, 64, 96), Runner("methods.linear.color_transfer_between_images")
    for f in range(9):
        batch = {k: v[None].cuda() for k, v in fr[f].items()}
        want = ct_hip.pack_u8(model(batch).clamp(0, 1).contiguous(), "chw")[0].cpu().numpy()
        assert got[f].shape == (64, 96, 3) and got[f].dtype == np.uint8 and np.array_equal(got[f], want)
        assert np.array_equal(want, oracle_u8(model(batch).clamp(0, 1)[0].permute(1, 2, 0).cpu().numpy()))
    # raw: one rgb24 file, frame f at offset f*H*W*3
    assert cli.main(["predict"] + args + ["--output", str(tmp_path / "raw"), "--format", "raw"]) == 9
    assert os.listdir(tmp_path / "raw") == ["frames.rgb"]
    assert (tmp_path / "raw" / "frames.rgb").read_bytes() == b"".join(a.tobytes() for a in got)
    # png (the default format): decoded, the same frames
    assert cli.main(["predict"] + args + ["--output", str(tmp_path / "png"), "--writer.workers", "2"]) == 9
    from PIL import Image
    assert sorted(os.listdir(tmp_path / "png")) == ["%06d.png" % i for i in range(9)]
    for f in range(9):
        with Image.open(tmp_path / "png" / ("%06d.png" % f)) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), got[f])
    assert cli.main(["predict"] + args + ["--output", str(tmp_path / "null"), "--format", "null"]) == 9
    assert os.listdir(tmp_path / "null") == []


def test_predict_grouped_u8_1080p(tmp_path):
    """the grouped uint8 path at the size tests/test_configs_gpu.py drives this loader: 19 frames in groups of 8 (the last one
    ragged), one reinhard_persist + one pack + one download per group"""
    import ct_hip
    from utils import cli
    from utils.data import SyntheticStereoVideoU8
    timing = {}
    n = cli.main(["predict", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr", "--data.data_dir", "null",
                  "--data.synthetic", "video_u8", "--data.n_frames", "19", "--data.height", "1080", "--data.width", "1920",
                  "--output", str(tmp_path), "--format", "npy"], timing=timing)
    assert n == 19
    assert timing["grouped"] is True and timing["frames"] == 19 and timing["frames_per_call"] == 8 and timing["seconds"] > 0
    assert timing["d2h_bytes"] == 19 * 1080 * 1920 * 3 and timing["h2d_bytes"] == 3 * timing["d2h_bytes"]
    assert sorted(os.listdir(tmp_path)) == ["%06d.npy" % i for i in range(19)]
    video = SyntheticStereoVideoU8(19, 1080, 1920, group=8)
    for first in (0, 8, 16):
        k = min(8, 19 - first)
        chunk = video.host_chunk(first).cuda()
        want = ct_hip.pack_u8(ct_hip.reinhard_persist(chunk[0, :k], chunk[1, :k], verify=True), "hwc").cpu().numpy()
        for j in range(k):
            got = np.load(tmp_path / ("%06d.npy" % (first + j)))
            assert got.shape == (1080, 1920, 3) and got.dtype == np.uint8 and np.array_equal(got, want[j]), first + j
    assert ct_hip.device_status() == 0


def test_predict_dcmcs3di(tmp_path):
    import ct_hip
    from methods.dcmcs3di import DCMCS3DI
    from utils import cli
    from utils.data import SyntheticStereoFrames
    torch.manual_seed(7)
    m = DCMCS3DI(extraction_layers=2, transfer_layers=2, channels=16).eval()
    ckpt = os.path.join(tmp_path, "dcmcs3di.ckpt")
    torch.save({"state_dict": m.state_dict()}, ckpt)
    n = cli.main(["predict", "--config", os.path.join(CFG, "dcmcs3di.yaml"), "--model.extraction_layers", "2", "--model.transfer_layers", "2",
                  "--model.channels", "16", "--ckpt_path", ckpt, "--data.n_frames", "3", "--data.height", "32", "--data.width", "48",
                  "--output", str(tmp_path / "out"), "--format", "npy"])
    assert n == 3
    got = _npy_frames(tmp_path / "out", 3)
    m = m.cuda()
    fr = SyntheticStereoFrames(3, 32, 48)
    with torch.no_grad():
        for f in range(3):
            l, r = fr[f]["target"][None].cuda(), fr[f]["reference"][None].cuda()
            want = ct_hip.pack_u8(m(l, r, inference=True)[0].contiguous(), "chw")[0].cpu().numpy()
            assert got[f].shape == (32, 48, 3) and np.array_equal(got[f], want)

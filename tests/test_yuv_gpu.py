"""GPU half of the Y'CbCr 4:2:0 path: ct_hip.yuv420_to_rgb / rgb_to_yuv420 (csrc/yuv.hip) give the BYTES of the int64 restatement
in tests/yuv_common.py -- on ragged, unaligned and vector-path shapes, on every (Y, Cb, Cr) triple and on every RGB colour -- and
the data path built on them (utils.data.StereoY4MVideo, prefetch_groups, `predict --format y4m`, utils.postprocess) moves those
bytes unchanged."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import yuv_common as yc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")
SHAPES = ((1, 1), (2, 2), (3, 5), (17, 31), (16, 64), (34, 130))       # ragged in both axes, one whole vector run, several + a tail


def _device_rows(host, stride, offset):
    """host uint8 [n, fb] -> a device view [n, fb] with row stride `stride` whose base address is `offset` bytes past an aligned
    allocation; the bytes around the frames are 0xAB"""
    n, fb = host.shape
    flat = torch.full((offset + n * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    view = flat[offset:].view(n, stride)[:, :fb]
    view.copy_(torch.from_numpy(host).cuda())
    assert view.data_ptr() % 16 == offset % 16
    return flat, view


def _device_frames(host, offset):
    """host uint8 [n,h,w,3] -> a contiguous device tensor whose base address is `offset` bytes past an aligned allocation"""
    flat = torch.empty(offset + host.size, dtype=torch.uint8, device="cuda")
    view = flat[offset:].view(host.shape)
    view.copy_(torch.from_numpy(host).cuda())
    return view


@pytest.mark.parametrize("matrix,range_,siting", yc.CONFIGS)
def test_both_directions_equal_the_oracle_on_small_shapes(matrix, range_, siting):
    """(1,1) .. (34,130), n = 1 and 5, dense frames, a stride larger than the frame, bases one byte off the 16-byte grid: the
    byte-wise, the mixed and the all-vector paths"""
    import ct_hip
    rng = np.random.default_rng(7 + yc.CONFIGS.index((matrix, range_, siting)))
    kw = dict(matrix=matrix, range=range_, siting=siting)
    for h, w in SHAPES:
        fb = yc.frame_bytes(h, w)
        assert ct_hip.yuv420_frame_bytes(h, w) == fb
        for n, pad, offset in ((1, 0, 0), (5, 0, 0), (5, 16, 0), (5, 7, 1), (1, 0, 1)):
            yuv = yc.random_yuv(rng, n, h, w)
            _, rows = _device_rows(yuv, fb + pad, offset)
            want = yc.decode_oracle(yuv, h, w, matrix, range_, siting)
            got = ct_hip.yuv420_to_rgb(rows, h, w, **kw)
            assert got.shape == (n, h, w, 3) and got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), want), ("decode", h, w, n, pad, offset)
            out = _device_frames(np.zeros((n, h, w, 3), np.uint8), offset)             # an output off the grid as well
            assert ct_hip.yuv420_to_rgb(rows, h, w, out=out, **kw) is out and np.array_equal(out.cpu().numpy(), want)
            rgb = yc.random_rgb(rng, n, h, w)
            want_yuv = yc.encode_oracle(rgb, matrix, range_, siting)
            flat, dst = _device_rows(np.full((n, fb), 0xAB, np.uint8), fb + pad, offset)
            ct_hip.rgb_to_yuv420(_device_frames(rgb, offset), out=dst, **kw)
            assert np.array_equal(dst.cpu().numpy(), want_yuv), ("encode", h, w, n, pad, offset)
            around = flat[offset:].view(n, fb + pad)[:, fb:]
            assert bool((around == 0xAB).all()) and bool((flat[:offset] == 0xAB).all())   # nothing outside the frames is written
        one = ct_hip.yuv420_to_rgb(torch.from_numpy(yuv[0]).cuda(), h, w, **kw)            # one frame as a 1-D tensor
        assert one.shape == (1, h, w, 3) and np.array_equal(one.cpu().numpy()[0], want[0])


def test_binding_argument_checks_and_float_frames():
    import ct_hip
    rng = np.random.default_rng(3)
    h, w = 6, 10
    fb = yc.frame_bytes(h, w)
    yuv = torch.from_numpy(yc.random_yuv(rng, 2, h, w)).cuda()
    for bad in (lambda: ct_hip.yuv420_to_rgb(yuv, h, w + 1), lambda: ct_hip.yuv420_to_rgb(yuv.int(), h, w),
                lambda: ct_hip.yuv420_to_rgb(yuv.view(2, fb // 2, 2)[:, :, 0], h // 2, w), lambda: ct_hip.yuv420_to_rgb(yuv, h, w, range="tv"),
                lambda: ct_hip.yuv420_to_rgb(yuv, h, w, siting="top"), lambda: ct_hip.yuv420_to_rgb(yuv, h, w, out=torch.empty((2, h, w, 3), device="cuda")),
                lambda: ct_hip.yuv420_to_rgb(yuv, h, w, out=torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")),
                lambda: ct_hip.rgb_to_yuv420(torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")),
                lambda: ct_hip.rgb_to_yuv420(torch.zeros((2, h, w, 3), dtype=torch.float64, device="cuda")),
                lambda: ct_hip.rgb_to_yuv420(torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda"), out=torch.empty((2, fb - 1), dtype=torch.uint8, device="cuda")),
                lambda: ct_hip.rgb_to_yuv420(torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda"), out=torch.empty((3, fb), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ct_hip.CtHipError):
            bad()
    # float32 frames are encoded as the bytes pack_u8 makes of them, in either layout
    x = torch.from_numpy(rng.random((2, h, w, 3), dtype=np.float32) * 1.2 - 0.1).cuda()
    want = yc.encode_oracle(ct_hip.pack_u8(x, "hwc").cpu().numpy(), "bt709", "limited", "center")
    assert np.array_equal(ct_hip.rgb_to_yuv420(x).cpu().numpy(), want)
    assert np.array_equal(ct_hip.rgb_to_yuv420(x.permute(0, 3, 1, 2).contiguous()).cpu().numpy(), want)


@pytest.mark.parametrize("matrix,range_,siting", [("bt601", "limited", "center"), ("bt601", "full", "left"), ("bt709", "limited", "left"),
                                                  ("bt709", "full", "center")])
def test_decode_of_every_yuv_triple(matrix, range_, siting):
    """two 4096 x 4096 frames (yuv_common.triple_frames): every (Y, Cb, Cr) with unblended chroma, the whole frames compared"""
    import ct_hip
    frames = yc.triple_frames()
    dev = torch.from_numpy(frames).cuda()
    for f in range(2):
        got = ct_hip.yuv420_to_rgb(dev[f:f + 1], 4096, 4096, matrix=matrix, range=range_, siting=siting).cpu().numpy()
        want = yc.decode_oracle(frames[f:f + 1], 4096, 4096, matrix, range_, siting)
        assert np.array_equal(got, want), f
    both = ct_hip.yuv420_to_rgb(dev, 4096, 4096, matrix=matrix, range=range_, siting=siting)       # frame 1 through the stride, too
    assert np.array_equal(both[1].cpu().numpy(), want[0])


@pytest.mark.parametrize("matrix,range_", [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")])
def test_encode_of_every_colour(matrix, range_):
    """all 2^24 colours as constant 2 x 2 blocks (centre siting: the block is the chroma footprint), compared per colour with the
    oracle's encode of that colour"""
    import ct_hip
    for r0 in range(0, 256, 64):
        blocks, colours = yc.colour_cube_blocks(r0, r0 + 64)                          # [64, 512, 512, 3]
        got = ct_hip.rgb_to_yuv420(torch.from_numpy(blocks).cuda(), matrix=matrix, range=range_, siting="center").cpu().numpy()
        want = yc.encode_oracle(colours.reshape(-1, 1, 1, 3), matrix, range_, "center").reshape(64, 256, 256, 3)
        y, cb, cr = got[:, :512 * 512].reshape(64, 256, 2, 256, 2), got[:, 512 * 512:512 * 512 + 65536], got[:, 512 * 512 + 65536:]
        assert np.array_equal(y, np.broadcast_to(want[:, :, None, :, None, 0], y.shape)), r0
        assert np.array_equal(cb.reshape(64, 256, 256), want[..., 1]) and np.array_equal(cr.reshape(64, 256, 256), want[..., 2]), r0


# ---- the data path -------------------------------------------------------------------------------------------------------------------
N, H, W, G = 19, 24, 40, 8
KW = dict(matrix="bt709", range="limited", siting="left")


@pytest.fixture(scope="module")
def triple(tmp_path_factory):
    """a 19-frame 24 x 40 Y4M triple (C420mpeg2, no XCOLORRANGE: limited), smooth enough for a colour transfer to make sense, and
    the oracle's RGB of it [3, 19, 24, 40, 3]; the gt file has one frame more (the length is the shortest file's)"""
    d = tmp_path_factory.mktemp("y4m")
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    yuv = np.empty((3, N + 1, yc.frame_bytes(H, W)), dtype=np.uint8)
    for r in range(3):
        for f in range(N + 1):
            luma = 110 + 70 * np.sin(xx / 7.0 + f * 0.3 + r) * np.cos(yy / 5.0) + rng.integers(-9, 10, (H, W))
            cb = 128 + 40 * np.cos(xx[::2, ::2] / 9.0 + r) + rng.integers(-5, 6, (H // 2, W // 2))
            cr = 128 + 30 * np.sin(yy[::2, ::2] / 6.0 + f * 0.2) + rng.integers(-5, 6, (H // 2, W // 2))
            yuv[r, f] = np.concatenate([np.clip(p, 0, 255).astype(np.uint8).reshape(-1) for p in (luma, cb, cr)])
    paths = {}
    for r, role in enumerate(("target", "reference", "gt")):
        paths[role] = str(d / (role + ".y4m"))
        yc.write_y4m(paths[role], yuv[r, :N + 1 if role == "gt" else N], W, H, tag="C420mpeg2", extra="")
    rgb = np.stack([yc.decode_oracle(yuv[r, :N], H, W, **{"range_" if k == "range" else k: v for k, v in KW.items()}) for r in range(3)])
    return paths, rgb


def _data_args(paths, gt=True):
    args = ["--data.data_dir", "null", "--data.y4m_target", paths["target"], "--data.y4m_reference", paths["reference"], "--data.group", str(G)]
    return args + (["--data.y4m_gt", paths["gt"]] if gt else [])


def test_y4m_video_groups_equal_the_oracle(triple):
    from utils.data import StereoY4MVideo, prefetch_groups
    paths, rgb = triple
    video = StereoY4MVideo(paths["target"], paths["reference"], paths["gt"], group=G)
    assert (len(video), video.height, video.width, video.group, video.siting, video.range, video.matrix) == (N, H, W, G, "left", "limited", "bt709")
    assert video.has_gt and video.upload_bytes_per_frame == 3 * yc.frame_bytes(H, W)
    chunk = video.host_chunk(16)
    assert tuple(chunk.shape) == (3, G, yc.frame_bytes(H, W)) and chunk.dtype == torch.uint8 and chunk.is_pinned()
    seen = []
    for ids, dev in prefetch_groups(video, range(N), torch.device("cuda", 0)):
        assert tuple(dev.shape) == (3, len(ids), H, W, 3) and dev.dtype == torch.uint8
        assert np.array_equal(dev.cpu().numpy(), rgb[:, ids]), ids
        seen += list(ids)
    assert seen == list(range(N))                                                   # 8 + 8 + 3: the last chunk is ragged
    strided = list(range(1, N, 2))                                                  # the frames of rank 1 of 2
    for ids, dev in prefetch_groups(video, strided, torch.device("cuda", 0)):
        assert np.array_equal(dev.cpu().numpy(), rgb[:, ids]), ids
    sample = video[5]                                                               # single frames: float32(byte) / 255, CHW
    for r, role in enumerate(("target", "reference", "gt")):
        assert sample[role].dtype == torch.float32 and sample[role].is_cuda
        assert torch.equal(sample[role].cpu(), torch.from_numpy(rgb[r, 5]).permute(2, 0, 1).float() / 255)
    with pytest.raises(ValueError):
        StereoY4MVideo(paths["target"], paths["reference"], paths["gt"], range="tv")


class _OracleVideo:
    """the oracle's RGB frames as a video_u8-style dataset: pinned [3][group][H][W][3] chunks of consecutive frames"""
    roles = ("target", "reference", "gt")

    def __init__(self, rgb, group):
        self.rgb, self.group = rgb, group
        self.n_frames, self.height, self.width = rgb.shape[1:4]

    def __len__(self):
        return self.n_frames

    def host_chunk(self, first_frame):
        chunk = np.zeros((3, self.group) + self.rgb.shape[2:], dtype=np.uint8)
        k = min(self.group, self.n_frames - first_frame)
        chunk[:, :k] = self.rgb[:, first_frame:first_frame + k]
        return torch.from_numpy(chunk).pin_memory()


def test_cli_test_on_y4m_equals_the_run_on_the_oracles_rgb(triple, monkeypatch, capsys):
    from utils import cli
    import utils.data as data
    paths, rgb = triple
    base = ["test", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr"]
    timing = {}
    table = cli.main(base + _data_args(paths), timing=timing)
    assert timing["grouped"] is True and timing["frames_per_call"] == G and timing["h2d_bytes"] == N * 3 * yc.frame_bytes(H, W)
    assert tuple(table.shape) == (N, 4) and bool(torch.isfinite(table[:, 0]).all())

    class Module:
        def __init__(self, **_):
            self.dataset = _OracleVideo(rgb, G)

        def test_dataloader(self):
            return [self.dataset]
    monkeypatch.setattr(data, "DataModule", Module)
    want = cli.main(base + ["--data.data_dir", "null"])
    assert torch.equal(table[:, 0], want[:, 0])
    assert "(%d frames, 1 GPU)" % N in capsys.readouterr().out


def _predict(paths, out, fmt, extra=()):
    from utils import cli
    return cli.main(["predict", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr"] + _data_args(paths) + list(extra)
                    + ["--output", str(out), "--format", fmt])


def test_predict_y4m_equals_the_encode_of_the_npy_bytes(triple, tmp_path):
    from utils import y4m
    paths, _ = triple
    timing = {}
    from utils import cli
    assert cli.main(["predict", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr"] + _data_args(paths)
                    + ["--output", str(tmp_path / "y4m"), "--format", "y4m"], timing=timing) == N
    assert timing["grouped"] is True and timing["d2h_bytes"] == N * yc.frame_bytes(H, W) and timing["h2d_bytes"] == 3 * timing["d2h_bytes"]
    assert _predict(paths, tmp_path / "npy", "npy") == N
    assert os.listdir(tmp_path / "y4m") == ["frames.y4m"]
    head, offsets = y4m.frame_offsets(str(tmp_path / "y4m" / "frames.y4m"))
    # rate, aspect, siting and range are the input's (F25:1 A1:1 C420mpeg2, limited)
    assert (head.width, head.height, head.fps, head.aspect, head.siting, head.color_range, len(offsets)) == (W, H, "25:1", "1:1", "left", "limited", N)
    data = (tmp_path / "y4m" / "frames.y4m").read_bytes()
    fb = yc.frame_bytes(H, W)
    assert len(data) == head.header_len + N * (6 + fb)
    for f, o in enumerate(offsets):
        frame = np.load(tmp_path / "npy" / ("%06d.npy" % f))
        want = yc.encode_oracle(frame[None], "bt709", "limited", "left")[0]
        assert np.array_equal(np.frombuffer(data[o:o + fb], dtype=np.uint8), want), f
    # the command line's rate wins over the input's
    assert _predict(paths, tmp_path / "fps", "y4m", ["--writer.y4m_fps", "30000:1001"]) == N
    other = (tmp_path / "fps" / "frames.y4m").read_bytes()
    assert y4m.parse_header(other).fps == "30000:1001" and other[y4m.parse_header(other).header_len:] == data[head.header_len:]


def test_sharded_writers_leave_the_file_of_one_writer(tmp_path):
    """two FrameWriters with the frames of rank 0 and of rank 1 of 2 (each writes only its own frames, the header comes from
    truncate_y4m once): the file of one writer with all frames"""
    import ct_hip
    from utils.writer import FrameWriter, truncate_y4m
    rng = np.random.default_rng(5)
    rgb = yc.random_rgb(rng, 7, 17, 31)
    dev = torch.from_numpy(rgb).cuda()
    opts = {"fps": "24:1", "matrix": "bt601", "range": "full", "siting": "center"}
    for name, shards in (("one", [list(range(7))]), ("two", [[0, 2, 4, 6], [1, 3, 5]])):
        truncate_y4m(tmp_path / name, 17, 31, opts)
        for ids in shards:
            with FrameWriter(tmp_path / name, fmt="y4m", depth=2, workers=2, n_frames=7, y4m=opts) as w:
                for c in range(0, len(ids), 3):
                    w.submit(ids[c:c + 3], dev[ids[c:c + 3]])
    one = (tmp_path / "one" / "frames.y4m").read_bytes()
    assert one == (tmp_path / "two" / "frames.y4m").read_bytes()
    from utils import y4m
    head, offsets = y4m.frame_offsets(str(tmp_path / "one" / "frames.y4m"))
    want = yc.encode_oracle(rgb, "bt601", "full", "center")
    fb = yc.frame_bytes(17, 31)
    assert (head.fps, head.siting, head.color_range) == ("24:1", "center", "full") and len(offsets) == 7
    assert all(np.array_equal(np.frombuffer(one[o:o + fb], dtype=np.uint8), want[f]) for f, o in enumerate(offsets))
    assert ct_hip.device_status() == 0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(rank, world, port, paths, out_dir):
    for p in (ROOT, os.path.join(ROOT, "color-transfer_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "LOCAL_WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    assert _predict(paths, os.path.join(out_dir, "world%d" % world), "y4m") == N


def test_predict_y4m_world1_and_world2_write_the_same_file(triple, tmp_path):
    """two ranks need two GPUs (one process drives one GPU here); the sharded writing itself is
    test_sharded_writers_leave_the_file_of_one_writer"""
    if torch.cuda.device_count() < 2:
        pytest.skip("world size 2 needs two GPUs; %d visible" % torch.cuda.device_count())
    paths, _ = triple
    mp.spawn(_run, args=(1, _free_port(), paths, str(tmp_path)), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), paths, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "world1" / "frames.y4m").read_bytes() == (tmp_path / "world2" / "frames.y4m").read_bytes()


def test_without_gt_predict_runs_and_test_is_refused(triple, tmp_path):
    from utils import cli
    from utils.data import StereoY4MVideo
    paths, rgb = triple
    video = StereoY4MVideo(paths["target"], paths["reference"], group=G)
    assert not video.has_gt and video.roles == ("target", "reference") and tuple(video.host_chunk(0).shape) == (2, G, yc.frame_bytes(H, W))
    assert video.upload_bytes_per_frame == 2 * yc.frame_bytes(H, W)                 # no third upload
    sample = video[3]
    assert torch.equal(sample["gt"], sample["target"])                              # the gt role is the target's frame
    base = ["--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr"] + _data_args(paths, gt=False)
    with pytest.raises(SystemExit) as e:
        cli.main(["test"] + base)
    assert "y4m_gt" in str(e.value)
    assert cli.main(["predict"] + base + ["--output", str(tmp_path / "a"), "--format", "npy"]) == N
    assert _predict(paths, tmp_path / "b", "npy") == N                              # the same frames as with a gt stream
    for f in range(N):
        assert (tmp_path / "a" / ("%06d.npy" % f)).read_bytes() == (tmp_path / "b" / ("%06d.npy" % f)).read_bytes()


def test_synthetic_video_yuv_runs_grouped(tmp_path):
    """--data.synthetic video_yuv: the grouped route on I420 chunks; the table equals the one of its decoded chunks as a
    video_u8-style dataset would give (checked through the chunks' oracle RGB and Runner.test_group)"""
    import ct_hip
    from methods import Runner
    from utils import cli
    from utils.data import SyntheticStereoVideoYUV
    timing = {}
    table = cli.main(["test", "--config", os.path.join(CFG, "others.yaml"), "--model.metrics", "psnr", "--data.data_dir", "null",
                      "--data.synthetic", "video_yuv", "--data.n_frames", "11", "--data.height", "18", "--data.width", "34", "--data.group", "4"],
                     timing=timing)
    assert timing["grouped"] is True and timing["h2d_bytes"] == 11 * 3 * yc.frame_bytes(18, 34)
    video = SyntheticStereoVideoYUV(11, 18, 34, group=4)
    runner = Runner("methods.linear.color_transfer_between_images", metrics="psnr")
    for first in (0, 4, 8):
        k = min(4, 11 - first)
        chunk = video.host_chunk(first).numpy()
        rgb = np.stack([yc.decode_oracle(chunk[r, :k], 18, 34, "bt709", "limited", "center") for r in range(3)])
        rec = torch.zeros((k, 2), dtype=torch.float64, device="cuda")
        runner.test_group(torch.from_numpy(rgb).cuda(), rec)
        assert torch.equal(table[first:first + k, 0].cpu(), rec[:, 1].cpu())
    assert ct_hip.device_status() == 0


def test_postprocess_takes_y4m_streams(triple, tmp_path):
    """list_streams / load_frames: left.y4m, left_gt.y4m, right.y4m in a sample directory next to PNG folders"""
    from PIL import Image
    from utils import postprocess as pp
    paths, rgb = triple
    sample = tmp_path / "s"
    os.makedirs(sample / "right")
    os.link(paths["target"], sample / "left.y4m")
    os.link(paths["gt"], sample / "left_gt.y4m")
    for f in range(3):
        Image.fromarray(rgb[1, f]).save(sample / "right" / ("%04d.png" % f))
    names = pp.list_streams(str(sample))
    assert len(names["left"]) == N and len(names["left_gt"]) == N + 1 and names["right"] == ["%04d.png" % f for f in range(3)]
    picks = [pp.frame_source(str(sample), "left", names["left"][f]) for f in (0, 7, 18)]
    got = pp.load_frames(picks, "cuda")
    # utils.postprocess reads the siting from the header (left) and defaults to bt709 / limited
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), rgb[0, [0, 7, 18]])
    right = pp.load_frames([pp.frame_source(str(sample), "right", n) for n in names["right"]], "cuda")
    assert np.array_equal(right.cpu().numpy(), rgb[1, :3])

"""The host half of `utils.cli predict`, without a GPU: utils.writer.FrameWriter on host uint8 tensors (formats, back-pressure,
frame-index naming, the raw video file, error propagation, thread lifetime), the CPU-mode quantisation against the numpy oracle of
the pack rule, and `utils.cli predict` end to end under CT_CLI_DEVICE=cpu with world 1 and world 2 (gloo), which must leave the
same files.  The device half (ct_pack_u8_f32, the download ring on a real stream) is tests/test_predict_gpu.py."""
import os
import socket
import sys
import threading

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the 7-frame 24x40 stub configuration of tests/test_cli_gloo.py
CFG = """
model:
  class_path: tests.cli_stub.StubRunner
  init_args:
    func_spec: tests.cli_stub.swap_means
data:
  init_args:
    n_frames: 7
    height: 24
    width: 40
trainer:
  logger: false
"""


def oracle_u8(x):
    """q = rint(clamp(x, 0, 1) * 255) with ONE float32 multiplication, ties to even, NaN -> 0 (skimage's img_as_ubyte on a float32
    image restated: np.multiply(image, 255, dtype=float32), np.rint, np.clip; the clip comes first here, which changes nothing)"""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.clip(np.nan_to_num(x, nan=0.0), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)


def tie_set():
    """for k = 0..254 the float32 nearest (k + 0.5) / 255 and its four neighbours on each side (2 295 values: 256 of them give an
    exact .5 after the float32 multiplication, where round-half-up and rounding the exact product both differ from the rule), plus
    the special values"""
    centre = ((np.arange(255, dtype=np.float64) + 0.5) / 255).astype(np.float32)
    vals = [centre]
    lo = hi = centre
    for _ in range(4):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        vals += [lo, hi]
    special = np.array([-0.0, -1e-7, 1 + 1e-7, np.inf, -np.inf, np.nan, 0.5, np.finfo(np.float32).smallest_subnormal], dtype=np.float32)
    return np.concatenate(vals + [special]).astype(np.float32)


def _frames(n, h, w, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def _writer_threads():
    return [t for t in threading.enumerate() if t.name.startswith("FrameWriter")]


def test_tie_set_separates_the_roundings():
    """the oracle's own sanity: the set does tell round-half-even of the float32 product from its two neighbours"""
    x = tie_set()[:2295]
    p32 = x * np.float32(255)
    assert int((p32 - np.floor(p32) == 0.5).sum()) == 256
    half_up = np.floor(p32 + np.float32(0.5)).astype(np.uint8)
    exact = np.rint(x.astype(np.float64) * 255).astype(np.uint8)
    want = oracle_u8(x)
    assert int((half_up != want).sum()) == 130 and int((exact != want).sum()) == 128
    assert len(set(np.floor(p32[p32 - np.floor(p32) == 0.5]).tolist())) == 255          # a tie between every pair of neighbouring levels


def test_cpu_mode_quantisation_equals_the_oracle():
    from utils import cli
    x = tie_set()
    assert np.array_equal(cli.quantise_u8(torch.from_numpy(x)).numpy(), oracle_u8(x))
    r = np.random.default_rng(3).random(5000).astype(np.float32) * 1.5 - 0.25
    assert np.array_equal(cli.quantise_u8(torch.from_numpy(r)).numpy(), oracle_u8(r))


@pytest.mark.parametrize("fmt", ["png", "npy", "raw"])
def test_writer_reads_back_what_was_submitted(tmp_path, fmt):
    from utils.writer import FrameWriter
    frames = _frames(5, 12, 20)
    with FrameWriter(tmp_path / "out", fmt=fmt, n_frames=5) as w:
        assert w.submit([0, 1], frames[:2]) is None              # host tensors: no download, no event
        w.submit([2, 3, 4], frames[2:])
    assert not _writer_threads()
    out = tmp_path / "out"
    if fmt == "raw":
        data = np.fromfile(out / "frames.rgb", dtype=np.uint8)
        assert data.size == 5 * 12 * 20 * 3 and np.array_equal(data.reshape(5, 12, 20, 3), frames.numpy())
    else:
        assert sorted(os.listdir(out)) == ["%06d.%s" % (i, fmt) for i in range(5)]
        for i in range(5):
            if fmt == "png":
                from PIL import Image
                with Image.open(out / ("%06d.png" % i)) as im:
                    assert im.mode == "RGB"
                    got = np.asarray(im)
            else:
                got = np.load(out / ("%06d.npy" % i))
            assert got.dtype == np.uint8 and np.array_equal(got, frames[i].numpy())


def test_writer_back_pressure_ten_frames_through_two_slots(tmp_path):
    from utils.writer import FrameWriter
    frames = _frames(10, 16, 24, seed=1)
    w = FrameWriter(tmp_path, fmt="npy", depth=2, workers=2)
    for i in range(10):
        w.submit([i], frames[i:i + 1])
        assert sum(1 for s in w._slots if s.pending) <= 2           # never more than `depth` groups in flight
    w.close()
    w.close()                                                       # a second close is a no-op
    for i in range(10):
        assert np.array_equal(np.load(tmp_path / ("%06d.npy" % i)), frames[i].numpy())
    assert not _writer_threads()
    with pytest.raises(RuntimeError):
        w.submit([0], frames[:1])


def test_writer_names_files_by_frame_index_in_any_order(tmp_path):
    from utils.writer import FrameWriter
    frames = _frames(6, 8, 8, seed=2)
    order = [4, 0, 5, 2, 1, 3]
    with FrameWriter(tmp_path / "npy", fmt="npy", depth=2, workers=3) as w:
        w.submit(order[:3], frames[order[:3]])
        w.submit(order[3:], frames[order[3:]])
    for i in range(6):
        assert np.array_equal(np.load(tmp_path / "npy" / ("%06d.npy" % i)), frames[i].numpy())
    # raw: frame f at offset f*H*W*3 whatever the order, a frame nobody wrote reads as zeros, the size is the whole video's
    with FrameWriter(tmp_path / "raw", fmt="raw", n_frames=7, workers=2) as w:
        w.submit(order[:3], frames[order[:3]])
        w.submit(order[3:], frames[order[3:]])
    data = np.fromfile(tmp_path / "raw" / "frames.rgb", dtype=np.uint8)
    assert data.size == 7 * 8 * 8 * 3
    data = data.reshape(7, 8, 8, 3)
    assert np.array_equal(data[:6], frames.numpy()) and not data[6].any()


def test_writer_raw_rules(tmp_path):
    from utils.writer import FrameWriter
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, fmt="raw")                            # n_frames is required
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, fmt="jpeg")
    w = FrameWriter(tmp_path, fmt="raw", n_frames=4)
    w.submit([0], _frames(1, 8, 8))
    with pytest.raises(ValueError):
        w.submit([1], _frames(1, 8, 10))                            # a second frame size
    with pytest.raises(ValueError):
        w.submit([4], _frames(1, 8, 8))                             # past the end of the video
    w.close()
    assert not _writer_threads()


def test_writer_workers_are_capped(tmp_path):
    from utils.writer import FrameWriter
    w = FrameWriter(tmp_path, fmt="null", workers=1000)
    try:
        assert len(_writer_threads()) == 16
    finally:
        w.close()
    assert not _writer_threads()
    with pytest.raises(ValueError):
        FrameWriter(tmp_path, fmt="null", workers=0)


def test_writer_error_surfaces_from_close(tmp_path):
    from utils.writer import FrameWriter
    blocker = tmp_path / "a_file"
    blocker.write_text("not a directory")
    w = FrameWriter(blocker / "below", fmt="npy", depth=2)
    w.submit([0], _frames(1, 8, 8))
    with pytest.raises(OSError):
        w.close()
    assert not _writer_threads()
    # ... or from the next submit, whichever comes first; close() then has nothing left to raise but still joins
    w = FrameWriter(blocker / "below", fmt="png", depth=1)
    w.submit([0], _frames(1, 8, 8))
    with pytest.raises(OSError):
        for i in range(1, 50):
            w.submit([i], _frames(1, 8, 8))
    w.close()
    assert not _writer_threads()


# ---- utils.cli predict under CT_CLI_DEVICE=cpu ---------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(rank, world, port, cfg_path, out_dir, fmt):
    for p in (ROOT, os.path.join(ROOT, "color-transfer_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "LOCAL_WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CT_CLI_DEVICE": "cpu"})
    from utils import cli
    log = open(os.path.join(out_dir, "stdout_%d_of_%d.txt" % (rank, world)), "w")
    old = sys.stdout
    sys.stdout = log
    try:
        n = cli.main(["predict", "--config", cfg_path, "--model.gain", "0.75", "--output", os.path.join(out_dir, "world%d" % world),
                      "--format", fmt, "--writer.depth", "2", "--writer.workers", "2"])
    finally:
        sys.stdout = old
        log.close()
    assert n == 7


def test_predict_world2_writes_the_files_of_world1(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    mp.spawn(_run, args=(1, _free_port(), str(cfg), str(tmp_path), "npy"), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), str(cfg), str(tmp_path), "npy"), nprocs=2, join=True)
    names = ["%06d.npy" % i for i in range(7)]
    assert sorted(os.listdir(tmp_path / "world1")) == names and sorted(os.listdir(tmp_path / "world2")) == names
    from tests.cli_stub import StubRunner
    from utils.data import SyntheticStereoFrames
    frames, model = SyntheticStereoFrames(7, 24, 40), StubRunner(gain=0.75)
    for f, name in enumerate(names):
        one = (tmp_path / "world1" / name).read_bytes()
        assert one == (tmp_path / "world2" / name).read_bytes()                      # byte-identical files
        batch = {k: v.unsqueeze(0) for k, v in frames[f].items()}
        want = oracle_u8(model(batch).clamp(0, 1)[0].permute(1, 2, 0).numpy())
        got = np.load(tmp_path / "world1" / name)
        assert got.shape == (24, 40, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    out1 = (tmp_path / "stdout_0_of_1.txt").read_text()
    out2 = (tmp_path / "stdout_0_of_2.txt").read_text()
    assert (tmp_path / "stdout_1_of_2.txt").read_text() == ""                         # only rank 0 prints
    assert "wrote 7 frames" in out1 and "(npy, 1 GPU)" in out1
    assert "wrote 7 frames" in out2 and "(npy, 2 GPUs)" in out2


def test_predict_raw_from_two_ranks_is_one_video(tmp_path):
    """all ranks write into the one frames.rgb; it equals the single-rank file"""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    mp.spawn(_run, args=(1, _free_port(), str(cfg), str(tmp_path), "raw"), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), str(cfg), str(tmp_path), "raw"), nprocs=2, join=True)
    one = (tmp_path / "world1" / "frames.rgb").read_bytes()
    assert len(one) == 7 * 24 * 40 * 3 and one == (tmp_path / "world2" / "frames.rgb").read_bytes()


def test_predict_argument_errors(tmp_path):
    from utils import cli
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    with pytest.raises(SystemExit) as e:
        cli.main(["predict", "--config", str(cfg)])
    assert "--output" in str(e.value)
    with pytest.raises(SystemExit):
        cli.main(["predict", "--config", str(cfg), "--output", str(tmp_path / "o"), "--format", "jpeg"])
    with pytest.raises(SystemExit) as e:
        cli.main(["validate"])
    assert "predict" in str(e.value) and "test" in str(e.value)

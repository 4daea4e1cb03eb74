"""The diagnostic views without a GPU: the numpy restatements of tests/views_common.py pinned to the reference's own outputs
(tests/golden/views.npz, made by tests/golden/make_golden_views.py), the ABI, `utils.cli predict --views` under CT_CLI_DEVICE=cpu
with world 1 and world 2 (gloo), and FrameWriter's name suffix.  The kernels themselves are tests/test_views_gpu.py."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import views_common as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.fixture(scope="module")
def golden():
    return np.load(vc.GOLDEN)


# ---- 1. the restatements against the reference's outputs -----------------------------------------------------------------------
def test_golden_inputs_are_the_ones_the_reference_saw(golden):
    assert vc.digest(*vc.chess_inputs()) == str(golden["chess/in_sha1"])
    assert vc.digest(*vc.rgbmse_inputs()) == str(golden["rgbmse/in_sha1"])
    for case in vc.FLOW_CASES:
        assert vc.digest(vc.flow_input(case)) == str(golden["flow/%s/in_sha1" % case])


@pytest.mark.parametrize("size", [25, 7])
def test_chess_mix_restatement_is_bitwise_the_reference(golden, size):
    x, y = vc.chess_inputs()
    got = vc.chess_mix_ref(x, y, size)
    assert got.dtype == np.float32 and np.array_equal(got, golden["chess/out_%d" % size].astype(np.float32))
    assert (got >= 0).any() and (got < 0).any()                     # both sources show


def test_rgbmse_restatement_is_bitwise_the_reference(golden):
    """torch's channel mean adds the three channels in their order and divides by 3: equality, not a tolerance"""
    x, y = vc.rgbmse_inputs()
    got = vc.rgbmse_ref(x, y)
    want = golden["rgbmse/out_ch0"]
    print("rgbmse restatement vs reference: max abs diff %g" % float(np.abs(got[:, 0] - want).max()))
    assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32)) and not got[:, 1:].any()
    for b in range(2):                                              # every frame spans exactly [0, 1] on its own
        assert got[b, 0].min() == 0 and got[b, 0].max() == 1


@pytest.mark.parametrize("case", vc.FLOW_CASES)
def test_flow_image_restatement_is_bitwise_the_reference(golden, case):
    flow = vc.flow_input(case)
    kept = flow.copy()
    got = vc.flow_to_image_ref(flow)
    assert np.array_equal(flow, kept, equal_nan=True)               # the restatement leaves its argument alone
    assert got.dtype == np.uint8 and np.array_equal(got, golden["flow/%s/out" % case])
    if case == "zero":
        assert (got == 255).all()
    if case == "unknown":
        assert not got[5, 7].any() and got.reshape(-1, 3).any(axis=1).sum() == got.shape[0] * got.shape[1] - 1
    # how far the last bit of the inputs moves the reference itself: under 0.1 % of the pixels
    assert float(golden["flow/%s/perturbed_share" % case]) < 1e-3


def test_flow_image_nan_counts_as_unknown():
    flow = vc.flow_input("amp20")
    flow[1, 3, 4] = np.nan
    img = vc.flow_to_image_ref(flow)
    clean = flow.copy()
    clean[:, 3, 4] = 0
    want = vc.flow_to_image_ref(clean)
    want[3, 4] = 0
    assert np.array_equal(img, want) and not img[3, 4].any()


def test_flow_image_in_float32_stays_inside_the_device_gate(golden):
    """numpy < 2 kept the reference's normalisation, radius, angle and fk in float32.  That arithmetic meets the gate the device
    kernel is held to: off the knife edges at most one grey level, on at most 0.5 % of the pixels."""
    for case in vc.FLOW_CASES:
        flow = vc.flow_input(case)
        worst, share = vc.flow_gate(vc.flow_to_image_ref(flow, dtype=np.float32), golden["flow/%s/out" % case], flow)
        print("%s: float32 arithmetic off the knife edges: worst %d levels, share %.2e" % (case, worst, share))
        assert worst <= 1 and share <= 0.005


# ---- 2. the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_stays_9_and_the_library_exports_the_view_entries():
    import ct_hip
    assert re.search(r"#define CT_ABI_VERSION 9\b", open(os.path.join(ROOT, "include", "ct_hip.h")).read())
    lib = ctypes.CDLL(ct_hip.LIB_PATH)
    for name in ("ct_view_chess_mix_f32", "ct_view_scaled_plane_f32", "ct_view_workspace_bytes", "ct_flow_to_image_u8"):
        assert hasattr(lib, name) and name in ct_hip.SIGNATURES
    assert ct_hip.lib().ct_abi_version() == 9
    assert ct_hip.lib().ct_view_workspace_bytes(3) >= 3 * 8 and ct_hip.lib().ct_view_workspace_bytes(0) == 0
    # argument errors come back as codes, before anything is launched (no GPU here)
    assert ct_hip.lib().ct_view_chess_mix_f32(None, None, None, 1, 3, 4, 4, 25, None) == -1
    assert ct_hip.lib().ct_view_scaled_plane_f32(None, None, None, None, 0, 1, 4, 4, 0, None) == -1
    assert ct_hip.lib().ct_flow_to_image_u8(None, None, None, 0, 1, 4, 4, None) == -1
    for fn in (ct_hip.chess_mix, ct_hip.rgbmse_view):
        with pytest.raises(ct_hip.CtHipError):
            fn(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))                 # host tensors: no CPU path
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.gray_view(torch.zeros(1, 1, 4, 4))
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.flow_to_image(torch.zeros(1, 2, 4, 4))


def test_drop_in_names():
    from utils import flow_viz, visualizations as viz
    for name in ("chess_mix", "minmaxscale", "rgbmse"):
        assert callable(getattr(viz, name))
    for name in ("labmse", "abmse", "rgbssim"):
        with pytest.raises(NotImplementedError) as e:
            getattr(viz, name)(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
        assert "kornia" in str(e.value)
    assert callable(flow_viz.flow_tensor_to_image) and callable(flow_viz.flow_to_image)


def test_view_selection_rules():
    from methods import select_views
    offered = ("corrected", "chess", "rgbmse", "disparity")
    assert select_views(offered, None, True) == offered
    assert select_views(offered, None, False) == ("corrected", "disparity")
    assert select_views(offered, "disparity, corrected", False) == ("disparity", "corrected")
    with pytest.raises(ValueError) as e:
        select_views(offered, ("flow",), True)
    assert "flow" in str(e.value)
    with pytest.raises(ValueError) as e:
        select_views(offered, ("chess",), False)
    assert "gt" in str(e.value)


# ---- 3. predict --views under CT_CLI_DEVICE=cpu ------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(rank, world, port, cfg_path, out_dir, fmt, views):
    for p in (ROOT, os.path.join(ROOT, "color-transfer_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "LOCAL_WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CT_CLI_DEVICE": "cpu"})
    from utils import cli
    argv = ["predict", "--config", cfg_path, "--model.gain", "0.75", "--output", out_dir, "--format", fmt, "--writer.depth", "2",
            "--writer.workers", "2"] + (["--views", views] if views else [])
    sys.stdout = open(os.devnull, "w")
    assert cli.main(argv) == 7


def test_predict_views_world2_writes_the_files_of_world1(tmp_path):
    from tests.cli_stub import StubRunner
    from utils import cli
    from utils.data import SyntheticStereoFrames
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    mp.spawn(_run, args=(1, _free_port(), str(cfg), str(tmp_path / "plain"), "npy", None), nprocs=1, join=True)
    mp.spawn(_run, args=(1, _free_port(), str(cfg), str(tmp_path / "world1"), "npy", "chess,rgbmse"), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), str(cfg), str(tmp_path / "world2"), "npy", "chess,rgbmse"), nprocs=2, join=True)
    plain = ["%06d.npy" % i for i in range(7)]
    names = sorted(plain + ["%06d.%s.npy" % (i, v) for i in range(7) for v in ("chess", "rgbmse")])
    assert sorted(os.listdir(tmp_path / "plain")) == plain                           # without --views: the files of today
    assert sorted(os.listdir(tmp_path / "world1")) == names and sorted(os.listdir(tmp_path / "world2")) == names
    frames, model = SyntheticStereoFrames(7, 24, 40), StubRunner(gain=0.75)
    for name in names:
        assert (tmp_path / "world1" / name).read_bytes() == (tmp_path / "world2" / name).read_bytes()
    for f in range(7):
        assert (tmp_path / "plain" / plain[f]).read_bytes() == (tmp_path / "world1" / plain[f]).read_bytes()
        batch = {k: v.unsqueeze(0) for k, v in frames[f].items()}
        corrected, gt = model(batch).clamp(0, 1).numpy(), batch["gt"].numpy()
        for view, want in (("chess", vc.chess_mix_ref(gt, corrected, 25)), ("rgbmse", vc.rgbmse_ref(gt, corrected))):
            got = np.load(tmp_path / "world1" / ("%06d.%s.npy" % (f, view)))
            want_u8 = cli.quantise_u8(torch.from_numpy(want))[0].permute(1, 2, 0).numpy()
            assert got.shape == (24, 40, 3) and got.dtype == np.uint8 and np.array_equal(got, want_u8)
        assert np.load(tmp_path / "world1" / ("%06d.rgbmse.npy" % f))[..., 0].max() == 255


def test_predict_views_argument_errors(tmp_path, monkeypatch):
    from utils import cli
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    base = ["predict", "--config", str(cfg), "--output", str(tmp_path / "o")]
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--format", "raw", "--views", "chess"])
    assert "raw" in str(e.value) and "--views" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--views", "chess,heatmap"])
    assert "unknown view" in str(e.value) and "heatmap" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--views", "chess,disparity"])
    assert "StubRunner" in str(e.value) and "disparity" in str(e.value) and "does not offer" in str(e.value)
    assert not os.path.exists(tmp_path / "o")                                        # refused before the first frame


# ---- 4. FrameWriter's suffix ----------------------------------------------------------------------------------------------------
def _frames(n, h, w, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def test_writer_suffix_names_the_file_and_shares_the_ring(tmp_path):
    from utils.writer import FrameWriter, frame_name
    assert frame_name(3, "png") == "000003.png" and frame_name(3, "png", "chess") == "000003.chess.png"
    plain, extra = _frames(6, 8, 12), _frames(6, 8, 12, seed=1)
    with FrameWriter(tmp_path / "o", fmt="npy", depth=2, workers=2) as w:
        for i in range(6):                                          # six frames, twelve submissions, two slots
            w.submit([i], plain[i:i + 1])
            w.submit([i], extra[i:i + 1], suffix="chess")
            assert sum(1 for s in w._slots if s.pending) <= 2
    assert sorted(os.listdir(tmp_path / "o")) == sorted(["%06d.npy" % i for i in range(6)] + ["%06d.chess.npy" % i for i in range(6)])
    for i in range(6):
        assert np.array_equal(np.load(tmp_path / "o" / ("%06d.npy" % i)), plain[i].numpy())
        assert np.array_equal(np.load(tmp_path / "o" / ("%06d.chess.npy" % i)), extra[i].numpy())
    with FrameWriter(tmp_path / "p", fmt="png") as w:
        w.submit([2], plain[:1], suffix="rgbmse")
    assert os.listdir(tmp_path / "p") == ["000002.rgbmse.png"]


def _closing(writer):
    """close the writer whatever the body does: its worker threads are not daemons, a writer left open would keep the test
    process alive after the last test"""
    import contextlib

    @contextlib.contextmanager
    def cm():
        try:
            yield writer
        finally:
            try:
                writer.close()
            except OSError:
                pass
    return cm()


def test_writer_suffix_rules_and_errors(tmp_path):
    import threading
    from utils.writer import FrameWriter
    with _closing(FrameWriter(tmp_path, fmt="raw", n_frames=2)) as w:
        with pytest.raises(ValueError):
            w.submit([0], _frames(1, 8, 8), suffix="chess")         # a raw video is one file
    with _closing(FrameWriter(tmp_path, fmt="npy")) as w:
        for bad in ("", "a/b", "a.b", 3):
            with pytest.raises(ValueError):
                w.submit([0], _frames(1, 8, 8), suffix=bad)
    blocker = tmp_path / "a_file"
    blocker.write_text("not a directory")
    with _closing(FrameWriter(blocker / "below", fmt="npy", depth=2)) as w:
        w.submit([0], _frames(1, 8, 8), suffix="chess")
        with pytest.raises(OSError):
            w.close()                                               # the failed suffixed write surfaces here
    assert not [t for t in threading.enumerate() if t.name.startswith("FrameWriter")]

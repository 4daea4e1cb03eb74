"""Host half of the bicubic resampling (csrc/resize.hip, ct_hip.bicubic_resize): the shape / scale rule of ct_hip.resize_geometry
against torch.nn.functional.interpolate on the CPU, the argument checks, the header entry, and the `inference` section of utils.cli
under CT_CLI_DEVICE=cpu with a stub model (world sizes 1 and 2 leave the same files).  No GPU.  The device half is
tests/test_resize_gpu.py."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ct_hip.h")

SIZES = [(1, 1), (3, 5), (7, 4), (17, 33), (31, 37), (135, 241), (273, 481), (1079, 1917), (1080, 1920)]
FACTORS = [0.75, 0.5, 0.6, 1 / 3, 1.5]


@pytest.mark.parametrize("h,w", SIZES)
def test_geometry_scale_factor_gives_the_shape_of_interpolate(h, w):
    import ct_hip
    x = torch.zeros(1, 1, h, w)
    for f in FACTORS + [(0.75, 0.5), (1.5, 1 / 3), 2, 2.0]:
        fh, fw = f if isinstance(f, tuple) else (f, f)
        if int(h * fh) < 1 or int(w * fw) < 1:
            with pytest.raises(ct_hip.CtHipError):
                ct_hip.resize_geometry((h, w), scale_factor=f)
            continue
        want = tuple(F.interpolate(x, scale_factor=f if isinstance(f, tuple) else float(f), mode="bicubic").shape[2:])
        (ho, wo), (sh, sw) = ct_hip.resize_geometry((h, w), scale_factor=f)
        assert (ho, wo) == want, (h, w, f)
        assert isinstance(ho, int) and isinstance(wo, int) and isinstance(sh, float) and isinstance(sw, float)
        assert sh == 1.0 / fh and sw == 1.0 / fw                     # the factor itself, not in / out


@pytest.mark.parametrize("h,w", SIZES)
def test_geometry_size_both_ways(h, w):
    import ct_hip
    for f in FACTORS:
        lo = (max(1, int(h * f)), max(1, int(w * f)))
        for src, dst in (((h, w), lo), (lo, (h, w))):                # down to the reduced size, and back up to the original
            (ho, wo), (sh, sw) = ct_hip.resize_geometry(src, size=dst)
            assert (ho, wo) == dst == tuple(F.interpolate(torch.zeros(1, 1, *src), size=dst, mode="bicubic").shape[2:])
            assert sh == src[0] / dst[0] and sw == src[1] / dst[1]   # in / out, in float64
    assert ct_hip.resize_geometry((h, w), size=7) == ((7, 7), (h / 7, w / 7))
    assert ct_hip.resize_geometry([h, w], size=[3, 9]) == ((3, 9), (h / 3, w / 9))


def test_geometry_bad_arguments_raise():
    import ct_hip
    bad = [dict(), dict(size=(4, 4), scale_factor=0.5), dict(size=(0, 4)), dict(size=(4, -1)), dict(size=(4.0, 4)), dict(size=(4, 4, 4)),
           dict(size="44"), dict(scale_factor=0), dict(scale_factor=-0.5), dict(scale_factor=float("nan")), dict(scale_factor=float("inf")),
           dict(scale_factor=(0.5, 0.5, 0.5)), dict(scale_factor="0.5"), dict(scale_factor=True), dict(scale_factor=0.01)]
    for kw in bad:
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.resize_geometry((8, 8), **kw)
    for in_hw in ((0, 8), (8,), (8.0, 8), 8.5):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.resize_geometry(in_hw, size=(4, 4))


def test_bicubic_resize_has_no_cpu_path():
    import ct_hip
    for bad in (torch.zeros(3, 8, 8), np.zeros((1, 3, 8, 8), np.float32)):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.bicubic_resize(bad, scale_factor=0.5)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.bicubic_resize(torch.zeros(1, 3, 8, 8), size=(4, 4), scale_factor=0.5)
    if not torch.cuda.is_available():
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.bicubic_resize(torch.zeros(1, 3, 8, 8), scale_factor=0.5)
        from methods.dcmcs3di import DCMCS3DI
        with pytest.raises(ct_hip.CtHipError):
            DCMCS3DI(extraction_layers=1, transfer_layers=1).forward_scaled(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_header_declares_the_entries():
    import ct_hip
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+ct_bicubic_resize_f32\s*\(([^)]*)\)", code)
    assert m, "include/ct_hip.h does not declare ct_bicubic_resize_f32"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(ct_hip.SIGNATURES["ct_bicubic_resize_f32"][1]) == 13
    assert sum(a.startswith("double") for a in args) == 2            # the two source steps travel as float64
    assert re.search(r"size_t\s+ct_bicubic_resize_workspace_bytes\s*\(", code)
    assert "ct_bicubic_resize_workspace_bytes" in ct_hip.SIGNATURES
    assert re.search(r"#define CT_ABI_VERSION 9\b", src)             # entries were only added
    lib = ct_hip.lib()
    assert lib.ct_bicubic_resize_workspace_bytes(6, 1080, 1440, 0) == 0
    assert lib.ct_bicubic_resize_workspace_bytes(6, 1080, 1440, 1) == 6 * 1080 * 1440 * 4
    # argument checks come before anything touches a device
    assert lib.ct_bicubic_resize_f32(None, None, 1, 4, 4, 2, 2, 2.0, 2.0, 0, None, 0, None) == -1
    assert lib.ct_bicubic_resize_f32(16, 32, 1, 4, 4, 0, 2, 2.0, 2.0, 0, None, 0, None) == -1
    assert lib.ct_bicubic_resize_f32(16, 32, 1, 4, 4, 2, 2, 0.0, 2.0, 0, None, 0, None) == -1
    assert lib.ct_bicubic_resize_f32(16, 32, 1, 4, 4, 2, 2, 2.0, float("nan"), 0, None, 0, None) == -1
    assert lib.ct_bicubic_resize_f32(18, 32, 1, 4, 4, 2, 2, 2.0, 2.0, 0, None, 0, None) == -3
    assert lib.ct_bicubic_resize_f32(16, 32, 1, 4, 4, 2, 2, 2.0, 2.0, 1, None, 0, None) == -2          # antialias without its workspace
    assert lib.ct_bicubic_resize_f32(16, 32, 1, 400, 400, 2, 2, 200.0, 200.0, 1, 64, 1 << 20, None) == -1   # beyond 128 taps


# ---- utils.cli `inference` section under CT_CLI_DEVICE=cpu -------------------------------------------------------------------------
class ScaledStub(torch.nn.Module):
    """a CNN-style module (no test_step) whose forward_scaled is torch on the CPU: the CLI's host logic only"""

    def __init__(self, gain=1.0):
        super().__init__()
        self.gain = gain

    def forward(self, target, reference, inference=False):
        return (target * self.gain + 0.1 * reference), None

    def forward_scaled(self, target, reference, scale_factor=0.75, antialias=False):
        h, w = target.shape[2:]
        lo = [F.interpolate(t, scale_factor=scale_factor, mode="bicubic", antialias=antialias) for t in (target, reference)]
        return F.interpolate(self.forward(*lo)[0], size=(h, w), mode="bicubic", antialias=antialias), None


CFG = """
model:
  class_path: tests.test_resize_host.ScaledStub
  init_args:
    gain: 0.9
data:
  init_args:
    n_frames: 5
    height: 24
    width: 40
inference:
  scale_factor: 0.75
"""


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(rank, world, port, cfg_path, out_dir):
    for p in (ROOT, os.path.join(ROOT, "color-transfer_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "LOCAL_WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CT_CLI_DEVICE": "cpu"})
    from utils import cli
    old = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        n = cli.main(["predict", "--config", cfg_path, "--output", os.path.join(out_dir, "world%d" % world), "--format", "npy"])
    finally:
        sys.stdout.close()
        sys.stdout = old
    assert n == 5


def test_cli_inference_section_world1_and_world2(tmp_path):
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    mp.spawn(_run, args=(1, _free_port(), str(cfg), str(tmp_path)), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), str(cfg), str(tmp_path)), nprocs=2, join=True)
    from utils.cli import quantise_u8
    from utils.data import SyntheticStereoFrames
    frames, model = SyntheticStereoFrames(5, 24, 40), ScaledStub(gain=0.9)
    for f in range(5):
        name = "%06d.npy" % f
        assert (tmp_path / "world1" / name).read_bytes() == (tmp_path / "world2" / name).read_bytes()
        full = model.forward_scaled(frames[f]["target"][None], frames[f]["reference"][None], scale_factor=0.75)[0]
        plain = model(frames[f]["target"][None], frames[f]["reference"][None])[0]
        got = np.load(tmp_path / "world1" / name)
        assert got.shape == (24, 40, 3) and np.array_equal(got, quantise_u8(full)[0].permute(1, 2, 0).numpy())
        assert not np.array_equal(got, quantise_u8(plain)[0].permute(1, 2, 0).numpy())          # the section is not ignored


def test_cli_inference_section_errors(tmp_path, monkeypatch):
    from utils import cli
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    for extra in (["--inference.scale_factor", "0"], ["--inference.scale_factor", "half"], ["--inference.antialias", "3"],
                  ["--inference.factor", "0.5"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["predict", "--config", str(cfg), "--output", str(tmp_path / "o"), "--format", "null"] + extra)
        assert "inference" in str(e.value)
    # a model without forward_scaled is refused with a message that names the section and the model
    stub = tmp_path / "stub.yaml"
    stub.write_text(CFG.replace("tests.test_resize_host.ScaledStub", "tests.cli_stub.StubRunner").replace("gain: 0.9", "gain: 0.75"))
    for sub in (["test"], ["predict", "--output", str(tmp_path / "o"), "--format", "null"]):
        with pytest.raises(SystemExit) as e:
            cli.main(sub[:1] + ["--config", str(stub)] + sub[1:])
        assert "forward_scaled" in str(e.value) and "inference" in str(e.value) and "StubRunner" in str(e.value)

"""iCID with the reference's full signature, without a GPU: the restatement of tests/icid_options_common.py against oracle.metrics
at the defaults and against runs of the reference's own utils/icid.py for all twelve option combinations
(tests/golden/icid_options.npz), and the argument checks of the public interface that need no device."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
from oracle import metrics as om     # noqa: E402
from tests import icid_options_common as ic     # noqa: E402

REINHARD_SPEC = "methods.linear.color_transfer_between_images"


@pytest.fixture(scope="module")
def frames(golden_dir):
    return ic.golden_frames(golden_dir)


def test_restatement_is_the_oracle_at_the_defaults(frames):
    for tag in "abcd":
        x, y = frames[tag]
        for dtype in (torch.float64, torch.float32):
            assert torch.equal(ic.icid(x, y, dtype=dtype), om.icid(x, y, dtype=dtype)), (tag, dtype)


def test_restatement_vs_reference_runs(frames, golden_dir):
    g = ic.golden_values(golden_dir)
    distinct = set()
    for tag, (x, y) in frames.items():
        for (intent, omit, down), idx in ic.COMBOS:
            want64, want32 = float(g[tag + "/f64"][idx]), float(g[tag + "/f32"][idx])
            assert abs(float(ic.icid(x, y, intent, omit, down)) - want64) <= 1e-10, (tag, intent, omit, down)
            assert abs(float(ic.icid(x, y, intent, omit, down, dtype=torch.float32)) - want32) <= 5e-6, (tag, intent, omit, down)
            assert abs(want32 - want64) <= 5e-6
            distinct.add((tag, round(want64, 4)))
        # the fixture tells the options apart: f = 1 (a, b, batch) leaves six values per pair, f > 1 (c, d) twelve
        assert len([1 for t, _ in distinct if t == tag]) == (12 if tag in "cd" else 6), tag
    # the batch value is the mean of its frames' values: what utils.icid.icid returns from the per-frame kernel
    assert abs(g["batch/frames_f64"].mean(0) - g["batch/f64"]).max() < 1e-14


def test_bad_intent_is_refused_without_a_device():
    from methods import Runner, icid as methods_icid
    from utils.icid import icid
    x = torch.rand(1, 3, 8, 8)
    for call in (lambda: icid(x, x, intent="saturation"), lambda: icid(x[0], x[0], "Perceptual"),
                 lambda: methods_icid(x, x, intent="saturation"), lambda: Runner(REINHARD_SPEC, icid_intent="saturation"),
                 lambda: Runner(REINHARD_SPEC, icid_intent=None)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == ic.BAD_INTENT
    with pytest.raises(ValueError) as e:
        ic.icid(x, x, intent="saturation")
    assert str(e.value) == ic.BAD_INTENT


def test_host_tensors_are_refused_by_name():
    import ct_hip
    from utils.icid import icid
    x = torch.rand(1, 3, 8, 8)
    for kw in ({}, {"intent": "chromatic", "downsampling": False}):
        with pytest.raises(ct_hip.CtHipError, match="device tensors"):
            icid(x, x, **kw)


def test_signature_is_the_reference_s():
    import inspect
    from utils.icid import icid
    sig = inspect.signature(icid)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("img1", inspect.Parameter.empty), ("img2", inspect.Parameter.empty), ("intent", "perceptual"), ("omit_maps67", False),
        ("downsampling", True)]


def test_runner_stores_the_options():
    from methods import Runner
    r = Runner(REINHARD_SPEC)
    assert (r.icid_intent, r.icid_omit_maps67, r.icid_downsampling) == ("perceptual", False, True)
    r = Runner(REINHARD_SPEC, icid_intent="hue-preserving", icid_omit_maps67=True, icid_downsampling=False)
    assert (r.icid_intent, r.icid_omit_maps67, r.icid_downsampling) == ("hue-preserving", True, False)
    assert r._icid_options() == {"intent": "hue-preserving", "omit_maps67": True, "downsampling": False}


def test_cli_flags_reach_the_runner():
    """`--model.icid_intent chromatic --model.icid_omit_maps67 true --model.icid_downsampling false` as utils.cli turns them into
    the model's constructor arguments; a bad intent is refused when the model is built"""
    from utils import cli
    cfg = {"model": {"class_path": "methods.Runner", "init_args": {"func_spec": REINHARD_SPEC}}}
    for key, value in (("icid_intent", "hue-preserving"), ("icid_omit_maps67", "true"), ("icid_downsampling", "false")):
        cli._set(cfg, "model." + key, value)
    model = cli._instantiate(cfg["model"])
    assert (model.icid_intent, model.icid_omit_maps67, model.icid_downsampling) == ("hue-preserving", True, False)
    cli._set(cfg, "model.icid_intent", "hue")
    with pytest.raises(ValueError) as e:
        cli._instantiate(cfg["model"])
    assert str(e.value) == ic.BAD_INTENT


def test_workspace_of_the_full_size_grid():
    """ct_icid_workspace_bytes: one float64 per 32 x 16 tile of the map grid + 64; with downsampling it fits the metric workspace,
    without it it outgrows that from min(H, W) = 384 on.  The entries refuse bad arguments before they touch a device."""
    import ct_hip
    lib = ct_hip.lib()
    for b, h, w in ((1, 6, 6), (2, 37, 53), (1, 383, 500), (1, 385, 387), (1, 640, 644), (16, 1080, 1920)):
        f = om.metric_factor(h, w)
        tiles = lambda hh, ww: ((ww + 31) // 32) * ((hh + 15) // 16)      # noqa: E731
        assert lib.ct_icid_workspace_bytes(h, w, b, 0) == tiles(h, w) * b * 8 + 64
        assert lib.ct_icid_workspace_bytes(h, w, b, 1) == tiles(h // f, w // f) * b * 8 + 64 <= lib.ct_metric_workspace_bytes(h, w, b)
        assert (lib.ct_icid_workspace_bytes(h, w, b, 0) > lib.ct_metric_workspace_bytes(h, w, b)) == (min(h, w) >= 384)
    assert lib.ct_icid_workspace_bytes(0, 8, 1, 0) == 0
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for entry in (lib.ct_frame_icid_opt_f32, lib.ct_frame_icid_opt_hwc_u8):
        assert entry(p, p, 40, 40, 1, 3, 0, 1, p, p, 1 << 20, None) == -1           # intent outside 0..2
        assert entry(p, p, 40, 40, 1, -1, 0, 1, p, p, 1 << 20, None) == -1
        assert entry(p, p, 5, 9, 1, 0, 0, 0, p, p, 1 << 20, None) == -1             # a grid below 6 x 6
        assert entry(p, p, 385, 387, 1, 2, 1, 0, p, p, lib.ct_metric_workspace_bytes(385, 387, 1), None) == -2
        assert entry(p, p, 385, 387, 0, 2, 1, 0, p, p, 0, None) == 0                # batch == 0: nothing to do
        assert entry(None, p, 40, 40, 1, 0, 0, 1, p, p, 1 << 20, None) == -1


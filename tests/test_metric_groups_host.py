"""CPU-only checks of the metric entries on frame groups: the declarations of include/ct_hip.h and the exports of the built library,
which func_specs `metric_groups` sends through whole groups of uint8 frames, the argument errors of the binding, and
`utils.cli test --model.metric_groups true` under CT_CLI_DEVICE=cpu.  The kernels are tests/test_metric_groups_gpu.py."""
import ctypes
import itertools
import re

import pytest

from tests.metric_groups_common import ACG_SPEC, IDT_SPEC, MK_SPEC, NEW_ENTRIES, REINHARD_SPEC, SPECS, XIAO_SPEC
from tests.test_abi_and_host import HEADER, header_functions

torch = pytest.importorskip("torch")


def test_header_declares_and_library_exports_the_entries():
    import ct_hip
    declared = header_functions()
    handle = ctypes.CDLL(ct_hip.LIB_PATH)
    for name, n_args in NEW_ENTRIES.items():
        assert name in declared, "include/ct_hip.h does not declare %s" % name
        assert name in ct_hip.SIGNATURES and len(ct_hip.SIGNATURES[name][1]) == n_args
        planar = name.replace("_hwc_u8", "_f32")
        assert ct_hip.SIGNATURES[name] == ct_hip.SIGNATURES[planar]                  # the planar entry's argument list
        assert hasattr(handle, name), "libct_hip.so does not export %s" % name
    assert re.search(r"#define CT_ABI_VERSION 9\b", open(HEADER).read())             # entries were only added
    assert ct_hip.lib().ct_abi_version() == 9
    assert callable(ct_hip.frame_ssim_hwc) and callable(ct_hip.frame_icid_hwc) and callable(ct_hip.frame_fsim_hwc)


def parent_takes_groups(spec, metrics, byte_groups, iterative_groups, grading_groups):
    """Runner.takes_groups() as it was before `metric_groups`, written out"""
    if metrics not in ("psnr", ("psnr",)):
        return False
    if spec == IDT_SPEC:
        return iterative_groups
    if spec == ACG_SPEC:
        return grading_groups
    return spec == REINHARD_SPEC or (byte_groups and spec in (MK_SPEC, XIAO_SPEC))


@pytest.mark.parametrize("spec", SPECS)
def test_takes_groups_truth_table(spec):
    """every spec x {psnr, psnr+ssim, ssim, all four} x the three flags: without metric_groups the table is the parent's, with it
    the parent's table at metrics = psnr"""
    from methods import Runner
    assert Runner(spec).metric_groups is False
    for metrics in ("psnr", "psnr,ssim", "ssim", None):
        for byte_groups, iterative_groups, grading_groups in itertools.product((False, True), repeat=3):
            flags = dict(byte_groups=byte_groups, iterative_groups=iterative_groups, grading_groups=grading_groups)
            want = parent_takes_groups(spec, metrics, byte_groups, iterative_groups, grading_groups)
            assert Runner(spec, metrics=metrics, **flags).takes_groups() is want, (spec, metrics, flags)
            assert Runner(spec, metrics=metrics, metric_groups=False, **flags).takes_groups() is want, (spec, metrics, flags)
            at_psnr = parent_takes_groups(spec, "psnr", byte_groups, iterative_groups, grading_groups)
            assert Runner(spec, metrics=metrics, metric_groups=True, **flags).takes_groups() is at_psnr, (spec, metrics, flags)


def test_binding_refuses_other_inputs():
    """before anything touches a device: dtype, layout, shapes, contiguity"""
    import ct_hip
    res, gt = torch.zeros((2, 12, 14, 3), dtype=torch.float32), torch.zeros((2, 12, 14, 3), dtype=torch.uint8)
    wide_res, wide_gt = torch.zeros((2, 12, 14, 6), dtype=torch.float32), torch.zeros((2, 12, 14, 6), dtype=torch.uint8)
    bad = {"a float32 ground truth": (res, gt.float()),
           "a uint8 result": (gt, gt),
           "a CHW result": (res.permute(0, 3, 1, 2).contiguous(), gt),
           "CHW both": (res.permute(0, 3, 1, 2).contiguous(), gt.permute(0, 3, 1, 2).contiguous()),
           "mismatched shapes": (res, gt[:, :, :13]),
           "mismatched batch": (res, gt[:1]),
           "a single frame without a batch axis": (res[0], gt[0]),
           "a non-contiguous result": (wide_res[..., ::2], gt),
           "a non-contiguous ground truth": (res, wide_gt[..., ::2]),
           "host tensors": (res, gt)}
    for fn in (ct_hip.frame_ssim_hwc, ct_hip.frame_icid_hwc, ct_hip.frame_fsim_hwc):
        for what, (a, b) in bad.items():
            with pytest.raises(ct_hip.CtHipError):
                fn(a, b)
                pytest.fail("%s took %s" % (fn.__name__, what))
    with pytest.raises(ct_hip.CtHipError, match="contiguous"):
        ct_hip.frame_ssim_hwc(wide_res[..., ::2], gt)
    with pytest.raises(ct_hip.CtHipError, match=r"float32 \[B,H,W,3\]"):
        ct_hip.frame_icid_hwc(res, gt.float())


CFG = """
model:
  class_path: tests.metric_groups_common.GroupStub
  init_args:
    gain: 0.75
data:
  init_args:
    data_dir: null
    synthetic: video_u8
    n_frames: 5
    height: 24
    width: 40
    group: 3
"""


def test_cli_cpu_takes_the_flag_and_the_per_frame_route(tmp_path, monkeypatch):
    """CT_CLI_DEVICE=cpu: a loader of uint8 groups and a model that would take groups, with and without the flag -- the per-frame
    route either way (the stub's grouped methods raise), the same table"""
    from utils import cli
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    plain = cli.main(["test", "--config", str(cfg)])
    timing = {}
    flagged = cli.main(["test", "--config", str(cfg), "--model.metric_groups", "true"], timing=timing)
    assert timing["grouped"] is False and timing["frames_per_call"] == 1
    assert tuple(flagged.shape) == (5, 4) and not bool(torch.isnan(flagged).any())
    assert torch.equal(flagged, plain)

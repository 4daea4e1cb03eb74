"""What tests/test_metric_groups_host.py and tests/test_metric_groups_gpu.py share: the five specs, the frames of a case (seeded
ground-truth bytes and an unclamped float32 result that overshoots [0, 1]), their conversion for the planar entries on the CPU, and
a stub model for the CLI without a GPU.  A case is made once per shape and never changed."""
import numpy as np
import pytest

from tests.cli_stub import StubRunner

torch = pytest.importorskip("torch")

REINHARD_SPEC = "methods.linear.color_transfer_between_images"
MK_SPEC = "methods.linear.monge_kantorovitch_color_transfer"
XIAO_SPEC = "methods.linear.color_transfer_in_correlated_color_space"
IDT_SPEC = "methods.iterative.iterative_distribution_transfer"
ACG_SPEC = "methods.iterative.automated_color_grading"
SPECS = (REINHARD_SPEC, MK_SPEC, XIAO_SPEC, IDT_SPEC, ACG_SPEC)
GROUP_FLAG = {REINHARD_SPEC: {}, MK_SPEC: {"byte_groups": True}, XIAO_SPEC: {"byte_groups": True}, IDT_SPEC: {"iterative_groups": True},
              ACG_SPEC: {"grading_groups": True}}
NEW_ENTRIES = {"ct_frame_ssim_hwc_u8": 9, "ct_frame_icid_hwc_u8": 9, "ct_frame_fsim_hwc_u8": 11}
# the tolerances tests/test_metrics.py asserts for the planar entries against the float64 oracle
ATOL = {"ssim": 2e-6, "fsim": 2e-5, "icid": 5e-6}

_cases = {}


def make_case(b, h, w):
    """(result float32 [b,h,w,3], gt uint8 [b,h,w,3]) on the CPU: a smooth field with its contrast stretched into the clipping ends
    plus byte noise as ground truth; the result is gt / 255 with a gain about mid-grey and noise, so that it leaves [0, 1] on
    both sides -- at least 1 % of every frame below 0 and 1 % above 1, which is asserted: the clamp of the HWC source is exercised"""
    key = (b, h, w)
    if key not in _cases:
        rng = np.random.default_rng(1000003 * b + 1009 * h + w)
        low = torch.from_numpy(rng.random((b, 3, h // 8 + 2, w // 8 + 2)))
        smooth = torch.nn.functional.interpolate(low, size=(h, w), mode="bilinear", align_corners=True).numpy()
        field = (smooth - 0.5) * 2.5 + 0.5 + 0.04 * rng.standard_normal((b, 3, h, w))
        gt = np.rint(np.clip(field, 0, 1) * 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()
        result = ((gt.astype(np.float64) / 255 - 0.5) * 1.25 + 0.5 + 0.03 * rng.standard_normal(gt.shape)).astype(np.float32)
        for f in range(b):
            below, above = float((result[f] < 0).mean()), float((result[f] > 1).mean())
            assert below >= 0.01 and above >= 0.01, (key, f, below, above)
        _cases[key] = (torch.from_numpy(result), torch.from_numpy(gt))
    return _cases[key]


def planar(result, gt_u8):
    """what the planar entries take, made on the CPU: (clamp(result, 0, 1) as NCHW, float32(gt) / 255 as NCHW), float32 contiguous"""
    assert not result.is_cuda and not gt_u8.is_cuda
    return result.clamp(0, 1).permute(0, 3, 1, 2).contiguous(), (gt_u8.float() / 255).permute(0, 3, 1, 2).contiguous()


class GroupStub(StubRunner):
    """a model that offers the grouped interface and takes `metric_groups`, whose grouped methods must not run (CT_CLI_DEVICE=cpu)"""

    def __init__(self, func_spec="tests.cli_stub.swap_means", gain=1.0, metric_groups=False):
        super().__init__(func_spec, gain)
        self.metric_groups = bool(metric_groups)

    def takes_groups(self):
        return True

    def test_group(self, group_u8, psnr_out):
        raise AssertionError("the grouped route ran under CT_CLI_DEVICE=cpu")

    test_group_metrics = test_group

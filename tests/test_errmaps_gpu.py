"""The error maps rgbssim, labmse and abmse on the device (csrc/errmaps.hip, ct_hip/views.py, the models' views(), `utils.cli predict
--views`) against tests/golden/errmaps.npz: the reference's own utils/visualizations.py, run in float64 and in float32 with the two
kornia calls restated (tests/golden/make_golden_errmaps.py).

The yardstick is the reference's own float32 run: e32 = |ref32 - ref64|.  The kernel's error |hip - ref64| must stay within
2 x e32, in rms and in max, per map and shape -- the margin this project uses for a float32 kernel held against a float32 reference
(gmflow_f64.npz) -- with an absolute floor of 1e-6.  The tests print the ratios (-s); DESIGN section 4.13 is where they
are recorded once the module has run on an MI355X."""
import os

import numpy as np
import pytest
import torch

from tests import errmaps_common as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")


@pytest.fixture(scope="module")
def golden():
    return np.load(ec.GOLDEN)


@pytest.fixture(scope="module")
def device_inputs():
    return {shape: tuple(torch.from_numpy(a).cuda() for a in ec.inputs(shape)) for shape in ec.SHAPES}


def _view(name):
    import ct_hip
    return getattr(ct_hip, name + "_view")


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.tag)
@pytest.mark.parametrize("name", ec.MAPS)
def test_map_within_twice_the_float32_reference(golden, device_inputs, name, shape):
    x, y = device_inputs[shape]
    kept = (x.clone(), y.clone())
    out = _view(name)(x, y)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(x, kept[0]) and torch.equal(y, kept[1])                        # the inputs are left alone
    got = out.cpu().numpy()
    ref64, ref32 = golden["%s/%s/f64" % (ec.tag(shape), name)], golden["%s/%s/f32" % (ec.tag(shape), name)]
    mine, ref, ok = ec.error_gate(got[:, 0], ref32, ref64)
    print("%s %s: rms %.3g (reference float32 %.3g, ratio %.2f), max %.3g (reference float32 %.3g, ratio %.2f)"
          % (name, ec.tag(shape), mine[0], ref[0], mine[0] / ref[0], mine[1], ref[1], mine[1] / ref[1]))
    assert not got[:, 1:].any() and not np.signbit(got[:, 1:]).any()                # channels 1 and 2: exactly zero
    for b in range(shape[0]):                                                        # every frame spans exactly [0, 1] on its own
        assert got[b, 0].min() == 0 and got[b, 0].max() == 1
    assert ok
    assert torch.equal(_view(name)(x, y), out)                                      # deterministic


@pytest.mark.parametrize("name", ec.MAPS)
def test_unaligned_bases_take_the_scalar_path_with_the_same_bits(name):
    """a base 4 bytes off 16 with a width that is a multiple of 4: the element-by-element path, bit for bit the vector path"""
    shape = (2, 3, 40, 72)
    gen = torch.Generator().manual_seed(7)
    x, y = torch.rand(shape, generator=gen).cuda(), torch.rand(shape, generator=gen).cuda()
    want = _view(name)(x, y)
    n = x.numel()
    xo, yo = torch.empty(n + 1, device="cuda")[1:].view(shape), torch.empty(n + 1, device="cuda")[1:].view(shape)
    xo.copy_(x)
    yo.copy_(y)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    assert torch.equal(_view(name)(xo, yo), want)


def test_constant_lab_maps_are_nan_and_the_interface():
    import ct_hip
    x = torch.rand(2, 3, 23, 37, generator=torch.Generator().manual_seed(1)).cuda()
    for fn in (ct_hip.labmse_view, ct_hip.abmse_view):
        out = fn(x, x)                                                               # a constant map: 0 / 0, as the reference's division
        assert torch.isnan(out[:, 0]).all() and not out[:, 1:].any()
    for fn in (ct_hip.rgbssim_view, ct_hip.labmse_view, ct_hip.abmse_view):
        with pytest.raises(ct_hip.CtHipError):
            fn(x, x[:, :, :, :36])
        with pytest.raises(ct_hip.CtHipError):
            fn(x, x.double())
        with pytest.raises(ct_hip.CtHipError):
            fn(x[:, :, :, ::2], x[:, :, :, ::2])
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.rgbssim_view(x[:, :, :5].contiguous(), x[:, :, :5].contiguous())      # the reflect padding needs more than 5 rows


def test_visualizations_drop_ins_are_the_ct_hip_functions(device_inputs):
    from utils import visualizations as viz
    x, y = device_inputs[(2, 23, 37)]
    for name in ec.MAPS:
        assert torch.equal(getattr(viz, name)(x, y), _view(name)(x, y)), name
    flipped = x.flip(3)                                                              # not contiguous: the drop-in makes it so
    assert torch.equal(viz.rgbssim(flipped, y), _view("rgbssim")(flipped.contiguous(), y))


# ---- 2. the models ----------------------------------------------------------------------------------------------------------------------
NAMES = ("corrected", "rgbssim", "labmse", "abmse")


def _views_equal(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == torch.uint8 and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k


def _composition(corrected, gt):
    import ct_hip
    want = {"corrected": ct_hip.pack_u8(corrected, "chw")}
    for name in ec.MAPS:
        want[name] = ct_hip.pack_u8(_view(name)(gt, corrected), "chw")
        assert want[name][..., 0].max() == 255 and not want[name][..., 1:].any()     # a scaled map, red only
    return want


def test_dcmcs3di_extra_views_are_the_composition():
    from methods.dcmcs3di import DCMCS3DI
    torch.manual_seed(3)
    net = DCMCS3DI(extraction_layers=1, transfer_layers=1).cuda().eval()
    gen = torch.Generator().manual_seed(2)
    left, gt = torch.rand(2, 3, 48, 96, generator=gen).cuda(), torch.rand(2, 3, 48, 96, generator=gen).cuda()
    right = (left.roll(3, dims=3) * 0.9 + 0.05).contiguous()
    got = net.views(left, right, gt=gt, names=NAMES)
    _views_equal(got, _composition(net(left, right, inference=True)[0], gt))
    assert list(net.views(left, right, gt=gt)) == ["corrected", "chess", "rgbmse", "disparity", "warped_right", "occlusions"]
    with pytest.raises(ValueError):
        net.views(left, right, names="rgbssim")


def test_runner_extra_views_are_the_composition():
    from methods import Runner
    model = Runner("methods.linear.color_transfer_between_images")
    gen = torch.Generator().manual_seed(4)
    batch = {k: torch.rand(1, 3, 40, 56, generator=gen).cuda() for k in ("target", "reference", "gt")}
    got = model.views(batch, names=NAMES)
    _views_equal(got, _composition(model(batch).clamp(0, 1).float().contiguous(), batch["gt"]))
    assert list(model.views(batch)) == ["corrected", "chess", "rgbmse"]
    with pytest.raises(ValueError):
        model.views({k: batch[k] for k in ("target", "reference")}, names="rgbssim")


# ---- 3. predict --views -----------------------------------------------------------------------------------------------------------------
def test_predict_writes_the_rgbssim_view(tmp_path):
    from methods import Runner
    from utils import cli
    from utils.data import SyntheticStereoFrames
    args = ["predict", "--config", os.path.join(CFG, "others.yaml"), "--data.n_frames", "3", "--data.height", "64", "--data.width", "96"]
    assert cli.main(args + ["--output", str(tmp_path / "o"), "--format", "npy", "--views", "corrected,rgbssim"]) == 3
    assert sorted(os.listdir(tmp_path / "o")) == sorted(["%06d%s.npy" % (f, v) for f in range(3) for v in ("", ".corrected", ".rgbssim")])
    fr, model = SyntheticStereoFrames(3, 64, 96), Runner("methods.linear.color_transfer_between_images")
    for f in range(3):
        want = model.views({k: v[None].cuda() for k, v in fr[f].items()}, names=("corrected", "rgbssim"))
        for v in ("corrected", "rgbssim"):
            assert np.array_equal(np.load(tmp_path / "o" / ("%06d.%s.npy" % (f, v))), want[v][0].cpu().numpy()), (f, v)

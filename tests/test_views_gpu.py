"""The diagnostic views on the device (csrc/views.hip, ct_hip/views.py, the models' views(), `utils.cli predict --views`) against
the numpy restatements of tests/views_common.py, which tests/test_views_host.py pins to the reference's own outputs.

chess_mix, rgbmse_view and gray_view are bitwise.  flow_to_image is compared with the reference's bytes: the device's atan2 / sqrt
may round differently from numpy's, so equality holds off the knife edges only (views_common.flow_gate): there every pixel is
within 1 grey level per channel and at most 0.5 % of them differ at all -- the reference against itself with inputs perturbed by
2^-22 relative moves at most 5.1e-4 of the pixels of these flows (views.npz: perturbed_share; only the maximum-radius pixel
jumps), so the cap leaves a tenfold margin or more.  The tests print the device's own figures (-s); none has been recorded yet:
this module has not run on an MI355X, only against a host build of csrc/views.hip."""
import os

import numpy as np
import pytest
import torch

from tests import views_common as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    return np.load(vc.GOLDEN)


# ---- 1. chess_mix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,size", [((2, 3, 60, 77), 25), ((2, 3, 60, 77), 7), ((1, 3, 25, 25), 25), ((1, 1, 1, 130), 25),
                                        ((1, 2, 9, 64), 25), ((1, 2, 9, 64), 6), ((2, 3, 60, 76), 7), ((1, 1, 300, 1024), 25)])
def test_chess_mix_bitwise(shape, size):
    """rows off the 16-byte grid (77, 25, 130 floats), on it with blocks that are multiples of four (64 / 25 is not: a 16-byte group
    then straddles two blocks, 76 / 7 likewise), and more than one workgroup's worth"""
    import ct_hip
    x, y = vc.chess_inputs(*shape)
    got = ct_hip.chess_mix(_dev(x), _dev(y), size).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(vc.chess_mix_ref(x, y, size)))


def test_chess_mix_unaligned_base_and_interface():
    import ct_hip
    from utils import visualizations as viz
    x, y = vc.chess_inputs(1, 1, 8, 64)
    pad = torch.zeros(8 * 64 + 1, device="cuda")
    xo = pad[1:].view(1, 1, 8, 64)                                  # 4 bytes off the 16-byte grid: the element-wise kernel
    xo.copy_(_dev(x))
    assert xo.data_ptr() % 16 == 4
    assert np.array_equal(ct_hip.chess_mix(xo, _dev(y), 5).cpu().numpy(), vc.chess_mix_ref(x, y, 5))
    assert np.array_equal(viz.chess_mix(_dev(x)[0], _dev(y)[0], size=5).cpu().numpy(), vc.chess_mix_ref(x, y, 5)[0])
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.chess_mix(_dev(x), _dev(y)[:, :, :4], 5)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.chess_mix(_dev(x), _dev(y), 0)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.chess_mix(_dev(x).double(), _dev(y).double(), 5)


# ---- 2. the min-max family ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 41, 67), (1, 3, 5, 1030), (2, 3, 64, 96)])
def test_rgbmse_and_gray_bitwise(shape):
    """41 x 67 (odd plane: the element-wise path), 5 x 1030 = 5150 pixels (no multiple of four either, more than one workgroup per
    frame), 64 x 96 (the 16-byte path, six workgroups); frame 1's error is a quarter of frame 0's: no statistic leaks"""
    import ct_hip
    from utils import visualizations as viz
    x, y = vc.rgbmse_inputs(shape)
    want = vc.rgbmse_ref(x, y)
    got = ct_hip.rgbmse_view(_dev(x), _dev(y))
    again = ct_hip.rgbmse_view(_dev(x), _dev(y))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and torch.equal(got, again)
    assert torch.equal(viz.rgbmse(_dev(x), _dev(y)), got)
    # the disparity stand-in: signed values, another range in every frame
    d = ((x[:, :1] - np.float32(0.5)) * np.arange(1, shape[0] + 1, dtype=np.float32)[:, None, None, None] * np.float32(37)).astype(np.float32)
    got = ct_hip.gray_view(_dev(d))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(vc.gray_ref(d))) and torch.equal(got, ct_hip.gray_view(_dev(d)))
    assert torch.equal(viz.minmaxscale(_dev(d)[:, 0]), got[:, 0])
    for b in range(shape[0]):
        assert float(got[b].min()) == 0 and float(got[b].max()) == 1


def test_min_max_views_constant_frame_is_nan_and_interface():
    import ct_hip
    x = torch.rand(2, 3, 12, 20, device="cuda")
    y = x.clone()
    y[1] += 0.125 * torch.rand(3, 12, 20, device="cuda")
    out = ct_hip.rgbmse_view(x, y)
    assert bool(torch.isnan(out[0, 0]).all()) and not bool(out[0, 1:].any())            # no error anywhere: 0 / 0, as the reference
    assert bool(torch.isfinite(out[1]).all()) and float(out[1, 0].max()) == 1
    assert not bool(ct_hip.pack_u8(out, "chw")[0].any())                                # the pack shows NaN black
    assert bool(torch.isnan(ct_hip.gray_view(torch.full((1, 1, 7, 9), 3.0, device="cuda"))).all())
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.rgbmse_view(x[:, :2].contiguous(), y[:, :2].contiguous())
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.gray_view(x)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.rgbmse_view(x, y.permute(0, 1, 3, 2))


# ---- 3. flow_to_image -------------------------------------------------------------------------------------------------------------
def _check_flow(got, want, flow, tag):
    worst, share = vc.flow_gate(got, want, flow)
    print("flow_to_image %s: off the knife edges worst %d grey levels, share of differing pixels %.3e" % (tag, worst, share))
    assert worst <= 1 and share <= 0.005
    return share


@pytest.mark.parametrize("case", vc.FLOW_CASES)
def test_flow_to_image_golden(golden, case):
    import ct_hip
    from utils import flow_viz
    flow = vc.flow_input(case)
    want = golden["flow/%s/out" % case]
    assert float(golden["flow/%s/perturbed_share" % case]) < 1e-3
    dev = _dev(flow[None])
    got = ct_hip.flow_to_image(dev)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + want.shape
    assert np.array_equal(dev.cpu().numpy(), flow[None])            # the input is left alone (the reference zeroes unknown pixels in place)
    _check_flow(got[0].cpu().numpy(), want, flow, case)
    if case == "zero":
        assert bool((got == 255).all())
    if case == "unknown":
        assert not bool(got[0, 5, 7].any())
    assert torch.equal(flow_viz.flow_tensor_to_image(dev[0]), got[0].permute(2, 0, 1))
    assert torch.equal(flow_viz.flow_to_image(dev[0].permute(1, 2, 0)), got[0])
    assert torch.equal(ct_hip.flow_to_image(dev), got)


def test_flow_to_image_batches_scale_every_frame_by_its_own_maximum(golden):
    import ct_hip
    cases = ("amp0.5", "unknown", "zero", "amp20")                  # amplitudes 0.5 / 20 / 0 / 20 side by side
    flows = np.stack([vc.flow_input(c) for c in cases])
    got = ct_hip.flow_to_image(_dev(flows)).cpu().numpy()
    for b, c in enumerate(cases):
        _check_flow(got[b], golden["flow/%s/out" % c], flows[b], "batch of 4, frame %d (%s)" % (b, c))
    assert (got[2] == 255).all() and not got[1, 5, 7].any()
    # 37 x 53 is odd: the pixel-wise path.  36 x 52 takes the four-pixel path; both against the restatement at that shape
    crop = np.ascontiguousarray(flows[:, :, :36, :52])
    got = ct_hip.flow_to_image(_dev(crop)).cpu().numpy()
    for b, c in enumerate(cases):
        _check_flow(got[b], vc.flow_to_image_ref(crop[b]), crop[b], "36 x 52 crop, frame %d (%s)" % (b, c))


def test_flow_to_image_nan_is_unknown():
    import ct_hip
    flow = vc.flow_input("amp20")[:, :36, :52].copy()
    flow[1, 3, 4] = np.nan
    flow[0, 9, 9] = -np.inf
    got = ct_hip.flow_to_image(_dev(flow[None]))[0].cpu().numpy()
    assert not got[3, 4].any() and not got[9, 9].any()
    _check_flow(got, vc.flow_to_image_ref(flow), flow, "NaN / inf pixels")
    assert got.reshape(-1, 3).any(axis=1).sum() == 36 * 52 - 2


# ---- 4. / 5. the models ---------------------------------------------------------------------------------------------------------------
def _views_equal(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == torch.uint8 and got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("batch", [1, 2])
def test_dcmcs3di_views_are_the_composition(batch):
    import ct_hip
    from methods.dcmcs3di import DCMCS3DI
    torch.manual_seed(3)
    net = DCMCS3DI(extraction_layers=2, transfer_layers=1).cuda().eval()
    gen = torch.Generator().manual_seed(batch)
    left, gt = torch.rand(batch, 3, 48, 96, generator=gen).cuda(), torch.rand(batch, 3, 48, 96, generator=gen).cuda()
    right = (left.roll(3, dims=3) * 0.9 + 0.05).contiguous()
    got = net.views(left, right, gt=gt)
    assert list(got) == ["corrected", "chess", "rgbmse", "disparity", "warped_right", "occlusions"]
    corrected = net(left, right, inference=True)[0]
    p = net.forward_parts(left, right, want_disp=True)
    occ = (~(p["valid_left"] > 0.5)).to(torch.uint8) * 255
    want = {"corrected": ct_hip.pack_u8(corrected, "chw"),
            "chess": ct_hip.pack_u8(ct_hip.chess_mix(gt, corrected), "chw"),
            "rgbmse": ct_hip.pack_u8(ct_hip.rgbmse_view(gt, corrected), "chw"),
            "disparity": ct_hip.pack_u8(ct_hip.gray_view(p["disp_left"]), "chw"),
            "warped_right": ct_hip.pack_u8(p["warped_rgb"].contiguous(), "chw"),
            "occlusions": occ.permute(0, 2, 3, 1).expand(-1, -1, -1, 3).contiguous()}
    _views_equal(got, want)
    _views_equal(net.views(left, right, names=("disparity",)), {"disparity": want["disparity"]})
    assert list(net.views(left, right)) == ["corrected", "disparity", "warped_right", "occlusions"]
    with pytest.raises(ValueError):
        net.views(left, right, names=("chess",))
    with pytest.raises(ValueError):
        net.views(left, right, gt=gt, names=("flow",))


def test_dmsct_views_are_the_composition():
    import ct_hip
    from methods.dmsct import DMSCT
    from utils import flow_viz
    torch.manual_seed(1)
    net = DMSCT().cuda().eval()
    gen = torch.Generator().manual_seed(5)
    target, gt = torch.rand(1, 3, 64, 96, generator=gen).cuda(), torch.rand(1, 3, 64, 96, generator=gen).cuda()
    reference = (target.roll(2, dims=3) * 0.8 + 0.1).contiguous()
    got = net.views(target, reference, gt=gt)
    assert list(got) == ["corrected", "chess", "rgbmse", "flow", "warped_right", "occlusions"]
    with torch.no_grad():
        corrected = net(target, reference)
    m = net.match(target, reference)
    want = {"corrected": ct_hip.pack_u8(corrected, "chw"),
            "chess": ct_hip.pack_u8(ct_hip.chess_mix(gt, corrected), "chw"),
            "rgbmse": ct_hip.pack_u8(ct_hip.rgbmse_view(gt, corrected), "chw"),
            "flow": ct_hip.flow_to_image(m["flow"]),
            "warped_right": ct_hip.pack_u8(ct_hip.flow_warp(reference, m["flow"]), "chw"),
            "occlusions": (m["fwd_occ"] * 255).to(torch.uint8).permute(0, 2, 3, 1).expand(-1, -1, -1, 3).contiguous()}
    _views_equal(got, want)
    assert torch.equal(got["flow"][0].permute(2, 0, 1), flow_viz.flow_tensor_to_image(m["flow"][0]))
    with pytest.raises(ValueError):
        net.views(target, reference, names="rgbmse")
    with pytest.raises(ValueError):
        net.views(target, reference, gt=gt, names="disparity")


# ---- 6. predict --views ------------------------------------------------------------------------------------------------------------------
def test_predict_views_writes_what_runner_views_gives(tmp_path):
    from PIL import Image
    from methods import Runner
    from utils import cli
    from utils.data import SyntheticStereoFrames
    args = ["predict", "--config", os.path.join(CFG, "others.yaml"), "--data.n_frames", "5", "--data.height", "64", "--data.width", "96"]
    assert cli.main(args + ["--output", str(tmp_path / "plain")]) == 5
    assert cli.main(args + ["--output", str(tmp_path / "views"), "--views", "corrected,chess,rgbmse"]) == 5
    plain = ["%06d.png" % f for f in range(5)]
    assert sorted(os.listdir(tmp_path / "plain")) == plain
    assert sorted(os.listdir(tmp_path / "views")) == sorted(plain + ["%06d.%s.png" % (f, v) for f in range(5) for v in ("corrected", "chess", "rgbmse")])
    fr, model = SyntheticStereoFrames(5, 64, 96), Runner("methods.linear.color_transfer_between_images")

    def png(path):
        with Image.open(path) as im:
            assert im.mode == "RGB"
            return np.asarray(im)

    for f in range(5):
        batch = {k: v[None].cuda() for k, v in fr[f].items()}
        want = model.views(batch)
        assert list(want) == ["corrected", "chess", "rgbmse"]
        for v in want:
            assert np.array_equal(png(tmp_path / "views" / ("%06d.%s.png" % (f, v))), want[v][0].cpu().numpy()), (f, v)
        assert np.array_equal(png(tmp_path / "views" / plain[f]), png(tmp_path / "plain" / plain[f]))
        assert np.array_equal(png(tmp_path / "views" / plain[f]), want["corrected"][0].cpu().numpy())
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--output", str(tmp_path / "no"), "--views", "flow"])
    assert "Runner" in str(e.value) and "flow" in str(e.value) and not os.path.exists(tmp_path / "no")

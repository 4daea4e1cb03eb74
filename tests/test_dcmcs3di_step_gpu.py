"""DCMCS3DI.step on the GPU: the reference's eleven logged quantities (methods/dcmcs3di.py:68-92) are the public pieces put together --
ct_hip.frame_losses, pasmnet.losses on forward(inference=False)'s outputs, the metric calls -- and the three parallax-attention losses
meet the error rule of tests/test_pam_losses_gpu.py against the float64 restatement on the device's own maps and masks (the maps' own
parity is held by tests/test_dcmcs3di_gpu.py).  The test prints the figures (-s).

Measured on an MI355X (loss before the 0.005; error against float64 / allowed / the float32 restatement's error; both masks all valid):
    Photometric Loss  0.253303395   1.1e-09 / 3.0e-08 / 1.3e-08
    Cycle Loss        3.89997996    8.9e-11 / 4.7e-07 / 1.0e-07
    Smoothness Loss   0.00979577904 2.6e-14 / 1.2e-09 / 3.3e-10
"""
import pytest
import torch

from tests import dcmcs3di_common as dc
from tests import pam_losses_common as plc

pytestmark = pytest.mark.gpu
NAMES = ("L1 Loss", "MSE Loss", "SSIM Loss", "Photometric Loss", "Cycle Loss", "Smoothness Loss", "PSNR", "SSIM", "FSIM", "iCID", "loss")


@pytest.fixture(scope="module")
def run():
    model = dc.build_model(seed=0, extraction_layers=2, transfer_layers=1, channels=64).cuda()
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(2, 3, 24, 40, generator=g)
    gt = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(gt, (2, 2, 2, 2), mode="reflect"), 5, stride=1)      # some structure to match
    right = torch.roll(gt, 3, dims=3)                        # the other view: shifted by three columns
    target = (gt * 0.8 + 0.1).clamp(0, 1)                    # the left view with a colour mismatch
    batch = {"target": target.cuda(), "reference": right.contiguous().cuda(), "gt": gt.cuda()}
    return model, batch, model.step(batch, prefix="Validation")


def _same(a, b):
    return torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


def test_step_keys_and_types(run):
    _, _, out = run
    assert tuple(out) == NAMES
    assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in out.values())
    assert all(bool(torch.isfinite(v)) for v in out.values())
    assert not any(v.requires_grad for v in out.values())   # no autograd is offered


def test_step_is_its_pieces(run):
    import ct_hip
    from methods import fsim, icid, psnr, ssim
    from pasmnet import losses
    model, batch, out = run
    with torch.no_grad():
        corrected, (att, att_cycle, valid, _) = model(batch["target"], batch["reference"], inference=False)
    assert valid[0].dtype == torch.bool and valid[1].dtype == torch.bool and att[0].shape == (2, 24, 40, 40)
    frame, _ = ct_hip.frame_losses(corrected.float().contiguous(), batch["gt"])
    assert _same(out["L1 Loss"], frame[0]) and _same(out["MSE Loss"], frame[1]) and _same(out["SSIM Loss"], frame[2])      # SSIM loss unscaled
    assert _same(out["Photometric Loss"], 0.005 * losses.loss_pam_photometric(batch["target"], batch["reference"], att, valid))
    assert _same(out["Smoothness Loss"], 0.005 * losses.loss_pam_smoothness(att))
    assert _same(out["Cycle Loss"], 0.005 * losses.loss_pam_cycle_from_att(att, valid))
    for name, fn in (("PSNR", psnr), ("SSIM", ssim), ("FSIM", fsim), ("iCID", icid)):
        assert _same(out[name], fn(corrected.float().contiguous(), batch["gt"]).mean()), name
    total = out["L1 Loss"] + out["MSE Loss"] + out["SSIM Loss"] + out["Photometric Loss"] + out["Cycle Loss"] + out["Smoothness Loss"]
    assert _same(out["loss"], total)
    # the cycle maps forward() returns, through the reference's own form of the loss: the same value by the error rule below
    case = dict(att_r2l=att[0].cpu(), att_l2r=att[1].cpu(), left=batch["target"].cpu(), right=batch["reference"].cpu(),
                valid_left=valid[0].cpu().to(torch.uint8), valid_right=valid[1].cpu().to(torch.uint8))
    ref64, ref32 = plc.restate(case, torch.float64), plc.restate(case, torch.float32)
    for v in (case["valid_left"], case["valid_right"]):
        print("valid fraction %.3f" % float(v.float().mean()))
    for q, (loss, key) in enumerate(zip(plc.LOSSES, ("Photometric Loss", "Cycle Loss", "Smoothness Loss"))):
        ok, err, allowed = plc.within_rule(out[key] / 0.005, ref64[q], ref32[q])
        print("%-16s %.9g  error %.3g  allowed %.3g (float32 restatement: %.3g)" % (key, float(out[key]) / 0.005, err, allowed,
                                                                                      abs(float(ref32[q]) - float(ref64[q]))))
        assert ok, (key, float(out[key]) / 0.005, float(ref64[q]), err, allowed)
    ok, err, allowed = plc.within_rule(losses.loss_pam_cycle(att_cycle, valid), ref64[1], ref32[1])
    assert ok, ("cycle from forward()'s maps", err, allowed)


def test_validation_step_still_raises(run):
    model, batch, _ = run
    with pytest.raises(NotImplementedError) as e:
        model.validation_step(batch)
    assert all(name in str(e.value) for name in ("Photometric", "Cycle", "Smoothness")) and "step" in str(e.value)
    assert type(model).VALIDATION_MISSING == ("Photometric Loss", "Cycle Loss", "Smoothness Loss")


def test_step_needs_the_gpu():
    import ct_hip
    model = dc.build_model(seed=0, extraction_layers=1, transfer_layers=1)
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ct_hip.CtHipError):
        model.step({"target": x, "reference": x, "gt": x})

"""pasmnet.losses / ct_hip.pam_cycle_l1 / ct_hip.pam_map_sweep (csrc/pam_losses.hip) against the float64 values of the three
parallax-attention losses: the cases of tests/golden/pam_losses.npz (the real reference's float64 and float32 runs) plus two cases built
here with the float64 / float32 restatement on the CPU -- 1x2x320 (the reference's crop width: ten K chunks of the cycle product, five
columns per lane in the sweep) and 1x11x33 (two row segments of the sweep, the second ragged).

Error rule (tests/pam_losses_common.within_rule): |kernel - float64| <= max(2 x |float32 run - float64|, 2^-23 |float64|); NaN exactly
where the float64 value is NaN.  The test prints the figures (-s).

Measured on an MI355X (error against float64):
    case                loss          error      allowed    (float32 run's error)
    2x4x70              photometric   2.4e-09    1.9e-07    1.4e-08
                        cycle         4.5e-09    2.5e-07    4.8e-09          from torch.matmul's maps: 3.1e-09
                        smoothness    7.6e-12    4.1e-09    7.6e-10
    1x3x33              photometric   8.5e-09    1.8e-07    5.6e-08
                        cycle         3.1e-09    2.5e-07    2.8e-08          7.5e-09
                        smoothness    4.1e-11    8.7e-09    1.1e-09
    1x2x96              photometric   2.8e-09    2.0e-07    2.3e-08
                        cycle         5.5e-09    5.6e-07    2.8e-07          7.9e-09
                        smoothness    4.5e-11    3.0e-09    2.1e-10
    1x1x40              photometric   5.1e-10    2.0e-07    4.6e-08
                        cycle         1.9e-08    2.4e-07    7.9e-08          1.1e-08
                        smoothness    NaN = NaN
    1x2x1               photometric   0          5.4e-08    0
                        cycle         0          0          0                0
                        smoothness    NaN = NaN
    1x3x33_none_valid   photometric, cycle  NaN = NaN
                        smoothness    2.6e-11    9.0e-09    2.8e-09
    1x3x33_one_valid    photometric   3.6e-08    2.1e-07    8.2e-09
                        cycle         2.0e-08    3.0e-07    1.2e-07          3.9e-08
                        smoothness    1.2e-10    8.3e-09    3.1e-09
    1x2x320             photometric   2.3e-09    1.9e-07    7.2e-08
                        cycle         2.0e-09    2.5e-07    2.1e-08          3.2e-10
                        smoothness    5.6e-12    9.0e-10    1.1e-10
    1x11x33             photometric   1.8e-09    2.1e-07    1.1e-07
                        cycle         3.8e-09    2.4e-07    5.9e-08          3.4e-09
                        smoothness    6.1e-11    8.7e-09    3.7e-09
Where the float32 run is within half a float32 ulp of float64 (most cases) the allowed figure is the ulp floor; the kernels are 5 to
500 times closer than the rule asks.
"""
import pytest
import torch

from tests import pam_losses_common as plc

pytestmark = pytest.mark.gpu
EXTRA = {"1x2x320": (1, 2, 320), "1x11x33": (1, 11, 33)}
NAMES = list(plc.CASES) + list(EXTRA)


@pytest.fixture(scope="module")
def cases():
    out = plc.load_golden()
    for k, (name, shape) in enumerate(EXTRA.items()):
        case = plc.build_case(shape, 2000 + k)
        case["ref64"], case["ref32"] = plc.restate(case, torch.float64), plc.restate(case, torch.float32)
        out[name] = case
    return out


def _device(case, bool_masks=True):
    att = (case["att_r2l"].cuda(), case["att_l2r"].cuda())
    valid = tuple(case[k].cuda().bool() if bool_masks else case[k].cuda().float() for k in ("valid_left", "valid_right"))
    return case["left"].cuda(), case["right"].cuda(), att, valid


def _same(a, b):
    """bitwise, NaN == NaN"""
    return torch.equal(a.cpu().view(torch.int64), b.cpu().view(torch.int64))


@pytest.mark.parametrize("name", NAMES)
def test_losses_against_float64(cases, name):
    from pasmnet import losses
    case = cases[name]
    left, right, att, valid = _device(case)
    got = {"photometric": losses.loss_pam_photometric(left, right, att, valid),
           "cycle": losses.loss_pam_cycle_from_att(att, valid),
           "smoothness": losses.loss_pam_smoothness(att)}
    att_cycle = (torch.matmul(att[0], att[1]), torch.matmul(att[1], att[0]))
    got_maps = losses.loss_pam_cycle(att_cycle, valid)
    for v in list(got.values()) + [got_maps]:
        assert v.dtype == torch.float64 and v.is_cuda and v.dim() == 0
    for q, loss in enumerate(plc.LOSSES):
        ok, err, allowed = plc.within_rule(got[loss], case["ref64"][q], case["ref32"][q])
        print("%-18s %-12s %.9g  error %.3g  allowed %.3g (float32 run: %.3g)" % (name, loss, float(got[loss]), err, allowed,
                                                                                    abs(float(case["ref32"][q]) - float(case["ref64"][q]))))
        assert ok, (loss, float(got[loss]), float(case["ref64"][q]), err, allowed)
    # the cycle loss from cycle maps that torch.matmul made on the device: the same value by the same rule
    ok, err, allowed = plc.within_rule(got_maps, case["ref64"][1], case["ref32"][1])
    print("%-18s %-12s %.9g  error %.3g  allowed %.3g" % (name, "cycle (maps)", float(got_maps), err, allowed))
    assert ok, (float(got_maps), float(case["ref64"][1]), err, allowed)
    # two calls are bitwise equal; bool and 0/1 float masks give bitwise equal results
    _, _, _, valid_f = _device(case, bool_masks=False)
    assert _same(got["photometric"], losses.loss_pam_photometric(left, right, att, valid))
    assert _same(got["photometric"], losses.loss_pam_photometric(left, right, att, valid_f))
    assert _same(got["cycle"], losses.loss_pam_cycle_from_att(att, valid))
    assert _same(got["cycle"], losses.loss_pam_cycle_from_att(att, valid_f))
    assert _same(got["smoothness"], losses.loss_pam_smoothness(att))
    assert _same(got_maps, losses.loss_pam_cycle(att_cycle, valid))
    assert _same(got_maps, losses.loss_pam_cycle(att_cycle, valid_f))


@pytest.mark.parametrize("name", ["2x4x70", "1x3x33_none_valid", "1x11x33"])
def test_masked_l1_loss_is_the_sweeps_terms(cases, name):
    """masked_l1_loss on tensors that exist adds the same float32 terms as the sweep, in another order: float64 rounding apart"""
    import ct_hip
    from pasmnet import losses
    left, right, att, valid = _device(cases[name])
    att_cycle = torch.matmul(att[0], att[1])
    w = att_cycle.shape[-1]
    eye = torch.eye(w, device="cuda").expand_as(att_cycle).contiguous()
    sweep = ct_hip.pam_map_sweep(att[0], src=right, dst=left, mask=valid[0])
    warped = torch.matmul(att[0], right.permute(0, 2, 3, 1)).permute(0, 3, 1, 2).contiguous()
    pairs = ((losses.masked_l1_loss(att_cycle, eye, valid[0].permute(0, 2, 3, 1)), losses.loss_pam_cycle((att_cycle, att_cycle), (valid[0], valid[0])) / 2, 1e-12),
             # the warp differs: torch.matmul's float32 sum against the kernel's
             (losses.masked_l1_loss(left, warped, valid[0]), sweep["photometric"].sum() / sweep["mask_sum"].sum(), 1e-5))
    for a, b, tol in pairs:
        a, b = float(a), float(b)
        assert (a != a and b != b) or abs(a - b) <= tol * abs(b), (a, b)
    num, count = ct_hip.masked_l1_sums(left, warped, valid[0])
    assert num.shape == count.shape == (left.shape[0],) and torch.equal(count.cpu(), cases[name]["valid_left"].double().sum(dim=(1, 2, 3)))


def test_sweep_sums_and_counts(cases):
    import ct_hip
    case = cases["2x4x70"]
    left, right, att, valid = _device(case)
    s = ct_hip.pam_map_sweep(att[0], src=right, dst=left, mask=valid[0])
    b, h, w = plc.CASES["2x4x70"][0]
    assert s["vertical_count"].tolist() == [(h - 1) * w * w] * b and s["diagonal_count"].tolist() == [h * (w - 1) * (w - 1)] * b      # per image
    a = case["att_r2l"].double()
    for key, ref in (("vertical", (a[:, :-1] - a[:, 1:]).abs().sum(dim=(1, 2, 3))),
                     ("diagonal", (a[:, :, :-1, :-1] - a[:, :, 1:, 1:]).abs().sum(dim=(1, 2, 3))),
                     ("mask_sum", case["valid_left"].double().sum(dim=(1, 2, 3)))):
        assert s[key].shape == (b,) and s[key].dtype == torch.float64
        assert torch.allclose(s[key].cpu(), ref, rtol=1e-7, atol=0), key        # per image; float32 differences against float64 ones
    plain = ct_hip.pam_map_sweep(att[0])                     # the nullable inputs only switch terms off
    assert plain["photometric"] is None and plain["identity"] is None and plain["mask_sum"] is None
    assert torch.equal(plain["vertical"], s["vertical"]) and torch.equal(plain["diagonal"], s["diagonal"])
    masked = ct_hip.pam_map_sweep(att[0], mask=valid[0])
    assert masked["photometric"] is None and torch.equal(masked["identity"], s["identity"]) and torch.equal(masked["mask_sum"], s["mask_sum"])


def test_padded_tiles_add_nothing():
    """W = 33 leaves 31 padded rows and columns in the second tile: with identity maps and an all-true mask the product is the
    identity and the numerator exactly 0 -- a padded diagonal element would add |0 - 1|"""
    import ct_hip
    from pasmnet import losses
    eye = torch.eye(33, device="cuda").expand(2, 3, 33, 33).contiguous()
    mask = torch.ones(2, 1, 3, 33, dtype=torch.bool, device="cuda")
    num, count = ct_hip.pam_cycle_l1(eye, eye, mask)
    assert num.dtype == torch.float64 and not num.any() and torch.equal(count.cpu(), torch.full((2,), 99.0, dtype=torch.float64))
    assert float(losses.loss_pam_cycle_from_att((eye, eye), (mask, mask))) == 0.0
    assert float(losses.loss_pam_cycle((eye, eye), (mask, mask))) == 0.0
    # a cyclic shift by one column: the product shifts by two, so every row adds its 1 off the diagonal and |0 - 1| on it
    shift = torch.roll(torch.eye(33, device="cuda"), 1, dims=1).expand(1, 1, 33, 33).contiguous()
    num, _ = ct_hip.pam_cycle_l1(shift, shift, torch.ones(1, 1, 1, 33, device="cuda"))
    assert float(num) == 66.0


def test_binding_refusals():
    import ct_hip
    from pasmnet import losses
    g = torch.Generator().manual_seed(3)
    att = torch.softmax(torch.randn(2, 3, 8, 8, generator=g), dim=-1).cuda()
    img = torch.rand(2, 3, 3, 8, generator=g).cuda()
    mask = torch.ones(2, 1, 3, 8, dtype=torch.bool, device="cuda")
    bad_maps = (att[:, :, :, :7].contiguous(), att.double(), att.cpu(), att.transpose(2, 3), att[0], att.half())
    for bad in bad_maps:
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pam_map_sweep(bad)
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pam_cycle_l1(bad, att, mask)
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pam_cycle_l1(att, bad, mask)
    for bad in (mask[:, :, :2], mask.cpu(), mask[:, 0], torch.ones(2, 1, 3, 7, device="cuda")):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pam_cycle_l1(att, att, bad)
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pam_map_sweep(att, mask=bad)
    for kw in (dict(src=img), dict(dst=img), dict(src=img, dst=img), dict(src=img, dst=img[:, :2].contiguous(), mask=mask),
               dict(src=img.double(), dst=img, mask=mask), dict(src=img.cpu(), dst=img, mask=mask),
               dict(src=img, dst=img.transpose(2, 3).contiguous().transpose(2, 3), mask=mask)):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.pam_map_sweep(att, **kw)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.pam_map_sweep(torch.zeros(1, 1, 1025, 1025, device="cuda"))
    with pytest.raises(ct_hip.CtHipError):
        losses.masked_l1_loss(img, img, mask[:, :, :, :7])
    with pytest.raises(ct_hip.CtHipError):
        losses.masked_l1_loss(img, img.double(), mask)
    with pytest.raises(ct_hip.CtHipError):
        losses.loss_pam_photometric(img, img, (att, att.cpu()), (mask, mask))

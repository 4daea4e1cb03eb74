"""The parallax-attention losses without a GPU: the torch restatement of tests/pam_losses_common.py against the values the real
reference gave (tests/golden/pam_losses.npz, tests/golden/make_golden_pam_losses.py), the names pasmnet.losses exposes, and the
argument checks of the C entries (csrc/pam_losses.hip), which answer before anything touches a device."""
import ctypes
import math

import pytest
import torch

from tests import pam_losses_common as plc


@pytest.fixture(scope="module")
def golden():
    return plc.load_golden()


@pytest.mark.parametrize("name", list(plc.CASES))
def test_golden_inputs_are_the_seeded_cases(golden, name):
    shape, left_mask = plc.CASES[name]
    built = plc.build_case(shape, plc.case_seed(name), left_mask)
    for k in ("valid_left", "valid_right"):
        assert golden[name][k].shape == (shape[0], 1, shape[1], shape[2]) and golden[name][k].dtype == torch.uint8
        assert torch.equal(built[k], golden[name][k]), k     # the masks follow from the maps by a threshold: the same on every host
    assert golden[name]["att_r2l"].shape == (shape[0], shape[1], shape[2], shape[2]) and golden[name]["att_r2l"].dtype == torch.float32
    if shape[2] > 1:
        for k in ("valid_left", "valid_right"):
            if k == "valid_left" and left_mask:
                continue
            frac = float(golden[name][k].float().mean())
            assert 0.0 < frac < 1.0, (k, frac)                # valid and invalid pixels in both masks
    if left_mask == "none":
        assert not golden[name]["valid_left"].any()
    if left_mask == "one":
        assert int(golden[name]["valid_left"].sum()) == 1


@pytest.mark.parametrize("name", list(plc.CASES))
def test_restatement_equals_the_reference_in_float64(golden, name):
    got, ref = plc.restate(golden[name], torch.float64), golden[name]["ref64"]
    for q, loss in enumerate(plc.LOSSES):
        g, r = float(got[q]), float(ref[q])
        if math.isnan(r):
            assert math.isnan(g), loss
        else:
            assert abs(g - r) <= 1e-12 * abs(r), (loss, g, r)


def test_golden_nan_pattern(golden):
    nan = {name: tuple(bool(torch.isnan(v)) for v in golden[name]["ref64"]) for name in plc.CASES}
    assert nan == {"2x4x70": (False, False, False), "1x3x33": (False, False, False), "1x2x96": (False, False, False),
                   "1x1x40": (False, False, True), "1x2x1": (False, False, True), "1x3x33_none_valid": (True, True, False),
                   "1x3x33_one_valid": (False, False, False)}
    for name in plc.CASES:                                   # the float32 run has NaN in the same places
        assert torch.equal(torch.isnan(golden[name]["ref32"]), torch.isnan(golden[name]["ref64"]))


def test_error_rule():
    assert plc.within_rule(1.0 + 1e-7, 1.0, 1.0 + 6e-8)[0] and not plc.within_rule(1.0 + 2e-7, 1.0, 1.0 + 6e-8)[0]
    assert plc.within_rule(1.0 + 1e-7, 1.0, 1.0)[0] and not plc.within_rule(1.0 + 2e-7, 1.0, 1.0)[0]        # the float32 ulp floor
    nan = float("nan")
    assert plc.within_rule(nan, nan, nan)[0] and not plc.within_rule(0.0, nan, nan)[0] and not plc.within_rule(nan, 1.0, 1.0)[0]


def test_pasmnet_losses_names():
    from pasmnet import losses
    for name in ("masked_l1_loss", "loss_pam_photometric", "loss_pam_cycle", "loss_pam_smoothness", "loss_pam_cycle_from_att"):
        assert callable(getattr(losses, name)), name
    import ct_hip
    for name in ("pam_cycle_l1", "pam_map_sweep", "masked_l1_sums"):
        assert callable(getattr(ct_hip, name)), name
    from methods.dcmcs3di import DCMCS3DI
    assert callable(DCMCS3DI.step) and "autograd" in DCMCS3DI.step.__doc__ and "[B,H,W,W]" in DCMCS3DI.step.__doc__


def test_no_cpu_path():
    import ct_hip
    from pasmnet import losses
    att = torch.softmax(torch.zeros(1, 2, 4, 4), dim=-1)
    img, mask = torch.zeros(1, 3, 2, 4), torch.ones(1, 1, 2, 4)
    with pytest.raises(ct_hip.CtHipError):
        losses.loss_pam_smoothness((att, att))
    with pytest.raises(ct_hip.CtHipError):
        losses.loss_pam_cycle((att, att), (mask, mask))
    with pytest.raises(ct_hip.CtHipError):
        losses.loss_pam_cycle_from_att((att, att), (mask, mask))
    with pytest.raises(ct_hip.CtHipError):
        losses.loss_pam_photometric(img, img, (att, att), (mask, mask))
    with pytest.raises(ct_hip.CtHipError):
        losses.masked_l1_loss(img, img, mask)


def test_abi_entries_refuse_bad_arguments_without_a_device():
    """Every call below fails an argument check, so none reaches a launch: the pointers are made-up addresses that are never read."""
    import ct_hip
    lib = ct_hip.lib()
    p = lambda a: ctypes.c_void_p(a)                         # noqa: E731
    null, x, y, m, out, ws = p(0), p(0x10000), p(0x20000), p(0x30000), p(0x40000), p(0x50000)
    n, h, w = 2, 4, 70
    need = lib.ct_pam_losses_workspace_bytes(n, h, w)
    # the largest of: cycle n h tiles^2, sweep n ceil(h / 8) ceil(w / 4) 4, masked L1 n 64 float64 partial sums
    assert need == 8 * max(2 * 4 * 4, 2 * 1 * 18 * 4, 2 * 64) and need % 8 == 0
    assert lib.ct_pam_losses_workspace_bytes(8, 160, 320) == 8 * 8 * 20 * 80 * 4     # the sweep: 20 segments of 80 workgroups
    assert lib.ct_pam_losses_workspace_bytes(1, 1, 1) == 8 * 64
    for bad in ((0, 4, 70), (2, 0, 70), (2, 4, 0), (-1, 4, 70)):
        assert lib.ct_pam_losses_workspace_bytes(*bad) == 0
    BADARG, WORKSPACE, ALIGN = -1, -2, -3
    cyc = lib.ct_pam_cycle_l1_f32
    for args in ((null, y, m, out), (x, null, m, out), (x, y, null, out), (x, y, m, null)):
        assert cyc(*args, null, 0, n, h, w, null) == BADARG
    for dims in ((0, h, w), (n, 0, w), (n, h, 0), (-1, h, w), (n, -1, w), (n, h, -1), (65536, h, w), (n, 65536, w)):
        assert cyc(x, y, m, out, null, 0, *dims, null) == BADARG
    assert cyc(x, y, m, out, null, need, n, h, w, null) == WORKSPACE
    assert cyc(x, y, m, out, ws, 8 * 2 * 4 * 4 - 1, n, h, w, null) == WORKSPACE
    assert cyc(x, y, m, out, p(0x50004), need, n, h, w, null) == WORKSPACE
    for args in ((p(0x10002), y, m, out), (x, p(0x20001), m, out), (x, y, p(0x30002), out), (x, y, m, p(0x40004))):
        assert cyc(*args, ws, need, n, h, w, null) == ALIGN
    swp = lib.ct_pam_map_sweep_f32
    assert swp(null, null, null, null, out, null, 0, n, h, w, null) == BADARG
    assert swp(x, null, null, null, null, null, 0, n, h, w, null) == BADARG
    assert swp(x, y, null, m, out, null, 0, n, h, w, null) == BADARG          # src without dst
    assert swp(x, null, y, m, out, null, 0, n, h, w, null) == BADARG          # dst without src
    assert swp(x, y, y, null, out, null, 0, n, h, w, null) == BADARG          # the photometric term without a mask
    for dims in ((0, h, w), (n, 0, w), (n, h, 0), (n, h, -3), (65536, h, w), (n, h, 1025)):
        assert swp(x, null, null, null, out, null, 0, *dims, null) == BADARG
    assert swp(x, null, null, null, out, null, need, n, h, w, null) == WORKSPACE
    assert swp(x, null, null, null, out, ws, 8 * 2 * 1 * 18 * 4 - 1, n, h, w, null) == WORKSPACE
    assert swp(x, null, null, null, out, p(0x50004), need, n, h, w, null) == WORKSPACE
    assert swp(p(0x10002), null, null, null, out, ws, need, n, h, w, null) == ALIGN
    assert swp(x, y, p(0x20002), m, out, ws, need, n, h, w, null) == ALIGN
    assert swp(x, null, null, p(0x30001), out, ws, need, n, h, w, null) == ALIGN
    assert swp(x, null, null, null, p(0x40004), ws, need, n, h, w, null) == ALIGN
    ml1 = lib.ct_masked_l1_f32
    for args in ((null, y, m, out), (x, null, m, out), (x, y, null, out), (x, y, m, null)):
        assert ml1(*args, null, 0, n, 3, 280, 1, null) == BADARG
    for dims in ((0, 3, 280, 1), (n, 0, 280, 1), (n, 3, 0, 1), (n, 3, 280, 0), (n, 1 << 30, 1 << 30, 1)):
        assert ml1(x, y, m, out, null, 0, *dims, null) == BADARG
    assert ml1(x, y, m, out, null, 8 * 64 * n, n, 3, 280, 1, null) == WORKSPACE
    assert ml1(x, y, m, out, ws, 8 * 64 * n - 1, n, 3, 280, 1, null) == WORKSPACE
    assert ml1(x, y, m, out, p(0x50004), 8 * 64 * n, n, 3, 280, 1, null) == WORKSPACE
    assert ml1(p(0x10002), y, m, out, ws, 8 * 64 * n, n, 3, 280, 1, null) == ALIGN

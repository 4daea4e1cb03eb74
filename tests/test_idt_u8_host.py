"""CPU-only checks of the uint8 route of the iterative distribution transfer: the declarations of include/ct_hip.h, the workspace
arithmetic of ct_idt_u8_workspace_bytes, the group draw of the rotations and which func_specs `iterative_groups` sends through whole
groups of uint8 frames."""
import re

import numpy as np
import pytest

from tests.test_abi_and_host import HEADER, header_functions

NEW_ENTRIES = ("ct_idt_u8_workspace_bytes", "ct_idt_u8")
REINHARD_SPEC = "methods.linear.color_transfer_between_images"
MK_SPEC = "methods.linear.monge_kantorovitch_color_transfer"
XIAO_SPEC = "methods.linear.color_transfer_in_correlated_color_space"
IDT_SPEC = "methods.iterative.iterative_distribution_transfer"


def test_header_declares_the_entries():
    import ct_hip
    declared = header_functions()
    for name in NEW_ENTRIES:
        assert name in declared, "include/ct_hip.h does not declare %s" % name
        assert name in ct_hip.SIGNATURES
    assert len(ct_hip.SIGNATURES["ct_idt_u8"][1]) == 20 and len(ct_hip.SIGNATURES["ct_idt_u8_workspace_bytes"][1]) == 5
    assert re.search(r"#define CT_ABI_VERSION 9\b", open(HEADER).read())           # entries were only added
    assert callable(ct_hip.idt_u8)


def test_workspace_bytes():
    import ct_hip
    f = ct_hip.lib().ct_idt_u8_workspace_bytes
    for bins in (0, -3, 1025):
        assert f(1, 4, bins, 1000, 0) == 0 and f(1, 4, bins, 1000, 1) == 0
    assert f(1, 4, 255, -1, 1) == 0 and f(-1, 4, 255, 10, 0) == 0
    for batch, n_iter, bins, n_t in ((1, 4, 255, 1), (1, 4, 255, 1920 * 1080), (16, 4, 255, 4099), (3, 5, 1024, 70002), (7, 1, 7, 17)):
        plain, state = f(batch, n_iter, bins, n_t, 0), f(batch, n_iter, bins, n_t, 1)
        assert plain >= ct_hip.lib().ct_idt_workspace_bytes(batch, n_iter, bins) > 0 and plain % 16 == 0
        assert state - plain == (24 * n_t * batch + 15) // 16 * 16           # the float64 working image, on the layout's 16-byte grid
        assert f(batch, n_iter, bins, 2 * n_t, 0) == plain                   # without the state the frame size does not enter


def test_draw_group_rotations():
    import methods.iterative as it
    for k, n_iter in ((5, 4), (1, 4), (3, 2), (0, 4)):
        np.random.seed(1234 + k)
        want = [it.draw_rotations(n_iter) for _ in range(k)]
        after = np.random.random()
        np.random.seed(1234 + k)
        got = it.draw_group_rotations(k, n_iter) if n_iter != 4 else it.draw_group_rotations(k)
        assert got.shape == (k, n_iter, 3, 3) and got.dtype == np.float64
        assert all(np.array_equal(got[i], want[i]) for i in range(k))
        assert np.random.random() == after                                   # the generator is where k single draws leave it


@pytest.mark.parametrize("spec", (REINHARD_SPEC, MK_SPEC, XIAO_SPEC, IDT_SPEC))
def test_takes_groups(spec):
    from methods import Runner
    idt = spec == IDT_SPEC
    for byte_groups in (False, True):
        plain = Runner(spec, metrics="psnr", byte_groups=byte_groups).takes_groups()
        assert Runner(spec, metrics="psnr", byte_groups=byte_groups, iterative_groups=False).takes_groups() is plain
        # the flag adds IDT with PSNR as the only metric, whatever byte_groups says, and changes no other spec
        assert Runner(spec, metrics="psnr", byte_groups=byte_groups, iterative_groups=True).takes_groups() is (True if idt else plain)
        if idt:
            assert plain is False
        for metrics in (None, "psnr,ssim", "ssim", ("psnr", "icid")):
            assert Runner(spec, metrics=metrics, byte_groups=byte_groups, iterative_groups=True).takes_groups() is False

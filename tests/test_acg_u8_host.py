"""CPU-only checks of automated colour grading on uint8 frame groups: the declarations of include/ct_hip.h and the exports of the
built library, the workspace arithmetic of ct_acg_u8_workspace_bytes / ct_regrain_u8_workspace_bytes, and which func_specs
`grading_groups` sends through whole groups of uint8 frames."""
import ctypes
import itertools
import re

import pytest

from tests.test_abi_and_host import HEADER, header_functions

NEW_ENTRIES = {"ct_acg_u8": 21, "ct_acg_u8_workspace_bytes": 6, "ct_regrain_u8": 16, "ct_regrain_u8_workspace_bytes": 4}
REINHARD_SPEC = "methods.linear.color_transfer_between_images"
MK_SPEC = "methods.linear.monge_kantorovitch_color_transfer"
XIAO_SPEC = "methods.linear.color_transfer_in_correlated_color_space"
IDT_SPEC = "methods.iterative.iterative_distribution_transfer"
ACG_SPEC = "methods.iterative.automated_color_grading"
SPECS = (REINHARD_SPEC, MK_SPEC, XIAO_SPEC, IDT_SPEC, ACG_SPEC)


def test_header_declares_and_library_exports_the_entries():
    import ct_hip
    declared = header_functions()
    handle = ctypes.CDLL(ct_hip.LIB_PATH)
    for name, n_args in NEW_ENTRIES.items():
        assert name in declared, "include/ct_hip.h does not declare %s" % name
        assert name in ct_hip.SIGNATURES and len(ct_hip.SIGNATURES[name][1]) == n_args
        assert hasattr(handle, name), "libct_hip.so does not export %s" % name
    assert re.search(r"#define CT_ABI_VERSION 9\b", open(HEADER).read())           # entries were only added
    assert callable(ct_hip.acg_u8) and callable(ct_hip.regrain_u8)


def pyramid_doubles(h, w, n_nbits):
    """per frame: two iterates and the weights on level 0, and on every further level (iterative.py:62-68: while entries are left
    and both halves exceed 20) the two halved images as well"""
    doubles, level = 8 * h * w, 1
    while level < n_nbits and (h + 1) // 2 > 20 and (w + 1) // 2 > 20:
        h, w, level = (h + 1) // 2, (w + 1) // 2, level + 1
        doubles += 14 * h * w
    return doubles


def test_workspace_bytes():
    import ct_hip
    f, g = ct_hip.lib().ct_acg_u8_workspace_bytes, ct_hip.lib().ct_regrain_u8_workspace_bytes
    # refused: batch, frame size, n_iter, bins, n_nbits
    for args in ((0, 40, 45, 4, 255, 6), (-1, 40, 45, 4, 255, 6), (1, 0, 45, 4, 255, 6), (1, 40, -2, 4, 255, 6), (1, 40, 45, 0, 255, 6),
                 (1, 40, 45, -1, 255, 6), (1, 40, 45, 4, 0, 6), (1, 40, 45, 4, 1025, 6), (1, 40, 45, 4, 255, 0), (1, 40, 45, 4, 255, 9),
                 (1, 65536, 65536, 4, 255, 6)):
        assert f(*args) == 0, args
    for args in ((0, 40, 45, 6), (1, 0, 45, 6), (1, 40, 45, 0), (1, 40, 45, 9), (70000, 40, 45, 6)):
        assert g(*args) == 0, args
    for h, w, n_iter, bins, n_nbits in ((40, 45, 4, 255, 6), (5, 7, 1, 7, 1), (83, 171, 4, 255, 6), (83, 171, 4, 255, 2), (1080, 1920, 4, 255, 6),
                                        (420, 500, 5, 1024, 8)):
        last = 0
        for batch in (1, 2, 3, 8, 16):
            need, rg = f(batch, h, w, n_iter, bins, n_nbits), g(batch, h, w, n_nbits)
            assert need > last and need % 16 == 0 and rg % 16 == 0                   # monotone in batch
            last = need
            assert rg >= 8 * batch * pyramid_doubles(h, w, n_nbits)
            # the IDT's own workspace, its float64 result (the state) and the regrain pyramid
            assert need >= ct_hip.lib().ct_idt_u8_workspace_bytes(batch, n_iter, bins, h * w, 0) + 24 * h * w * batch + rg
            assert need >= 24 * h * w * batch + 8 * batch * pyramid_doubles(h, w, n_nbits)
        assert f(1, h, w, n_iter, bins, n_nbits) > ct_hip.lib().ct_idt_u8_workspace_bytes(1, n_iter, bins, h * w, 1)


@pytest.mark.parametrize("spec", SPECS)
def test_takes_groups_truth_table(spec):
    """five specs x the three flags x metrics: the new flag touches the ACG spec only, and the old flags do not touch ACG"""
    from methods import Runner
    for metrics in ("psnr", ("psnr",), None, "psnr,ssim", "ssim", ("psnr", "icid")):
        only_psnr = metrics in ("psnr", ("psnr",))
        for byte_groups, iterative_groups, grading_groups in itertools.product((False, True), repeat=3):
            got = Runner(spec, metrics=metrics, byte_groups=byte_groups, iterative_groups=iterative_groups,
                         grading_groups=grading_groups).takes_groups()
            if spec == ACG_SPEC:
                want = only_psnr and grading_groups
            else:
                want = Runner(spec, metrics=metrics, byte_groups=byte_groups, iterative_groups=iterative_groups).takes_groups()
                assert want is (only_psnr and (spec == REINHARD_SPEC or (spec in (MK_SPEC, XIAO_SPEC) and byte_groups)
                                               or (spec == IDT_SPEC and iterative_groups)))
            assert got is want, (spec, metrics, byte_groups, iterative_groups, grading_groups)
    assert Runner(ACG_SPEC, metrics="psnr", iterative_groups=True).takes_groups() is False        # iterative_groups keeps meaning IDT only
    assert Runner(ACG_SPEC, metrics="psnr").grading_groups is False

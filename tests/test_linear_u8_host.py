"""CPU-only checks of the uint8 MK / Xiao path: the fixture against the float64 oracle, the exact-moments helper against np.cov,
the new declarations of include/ct_hip.h, and which func_specs the Runner sends through whole groups of uint8 frames."""
import os
import re

import numpy as np
import pytest

from oracle import linear as olin
from tests.linear_u8_common import (DECOMPS, GOLDEN, MAX_TIE_SHARE, MK_SPEC, PAIRS, REINHARD_SPEC, RESULTS, XIAO_SPEC, exact_moments,
                                    fixture, rel_error, tie_mask)
from tests.test_abi_and_host import HEADER, header_functions

NEW_ENTRIES = ("ct_rgb_meancov_u8", "ct_affine3x3_u8_f32", "ct_affine3x3_u8_u8", "ct_mk_u8")


def test_fixture_is_small_and_whole():
    assert os.path.getsize(GOLDEN) < 300 * 1024
    fx = fixture()
    assert [fx[p]["target"].shape for p in PAIRS] == [(37, 53, 3), (1, 257, 3), (64, 48, 3)]
    for p in PAIRS:
        for r in RESULTS:
            ref = fx[p][r]
            assert ref.dtype == np.float64 and ref.shape == fx[p]["target"].shape and np.isfinite(ref).all()
            # the stored bytes are the stored float64 result's own: the fit + residual form of the file lost nothing
            assert np.array_equal(fx[p][r + "_u8"], np.rint(np.clip(ref, 0, 1) * 255).astype(np.uint8))
            assert tie_mask(ref).mean() <= MAX_TIE_SHARE


@pytest.mark.parametrize("pair", PAIRS)
def test_oracle_reproduces_the_fixture(pair):
    fx = fixture()[pair]
    t, r = fx["target"] / 255.0, fx["reference"] / 255.0
    for d in DECOMPS:
        err = np.abs(np.real(olin.monge_kantorovitch_color_transfer(t, r, d)) - fx["mk_" + d]).max()
        print("%s mk_%s: oracle - fixture max %.3g" % (pair, d, err))
        assert err <= 1e-10
    err = np.abs(olin.color_transfer_in_correlated_color_space(t, r) - fx["xiao"]).max()
    print("%s xiao: oracle - fixture max %.3g" % (pair, err))
    assert err <= 1e-10


@pytest.mark.parametrize("pair", PAIRS)
def test_exact_moments_agree_with_numpy(pair):
    for role in ("target", "reference"):
        img = fixture()[pair][role]
        mean, cov = exact_moments(img)
        x = (img / 255.0).reshape(-1, 3)
        m_np, c_np = x.mean(axis=0), np.cov(x.T)
        for i in range(3):
            assert abs(m_np[i] - float(mean[i])) <= 1e-12
            for j in range(3):
                assert cov[i][j] == cov[j][i]
                assert abs(c_np[i, j] - float(cov[i][j])) <= 1e-12


def test_exact_moments_closed_forms():
    mean, cov = exact_moments(np.full((4, 5, 3), 255, dtype=np.uint8))
    assert mean == [1, 1, 1] and all(c == 0 for row in cov for c in row)
    half = np.zeros((6, 1, 3), dtype=np.uint8)
    half[3:] = 255
    mean, cov = exact_moments(half)                       # n/2 zeros, n/2 ones: mean 1/2, cov n / (4 (n - 1)) in every entry
    assert all(m * 2 == 1 for m in mean) and all(c * 20 == 6 for row in cov for c in row)
    assert rel_error(0.0, cov[0][0] - cov[0][0]) == 0.0 and rel_error(1e-300, cov[0][0] - cov[0][0]) == float("inf")


def test_header_declares_the_uint8_entries():
    import ct_hip
    declared = header_functions()
    src = open(HEADER).read()
    for name in NEW_ENTRIES:
        assert name in declared, "include/ct_hip.h does not declare %s" % name
        assert name in ct_hip.SIGNATURES
    assert re.search(r"\bCT_WS_MK_U8\s*=\s*6\b", src)
    assert ct_hip.CT_WS_MK_U8 == 6
    assert re.search(r"#define CT_ABI_VERSION 9\b", src)           # entries were only added
    lib = ct_hip.lib()
    one, four = lib.ct_workspace_bytes(ct_hip.CT_WS_MK_U8, 1920 * 1080, 1), lib.ct_workspace_bytes(ct_hip.CT_WS_MK_U8, 1920 * 1080, 4)
    assert 0 < one < four and four == 4 * one
    assert lib.ct_workspace_bytes(ct_hip.CT_WS_MK_U8, 2, 4) == four           # the frame size does not enter
    assert one >= lib.ct_workspace_bytes(ct_hip.CT_WS_RGB_MEANCOV, 1920 * 1080, 2)


SPECS = (REINHARD_SPEC, MK_SPEC, XIAO_SPEC, "methods.iterative.iterative_distribution_transfer")


@pytest.mark.parametrize("spec", SPECS)
def test_takes_groups(spec):
    from methods import Runner
    reinhard = spec == REINHARD_SPEC
    # the default: exactly what it was -- Reinhard with PSNR as the only metric
    assert Runner(spec).takes_groups() is False
    assert Runner(spec, metrics="psnr").takes_groups() is reinhard
    assert Runner(spec, metrics=("psnr",), byte_groups=False).takes_groups() is reinhard
    assert Runner(spec, metrics="psnr,ssim").takes_groups() is False
    # byte_groups adds MK and Xiao, with psnr-only metrics, and nothing else
    want = reinhard or spec in (MK_SPEC, XIAO_SPEC)
    assert Runner(spec, metrics="psnr", byte_groups=True).takes_groups() is want
    assert Runner(spec, byte_groups=True).takes_groups() is False
    assert Runner(spec, metrics="psnr,ssim", byte_groups=True).takes_groups() is False
    assert Runner(spec, metrics="ssim", byte_groups=True).takes_groups() is False

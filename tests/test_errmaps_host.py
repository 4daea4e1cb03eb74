"""The error maps rgbssim, labmse and abmse without a GPU: the restatements of tests/errmaps_common.py pinned to the reference's own
float64 outputs (tests/golden/errmaps.npz, made by tests/golden/make_golden_errmaps.py), the C entries' argument checks, the
binding, the view selection and `utils.cli predict --views` under CT_CLI_DEVICE=cpu.  The kernels are tests/test_errmaps_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import errmaps_common as ec
from tests import views_common as vc
from tests.test_views_host import CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(ec.GOLDEN)


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.tag)
def test_golden_inputs_are_the_ones_the_reference_saw(golden, shape):
    x, y = ec.inputs(shape)
    assert x.shape == (shape[0], 3) + shape[1:] and x.dtype == np.float32 and y.dtype == np.float32
    assert min(x.min(), y.min()) >= 0 and max(x.max(), y.max()) <= 1
    assert vc.digest(x, y) == str(golden["%s/in_sha1" % ec.tag(shape)])


@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.tag)
@pytest.mark.parametrize("name", ec.MAPS)
def test_restatements_reproduce_the_reference_in_float64(golden, name, shape):
    """The same torch calls in the same order: equality is expected (a difference of the last bit, 2.2e-16, at most where another
    torch build orders a convolution's sum or rounds pow differently).  The bound allows ten such bits in the moments, amplified
    by the cancellation in the variances (values of 0.3 over variances of 1e-3) and by the division by the map's range
    (> 1e-2, asserted): 2.2e-16 * 10 * 3e2 * 1e2 < 1e-10."""
    x, y = (torch.from_numpy(a).double() for a in ec.inputs(shape))
    m = ec.unscaled(name, x, y)
    span = float((m.amax(dim=(-1, -2)) - m.amin(dim=(-1, -2))).min())
    want = golden["%s/%s/f64" % (ec.tag(shape), name)]
    got = ec.scaled(m).numpy()
    err = float(np.abs(got - want).max())
    print("%s %s: unscaled range %.3g, restatement vs reference max abs diff %.3g" % (name, ec.tag(shape), span, err))
    assert span > 1e-2                                              # the map's range is far from zero on every input
    assert got.shape == want.shape == (shape[0],) + shape[1:] and err <= 1e-10
    for b in range(shape[0]):                                       # every frame spans exactly [0, 1] on its own
        assert want[b].min() == 0 and want[b].max() == 1
    ref32 = golden["%s/%s/f32" % (ec.tag(shape), name)]
    assert ref32.dtype == np.float32 and ref32.shape == want.shape and 0 < np.abs(ref32 - want).max() < 1e-2


def test_error_gate_is_twice_the_float32_run_with_a_floor():
    ref64 = np.linspace(0, 1, 50).reshape(1, 5, 10)
    ref32 = (ref64 + 1e-5).astype(np.float32)
    assert ec.error_gate((ref64 + 1.9e-5).astype(np.float32), ref32, ref64)[2]
    assert not ec.error_gate((ref64 + 2.2e-5).astype(np.float32), ref32, ref64)[2]
    spike = ref64.copy()
    spike[0, 0, 0] += 1e-4                                          # the rms passes, the maximum does not
    assert not ec.error_gate(spike, ref32, ref64)[2]
    exact = ref64.astype(np.float32)                                # e32 next to nothing: the floor of 1e-6 holds
    assert ec.error_gate(exact + np.float32(5e-7), exact, exact.astype(np.float64))[2]
    assert not ec.error_gate(exact + np.float32(2e-6), exact, exact.astype(np.float64))[2]


# ---- 2. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entries_and_checks_their_arguments():
    """argument errors come back as CT_E_BADARG = -1 before anything is launched: no GPU is needed"""
    import ct_hip
    raw = ctypes.CDLL(ct_hip.LIB_PATH)
    for name in ("ct_view_ssim_map_f32", "ct_view_lab_map_f32"):
        assert hasattr(raw, name) and name in ct_hip.SIGNATURES
    assert (ct_hip.CT_VIEW_LABMSE, ct_hip.CT_VIEW_ABMSE) == (2, 3)
    header = open(os.path.join(ROOT, "include", "ct_hip.h")).read()
    assert "#define CT_VIEW_LABMSE 2" in header and "#define CT_VIEW_ABMSE 3" in header and re.search(r"#define CT_ABI_VERSION 9\b", header)
    lib = ct_hip.lib()
    assert lib.ct_abi_version() == 9
    buf = ctypes.create_string_buffer(256)                          # stands for x, y, out and the workspace: never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.ct_view_workspace_bytes(1)
    assert lib.ct_view_ssim_map_f32(None, None, None, None, 0, 1, 8, 8, None) == -1
    assert lib.ct_view_lab_map_f32(None, None, None, None, 0, 1, 8, 8, 2, None) == -1
    for nulls in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.ct_view_ssim_map_f32(*nulls, need, 1, 8, 8, None) == -1
        assert lib.ct_view_lab_map_f32(*nulls, need, 1, 8, 8, 3, None) == -1
    for b, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.ct_view_ssim_map_f32(p, p, p, p, 64, b, h, w, None) == -1
        assert lib.ct_view_lab_map_f32(p, p, p, p, 64, b, h, w, 2, None) == -1
    assert lib.ct_view_ssim_map_f32(p, p, p, p, need, 1, 5, 8, None) == -1          # reflect padding of 5 needs more than 5 pixels
    assert lib.ct_view_ssim_map_f32(p, p, p, p, need, 1, 8, 5, None) == -1
    assert lib.ct_view_ssim_map_f32(p, p, p, p, need - 1, 1, 8, 8, None) == -1      # a short workspace
    assert lib.ct_view_lab_map_f32(p, p, p, p, need - 1, 1, 8, 8, 2, None) == -1
    assert lib.ct_view_lab_map_f32(p, p, p, p, lib.ct_view_workspace_bytes(3) - 1, 3, 8, 8, 3, None) == -1
    for kind in (0, 1, 4, -1):                                      # RGBMSE and GRAY belong to ct_view_scaled_plane_f32
        assert lib.ct_view_lab_map_f32(p, p, p, p, need, 1, 8, 8, kind, None) == -1


def test_the_binding_has_no_cpu_path():
    import ct_hip
    for fn in (ct_hip.rgbssim_view, ct_hip.labmse_view, ct_hip.abmse_view):
        with pytest.raises(ct_hip.CtHipError):
            fn(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
        with pytest.raises(ct_hip.CtHipError):
            fn(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    from utils import visualizations as viz
    for name in ec.MAPS:
        with pytest.raises(NotImplementedError) as e:
            getattr(viz, name)(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
        assert "kornia" in str(e.value) and getattr(viz, name).__name__ == name


# ---- 3. the view selection ------------------------------------------------------------------------------------------------------------
def test_extra_views_come_only_when_named():
    import methods
    from methods import select_views
    from methods.dcmcs3di import DCMCS3DI
    from methods.dmsct import DMSCT
    assert methods.EXTRA_VIEWS == ("rgbssim", "labmse", "abmse") and set(methods.EXTRA_VIEWS) <= set(methods.GT_VIEWS)
    for cls in (DCMCS3DI, DMSCT, methods.Runner):
        assert not set(cls.VIEWS) & set(methods.EXTRA_VIEWS)
        assert select_views(cls.VIEWS, None, True) == cls.VIEWS                      # the defaults stay what they are
        assert not set(select_views(cls.VIEWS, None, False)) & set(methods.GT_VIEWS)
        assert select_views(cls.VIEWS, "corrected,rgbssim, labmse,abmse", True) == ("corrected", "rgbssim", "labmse", "abmse")
        assert select_views(cls.VIEWS, ("abmse",), True) == ("abmse",)
        for name in methods.EXTRA_VIEWS:
            with pytest.raises(ValueError) as e:
                select_views(cls.VIEWS, name, False)
            assert "gt" in str(e.value) and name in str(e.value)
        with pytest.raises(ValueError) as e:
            select_views(cls.VIEWS, ("rgbssim", "heatmap"), True)
        assert "heatmap" in str(e.value) and all(n in str(e.value) for n in cls.VIEWS + methods.EXTRA_VIEWS)


# ---- 4. predict --views under CT_CLI_DEVICE=cpu ------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", ["rgbssim", "corrected,labmse", "chess,abmse"])
def test_predict_on_the_cpu_refuses_the_device_only_views(tmp_path, monkeypatch, views):
    from utils import cli
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(CFG)
    with pytest.raises(ValueError) as e:
        cli.main(["predict", "--config", str(cfg), "--output", str(tmp_path / "o"), "--views", views])
    assert "device only" in str(e.value) and views.split(",")[-1] in str(e.value)
    assert not os.path.exists(tmp_path / "o")                                        # refused before the first frame

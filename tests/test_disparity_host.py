"""CPU checks of the disparity feature (pasmnet/utils.py:55-105 regress_disp; csrc/disparity.hip):
  * the restatement of the contract in tests/disparity_common.py agrees with the reference's own output (tests/golden/
    disparity.npz): bitwise on one-hot attention maps, hole fill included, <= 1e-5 px on softmax maps;
  * the new C entries check their arguments before anything touches the device."""
import os

import numpy as np
import pytest
import torch

from tests import disparity_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 37, 64, 130, 300)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "disparity.npz"), allow_pickle=False)


def bitwise_equal(a, b):
    """equal as float32 bit patterns, +0 and -0 counted equal"""
    a = np.asarray(a, np.float32) + np.float32(0)
    b = np.asarray(b, np.float32) + np.float32(0)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("w", WIDTHS)
def test_restatement_bitwise_on_onehot_golden(golden, w):
    cols, valid, want = golden["onehot%d/cols" % w], golden["onehot%d/valid" % w], golden["onehot%d/disp" % w]
    got = dc.fill(dc.onehot_index(cols), valid, np.float32)
    assert bitwise_equal(got, want), np.abs(got - want).max()
    # the float64 restatement, same divisor, differs by rounding only
    assert np.abs(dc.fill(dc.onehot_index(cols), valid, np.float64) - want).max() <= 1e-5 * w


def test_golden_covers_the_cases_the_issue_names(golden):
    for w in WIDTHS:
        v = golden["onehot%d/valid" % w].astype(bool)
        assert (~v).all(axis=1).any() and v.all(axis=1).any()              # empty and full rows
        if w > 1:
            assert any(r[0] and not r[1:].any() for r in v) and any(r[-1] and not r[:-1].any() for r in v)
    v = golden["onehot300/valid"].astype(bool)
    hole = [max((len(s) for s in "".join("1" if x else "0" for x in r).split("1")), default=0) for r in v]
    assert max(hole) >= 100
    assert any(not r[0] and not r[-1] and r.any() for r in v)              # holes at both row ends
    assert any(np.array_equal(r, np.arange(300) % 2 == 1) for r in v)        # alternating


def test_restatement_on_softmax_golden(golden):
    att, valid, want = golden["soft/att"], golden["soft/valid"], golden["soft/disp"]
    for dtype in (np.float64, np.float32):
        got = dc.regress_disp(att, valid[:, 0], dtype)[:, None]
        assert np.abs(got - want).max() <= 1e-5, (dtype, np.abs(got - want).max())


@pytest.mark.parametrize("name", ["a", "b"])
def test_model_golden_is_the_fill_of_its_index(golden, name):
    """the model goldens are consistent: disp = fill(disp_ini, valid), bitwise (the reference's disp_ini in float32)"""
    disp, disp_ini, valid = golden["model_%s/disp" % name], golden["model_%s/disp_ini" % name], golden["model_%s/valid" % name]
    assert bitwise_equal(dc.fill(disp_ini, valid, np.float32), disp)
    assert 0.3 < valid.mean() < 0.95


def test_disparity_entries_check_arguments_without_a_gpu():
    import ctypes
    import ct_hip
    lib = ct_hip.lib()
    null = None
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)
    for fn in (lib.ct_pam_disp_fill_f32, lib.ct_pam_regress_disp_f32):
        assert fn(null, null, null, 0, 4, 8, null) == 0                   # an empty batch is a no-op
        assert fn(null, null, null, 2, 0, 8, null) == 0
        assert fn(null, null, null, -1, 4, 8, null) == -1                 # negative sizes
        assert fn(p, p, p, 1, -1, 8, null) == -1
        assert fn(p, p, p, 1, 4, -8, null) == -1
        assert fn(null, p, p, 1, 4, 8, null) == -1                        # null pointers
        assert fn(p, null, p, 1, 4, 8, null) == -1
        assert fn(p, p, null, 1, 4, 8, null) == -1
        assert fn(p, p, p, 1, 1, 32769, null) == -1                       # beyond the widest row
    rows = lib.ct_attention_rows64_disp_f32
    assert rows(null, null, null, null, null, 0, 16, 1.0 / 64, null) == 0  # an empty batch is a no-op
    assert rows(p, p, null, null, p, -1, 16, 1.0 / 64, null) == -1
    assert rows(p, p, null, null, p, 1, 0, 1.0 / 64, null) == -1
    assert rows(null, p, null, null, p, 1, 16, 1.0 / 64, null) == -1
    assert rows(p, null, null, null, p, 1, 16, 1.0 / 64, null) == -1
    assert rows(p, p, null, null, null, 1, 16, 1.0 / 64, null) == -1       # no disp_ini
    assert rows(p, p, p, null, p, 1, 16, 1.0 / 64, null) == -1             # v without out
    assert ct_hip.CT_ABI_VERSION == 9 and lib.ct_abi_version() == 9


def test_python_entries_refuse_cpu_tensors():
    import ct_hip
    from pasmnet.utils import regress_disp
    att = torch.zeros(1, 2, 5, 5)
    valid = torch.ones(1, 1, 2, 5, dtype=torch.bool)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.regress_disp(att, valid)
    with pytest.raises(ct_hip.CtHipError):
        regress_disp(att, valid.float())
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.pam_disp_fill(torch.zeros(1, 1, 2, 5), valid)
    if not torch.cuda.is_available():
        from methods.dcmcs3di import DCMCS3DI
        with pytest.raises(ct_hip.CtHipError):
            DCMCS3DI(extraction_layers=1, transfer_layers=1).disparity(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))

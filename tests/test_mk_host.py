"""CPU side of the Monge-Kantorovich tests: the mpmath oracle of the 3x3 algebra is tied to recorded output of the reference,
and the batch the device algebra is held to (tests/mk_common.py) is what tests/test_mk_gpu.py says it is."""
import os

import numpy as np
import pytest

from oracle import linear as olin

from tests import mk_common as mc


@pytest.mark.parametrize("case", ["uniform", "graded"])
@pytest.mark.parametrize("decomposition", mc.DECOMPS)
def test_mk_matrix_mp_reproduces_reference_output(golden_dir, case, decomposition):
    """(t - mean_t) @ mk_matrix_mp(cov_t, cov_r) + mean_r with numpy float64 moments against what the reference wrote."""
    g = np.load(os.path.join(golden_dir, "linear_small.npz"), allow_pickle=False)
    t = g[case + "/target"].astype(np.float64).reshape(-1, 3)
    r = g[case + "/reference"].astype(np.float64).reshape(-1, 3)
    T = olin.mk_matrix_mp(np.cov(t.T), np.cov(r.T), decomposition)
    assert T.dtype == np.float64 and T.shape == (3, 3)
    out = (t - t.mean(axis=0)) @ T + r.mean(axis=0)
    np.testing.assert_allclose(out.reshape(g[case + "/target"].shape), g[case + "/mk_" + decomposition], rtol=0, atol=1e-11)


def test_mk_matrix_mp_rejects_unknown_decomposition():
    with pytest.raises(ValueError):
        olin.mk_matrix_mp(np.eye(3), np.eye(3), "nope")


def test_algebra_batch_is_what_the_device_test_needs():
    st, sr, cond, kind = mc.algebra_batch()
    assert st.shape == sr.shape == (mc.N_RECORDS, 16) and mc.N_RECORDS >= 130 > max(mc.BLOCK_EDGES)
    ct, cr = st[:, 3:12].reshape(-1, 3, 3), sr[:, 3:12].reshape(-1, 3, 3)
    assert np.array_equal(ct, ct.transpose(0, 2, 1)) and np.array_equal(cr, cr.transpose(0, 2, 1))      # symmetric exactly
    assert np.linalg.cond(cr).max() <= 100 * (1 + 1e-9)
    for c in mc.CONDS:                                             # every condition number is there, as built
        sel = np.array([k == "cond %g" % c for k in kind])
        assert sel.sum() >= 20
        got = np.linalg.cond(ct[sel])
        assert np.all(np.abs(got / c - 1) <= 8 * mc.EPS * c + 1e-12), (c, got)      # roundings of S and of the SVD: a few ulp of lambda_max
    assert {"cond 1", "cond 1e+10"} <= {kind[i] for i in mc.BLOCK_EDGES}                                 # both ends of the range at a block edge
    assert np.linalg.eigvalsh(ct).min() > 0 and np.linalg.eigvalsh(cr).min() > 0
    dt, dr = mc.degenerate_batch()
    changed = np.flatnonzero((dt != st).any(axis=1) | (dr != sr).any(axis=1))
    assert changed.tolist() == sorted([mc.ZERO_TARGET, mc.ZERO_REFERENCE, mc.RANK1_TARGET])
    assert np.linalg.matrix_rank(dt[mc.RANK1_TARGET, 3:12].reshape(3, 3)) == 1


@pytest.mark.parametrize("decomposition", mc.DECOMPS)
def test_reference_algebra_meets_its_own_bound_shape(decomposition):
    """The bound of the device test is C 2^-52 cond_2(S_t) with C = 4 x the worst normalised error of the reference's own
    algebra over the batch: that worst value must be a small number for the bound to mean anything (a constant in the
    hundreds would say that cond_2(S_t) is the wrong scale, or mk_matrix_mp the wrong oracle)."""
    worst = mc.reference_algebra_error(decomposition)
    print("reference algebra, %s: worst normalised error %.3f, C = %.3f" % (decomposition, worst, 4 * worst))
    assert 0.25 <= worst <= 32.0

"""What tests/test_mk_host.py and tests/test_mk_gpu.py share: the seeded batch of rgb_meancov records that the device 3x3 algebra
(csrc/mk.hip: mk_coef_kernel) is held to, its mpmath expectation, and the reference algebra's own error on that batch, from
which the bound of the device test is taken.  Everything here runs on the CPU and is computed once per process."""
import functools

import numpy as np

from oracle import linear as olin

DECOMPS = ("MK", "sqrt", "cholesky")
CONDS = (1.0, 1e2, 1e4, 1e6, 1e8, 1e10)
EPS = 2.0 ** -52
N_SPECIAL = 14
N_RECORDS = 134                       # three 64-thread blocks of mk_coef_kernel, the last one with 6 live threads
BLOCK_EDGES = (63, 64, 65, 127, 128, 129)
ZERO_TARGET, ZERO_REFERENCE, RANK1_TARGET = 62, 66, 130     # where the degenerate batch differs from the ordinary one


def _orthogonal(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


def _spd(rng, lam):
    """Q diag(lam) Q^T with a random orthogonal Q, symmetrised exactly."""
    q = _orthogonal(rng)
    s = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return (s + s.T) / 2


def _reference_cov(rng):
    """condition number <= 100: with both sides ill-conditioned the closed forms themselves lose the digits"""
    lam = 0.02 * 10.0 ** rng.uniform(0.0, 2.0, 3)
    return _spd(rng, lam)


@functools.lru_cache(maxsize=None)
def algebra_batch():
    """(stats_t [B,16], stats_r [B,16], cond_t [B], kind [B]) float64: mean[3], cov[9] row-major, n, 0 0 0."""
    rng = np.random.default_rng(20260)
    cov_t, cov_r, cond, kind = [], [], [], []

    def add(name, ct, c, cr=None):
        cov_t.append(np.asarray(ct, dtype=np.float64))
        cov_r.append(_reference_cov(rng) if cr is None else cr)
        cond.append(c)
        kind.append(name)

    # -- special structure (N_SPECIAL records) --
    add("diagonal", np.diag([0.3, 0.02, 0.7]), 35.0)                         # apq == 0 everywhere, off <= tiny at once
    add("c*I", 0.25 * np.eye(3), 1.0)
    add("diagonal, two equal", np.diag([0.5, 0.5, 0.01]), 50.0)
    add("two equal, rotated block", [[0.5, 0, 0], [0, 0.3, 0.2], [0, 0.2, 0.3]], 5.0)     # eigenvalues 0.5, 0.5, 0.1
    add("two equal, random Q", _spd(rng, [0.4, 0.4, 0.004]), 100.0)
    add("two equal small, random Q", _spd(rng, [0.4, 0.004, 0.004]), 100.0)
    s = 1e-9
    add("scale 1e-9, both", s * _spd(rng, [1.0, 0.3, 0.01]), 100.0, s * _reference_cov(rng))
    add("scale 1e-9, target", s * _spd(rng, [1.0, 0.1, 0.01]), 100.0)
    s = 5e3
    add("scale 5e3, both", s * _spd(rng, [1.0, 0.3, 0.01]), 100.0, s * _reference_cov(rng))
    add("scale 5e3, cond 1e6", s * _spd(rng, [1.0, 1e-3, 1e-6]), 1e6, s * _reference_cov(rng))
    t = np.diag([0.3, 0.02, 0.7])
    t[0, 1] = t[1, 0] = 1e-300                                               # theta = 0.14 / 1e-300 overflows when squared
    add("off-diagonal 1e-300", t, 35.0)
    t = np.diag([0.6, 0.05, 0.2])
    t[1, 2] = t[2, 1] = -3e-300
    t[0, 2] = t[2, 0] = 0.01
    add("off-diagonal 1e-300 beside a real one", t, float(np.linalg.cond(t)))
    add("diagonal reference", _spd(rng, [0.2, 0.1, 0.01]), 20.0, np.diag([0.04, 0.09, 0.01]))
    add("identical", cov_r[4], float(np.linalg.cond(cov_r[4])), cov_r[4])   # T = I
    assert len(cov_t) == N_SPECIAL
    # -- condition numbers, cycled so that every block edge sees a different one --
    i = 0
    while len(cov_t) < N_RECORDS:
        c = CONDS[i % len(CONDS)]
        i += 1
        mid = 10.0 ** (-rng.uniform(0.0, np.log10(c)))
        add("cond %g" % c, _spd(rng, 0.1 * np.array([1.0, mid, 1.0 / c])), c)
    b = len(cov_t)
    st, sr = np.zeros((b, 16)), np.zeros((b, 16))
    st[:, 0:3], sr[:, 0:3] = rng.uniform(0, 1, (b, 3)), rng.uniform(0, 1, (b, 3))
    st[:, 3:12], sr[:, 3:12] = np.reshape(cov_t, (b, 9)), np.reshape(cov_r, (b, 9))
    st[:, 12], sr[:, 12] = 3072.0, 3072.0
    for a in (st, sr):
        a.setflags(write=False)
    return st, sr, np.array(cond), tuple(kind)


@functools.lru_cache(maxsize=None)
def degenerate_batch():
    """algebra_batch() with three records made degenerate: an all-zero target covariance, an all-zero reference covariance,
    an exactly rank-1 target (a grey frame: all nine entries equal)."""
    st, sr, _, _ = algebra_batch()
    st, sr = st.copy(), sr.copy()
    st[ZERO_TARGET, 3:12] = 0.0
    sr[ZERO_REFERENCE, 3:12] = 0.0
    st[RANK1_TARGET, 3:12] = 0.0625
    return st, sr


@functools.lru_cache(maxsize=None)
def algebra_expected(decomposition):
    """oracle.linear.mk_matrix_mp of every record of algebra_batch(): float64 [B, 3, 3]."""
    st, sr, _, _ = algebra_batch()
    out = np.stack([olin.mk_matrix_mp(st[b, 3:12].reshape(3, 3), sr[b, 3:12].reshape(3, 3), decomposition)
                    for b in range(st.shape[0])])
    out.setflags(write=False)
    return out


def normalised_error(T, T_mp, cond):
    """max|T - T_mp| / max|T_mp| in units of 2^-52 cond_2(S_t), per record"""
    T, T_mp = np.asarray(T).reshape(-1, 3, 3), np.asarray(T_mp).reshape(-1, 3, 3)
    return np.abs(T - T_mp).max(axis=(1, 2)) / np.abs(T_mp).max(axis=(1, 2)) / (EPS * np.asarray(cond))


@functools.lru_cache(maxsize=None)
def reference_algebra_error(decomposition):
    """Worst normalised error of the reference's own algebra (oracle.linear.mk_matrix: scipy / numpy) over algebra_batch()."""
    st, sr, cond, _ = algebra_batch()
    T = np.stack([np.real(olin.mk_matrix(st[b, 3:12].reshape(3, 3), sr[b, 3:12].reshape(3, 3), decomposition))
                  for b in range(st.shape[0])])
    return float(normalised_error(T, algebra_expected(decomposition), cond).max())


def algebra_bound(decomposition):
    """C of the device test: 4 x the reference's own worst error; the margin is for Jacobi's summation order, which is
    different from Schur's and equally valid."""
    return 4.0 * reference_algebra_error(decomposition)

"""The Monge-Kantorovich family on the device (csrc/mk.hip, the RGB sweep of csrc/ct_moments.h) against oracles: the 3x3 algebra
of ct_hip.mk_coef against mpmath, the float32 I/O path of affine3x3_kernel (per-wave LDS transpose, its hand-over to the
per-lane path, the grid-stride loop) per pixel, the fused entries in the configuration bench.py times, and the argument
checks of the Python wrappers.  The batch of covariances and its bound are tests/mk_common.py (CPU side: test_mk_host.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import linear as olin          # noqa: E402
from tests import mk_common as mc          # noqa: E402

TOL = 1e-9                                 # the project's bound on float64 results (tests/test_linear_gpu.py)
# [B, H, W]: 256 images cap the grid at 8 workgroups per image, so 2256 / 2255 four-pixel chunks take two trips of the
# grid-stride loop, the second one three full waves and a 16 / 15 lane one.  96 x 94: every image 16-byte aligned.  97 x 93: a
# one-pixel tail, and only every fourth image aligned, so the transpose path and the per-lane path alternate in one launch.
BENCH_SHAPES = [(256, 96, 94), (256, 97, 93)]


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


@pytest.fixture(scope="module")
def lin():
    import methods.linear as m
    return m


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the shared inputs are read-only


# ------------------------------------------------------------------------------------------------------------------------
# 2. mk_coef_kernel against mpmath
# ------------------------------------------------------------------------------------------------------------------------
def _check_record_copy(coef, st, sr):
    assert coef.shape == (st.shape[0], 16) and coef.dtype == np.float64
    assert np.array_equal(coef[:, 9:12], st[:, 0:3])           # mu_t, bit for bit
    assert np.array_equal(coef[:, 12:15], sr[:, 0:3])          # mu_r
    assert np.array_equal(coef[:, 15], np.zeros(st.shape[0]))  # pad


@pytest.mark.parametrize("decomposition", mc.DECOMPS)
def test_mk_coef_vs_mpmath(hip, decomposition):
    """max|T_dev - T_mp| / max|T_mp| <= C 2^-52 cond_2(S_t) on every record of the batch (134: three blocks of 64 threads),
    T_mp = oracle.linear.mk_matrix_mp at 60 digits.  C = 4 x the worst such error of the reference's own algebra
    (oracle.linear.mk_matrix: scipy sqrtm / numpy) over the same batch, measured on the CPU (tests/mk_common.py):
        reference worst   MK 5.107   sqrt 6.746   cholesky 0.999      ->      C   MK 20.43   sqrt 26.98   cholesky 3.995
    (the worst cases are the condition-1 records, where the bound is a few ulp of T; from 1e2 up both algebras stay below 1.5).
    Measured on an MI355X: worst 6.875 (MK), 6.875 (sqrt), 1.778 (cholesky); from condition 1e2 up 1.27, 0.19, 0.11.
    A numpy transcription of the kernel as it was before this test (the Jacobi sweep rotating away every non-zero
    off-diagonal entry) gives 20.64 (MK) on the c I + rounding-noise records, above C, and 6.875 with the threshold."""
    st, sr, cond, kind = mc.algebra_batch()
    coef = hip.mk_coef(dev(st), dev(sr), decomposition).cpu().numpy()
    _check_record_copy(coef, st, sr)
    T, T_mp = coef[:, 0:9].reshape(-1, 3, 3), mc.algebra_expected(decomposition)
    err = mc.normalised_error(T, T_mp, cond)
    C = mc.algebra_bound(decomposition)
    print("\n[%s] C = %.3f, device worst %.3f at record %d (%s)" % (decomposition, C, np.nanmax(err), np.nanargmax(err), kind[np.nanargmax(err)]))
    for c in mc.CONDS:
        print("    cond %-6g worst %.3f" % (c, max(err[i] for i in range(len(kind)) if kind[i] == "cond %g" % c)))
    print("    special records: " + ", ".join("%s %.3f" % (kind[i], err[i]) for i in range(mc.N_SPECIAL)))
    for i in mc.BLOCK_EDGES:                                   # either side of the 64-thread block boundaries, by index
        assert err[i] <= C, (i, kind[i], err[i])
    bad = [(i, kind[i], err[i]) for i in range(len(kind)) if not err[i] <= C]
    assert not bad, bad
    if decomposition != "MK":                                  # T = B A^-1 is not symmetric: row-major, applied as x @ T
        generic = np.array([k.startswith("cond ") and k != "cond 1" for k in kind])      # S_t = c I makes sqrt's T symmetric
        assert mc.normalised_error(T.transpose(0, 2, 1), T_mp, cond)[generic].min() > C


@pytest.mark.parametrize("decomposition", mc.DECOMPS)
def test_mk_coef_degenerate_records(hip, decomposition):
    """A constant target (covariance 0) gives an all-NaN T, a constant reference T == 0, a grey target (rank 1) whatever
    the rounding decides -- and no record of the batch notices its neighbours (include/ct_hip.h: ct_mk_coef_f64)."""
    st, sr, _, _ = mc.algebra_batch()
    dt, dr = mc.degenerate_batch()
    good = hip.mk_coef(dev(st), dev(sr), decomposition).cpu().numpy()
    coef = hip.mk_coef(dev(dt), dev(dr), decomposition).cpu().numpy()          # returns: CT_OK with the rank-1 record in it
    _check_record_copy(coef, dt, dr)
    assert np.isnan(coef[mc.ZERO_TARGET, 0:9]).all(), coef[mc.ZERO_TARGET, 0:9]
    assert np.array_equal(coef[mc.ZERO_REFERENCE, 0:9], np.zeros(9)), coef[mc.ZERO_REFERENCE, 0:9]
    others = np.setdiff1d(np.arange(st.shape[0]), [mc.ZERO_TARGET, mc.ZERO_REFERENCE, mc.RANK1_TARGET])
    assert np.array_equal(coef[others].view(np.uint64), good[others].view(np.uint64))
    assert np.isfinite(good).all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. affine3x3_kernel, float32 in and out
# ------------------------------------------------------------------------------------------------------------------------
def _affine_case(B, n, seed):
    """per-pixel distinct float32 input [B, 1, n, 3], per-image asymmetric well-conditioned coef [B, 16], float64 expectation"""
    rng = np.random.default_rng(seed)
    x = rng.random((B, 1, n, 3), dtype=np.float32)
    A = np.array([[0.9, 0.2, -0.1], [-0.3, 1.1, 0.25], [0.15, -0.2, 0.8]]) + 0.05 * rng.standard_normal((B, 3, 3))
    coef = np.zeros((B, 16))
    coef[:, 0:9] = A.reshape(B, 9)
    coef[:, 9:12] = rng.uniform(0.2, 0.8, (B, 3))
    coef[:, 12:15] = rng.uniform(0.2, 0.8, (B, 3))
    want = np.einsum("bni,bij->bnj", x.astype(np.float64).reshape(B, n, 3) - coef[:, None, 9:12], A) + coef[:, None, 12:15]
    return x, coef, want.reshape(x.shape)


def _check_affine(hip, x, coef, want, xd=None, out=None):
    """float64 out within 1e-9 of numpy; float32 out == that float64 result rounded once, bit for bit"""
    xd = dev(x) if xd is None else xd
    cd = dev(coef)
    o64 = hip.affine3x3(xd, cd, out_dtype=torch.float64)
    o32 = hip.affine3x3(xd, cd, out_dtype=torch.float32, out=out)
    assert o32.dtype == torch.float32 and o32.shape == xd.shape and o64.dtype == torch.float64
    err = np.abs(o64.cpu().numpy() - want).max()
    assert err <= TOL, err
    same = o32.view(torch.int32) == o64.to(torch.float32).view(torch.int32)
    assert bool(same.all()), "%d of %d float32 elements differ from the rounded float64 result, first at flat index %d" % (
        int((~same).sum()), same.numel(), int((~same).flatten().nonzero()[0]))
    return o32


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 260])
def test_affine_f32_one_image(hip, n):
    """tail only / one chunk (1..5 pixels); below, at and above one full wave of 64 four-pixel chunks (255..260)"""
    _check_affine(hip, *_affine_case(1, n, 100 + n))


@pytest.mark.parametrize("shape", BENCH_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_affine_f32_grid_stride_and_alignment(hip, shape):
    B, H, W = shape
    x, coef, want = _affine_case(B, H * W, 7 + H)
    xd = dev(x)
    assert [(xd.data_ptr() + 12 * H * W * b) % 16 == 0 for b in range(4)] == ([True] * 4 if H * W % 4 == 0 else [True, False, False, False])
    _check_affine(hip, x, coef, want, xd=xd)


def _view_in(numel, offset, dtype, fill):
    """a contiguous view of `numel` elements that starts `offset` elements into a buffer filled with `fill`; behind the view
    lies more than a wave's 64 chunks of 12 floats, so that a transpose pass that ran beyond the last chunk of the last image
    would land on sentinels, inside the buffer"""
    buf = torch.full((numel + offset + 1024,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[offset:offset + numel]


def _untouched(buf, offset, numel, fill):
    return bool((buf[:offset] == fill).all()) and bool((buf[offset + numel:] == fill).all())


@pytest.mark.parametrize("in_off,out_off", [(0, 1), (1, 0), (0, 64), (1, 1), (3, 2)])
@pytest.mark.parametrize("n", [1028, 1029])
def test_affine_f32_offset_views_and_sentinels(hip, n, in_off, out_off):
    """Input and output 16-byte aligned or not, independently (an offset of 1 float is 4 bytes): n = 1028 keeps every image of
    the batch at the alignment of the first one, n = 1029 walks the four residues.  `out` lies inside a buffer of sentinels:
    nothing outside the view may change (257 chunks: four full waves and a one-lane fifth, plus a one-pixel tail for 1029)."""
    B, fill = 4, -12345.0
    x, coef, want = _affine_case(B, n, 31 * n + 5 * in_off + out_off)
    _, xin = _view_in(x.size, in_off, torch.float32, 0.0)
    xin.copy_(dev(x).flatten())
    xin = xin.view(x.shape)
    obuf, out = _view_in(x.size, out_off, torch.float32, fill)
    assert xin.data_ptr() % 16 == 4 * in_off % 16 and out.data_ptr() % 16 == 4 * out_off % 16
    assert xin.is_contiguous() and out.is_contiguous()
    o32 = _check_affine(hip, x, coef, want, xd=xin, out=out.view(x.shape))
    assert o32.data_ptr() == out.data_ptr()
    assert _untouched(obuf, out_off, x.size, fill)


# ------------------------------------------------------------------------------------------------------------------------
# 4. the fused entries
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pairs(B, H, W):
    """float32 pairs [B, H, W, 3], every pair with its own gains, offsets and channel mixing (so that a mix-up between the
    pairs of a batch cannot pass), read-only"""
    rng = np.random.default_rng(1000 * B + H * W)
    out = []
    for _ in range(2):
        u = rng.random((B, H, W, 3), dtype=np.float32)
        gain = rng.uniform(0.3, 1.0, (B, 1, 1, 3)).astype(np.float32)
        off = rng.uniform(0.0, 0.3, (B, 1, 1, 3)).astype(np.float32)
        mix = rng.uniform(0.0, 0.5, (B, 1, 1)).astype(np.float32)
        x = u * gain
        x[..., 1] += mix * x[..., 0]
        x = (x * np.float32(0.7) + off).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _pairs_expected(B, H, W, decomposition):
    t, r = _pairs(B, H, W)
    e = np.stack([olin.monge_kantorovitch_color_transfer(t[b], r[b], decomposition) for b in range(B)])
    e.setflags(write=False)
    return e


def _out_tol(expected, dtype):
    """1e-9, plus half a float32 ulp of the expected value where the result is rounded to float32"""
    if dtype == torch.float64:
        return TOL
    return TOL + 0.5 * np.spacing(np.abs(expected).astype(np.float32)).astype(np.float64)


def _check_pairs(got, expected):
    g = got.cpu().numpy().astype(np.float64)
    excess = np.abs(g - expected) - _out_tol(expected, got.dtype)
    assert excess.max() <= 0, "pair %d: error %.3e" % (np.unravel_index(excess.argmax(), excess.shape)[0], np.abs(g - expected).max())


IO = {"f32-f32": (torch.float32, torch.float32), "f32-f64": (torch.float32, torch.float64), "f64-f64": (torch.float64, torch.float64)}


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("decomposition", mc.DECOMPS)
@pytest.mark.parametrize("io", list(IO))
def test_mk_fused_entries_vs_oracle(hip, lin, io, decomposition, B):
    """ct_mk_f32_f32 / _f32_f64 / _f64_f64 at 257 pixels per image, with `out` given and omitted, through ct_hip.mk and through
    methods.linear.monge_kantorovitch_color_transfer_cuda: every pair against the float64 oracle."""
    in_dtype, out_dtype = IO[io]
    t, r = _pairs(B, 1, 257)
    expected = _pairs_expected(B, 1, 257, decomposition)
    td, rd = dev(t).to(in_dtype), dev(r).to(in_dtype)
    for fn in (hip.mk, lin.monge_kantorovitch_color_transfer_cuda):
        got = fn(td, rd, decomposition, out_dtype=out_dtype)
        assert got.dtype == out_dtype and got.shape == td.shape
        _check_pairs(got, expected)
        buf = torch.full(td.shape, float("nan"), dtype=out_dtype, device="cuda")
        got = fn(td, rd, decomposition, out=buf)                # out_dtype left at its default: `out` decides
        assert got.data_ptr() == buf.data_ptr() and got.dtype == out_dtype
        _check_pairs(buf, expected)


@pytest.mark.parametrize("shape", BENCH_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_mk_bench_configuration_vs_oracle(lin, shape):
    """What bench.py times as mk_pairs_per_s_f32out_device_algebra: float32 in, float32 out into `out=`, "MK", a batch; here
    at the smallest frames that run the sweeps' grid-stride loops twice.  Every pixel of every pair; a second call is bit-identical."""
    t, r = _pairs(*shape)
    expected = _pairs_expected(*shape, "MK")
    td, rd = dev(t), dev(r)
    out = torch.full(td.shape, float("nan"), dtype=torch.float32, device="cuda")
    got = lin.monge_kantorovitch_color_transfer_cuda(td, rd, out_dtype=torch.float32, out=out)
    assert got.data_ptr() == out.data_ptr()
    _check_pairs(out, expected)
    again = lin.monge_kantorovitch_color_transfer_cuda(td, rd, out_dtype=torch.float32, out=torch.empty_like(out))
    assert torch.equal(again.view(torch.int32), out.view(torch.int32))


def _np_meancov(x):
    x = x.astype(np.float64).reshape(x.shape[0], -1, 3)
    return np.stack([np.mean(i, axis=0) for i in x]), np.stack([np.cov(i.T) for i in x])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(1, 1, 257), (3, 1, 257), (65, 1, 257)] + BENCH_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_rgb_meancov_vs_numpy(hip, shape, dtype):
    t, _ = _pairs(*shape)
    s = hip.rgb_meancov(dev(t.astype(dtype))).cpu().numpy()
    mean, cov = _np_meancov(t)
    np.testing.assert_allclose(s[:, 0:3], mean, rtol=0, atol=1e-13)
    np.testing.assert_allclose(s[:, 3:12].reshape(-1, 3, 3), cov, rtol=0, atol=1e-13)
    assert np.array_equal(s[:, 12], np.full(shape[0], float(shape[1] * shape[2]))) and not s[:, 13:].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rgb_meancov_near_constant_frames(hip, dtype):
    """0.7 + 1e-6 noise: the case the pivot form of the sweep exists for (ct_moments.h).  The bound is measured, not chosen:
    the shifted-sum formula of moments_finalize_kernel in numpy float64 against a two-pass np.longdouble covariance of the
    same frames, 8 x its error, relative to the largest covariance entry of the frame (and no less than 8 x half an ulp, which no
    float64 result can beat)."""
    rng = np.random.default_rng(77)
    B, H, W = 16, 97, 93
    x = (0.7 + 1e-6 * rng.standard_normal((B, H, W, 3))).astype(dtype)
    s = hip.rgb_meancov(dev(x)).cpu().numpy()
    flat = x.reshape(B, -1, 3)
    n = flat.shape[1]
    e_formula, e_device = 0.0, 0.0
    for b in range(B):
        xl = flat[b].astype(np.longdouble)
        dl = xl - xl.mean(axis=0)
        cov_ld = (dl.T @ dl) / (n - 1)
        scale = float(np.abs(cov_ld).max())
        d = flat[b].astype(np.float64) - flat[b, 0].astype(np.float64)           # the pivot is pixel 0
        s1, s2 = d.sum(axis=0), d.T @ d
        cov_f = (s2 - np.outer(s1, s1 / n)) / (n - 1)
        e_formula = max(e_formula, float(np.abs(cov_f - cov_ld).max()) / scale)
        e_device = max(e_device, float(np.abs(s[b, 3:12].reshape(3, 3) - cov_ld).max()) / scale)
        np.testing.assert_allclose(s[b, 0:3], xl.mean(axis=0).astype(np.float64), rtol=0, atol=1e-13)
    bound = 8 * max(e_formula, 2.0 ** -53)
    print("\n[%s] shifted-sum formula in numpy: %.3e, device: %.3e, bound %.3e (relative to the largest entry)" % (np.dtype(dtype).name, e_formula, e_device, bound))
    # measured: formula 5.66e-16 (float32 frames), 1.81e-15 (float64 frames) -> bounds 4.53e-15, 1.45e-14; device 5.64e-16, 6.81e-16
    assert e_device <= bound, (e_device, bound)


@pytest.mark.parametrize("decomposition", mc.DECOMPS)
def test_mk_constant_target_inside_a_batch(hip, decomposition):
    """A constant target frame has covariance exactly 0 (the pivot is its own value): that pair's output is NaN, the pairs
    around it are what they are with an ordinary frame in its place, bit for bit."""
    t, r = _pairs(3, 1, 257)
    flat = t.copy()
    flat[1] = np.float32(0.3)
    good = hip.mk(dev(t), dev(r), decomposition, out_dtype=torch.float32).cpu().numpy()
    got = hip.mk(dev(flat), dev(r), decomposition, out_dtype=torch.float32).cpu().numpy()
    assert np.isnan(got[1]).all()
    assert np.isfinite(good).all()
    assert np.array_equal(got[[0, 2]].view(np.uint32), good[[0, 2]].view(np.uint32))


@pytest.mark.parametrize("decomposition", mc.DECOMPS)
def test_mk_near_grey_target_vs_mpmath(hip, decomposition):
    """R = G = B plus 1e-3 of chroma noise: cond_2(S_t) about 1e6, where 1e-9 is no longer the right bound.  Expected
    (x - mu_t) @ mk_matrix_mp(S_t, S_r) + mu_r from numpy float64 moments; tolerance: the bound of test_mk_coef_vs_mpmath on
    T, C 2^-52 cond_2(S_t) max|T|, times 3 max|x - mu_t| (three terms per output channel)."""
    rng = np.random.default_rng(4242)
    H, W = 97, 93
    grey = rng.random((H, W, 1), dtype=np.float32)
    t = (grey + np.float32(1e-3) * rng.standard_normal((H, W, 3)).astype(np.float32)).astype(np.float32)
    r = _pairs(1, H, W)[1][0]
    (mt, ct), (mr, cr) = olin.rgb_mean_cov(t), olin.rgb_mean_cov(r)
    cond = np.linalg.cond(ct)
    assert 1e5 <= cond <= 1e7
    T = olin.mk_matrix_mp(ct, cr, decomposition)
    d = t.astype(np.float64).reshape(-1, 3) - mt
    expected = (d @ T + mr).reshape(t.shape)
    tol = mc.algebra_bound(decomposition) * mc.EPS * cond * np.abs(T).max() * 3 * np.abs(d).max()
    got = hip.mk(dev(t), dev(r), decomposition, out_dtype=torch.float64).cpu().numpy()
    err = np.abs(got - expected).max()
    print("\n[%s] cond %.3g, max|T| %.3g, error %.3e, tolerance %.3e" % (decomposition, cond, np.abs(T).max(), err, tol))
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------------------------------------------------------------
# 5. the wrappers refuse what the kernels would run off the end of
# ------------------------------------------------------------------------------------------------------------------------
def _bad_outs(shape):
    numel = int(np.prod(shape))
    return {
        "on the host": lambda: torch.empty(shape, dtype=torch.float32),
        "not contiguous": lambda: torch.empty(shape[:-1] + (6,), dtype=torch.float32, device="cuda")[..., ::2],
        "float16": lambda: torch.empty(shape, dtype=torch.float16, device="cuda"),
        "int32": lambda: torch.empty(shape, dtype=torch.int32, device="cuda"),
        "one pixel short": lambda: torch.empty(numel - 3, dtype=torch.float32, device="cuda"),
        "one image long": lambda: torch.empty((shape[0] + 1,) + shape[1:], dtype=torch.float32, device="cuda"),
        "float64 of the byte count of float32": lambda: torch.empty(numel // 2, dtype=torch.float64, device="cuda"),
    }


BAD_OUTS = list(_bad_outs((2, 4, 6, 3)))


@pytest.mark.parametrize("what", BAD_OUTS)
def test_wrappers_refuse_a_wrong_out(hip, what):
    shape = (2, 4, 6, 3)
    x = torch.rand(shape, device="cuda")
    coef = dev(_affine_case(2, 24, 0)[1])
    out = _bad_outs(shape)[what]()
    if what == "not contiguous":
        assert out.numel() == x.numel() and not out.is_contiguous()
    with pytest.raises(hip.CtHipError):
        hip.mk(x, x.flip(1), "MK", out=out)
    with pytest.raises(hip.CtHipError):
        hip.affine3x3(x, coef, out=out)


def test_wrappers_refuse_a_wrong_coef(hip):
    x = torch.rand((3, 4, 6, 3), device="cuda")
    good = dev(_affine_case(3, 24, 0)[1])
    hip.affine3x3(x, good)                                                         # the good one is accepted
    hip.affine3x3(x, torch.cat([good, good]))                                      # more records than images: fine
    bad = {
        "float32": good.float(),
        "fewer records than images": good[:2],
        "not contiguous": torch.cat([good, good], dim=1)[:, ::2],
        "records of 12": good[:, :12].contiguous(),
        "flat": good.flatten()[:16],
        "on the host": good.cpu(),
    }
    assert not bad["not contiguous"].is_contiguous() and bad["not contiguous"].shape == good.shape
    for what, coef in bad.items():
        with pytest.raises(hip.CtHipError):
            hip.affine3x3(x, coef)
            pytest.fail("accepted a coef that is " + what)


def test_mk_coef_refuses_wrong_statistics(hip):
    st = dev(mc.algebra_batch()[0][:5])
    sr = dev(mc.algebra_batch()[1][:5])
    assert hip.mk_coef(st, sr).shape == (5, 16)
    bad = {
        "batch sizes differ": (st, sr[:4]),
        "batch sizes differ the other way": (st[:4], sr),
        "float32": (st.float(), sr.float()),
        "float32 reference": (st, sr.float()),
        "records of 12": (st[:, :12].contiguous(), sr[:, :12].contiguous()),
        "flat": (st.flatten(), sr.flatten()),
        "not contiguous": (torch.cat([st, st], dim=1)[:, ::2], sr),
        "on the host": (st.cpu(), sr.cpu()),
    }
    for what, (a, b) in bad.items():
        with pytest.raises(hip.CtHipError):
            hip.mk_coef(a, b)
            pytest.fail("accepted statistics that are " + what)

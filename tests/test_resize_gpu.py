"""ct_bicubic_resize_f32 (csrc/resize.hip) on the GPU against torch.nn.functional.interpolate(mode="bicubic") on the CPU, in float64
(g64, the oracle) and in float32 (g32, the reference's own arithmetic).  Input: uniform noise in [0, 1], the worst case for
coordinate error.  "The HIP error" is max |HIP - g64| over EVERY output pixel (borders included, nothing masked).

  case A  exact coordinates (scale 0.5 / 2: (o + 0.5) * scale - 0.5 is exact in float32): HIP error <= max(2 |g32 - g64|, 1e-6);
          torch's own figure there is 2.3e-7 .. 2.7e-7, the factor 2 stands for two independent float32 roundings.
  case B  inexact coordinates (0.75, 0.6, size= back up): HIP error <= the case A bound of the SAME input's exact sibling (scale 0.5
          when the call reduces, 2 when it enlarges), and strictly below |g32 - g64| of the same call -- torch's float32 kernel
          rounds the coordinate (1.5e-4 at 1080p x 0.75), this one must not.
  case C  antialias=True: A or B by that call's coordinates (center = scale * (o + 0.5); 810 -> 1080 has scale 0.75, which IS exact
          in float32, so that call is held to A).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F     # noqa: E402


def _noise(h, w, seed, n=1, c=3):
    return torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(seed))


def _cpu(x, dtype, aa, **kw):
    return F.interpolate(x.to(dtype), mode="bicubic", align_corners=False, antialias=aa, **kw).double()


def _err(a, b):
    return float((a.double() - b).abs().max())


def _bound_a(x, aa, **kw):
    """max(2 |g32 - g64|, 1e-6) of an exact-coordinate call on x; also returns the two CPU results' distance"""
    e32 = _err(_cpu(x, torch.float32, aa, **kw), _cpu(x, torch.float64, aa, **kw))
    return max(2.0 * e32, 1e-6), e32


def _coordinates_exact_in_f32(n_out, scale, aa):
    o = np.arange(n_out, dtype=np.float64)
    s32 = np.float32(scale)
    if float(s32) != scale:
        return False
    f32 = (o.astype(np.float32) + np.float32(0.5)) * s32 - (np.float32(0.0) if aa else np.float32(0.5))
    return bool(np.array_equal(f32.astype(np.float64), (o + 0.5) * scale - (0.0 if aa else 0.5)))


def _check(x, aa, case, tag, **kw):
    import ct_hip
    g64 = _cpu(x, torch.float64, aa, **kw)
    e32 = _err(_cpu(x, torch.float32, aa, **kw), g64)
    got = ct_hip.bicubic_resize(x.cuda(), antialias=aa, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(g64.shape)
    err = _err(got.cpu(), g64)
    (ho, wo), (sh, sw) = ct_hip.resize_geometry(tuple(x.shape[2:]), **kw)
    exact = _coordinates_exact_in_f32(ho, sh, aa) and _coordinates_exact_in_f32(wo, sw, aa)
    if case == "A":
        assert exact, "case A is for exact coordinates"
        bound = max(2.0 * e32, 1e-6)
        print("\n[%s aa=%s %s -> %s] A: HIP error %.3g, g32 error %.3g, bound %.3g" % (tag, aa, tuple(x.shape[2:]), (ho, wo), err, e32, bound))
        assert err <= bound
    else:
        assert not exact, "case B is for coordinates float32 cannot hold"
        sibling = 0.5 if ho < x.shape[2] else 2.0
        bound, s32 = _bound_a(x, aa, scale_factor=sibling)
        print("\n[%s aa=%s %s -> %s] B: HIP error %.3g, g32 error %.3g of the same call, sibling (x%s) g32 error %.3g, bound %.3g"
              % (tag, aa, tuple(x.shape[2:]), (ho, wo), err, e32, sibling, s32, bound))
        assert err <= bound
        assert err < e32
    return got


@pytest.mark.parametrize("h,w,f", [(1080, 1920, 0.5), (1080, 1920, 2.0), (540, 960, 0.5)])
def test_case_a_exact_coordinates(h, w, f):
    got = _check(_noise(h, w, h + int(10 * f)), False, "A", "plain", scale_factor=f)
    if f > 1:
        assert float(got.max()) > 1.0 and float(got.min()) < 0.0        # the overshoot stays: nothing clamps the result


@pytest.mark.parametrize("h,w,f", [(1080, 1920, 0.75), (1079, 1917, 0.75), (273, 481, 0.6)])
def test_case_b_inexact_coordinates_down_and_back_up(h, w, f):
    """1917 -> 1437 and back: both widths off the 16-byte grid (the element-wise path); 1920 / 1440 take the 16-byte stores"""
    import ct_hip
    x = _noise(h, w, h * 7 + w)
    low = _check(x, False, "B", "down", scale_factor=f)
    assert tuple(low.shape[2:]) == ct_hip.resize_geometry((h, w), scale_factor=f)[0]
    if (h, w) == (1080, 1920):
        # 810 / 1080 = 0.75 is exact in float32, yet the figure stays below torch's float32 one: the 16 taps are summed in float64
        assert _coordinates_exact_in_f32(1080, 0.75, False)
        y = _noise(low.shape[2], low.shape[3], 99)
        g64 = _cpu(y, torch.float64, False, size=(h, w))
        e32 = _err(_cpu(y, torch.float32, False, size=(h, w)), g64)
        bound, s32 = _bound_a(y, False, scale_factor=2.0)
        err = _err(ct_hip.bicubic_resize(y.cuda(), size=(h, w)).cpu(), g64)
        print("\n[up plain (810, 1440) -> (1080, 1920)] B: HIP error %.3g, g32 error %.3g of the same call, sibling g32 error %.3g, bound %.3g"
              % (err, e32, s32, bound))
        assert err <= bound and err < e32
    else:
        _check(_noise(low.shape[2], low.shape[3], 99), False, "B", "up", size=(h, w))


@pytest.mark.parametrize("h,w,f,case", [(1080, 1920, 0.5, "A"), (540, 960, 0.5, "A"), (540, 960, 2.0, "A"), (1080, 1920, 0.75, "B"),
                                        (1079, 1917, 0.75, "B"), (273, 481, 0.6, "B")])
def test_case_c_antialias(h, w, f, case):
    x = _noise(h, w, h * 3 + w + 1)
    low = _check(x, True, case, "aa", scale_factor=f)
    if case == "B":                                                     # and back up to the original size, under the same flag
        up_case = "A" if (h, w) == (1080, 1920) else "B"                # 810 / 1080 = 0.75: exact in float32
        _check(_noise(low.shape[2], low.shape[3], 98), True, up_case, "aa up", size=(h, w))


@pytest.mark.parametrize("aa", [False, True])
def test_small_and_odd_shapes_every_pixel(aa):
    """tiny planes (every tap clamped or cut), batches, non-square factors, up and down: <= 1e-6 of g64 -- one float32 rounding of a
    value below 2 is 1.2e-7 without antialias; with it, float32 weights, a float32 intermediate and two fmaf chains of at most
    ~2 * 2 / factor + 1 terms stay below 1e-6 on values in [0, 1]"""
    import ct_hip
    cases = [((1, 1), dict(size=(5, 7))), ((2, 3), dict(size=(9, 4))), ((5, 7), dict(size=(1, 1))), ((17, 33), dict(scale_factor=1 / 3)),
             ((31, 37), dict(scale_factor=1.5)), ((31, 37), dict(scale_factor=(0.6, 2.0))), ((64, 96), dict(scale_factor=0.2)),
             ((135, 241), dict(scale_factor=0.6)), ((40, 52), dict(size=(40, 52))), ((33, 64), dict(size=(70, 20)))]
    for i, ((h, w), kw) in enumerate(cases):
        x = _noise(h, w, 100 + i, n=2, c=3)
        g64 = _cpu(x, torch.float64, aa, **kw)
        got = ct_hip.bicubic_resize(x.cuda(), antialias=aa, **kw)
        assert tuple(got.shape) == tuple(g64.shape)
        err = _err(got.cpu(), g64)
        print("\n[aa=%s %s %s] HIP error %.3g" % (aa, (h, w), kw, err))
        assert err <= 1e-6, ((h, w), kw, err)


@pytest.mark.parametrize("aa", [False, True])
def test_out_path_bases_and_determinism(aa):
    import ct_hip
    x = _noise(270, 480, 5, n=2, c=3).cuda()
    a = ct_hip.bicubic_resize(x, scale_factor=0.75, antialias=aa)
    b = ct_hip.bicubic_resize(x, scale_factor=0.75, antialias=aa)
    assert torch.equal(a, b)                                            # bitwise, run to run
    out = torch.full((2, 3, 202, 360), -7.0, device="cuda")
    torch.cuda.synchronize()
    got = ct_hip.bicubic_resize(x, scale_factor=0.75, antialias=aa, out=out)
    assert got is out and torch.equal(out, a)
    # size= with the same steps as the factor gives: 270 * 0.75 = 202.5 -> 202 rows (in / out differs), 480 -> 360 columns (equal)
    c = ct_hip.bicubic_resize(x, size=(202, 360), antialias=aa)
    assert not torch.equal(c, a) and _err(c.cpu(), _cpu(x.cpu(), torch.float64, aa, size=(202, 360))) <= 1e-6
    # an output base off the 16-byte grid takes the element-wise path: the same bits, and nothing outside the view is written
    flat = torch.full((1 + a.numel() + 1,), -7.0, device="cuda")
    view = flat[1:1 + a.numel()].view(a.shape)
    ct_hip.bicubic_resize(x, scale_factor=0.75, antialias=aa, out=view)
    assert torch.equal(view, a) and float(flat[0]) == -7.0 and float(flat[-1]) == -7.0
    # an input base off the grid as well
    xin = torch.empty(1 + x.numel(), device="cuda")
    xin[1:].copy_(x.flatten())
    assert torch.equal(ct_hip.bicubic_resize(xin[1:].view(x.shape), scale_factor=0.75, antialias=aa), a)
    # planes are independent: a batch is its frames one by one
    assert torch.equal(ct_hip.bicubic_resize(x[1:], scale_factor=0.75, antialias=aa), a[1:])
    for bad in (x.double(), x.cpu(), x[0], x.permute(0, 1, 3, 2)):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.bicubic_resize(bad, scale_factor=0.75, antialias=aa)
    for bad_out in (torch.empty(2, 3, 202, 361, device="cuda"), torch.empty(2, 3, 202, 360), torch.empty(2, 3, 202, 360, device="cuda").double()):
        with pytest.raises(ct_hip.CtHipError):
            ct_hip.bicubic_resize(x, scale_factor=0.75, antialias=aa, out=bad_out)
    with pytest.raises(ct_hip.CtHipError):
        ct_hip.bicubic_resize(x, size=(4, 4), scale_factor=0.5)

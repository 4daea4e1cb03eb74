"""The GMFlow glue kernels (csrc/gmflow.hip: ct_instance_norm_f32, ct_eltwise_f32, ct_bilinear_resize_f32, ct_flow_warp_f32,
ct_convex_upsample_f32, ct_fb_check_f32; csrc/linear_tokens.hip: ct_layernorm128_f32) against the float64 oracle at the sizes
DMSCT runs them (68x120 .. 544x960, 1080p) and at their edges.  Cases and gate: tests/gmflow_glue_common.py (its docstring states
the gate, max|y - y64| <= max(2 max|y32 - y64|, g)); tests/test_gmflow_glue_host.py proves the cases' own conditions on the CPU.
Every continuous case prints `glue <case>: dev <max|y - y64|> ref32 <max|y32 - y64|> gate <gate>` (DESIGN section 4.5 carries the table)."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F   # noqa: E402

from oracle import gmflow as og   # noqa: E402
from tests import gmflow_glue_common as C   # noqa: E402


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


def hold(name, y, y64, y32, g):
    """the gate of tests/gmflow_glue_common.py on the whole tensor; a NaN anywhere fails it"""
    gt, floor = C.gate(y32, y64, g)
    y = y.detach().cpu()
    assert y.shape == y64.shape, (name, y.shape, y64.shape)
    err = (y.double() - y64).abs().max().item() if y.numel() else 0.0
    print("glue %s: dev %.3e ref32 %.3e gate %.3e" % (name, err, floor, gt))
    assert err <= gt, "%s: max|y - y64| = %.3e above the gate %.3e (float32 reference: %.3e)" % (name, err, gt, floor)
    return y


# ---- flow_warp ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_warp(hip, shape):
    """Smooth flows, flows that leave the image through every side and corner, constant integer / half-integer flows and finite huge
    flows.  Constant integer flows are NOT bitwise a shift: the reference normalises the source point to [-1, 1] and grid_sample maps
    it back, both in float32 (geometry.py:43-65), so x + 1 may come back as x + 1 - 2^-17 and mix in a 2^-17 share of the neighbour;
    the kernel copies that arithmetic and is held through the gate like every other flow.  Where the float64 source point lies
    >= 1.5 px outside the image no tap can be inside under any rounding: exactly 0.0, which covers flows of +-1e4, +-3e9 (beyond
    int32: the kernel clamps the tap index in float before it converts, so neither x0 nor x0 + 1 can wrap into [0, W)) and +-1e30.  NaN and +-inf flows are
    left out: grid_sample defines neither."""
    for name in C.warp_case_names(shape):
        case = C.warp_case(shape, name)
        y = hold(case.name, hip.flow_warp(case.img.cuda(), case.flow.cuda()), case.y64, case.y32, case.g)
        zero = case.zero[:, None].expand_as(y)
        assert y[zero].abs().sum().item() == 0.0, case.name + ": a tap from a source point >= 1.5 px outside the image"
        if case.huge is not None:
            assert y[case.huge[:, None].expand_as(y)].abs().sum().item() == 0.0, case.name


# ---- bilinear_resize ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.RESIZE_CASES))
def test_bilinear_resize(hip, name):
    """F.interpolate(bilinear, align_corners=True) x (mul0 on channel 0 of every image, mul1 on the others), N > 1 with mul0 != mul1"""
    case = C.resize_case(name)
    y = hold(case.name, hip.bilinear_resize(case.x.cuda(), case.size, case.mul0, case.mul1), case.y64, case.y32, case.g)
    x = case.x
    mul = torch.tensor([case.mul0] + [case.mul1] * (x.shape[1] - 1), dtype=torch.float32).view(1, -1, 1, 1)
    if name.startswith("same"):
        assert torch.equal(y, x * mul)                                          # the identity resampling: bitwise x * mul
    if name.startswith("5x7_to_1x1"):
        assert torch.equal(y, x[:, :, :1, :1] * mul)                            # pixel [0, 0]
    if name.startswith("1x1_to"):
        assert torch.equal(y, (x * mul).expand_as(y))
    if name.startswith("11x17_to_21x33"):                                       # scale exactly 1/2, weights exactly 1/2
        assert torch.equal(y[:, :, ::2, ::2], x * mul)                          # even outputs are input pixels, bit for bit
        y1 = hip.bilinear_resize(x.cuda(), case.size).cpu()                     # without multipliers
        assert torch.equal(y1[:, :, ::2, ::2], x)
        xd = x.double()
        odd = {(0, 1): [xd[:, :, :, :-1], xd[:, :, :, 1:]], (1, 0): [xd[:, :, :-1], xd[:, :, 1:]],
               (1, 1): [xd[:, :, :-1, :-1], xd[:, :, :-1, 1:], xd[:, :, 1:, :-1], xd[:, :, 1:, 1:]]}
        for (oy, ox), taps in odd.items():                                      # odd ones: the average, within one ulp of the largest tap
            big = torch.stack([t.abs() for t in taps]).amax(dim=0)              # (each rounded sum of halves is off by half an ulp of itself)
            assert ((y1[:, :, oy::2, ox::2].double() - sum(taps) / len(taps)).abs() <= C.ULP * big).all(), (oy, ox)


# ---- convex_upsample ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(C.CONVEX_CASES), ids=lambda s: "x".join(map(str, s)))
def test_convex_upsample(hip, cfg):
    """utils.py:137-155 at factors 1, 2, 4, 8: N(0,1) logits, equal logits (uniform 1/9 over the zero-padded window), logits of +-80
    (finite), and one-hot masks per tap position.  One tap at +60 over eight at 0 leaves e^-60 = 8.8e-27 on each of the others -- a
    normal float32 and float64 number, so where the chosen neighbour lies outside the image the output is what those eight hold, not
    an exact 0: it is held to 8 e^-60 factor max|flow| there (a tap read from a wrong row would be 25 decades above), and the same
    masks at +120, where e^-120 is below float32's smallest number, must give the exact 0 of F.unfold's zero padding."""
    b, h, w, f = cfg
    for kind in C.CONVEX_CASES[cfg]:
        case = C.convex_case(cfg, kind)
        y = hold(case.name, hip.convex_upsample(case.flow.cuda(), case.mask.cuda(), f), case.y64, case.y32, case.g)
        assert torch.isfinite(y).all()
        if kind == "equal":
            want = C.up_nearest(F.avg_pool2d(f * case.flow.double(), 3, stride=1, padding=1, count_include_pad=True), f)
            assert (y.double() - want).abs().max().item() <= C.gate(case.y32, case.y64, case.g)[0]
        if case.tap is not None:
            nb, inside = C.neighbour(case.flow.double(), case.tap)
            assert (y.double() - C.up_nearest(f * nb, f)).abs().max().item() <= C.gate(case.y32, case.y64, case.g)[0]
            outside = ~C.up_nearest(inside, f).expand_as(y)
            level = float(kind[3:kind.index("_")])
            rest = 8 * float(torch.exp(torch.tensor(-level))) * f * case.flow.abs().max().item() if level < 100 else 0.0
            assert y[outside].abs().max().item() <= rest * (1 + 1e-5) if outside.any() else True, case.name


# ---- fb_check -----------------------------------------------------------------------------------------------------------------
def assert_masks(what, got, want, band):
    got = got.cpu().double()
    assert got.shape == want.shape and ((got == 0) | (got == 1)).all(), what
    wrong = (got != want) & ~band
    assert not wrong.any(), "%s: %d pixels outside the margin band differ, first at %s" % (what, wrong.sum().item(), wrong.nonzero()[0].tolist())


@pytest.mark.parametrize("shape", C.FB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fb_check(hip, shape):
    """occlusion masks are exactly 0 / 1 and equal the float64 oracle on EVERY pixel whose margin |diff| - (alpha mag + beta) is not
    within 1e-4 max(1, mag) of zero (at most 0.5 % of the pixels are: host test)"""
    fwd, bwd = C.fb_flows(shape)
    focc, bocc, fband, bband = C.fb_reference(fwd, bwd)
    fo, bo = hip.fb_check(fwd.cuda(), bwd.cuda())
    assert_masks("fwd_occ %s" % (shape,), fo, focc, fband)
    assert_masks("bwd_occ %s" % (shape,), bo, bocc, bband)
    print("glue fb_check %s: fwd_occ mean %.3f bwd_occ mean %.3f, band %d + %d pixels, differing inside the band %d + %d" % (
        "x".join(map(str, shape)), fo.mean().item(), bo.mean().item(), fband.sum().item(), bband.sum().item(),
        (fo.cpu().double() != focc).sum().item(), (bo.cpu().double() != bocc).sum().item()))


def test_fb_check_threshold_is_strict(hip):
    """geometry.py:96 compares with >: at alpha = 0, beta = 0.5 a difference of exactly 0.5 is not occluded, the next float32 is
    (W - 1, H - 1 powers of two: the warp of a constant field is that constant, see the host test)"""
    fwd, bwd = torch.zeros(2, 2, 5, 257), torch.zeros(2, 2, 5, 257)
    fwd[:, 0] = 0.5
    fo, bo = hip.fb_check(fwd.cuda(), bwd.cuda(), alpha=0.0, beta=0.5)
    assert fo.abs().max().item() == 0.0 and bo.abs().max().item() == 0.0
    fwd[:, 0] = 0.50000006
    fo, bo = hip.fb_check(fwd.cuda(), bwd.cuda(), alpha=0.0, beta=0.5)
    assert fo.min().item() == 1.0
    rf, rb = og.forward_backward_consistency_check(fwd, bwd, alpha=0.0, beta=0.5)
    assert torch.equal(bo.cpu(), rb)


# ---- instance_norm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.INORM_SHAPES))
def test_instance_norm(hip, name):
    """modes 0 / 1 / 2 on N(0,1) * 3 + 1 at every plane size around the 256-thread workgroup, the split path's thresholds
    (planes < 1024 and plane >= 16384) and the half-resolution stage; constant planes (exactly 0 / relu(skip), no NaN), a spread of
    1e-4 (far below sqrt(eps)) and mean 1e3 with spread 1e-2 (contract bound: inorm_offset_bound)"""
    kinds = ["randn"] + (["tiny", "constant", "offset"] if name in C.INORM_SPECIAL_SHAPES else [])
    for kind in kinds:
        case = C.inorm_case(name, kind)
        xc, sc = case.x.cuda(), case.skip.cuda()
        got = [hip.instance_norm(xc, 0), hip.instance_norm(xc, 1), hip.instance_norm(xc, 2, sc)]
        want64, want32 = C.inorm_modes(case.y64, case.skip), C.inorm_modes(case.y32, case.skip)
        if kind == "constant":
            assert got[0].abs().max().item() == 0.0 and got[1].abs().max().item() == 0.0
            assert torch.equal(got[2].cpu(), torch.relu(case.skip))
        elif kind == "offset":
            bound = C.inorm_offset_bound(case.x, case.y64)
            for mode in range(3):
                err = (got[mode].cpu().double() - want64[mode]).abs()
                print("glue %s mode %d: dev %.3e bound %.3e" % (case.name, mode, err.max().item(), bound.max().item()))
                assert (err <= bound).all(), (case.name, mode)
        else:
            for mode in range(3):
                hold("%s mode %d" % (case.name, mode), got[mode], want64[mode], want32[mode], case.g)


@pytest.mark.parametrize("name", ["p257", "p16384"])
def test_instance_norm_propagates_nan(hip, name):
    """one NaN in a plane makes its mean NaN: F.instance_norm + relu return a NaN plane, and so must the kernels' ReLUs (both the
    one-workgroup and the split form); the other planes are untouched"""
    x, skip = C.inorm_data(name, "randn")
    x[-1, 1, 0, 100] = float("nan")
    ref = C.inorm_modes(C.inorm_plain(x), skip)
    for mode in (1, 2):
        y = hip.instance_norm(x.cuda(), mode, skip.cuda() if mode == 2 else None).cpu()
        assert torch.equal(torch.isnan(y), torch.isnan(ref[mode])) and torch.isnan(y[-1, 1]).all(), (name, mode)
        ok = ~torch.isnan(ref[mode])
        assert (y[ok] - ref[mode][ok]).abs().max().item() <= 2e-5


def test_instance_norm_split_on_two_streams(hip):
    """the split form keeps its partial sums in the per-stream workspace: two streams normalising different tensors at the same time
    give the bits each gives alone"""
    xa, sa = C.inorm_data("p16385", "randn")
    xb, sb = C.inorm_data("p16384", "randn")
    xa, sa, xb, sb = xa.cuda(), sa.cuda(), (xb * 5 - 40).cuda(), sb.cuda()
    alone_a, alone_b = hip.instance_norm(xa, 2, sa), hip.instance_norm(xb, 2, sb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs_a, outs_b = [], []
    for _ in range(8):
        outs_a.append(hip.instance_norm(xa, 2, sa))
        with torch.cuda.stream(side):
            outs_b.append(hip.instance_norm(xb, 2, sb))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(o, alone_a) for o in outs_a) and all(torch.equal(o, alone_b) for o in outs_b)


# ---- eltwise --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.ELT_LENGTHS)
def test_eltwise_flat_ops(hip, n):
    """ops 0 (a + b), 1 (a * b), 4 (a * s0): bitwise the float32 expression on the CPU"""
    a, b, _, _ = C.eltwise_operands(n)
    ac, bc = a.cuda(), b.cuda()
    assert torch.equal(hip.eltwise(0, ac, bc).cpu(), a + b)
    assert torch.equal(hip.eltwise(1, ac, bc).cpu(), a * b)
    assert torch.equal(hip.eltwise(4, ac, s0=2.5).cpu(), a * 2.5)
    assert torch.equal(hip.eltwise(4, ac, s0=-0.3).cpu(), a * torch.tensor(-0.3, dtype=torch.float32))


@pytest.mark.parametrize("n", C.ELT_LENGTHS)
def test_eltwise_gru_blend(hip, n):
    """op 2, the GRU blend (1 - z) h + z q (reg_refine.py:41-55), within 2 ulp of its largest term of the float64 value.  The kernel
    evaluates it as two fused steps (gru_blend, csrc/ct_common.h: worst case 1.5 ulp); the plain float32 expression has four
    roundings, reaches 2.5 ulp and was measured at 2.094 on one of these 4099 elements."""
    _, b, c, z = C.eltwise_operands(n)
    zd, bd, cd = z.double(), b.double(), c.double()
    want = (1 - zd) * bd + zd * cd
    term = torch.maximum(((1 - zd) * bd).abs(), (zd * cd).abs())
    err = (hip.eltwise(2, z.cuda(), b.cuda(), c.cuda()).cpu().double() - want).abs()
    plain = (((1 - z) * b + z * c).double() - want).abs()
    print("glue eltwise gru n %d: worst error %.3f ulp of the largest term (plain float32 expression on the CPU: %.3f)" % (
        n, (err / (C.ULP * term)).max().item(), (plain / (C.ULP * term)).max().item()))
    assert (err <= 2 * C.ULP * term).all()


def test_eltwise_channel_ops(hip):
    """op 3 (normalize_img) and op 5 (tanh | relu) pick a constant / a function by channel = (i / plane) % chans: N = 2, every element
    compared (a wrong channel is off by >= 0.12 in op 3), plane sizes off and on the workgroup size, split at 0, in the middle, at chans"""
    for plane in (35, 8160):
        case = C.normalize_case(plane)
        hold(case.name, hip.eltwise(3, case.x.cuda(), plane=plane), case.y64, case.y32, case.g)
    for chans, split, plane in ((256, 128, 68 * 120), (6, 0, 35), (6, 6, 35)):
        case = C.tanh_relu_case(chans, split, plane)
        y = hold(case.name, hip.eltwise(5, case.x.cuda(), plane=plane, chans=chans, split=split), case.y64, case.y32, case.g)
        assert torch.equal(y[:, split:], torch.relu(case.x[:, split:]))         # the relu half: bitwise


def test_eltwise_tanh_relu_propagates_nan(hip):
    """torch.tanh and torch.relu both return NaN for NaN (unimatch.py:320-323): op 5 must, on both sides of `split`"""
    x = torch.randn(2, 6, 1, 35, generator=C.gen(1)) * 2
    x[0, 1, 0, 3] = x[1, 4, 0, 30] = x[1, 2, 0, 0] = x[0, 5, 0, 34] = float("nan")
    y = hip.eltwise(5, x.cuda(), plane=35, chans=6, split=3).cpu()
    ref = C.tanh_relu_ref(x, 3)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.isnan(y).sum().item() == 4
    ok = ~torch.isnan(ref)
    assert (y[ok] - ref[ok]).abs().max().item() <= 2e-5


# ---- layernorm128 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", C.LN_TOKENS)
def test_layernorm128(hip, tokens):
    """token counts around the 4 tokens of a workgroup, with and without residual; partial slabs (summed in float32 in slab order,
    normalised in float64); constant rows (beta + residual); rows of 1e3 +- 1e-2 against the contract bound (ln_offset_bound)"""
    def run(case):
        return hip.layernorm128(case.x.cuda(), case.gamma.cuda(), case.beta.cuda(), residual=case.res.cuda() if case.res is not None else None,
                                partials=case.partials)
    for res in (False, True):
        for kind in ("randn", "constant"):
            case = C.ln_case(tokens, 1, res, kind)
            y = hold(case.name, run(case), case.y64, case.y32, case.g)
            if kind == "constant":
                want = case.beta.expand(tokens, 128) + (case.res if res else 0)
                assert (y - want).abs().max().item() <= case.g
        for partials in C.LN_PARTIALS:
            case = C.ln_case(tokens, partials, res)
            hold(case.name, run(case), case.y64, case.y32, case.g)
    case = C.ln_case(tokens, 1, False, "offset")
    err, bound = (run(case).cpu().double() - case.y64).abs(), C.ln_offset_bound(case)
    print("glue %s: dev %.3e bound %.3e" % (case.name, err.max().item(), bound.max().item()))
    assert (err <= bound).all()

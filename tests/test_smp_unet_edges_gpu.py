"""f4 (GPU): every layer of DMSCT's colour-correction network on its own, against float64 at its edges -- csrc/unet.hip (depthwise
convolution + tile sums, SE gate, plane scaling, up-sampling + concatenation), ct_gconv2d_pad_f32, the 1 x 1 convolutions of the
MBConv blocks at EfficientNet channel counts, each of the 14 distinct block kinds, the decoder block, the depth-5 encoder at sizes
off the 16-pixel grid, the packed-operand caches of smp_hip, and every refusal of the five entries and of ct_hip/unet.py.

The references, the error bounds and the cases are in tests/smp_unet_edges_common.py (its docstring has the error model);
tests/test_smp_unet_edges_host.py proves on the CPU that the references are the torch calls they restate and that each case tells
a kernel with a swapped pad, a rolled gate, bilinear sampling or swapped operands from the right one by > 1000 tolerances.
oracle/smp_unet.py stays a restatement of smp / efficientnet_pytorch ("parity unpinned"): this file pins the kernels to it.

Bounds: derived in the common module (depthwise, tile sums, SE gate), bitwise (plane scaling, up-sampling + concatenation, caches),
or quoted: test_gmflow_kernels_gpu.py::test_gconv (atol = rtol = 2e-5) for the padded convolution, ::test_conv_split_bf16
(2e-6 * max(1, max|ref|)) for the 1 x 1 convolutions, test_smp_unet_gpu.py::test_encoder_decoder_head_vs_restatement (4e-6 of the
largest feature per scale for blocks and encoder, 1e-5 for the decoder).

Measured on an MI355X (largest error / bound of every case, printed with -s): see MEASURED below.
"""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F   # noqa: E402

from oracle import smp_unet as o   # noqa: E402
from tests import smp_unet_edges_common as c   # noqa: E402

MEASURED = """
    depthwise convolution   error / bound 0.04 .. 0.47 (no activation), 0.05 .. 0.35 (swish) over the 30 geometries; tile sums <= 0.22
    SE gate                 error / bound 0.03 (C 2112, NSQ 88) .. 0.23 (C 255, NSQ 1) over the nine (C, NSQ), tile counts and planes
    padded convolution      error / (2e-5 + 2e-5 |ref|) <= 0.06
    block 1 x 1 convs       error / (2e-6 max(1, max|ref|)): expand + swish <= 0.31, project and project + skip <= 0.56 (split
                            mode), <= 0.63 (exact mode)
    block kinds             max error / max|want| 1.6e-7 .. 1.7e-6, outermost two rows and columns 1.5e-7 .. 1.5e-6; the oracle in
                            float32 on the CPU against itself in float64: 1.5e-7 .. 7.9e-7; gate 4e-6
    decoder block           max error / max|want| 4.0e-7 .. 1.5e-6; gate 1e-5
    encoder, depth 5        per scale <= 1.3e-6 at 64 x 96 and <= 1.8e-6 at 50 x 70; gate 4e-6
No comparison went red.  The one finding was in the binding: scale_planes_ on an empty batch handed the library the null address
of an empty tensor and got CT_E_BADARG for what the C entry defines as a no-op (planes = 0); the wrapper now returns at once.
"""

SENTINEL = 12345.0
CT_E_BADARG, CT_E_ALIGN = -1, -3


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


def ratio(got, ref, bound):
    """largest |got - ref| / bound over the elements (NaN counts as a miss)"""
    r = (got.detach().cpu().double() - ref).abs() / bound
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", list(enumerate(c.dw_cases())), ids=lambda v: c.dw_case_id(v) if isinstance(v, tuple) else str(v))
def test_dwconv_vs_float64_within_the_fma_chain_bound(hip, index, case):
    """all four (k, s) kernels; outputs on, one past and one short of the 16 x 64 tile grid, a single pixel, and 3 x 3 tiles; both
    input parities at stride 2; the network's pads and pads with pad_top != pad_left; channels 1 / 7 / 96; act 0 and swish;
    tile sums requested (every tile on its own) and NULL; a second call bitwise equal"""
    k, s, _, out = case
    worst = {0: 0.0, 5: 0.0, "sums": 0.0}
    for pad, ch in c.dw_subcases(index):
        x, wt, b = c.dw_inputs(case, pad, ch)
        xc, wc, bc = x.cuda(), wt.cuda(), b.cuda()
        for act in (c.ACT_NONE, c.ACT_SWISH):
            ref, bound = c.dwconv_reference(x, wt, b, k, s, pad, out, act)
            got, sums = hip.dwconv(xc, wc, bc, k, s, pad, out, act=act, want_sums=True)
            assert got.shape == ref.shape and sums.shape == (x.shape[0], ch, hip.lib().ct_dwconv_tiles(*out))
            got_cpu = got.cpu()
            worst[act] = max(worst[act], ratio(got_cpu, ref, bound))
            want_sums, sums_bound = c.tile_sums_reference(got_cpu)
            assert sums.shape == want_sums.shape
            worst["sums"] = max(worst["sums"], ratio(sums, want_sums, sums_bound + 1e-300))
            plain = hip.dwconv(xc, wc, bc, k, s, pad, out, act=act)                      # tile_sums == NULL
            again, sums2 = hip.dwconv(xc, wc, bc, k, s, pad, out, act=act, want_sums=True)
            assert torch.equal(plain, got) and torch.equal(again, got) and torch.equal(sums2, sums)
    print("\n[dwconv %s] error / bound: act 0 %.3f, swish %.3f, tile sums %.3f" % (c.dw_case_id(case), worst[0], worst[5], worst["sums"]))
    assert worst[0] < 1.0 and worst[5] < 1.0 and worst["sums"] < 1.0, worst


@pytest.mark.parametrize("k,s,pad", [(3, 1, (1, 1)), (3, 2, (0, 0)), (5, 1, (2, 2)), (5, 2, (2, 2)), (3, 1, (0, 1))])
def test_dwconv_zero_padding_is_a_select(hip, k, s, pad):
    """an inf at input pixel (0, 0) stays within the taps that see it (model: test_gmflow_kernels_gpu.py::
    test_small_cout_conv_zero_padding_is_a_select): padding is a zero that is selected, never a product with zero"""
    n, ch, h, w = 2, 7, 35, 131
    out = ((h + pad[0] + k // 2 - k) // s + 1, (w + pad[1] + k // 2 - k) // s + 1)
    x, wt, b = c.distinct_planes(77, n, ch, h, w), c.rand(78, ch, k * k) / k + 0.01, c.rand(79, ch)
    x[:, :, 0, 0] = float("inf")
    for act in (c.ACT_NONE, c.ACT_SWISH):
        ref, bound = c.dwconv_reference(x, wt, b, k, s, pad, out, act)
        bad = ~torch.isfinite(ref)
        assert 0 < int(bad.sum()) <= n * ch * k * k
        got, sums = hip.dwconv(x.cuda(), wt.cuda(), b.cuda(), k, s, pad, out, act=act, want_sums=True)
        got = got.cpu()
        assert torch.equal(~torch.isfinite(got), bad)
        assert float(((got.double() - ref).abs() / bound)[~bad].max()) < 1.0
        assert bool(torch.isfinite(sums[:, :, 1:]).all()) and not bool(torch.isfinite(sums[:, :, 0]).any())


# ---- writes stay inside the output ---------------------------------------------------------------------------------------------
class Guarded:
    """`numel` floats inside a larger sentinel-filled buffer (model: test_conv_ws_gpu.py::test_conv_ws_writes_only_its_output)"""

    def __init__(self, numel, lead=256, tail=8192):
        self.big = torch.full((lead + numel + tail,), SENTINEL, device="cuda")
        self.lead, self.numel = lead, numel
        self.ptr = self.big.data_ptr() + 4 * lead
        assert self.ptr % 16 == 0

    def check(self, what):
        torch.cuda.synchronize()
        inside = self.big[self.lead:self.lead + self.numel]
        assert bool((self.big[:self.lead] == SENTINEL).all()), what + ": written before the tensor"
        assert bool((self.big[self.lead + self.numel:] == SENTINEL).all()), what + ": written behind the tensor"
        assert not bool((inside == SENTINEL).any()), what + ": not every element was written"
        return inside


@pytest.mark.parametrize("k,s,h,w,out", [(3, 1, 17, 65, (17, 65)), (3, 1, 16, 64, (16, 64)), (5, 2, 33, 129, (17, 65)), (5, 2, 32, 128, (16, 64))])
def test_dwconv_writes_only_out_and_tile_sums(hip, k, s, h, w, out):
    n, ch = 2, 3
    lib = hip.lib()
    x, wt, b = c.rand(1, n, ch, h, w).cuda(), c.rand(2, ch, k * k).cuda(), c.rand(3, ch).cuda()
    tiles = lib.ct_dwconv_tiles(*out)
    o_, s_ = Guarded(n * ch * out[0] * out[1]), Guarded(n * ch * tiles)
    rc = lib.ct_dwconv_f32(x.data_ptr(), wt.data_ptr(), b.data_ptr(), o_.ptr, n, ch, h, w, k, s, k // 2, k // 2, out[0], out[1], 5, s_.ptr, None)
    assert rc == 0
    got = o_.check("dwconv out").reshape(n, ch, *out)
    assert torch.equal(got, hip.dwconv(x, wt, b, k, s, (k // 2, k // 2), out))
    s_.check("dwconv tile sums")


@pytest.mark.parametrize("ch,nsq", [(65, 5), (256, 8)])
def test_se_gate_writes_only_the_gate(hip, ch, nsq):
    n, tiles = 3, 2
    sums, wr, br, we, be = [t.cuda() for t in c.se_inputs(ch, nsq, tiles, 2000, n)]
    g = Guarded(n * ch)
    rc = hip.lib().ct_se_gate_f32(sums.data_ptr(), tiles, 2000, wr.data_ptr(), br.data_ptr(), we.data_ptr(), be.data_ptr(), g.ptr, n, ch, nsq, None)
    assert rc == 0
    assert torch.equal(g.check("se gate").reshape(n, ch), hip.se_gate(sums, 2000, wr, br, we, be))


@pytest.mark.parametrize("planes,plane", [(5, 131 * 3), (5, 1024), (3, 65560)])
def test_scale_planes_writes_only_its_planes(hip, planes, plane):
    x = c.rand(4, planes, plane) + 3.0
    gate = torch.rand(planes, generator=torch.Generator().manual_seed(5)) + 0.5
    g = Guarded(planes * plane)
    g.big[g.lead:g.lead + g.numel] = x.reshape(-1).cuda()
    rc = hip.lib().ct_scale_planes_f32(g.ptr, gate.cuda().data_ptr(), planes, plane, None)
    assert rc == 0
    assert torch.equal(g.check("scale_planes").reshape(planes, plane).cpu(), x * gate[:, None])


@pytest.mark.parametrize("cx,cs,h,w", [(3, 2, 5, 7), (3, 2, 8, 128), (2, 0, 5, 7)])
def test_upsample2_concat_writes_only_its_output(hip, cx, cs, h, w):
    n = 2
    x = c.rand(6, n, cx, h, w)
    skip = c.rand(7, n, cs, 2 * h, 2 * w) if cs else None
    g = Guarded(n * (cx + cs) * 4 * h * w)
    skc = skip.cuda() if cs else None
    rc = hip.lib().ct_upsample2_concat_f32(x.cuda().data_ptr(), skc.data_ptr() if cs else None, g.ptr, n, cx, cs, h, w, None)
    assert rc == 0
    assert torch.equal(g.check("upsample2_concat").reshape(n, cx + cs, 2 * h, 2 * w).cpu(), c.upsample2_concat_reference(x, skip))


@pytest.mark.parametrize("out,cout", [((5, 33), 40), ((4, 32), 64)])
def test_gconv2d_pad_writes_only_its_output(hip, out, cout):
    n, cin = 2, 5
    x, wt, b = c.gconv_pad_inputs(3, (0, 1), out, cin, cout, n)
    wp, bp = hip.pack_gconv_weight(wt.cuda(), b.cuda())
    xc = x.cuda()
    g = Guarded(n * cout * out[0] * out[1])
    rc = hip.lib().ct_gconv2d_pad_f32(xc.data_ptr(), wp.data_ptr(), bp.data_ptr(), g.ptr, n, cin, cout, x.shape[2], x.shape[3], 3, 3, 2, 0, 1,
                                      out[0], out[1], cin * x.shape[2] * x.shape[3], cout * out[0] * out[1], 5, None)
    assert rc == 0
    got = g.check("gconv2d_pad").reshape(n, cout, *out)
    assert torch.equal(got, hip.gconv2d_pad(xc, wp, bp, cout, 3, 2, (0, 1), out, act=hip.ACT_SWISH))


# ---- SE gate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,nsq", c.SE_SHAPES)
def test_se_gate_vs_float64_from_the_same_tile_sums(hip, ch, nsq):
    """every round count of the `c += 256` loops and of the `j += 4` wave loop, the network's extremes (720, 30) and (2112, 88);
    1 and 35 tiles of mixed sign that nearly cancel; planes of 3 and 35 * 1024 - 5 elements; saturated gates exactly 0 / 1"""
    worst = 0.0
    for tiles in c.SE_TILES:
        for plane in c.SE_PLANES:
            sums, wr, br, we, be = c.se_inputs(ch, nsq, tiles, plane)
            ref, bound = c.se_gate_reference(sums, plane, wr, br, we, be)
            got = hip.se_gate(sums.cuda(), plane, wr.cuda(), br.cuda(), we.cuda(), be.cuda()).cpu()
            assert got.shape == (3, ch) and bool(torch.isfinite(got).all())
            assert bool((got[:, c.SE_HOT] == 1.0).all()) and bool((got[:, c.SE_COLD] == 0.0).all())
            worst = max(worst, ratio(got, ref, bound))
    print("\n[se_gate C %d NSQ %d] error / bound %.3f" % (ch, nsq, worst))
    assert worst < 1.0


# ---- plane scaling and up-sampling + concatenation: bitwise -------------------------------------------------------------------
def test_scale_planes_bitwise_on_both_paths(hip):
    gen = torch.Generator().manual_seed(21)
    for n, ch, h, w, why in [(2, 3, 149, 440, "vector path, 65 560 elements: second round of the 64-workgroup loop"),
                             (2, 3, 131, 127, "scalar path, second round"), (1, 2, 8, 10, "one partial workgroup")]:
        x, gate = c.distinct_planes(h, n, ch, h, w), torch.rand(n, ch, generator=gen) + 0.5
        z = x.cuda()
        assert hip.scale_planes_(z, gate.cuda()) is z
        assert torch.equal(z.cpu(), x * gate[:, :, None, None]), why
    # plane % 4 == 0 but the base 4 bytes off a 16-byte boundary: the scalar path, same bits
    n, ch, h, w = 2, 3, 40, 100
    x, gate = c.distinct_planes(5, n, ch, h, w), torch.rand(n, ch, generator=gen) + 0.5
    buf = torch.full((n * ch * h * w + 8,), SENTINEL, device="cuda")
    view = buf[1:1 + n * ch * h * w].view(n, ch, h, w)
    view.copy_(x.cuda())
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    hip.scale_planes_(view, gate.cuda())
    assert torch.equal(view.cpu(), x * gate[:, :, None, None])
    assert float(buf[0]) == SENTINEL and bool((buf[1 + n * ch * h * w:] == SENTINEL).all())
    empty = torch.empty(0, 3, 4, 4, device="cuda")
    assert hip.scale_planes_(empty, torch.empty(0, 3, device="cuda")) is empty                    # planes = 0: an empty batch is no error
    assert hip.lib().ct_scale_planes_f32(buf.data_ptr(), gate.cuda().data_ptr(), 0, h * w, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(view.cpu(), x * gate[:, :, None, None])


def test_upsample2_concat_bitwise(hip):
    lib = hip.lib()
    for h, w in ((129, 128), (130, 127)):                    # > 32 768 pairs: second round of the 128-workgroup loop
        assert 2 * h * w > 128 * 256
        x, skip = c.distinct_planes(40 + h, 2, 3, h, w), c.distinct_planes(41 + h, 2, 2, 2 * h, 2 * w)
        assert torch.equal(hip.upsample2_concat(x.cuda(), skip.cuda()).cpu(), c.upsample2_concat_reference(x, skip))
        assert torch.equal(hip.upsample2_concat(x.cuda()).cpu(), c.upsample2_concat_reference(x))            # cs = 0, no skip pointer
    n, cx, h, w = 2, 3, 6, 9
    x, skip = c.distinct_planes(50, n, cx, h, w), c.distinct_planes(51, n, 2, 2 * h, 2 * w).cuda()
    want = c.upsample2_concat_reference(x)
    out = torch.full((n, cx, 2 * h, 2 * w), SENTINEL, device="cuda")
    assert lib.ct_upsample2_concat_f32(x.cuda().data_ptr(), skip.data_ptr(), out.data_ptr(), n, cx, 0, h, w, None) == 0   # cs = 0 with a pointer
    assert torch.equal(out.cpu(), want)
    buf = torch.zeros(n * cx * h * w + 4, device="cuda")    # x based 4 bytes off alignment is allowed
    xv = buf[1:1 + n * cx * h * w].view(n, cx, h, w)
    xv.copy_(x.cuda())
    assert xv.data_ptr() % 8 == 4
    assert torch.equal(hip.upsample2_concat(xv, skip).cpu(), c.upsample2_concat_reference(x, skip.cpu()))
    out.fill_(SENTINEL)
    big = torch.full((out.numel() + 4,), SENTINEL, device="cuda")
    assert lib.ct_upsample2_concat_f32(x.cuda().data_ptr(), None, big.data_ptr() + 4, n, cx, 0, h, w, None) == CT_E_ALIGN
    assert lib.ct_upsample2_concat_f32(x.cuda().data_ptr(), skip.data_ptr() + 4, out.data_ptr(), n, cx, 1, h, w, None) == CT_E_ALIGN
    assert lib.ct_upsample2_concat_f32(x.cuda().data_ptr(), skip.data_ptr(), out.data_ptr(), 0, cx, 2, h, w, None) == 0      # n = 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((big == SENTINEL).all())


# ---- padded dense convolution ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pad", c.GCONV_PAD_GEOMS)
@pytest.mark.parametrize("out", c.GCONV_PAD_OUT_SIZES)
def test_gconv2d_pad_vs_float64(hip, k, pad, out):
    """stride 2 with every pad geometry of the network's stems and more, outputs around the 4 x 32 tile, odd cin (the zero half of
    the last channel pair), cout of half a group, a ragged group and two groups; tolerance of test_gmflow_kernels_gpu.py::test_gconv"""
    worst = 0.0
    for cin in c.GCONV_PAD_CIN:
        for cout in c.GCONV_PAD_COUT:
            x, wt, b = c.gconv_pad_inputs(k, pad, out, cin, cout)
            wp, bp = hip.pack_gconv_weight(wt.cuda(), b.cuda())
            for act in (c.ACT_NONE, c.ACT_SWISH):
                ref = c.gconv_pad_reference(x, wt, b, 2, pad, out, act)
                got = hip.gconv2d_pad(x.cuda(), wp, bp, cout, k, 2, pad, out, act=act)
                assert got.shape == ref.shape
                worst = max(worst, ratio(got, ref, 2e-5 + 2e-5 * ref.abs()))
    print("\n[gconv2d_pad %dx%d pad %s out %s] error / (2e-5 + 2e-5 |ref|) %.3f" % (k, k, pad, out, worst))
    assert worst < 1.0


# ---- the 1 x 1 convolutions of the blocks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [36, 37])
@pytest.mark.parametrize("cin,mid", [(16, 96), (24, 144), (48, 288), (88, 528), (120, 720)])
def test_block_pointwise_convs(hip, cin, mid, w, conv_mode):
    """MBConvBlock's expand (swish epilogue) and project (identity skip added) convolutions at EfficientNet-B2 channel counts; W = 36
    takes the split family (in split mode), W = 37 the exact kernel; tolerance of test_gmflow_kernels_gpu.py::test_conv_split_bf16"""
    n, h = 2, 9
    figures = []
    for a, b_, act in ((cin, mid, hip.ACT_SWISH), (mid, cin, hip.ACT_NONE)):
        x, wt, bias = c.distinct_planes(a + w, n, a, h, w), c.rand(a + 1, b_, a, 1, 1) / a ** 0.5, c.rand(a + 2, b_)
        ref = F.conv2d(x.double(), wt.double(), bias.double())
        tol = 2e-6 * max(1.0, float(ref.abs().max()))
        wp, bp = hip.pack_gconv_weight(wt.cuda(), bias.cuda())
        if act == hip.ACT_SWISH:
            got = hip.gconv2d(x.cuda(), wp, bp, b_, 1, act=hip.ACT_SWISH)
            want = c.swish(ref)
        else:
            res = c.distinct_planes(a + 3, n, b_, h, w)
            got = hip.gconv2d(x.cuda(), wp, bp, b_, 1, act=hip.ACT_NONE, residual=res.cuda())
            want = ref + res.double()
            plain = hip.gconv2d(x.cuda(), wp, bp, b_, 1, act=hip.ACT_NONE)
            figures.append(float((plain.cpu().double() - ref).abs().max()) / tol)
        assert got.shape == want.shape
        figures.append(float((got.cpu().double() - want).abs().max()) / tol)
    print("\n[1x1 %d <-> %d, W %d, %s] error / tolerance: expand+swish %.3f, project %.3f, project+skip %.3f" % ((cin, mid, w, conv_mode) + tuple(figures)))
    assert max(figures) < 1.0


# ---- every block kind on its own -------------------------------------------------------------------------------------------------
_WANT = {}


def block_reference(idx, b, size):
    """(input, float64 oracle output, the oracle's own float32-on-CPU figure), computed once and shared by the conv modes"""
    key = (idx, size)
    if key not in _WANT:
        x = c.block_input(idx, b, size)
        full, prefix = c.encoder_state(), "_blocks.%d." % idx
        want = o.mbconv(full, prefix, b, x.double())
        sd32 = {k: v.float() for k, v in full.items() if k.startswith(prefix)}
        _WANT[key] = (x, want, c.rel_err(o.mbconv(sd32, prefix, b, x), want))
    return _WANT[key]


def load(module, sd):
    module.load_state_dict({k: v.float() for k, v in sd.items()})
    return module.cuda().eval()


@pytest.mark.parametrize("idx,b", c.block_kinds(), ids=lambda v: "block%d" % v if isinstance(v, int) else "")
def test_every_block_kind_vs_float64(hip, idx, b, conv_mode):
    import smp_hip
    block = load(smp_hip.MBConvBlock(b["cin"], b["cout"], b["k"], b["s"], b["e"], b["image_size"]), c.block_state(idx))
    assert block.pad == o.same_pad(b["image_size"], b["k"], b["s"])
    for size in c.BLOCK_SIZES:
        x, want, cpu32 = block_reference(idx, b, size)
        got = block(x.cuda()).cpu()
        assert got.shape == want.shape
        m = c.border_mask(*want.shape[2:])
        e_all, e_border = c.rel_err(got, want), c.rel_err(got[:, :, m], want[:, :, m])
        print("\n[block %d k%d s%d e%d %d->%d at %dx%d, %s convs] max error / max|want| %.1e, outermost two rows and columns %.1e "
              "(the oracle in float32 on the CPU: %.1e)" % ((idx, b["k"], b["s"], b["e"], b["cin"], b["cout"]) + size + (conv_mode, e_all, e_border, cpu32)))
        assert e_all < c.BLOCK_GATE and e_border < c.BLOCK_GATE


# ---- decoder ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [9, 10])                      # 2w = 18: the exact kernel; 2w = 20: the split family
@pytest.mark.parametrize("cx,cs,cout", [(241, 97, 256), (64, 0, 32)])
def test_decoder_block_vs_float64(hip, cx, cs, cout, w, conv_mode):
    import smp_hip
    n, h = 2, 5
    shapes = {"blocks.0.conv1.0.weight": (cout, cx + cs, 3, 3), "blocks.0.conv1.0.bias": (cout,),
              "blocks.0.conv2.0.weight": (cout, cout, 3, 3), "blocks.0.conv2.0.bias": (cout,)}
    sd = o.random_state(shapes, 60 + w, torch.float64)
    block = load(smp_hip.DecoderBlock(cx, cs, cout), {k[len("blocks.0."):]: v for k, v in sd.items()})
    x = c.distinct_planes(61, n, cx, h, w)
    skip = c.distinct_planes(62, n, cs, 2 * h, 2 * w) if cs else None
    feats = [None, skip.double(), x.double()] if cs else [None, x.double()]
    want = o.decoder_forward(sd, *feats)
    got = block(x.cuda(), skip.cuda() if cs else None).cpu()
    assert got.shape == want.shape
    e = c.rel_err(got, want)
    print("\n[decoder block %d+%d->%d at %dx%d, %s convs] max error / max|want| %.1e" % (cx, cs, cout, h, w, conv_mode, e))
    assert e < 1e-5                                          # test_smp_unet_gpu.py::test_encoder_decoder_head_vs_restatement


# ---- encoder at depth 5 and off the grid -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 64, 96), (2, 50, 70)])
def test_encoder_depth5_vs_restatement(hip, n, h, w, conv_mode):
    """smp_hip.get_encoder's default depth: blocks 16 to 22 (208 and 352 channels) run; 50 x 70 gives features of 25 x 35, 12 x 17,
    6 x 9, 3 x 5 and 2 x 3: every stride-2 layer meets an odd size, the last blocks planes smaller than their 5 x 5 kernel"""
    import smp_hip
    esd = c.encoder_state()
    enc = load(smp_hip.get_encoder("efficientnet-b2", depth=5, weights=None), esd)
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(h))
    want = o.encoder_forward(esd, x.double(), depth=5)
    if (h, w) == (50, 70):
        assert [tuple(f.shape[2:]) for f in want[1:]] == [(25, 35), (12, 17), (6, 9), (3, 5), (2, 3)]
    got = enc(x.cuda())
    assert len(got) == 6 and tuple(enc.out_channels) == o.OUT_CHANNELS
    errs = []
    for g_, w_ in zip(got, want):
        assert g_.shape == w_.shape
        errs.append(c.rel_err(g_.cpu(), w_))
    print("\n[efficientnet-b2 encoder depth 5, %dx%dx%d, %s convs] sizes %s, max error / max|feature| per scale: %s"
          % (n, h, w, conv_mode, [tuple(f.shape[2:]) for f in want], ["%.1e" % e for e in errs]))
    assert max(errs) < c.BLOCK_GATE


# ---- packed-operand caches -------------------------------------------------------------------------------------------------------
def test_packed_operands_follow_the_parameters(hip):
    """after load_state_dict of a second state, and after an in-place weight.mul_(2), a block, the stem and a decoder convolution
    compute what a freshly built module computes, bitwise: the cached packings are keyed on the parameters' versions"""
    import smp_hip
    idx, b = c.block_kinds()[3]
    x = c.block_input(idx, b, (20, 36)).cuda()
    img = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(3)).cuda()
    dshapes = {"0.weight": (32, b["cin"], 3, 3), "0.bias": (32,)}

    def modules(seed, double_it):
        blk = load(smp_hip.MBConvBlock(b["cin"], b["cout"], b["k"], b["s"], b["e"], b["image_size"]), c.block_state(idx, seed))
        enc = load(smp_hip.get_encoder("efficientnet-b2", depth=1, weights=None), c.encoder_state(seed))
        dec = load(smp_hip._Conv2dReLU(b["cin"], 32), o.random_state(dshapes, seed, torch.float64))
        if double_it:
            double(blk, enc, dec)
        return blk, enc, dec

    def double(blk, enc, dec):
        with torch.no_grad():
            for p in (blk._depthwise_conv.weight, blk._project_conv.weight, blk._se_expand.weight, enc._conv_stem.weight, dec[0].weight):
                p.mul_(2)

    def run(blk, enc, dec):
        return blk(x), enc(img)[1], dec(x)

    live = modules(5, False)
    first = run(*live)
    for m, (sd) in zip(live, (c.block_state(idx, 6), c.encoder_state(6), o.random_state(dshapes, 6, torch.float64))):
        m.load_state_dict({k: v.float() for k, v in sd.items()})
    second = run(*live)
    for a_, b_, f_ in zip(second, run(*modules(6, False)), first):
        assert torch.equal(a_, b_) and not torch.equal(a_, f_)
    double(*live)
    for a_, b_, s_ in zip(run(*live), run(*modules(6, True)), second):
        assert torch.equal(a_, b_) and not torch.equal(a_, s_)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_every_badarg_precedes_the_launch(hip):
    """every CT_E_BADARG of the five entries, once; the outputs keep their sentinel"""
    lib = hip.lib()
    n, ch, h, w = 1, 4, 8, 8
    x, wt, b = torch.zeros(n, ch, h, w, device="cuda"), torch.zeros(ch, 49, device="cuda"), torch.zeros(ch, device="cuda")
    out = torch.full((n, 64, h, w), SENTINEL, device="cuda")
    sums = torch.full((n, ch, 4), SENTINEL, device="cuda")
    X, W, B, O, S = x.data_ptr(), wt.data_ptr(), b.data_ptr(), out.data_ptr(), sums.data_ptr()

    def dw(inp=X, wp=W, bp=B, op=O, n_=n, c_=ch, h_=h, w_=w, k=3, s=1, pt=1, pl=1, oh=h, ow=w, act=5):
        return lib.ct_dwconv_f32(inp, wp, bp, op, n_, c_, h_, w_, k, s, pt, pl, oh, ow, act, S, None)
    assert dw() == 0
    torch.cuda.synchronize()
    out.fill_(SENTINEL); sums.fill_(SENTINEL)
    bad = [dw(k=7), dw(k=4), dw(s=3), dw(s=0), dw(pt=-1), dw(pl=-1), dw(oh=h + 2), dw(ow=w + 2), dw(c_=65536), dw(c_=0), dw(n_=65536), dw(n_=-1),
           dw(act=1), dw(h_=0), dw(w_=0), dw(oh=0), dw(ow=0), dw(inp=None), dw(wp=None), dw(bp=None), dw(op=None)]
    assert bad == [CT_E_BADARG] * len(bad), bad
    assert dw(n_=0) == 0

    def se(ts=S, tiles=4, plane=64, wr=W, br=B, we=W, be=B, g=O, n_=n, c_=ch, nsq=2):
        return lib.ct_se_gate_f32(ts, tiles, plane, wr, br, we, be, g, n_, c_, nsq, None)
    bad = [se(c_=14999, nsq=2), se(c_=15000, nsq=1), se(tiles=0), se(plane=0), se(n_=-1), se(c_=0), se(nsq=0), se(ts=None), se(wr=None), se(br=None),
           se(we=None), se(be=None), se(g=None)]
    assert bad == [CT_E_BADARG] * len(bad), bad
    assert se(n_=0) == 0

    def sp(xp=O, g=B, planes=ch, plane=64):
        return lib.ct_scale_planes_f32(xp, g, planes, plane, None)
    bad = [sp(planes=65536), sp(planes=65535 * 64 + 1), sp(planes=-1), sp(plane=0), sp(xp=None), sp(g=None)]
    assert bad == [CT_E_BADARG] * len(bad), bad
    assert sp(planes=0) == 0

    def up(xp=X, sk=X, op=O, n_=n, cx=2, cs=0, h_=4, w_=4):
        return lib.ct_upsample2_concat_f32(xp, sk, op, n_, cx, cs, h_, w_, None)
    bad = [up(xp=None), up(op=None), up(n_=-1), up(n_=65536), up(cx=0), up(cs=-1), up(h_=0), up(w_=0), up(sk=None, cs=1), up(cx=65535, cs=1)]
    assert bad == [CT_E_BADARG] * len(bad), bad

    def gp(inp=X, wp=W, op=O, n_=n, cin=ch, cout=8, h_=h, w_=w, k=3, s=2, pt=0, pl=0, oh=4, ow=4):
        return lib.ct_gconv2d_pad_f32(inp, wp, B, op, n_, cin, cout, h_, w_, k, k, s, pt, pl, oh, ow, cin * h_ * w_, cout * oh * ow, 0, None)
    bad = [gp(inp=None), gp(wp=None), gp(op=None), gp(n_=-1), gp(cin=0), gp(cout=0), gp(h_=0), gp(w_=0), gp(k=0), gp(s=0), gp(pt=-1), gp(pl=-1),
           gp(oh=0), gp(ow=0), gp(oh=5), gp(ow=5), gp(k=64, s=1, oh=1, ow=1)]                 # the last: a tap window that LDS cannot hold
    assert bad == [CT_E_BADARG] * len(bad), bad
    assert gp(n_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((sums == SENTINEL).all())


def test_every_shape_check_of_the_wrappers(hip):
    """the CtHipError shape checks of ct_hip/unet.py on device tensors: nothing is launched, the would-be outputs are never made"""
    z = lambda *s: torch.zeros(*s, device="cuda")           # noqa: E731
    x = z(2, 6, 8, 9)
    for args in [(x, z(6, 9), z(6), 5, 1), (x, z(5, 9), z(6), 3, 1), (x, z(6, 9), z(5), 3, 1), (x, z(6, 49), z(6), 7, 1), (x, z(6, 9), z(6), 3, 3)]:
        with pytest.raises(hip.CtHipError, match="dwconv: .*must be"):
            hip.dwconv(*args, (1, 1), (8, 9))
    good = [z(3, 8, 4), 100, z(2, 8), z(2), z(8, 2), z(8)]
    for i, t in [(0, z(3, 8)), (2, z(2, 7)), (3, z(3)), (4, z(2, 8)), (5, z(7))]:
        args = list(good)
        args[i] = t
        with pytest.raises(hip.CtHipError, match="se_gate: .*must be"):
            hip.se_gate(*args)
    with pytest.raises(hip.CtHipError, match="scale_planes_: gate must be"):
        hip.scale_planes_(x, z(2, 5))
    wp, bp = hip.pack_gconv_weight(c.rand(1, 40, 5, 3, 3).cuda(), c.rand(2, 40).cuda())
    for xx, cout, k in [(z(2, 8, 8, 9), 40, 3), (z(2, 5, 8, 9), 65, 3), (z(2, 5, 8, 9), 40, 5), (z(2, 6, 8, 9), 40, 3), (z(2, 5, 8, 9), 33, 3)]:
        with pytest.raises(hip.CtHipError, match="gconv2d_pad: "):
            hip.gconv2d_pad(xx, wp, bp, cout, k, 2, (0, 0), (4, 5))
    with pytest.raises(hip.CtHipError, match="upsample2_concat: skip must be"):
        hip.upsample2_concat(z(2, 3, 4, 5), z(2, 2, 8, 9))
    # the library's own refusals reach Python as CtHipError too
    with pytest.raises(hip.CtHipError, match="code -1"):
        hip.dwconv(x, z(6, 9), z(6), 3, 1, (1, 1), (12, 9))

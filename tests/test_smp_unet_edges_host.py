"""No GPU: the helpers of tests/smp_unet_edges_common.py are what they claim to be, the cases of tests/test_smp_unet_edges_gpu.py
discriminate, and the shape checks of ct_hip/unet.py refuse before the library is touched.

* On float64 inputs every helper reference equals the torch call (or the line of oracle.smp_unet.mbconv) it restates, to 1e-12.
* Each case is mutated the way a kernel would go wrong -- (lo, hi) padding swapped, pad_top and pad_left swapped, the SE gate
  rolled by one channel, bilinear for nearest, the skip tensor first -- and the mutated reference must leave the true one by more
  than 1000 times the tolerance the GPU file applies to that case: a kernel with that mistake cannot pass.
* The wrappers are called with CPU tensors of wrong shapes and a `lib()` that fails the test when it is touched."""
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F   # noqa: E402

from oracle import smp_unet as o   # noqa: E402
from tests import smp_unet_edges_common as c   # noqa: E402

TOL = 1e-12
FACTOR = 1000.0


def same(a, b):
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


# ---- the references are the torch calls they restate ---------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", list(enumerate(c.dw_cases()))[::3], ids=lambda v: c.dw_case_id(v) if isinstance(v, tuple) else str(v))
def test_depthwise_reference_is_conv2d_of_the_padded_input(index, case):
    k, s, (h, w), out = case
    for pad, ch in c.dw_subcases(index):
        x, wt, b = [t.double() for t in c.dw_inputs(case, pad, ch)]
        big = F.conv2d(F.pad(x, (pad[1], k + s, pad[0], k + s)), wt.reshape(ch, 1, k, k), b, stride=s, groups=ch)[:, :, :out[0], :out[1]]
        ref, bound = c.dwconv_reference(x, wt, b, k, s, pad, out, c.ACT_NONE)
        assert same(ref, big) and bool((bound > 0).all())
        act, _ = c.dwconv_reference(x, wt, b, k, s, pad, out, c.ACT_SWISH)
        assert same(act, big * torch.sigmoid(big))
    if s == 1:                                              # the network's stride-1 form is plain "same" padding
        x, wt, b = [t.double() for t in c.dw_inputs(case, (k // 2, k // 2), 7)]
        ref, _ = c.dwconv_reference(x, wt, b, k, 1, (k // 2, k // 2), out, c.ACT_NONE)
        assert same(ref, F.conv2d(x, wt.reshape(7, 1, k, k), b, padding=k // 2, groups=7))


def test_padded_dense_reference_is_conv2d_of_the_padded_input():
    for k, pad in c.GCONV_PAD_GEOMS:
        for out in c.GCONV_PAD_OUT_SIZES:
            x, wt, b = [t.double() for t in c.gconv_pad_inputs(k, pad, out, 5, 40)]
            big = F.conv2d(F.pad(x, (pad[1], k + 2, pad[0], k + 2)), wt, b, stride=2)[:, :, :out[0], :out[1]]
            assert same(c.gconv_pad_reference(x, wt, b, 2, pad, out), big)
            assert same(c.gconv_pad_reference(x, wt, b, 2, pad, out, c.ACT_SWISH), big * torch.sigmoid(big))
    # the stem as oracle.smp_unet writes it: _same_conv at the nominal size 260 = pad (0, 1)
    x, wt = c.rand(3, 2, 3, 64, 96).double(), c.rand(4, 32, 3, 3, 3).double()
    assert o.same_pad(o.IMAGE_SIZE, 3, 2) == (0, 1)
    assert same(c.gconv_pad_reference(x, wt, None, 2, (0, 0), (32, 48)), o._same_conv(x, wt, None, 3, 2, o.IMAGE_SIZE))


def test_tile_sums_reference_is_the_sum_over_each_tile():
    v = c.rand(5, 2, 3, 33, 129)
    sums, bound = c.tile_sums_reference(v)
    assert sums.shape == (2, 3, 9)
    for ty in range(3):
        for tx in range(3):
            t = v[:, :, 16 * ty:16 * ty + 16, 64 * tx:64 * tx + 64].double()
            assert same(sums[:, :, 3 * ty + tx], t.sum((2, 3)))
            assert same(bound[:, :, 3 * ty + tx], 12 * c.U * t.abs().sum((2, 3)))


def test_se_gate_reference_is_the_squeeze_and_excitation_of_mbconv():
    n, ch, nsq, h, w = 2, 24, 6, 5, 7
    x = c.rand(6, n, ch, h, w).double()
    wr, br, we, be = c.rand(7, nsq, ch).double(), c.rand(8, nsq).double(), c.rand(9, ch, nsq).double(), c.rand(10, ch).double()
    sq = F.adaptive_avg_pool2d(x, 1)                                                       # oracle.smp_unet.mbconv
    sq = o._swish(F.conv2d(sq, wr.reshape(nsq, ch, 1, 1), br))
    sq = F.conv2d(sq, we.reshape(ch, nsq, 1, 1), be)
    gate, bound = c.se_gate_reference(x.reshape(n, ch, 1, h * w).sum(-1), h * w, wr, br, we, be)
    assert same(gate, torch.sigmoid(sq).reshape(n, ch)) and bool((bound > 0).all())
    halves = torch.stack([x[:, :, :2].sum((2, 3)), x[:, :, 2:].sum((2, 3))], -1)          # two tiles: same mean
    assert same(c.se_gate_reference(halves, h * w, wr, br, we, be)[0], gate)


def test_upsample_concat_reference_is_interpolate_and_cat():
    x, skip = c.rand(11, 2, 3, 5, 7).double(), c.rand(12, 2, 4, 10, 14).double()
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    assert torch.equal(c.upsample2_concat_reference(x), up)
    assert torch.equal(c.upsample2_concat_reference(x, skip), torch.cat([up, skip], dim=1))


def test_block_kinds_are_the_fourteen_distinct_blocks():
    kinds = c.block_kinds()
    assert tuple(i for i, _ in kinds) == c.BLOCK_KIND_INDICES and len(kinds) == 14
    table = o.block_table()
    assert len({(b["k"], b["s"], b["e"], b["cin"], b["cout"]) for b in table}) == 14
    assert {i for i, b in kinds if b["s"] == 2 and o.same_pad(b["image_size"], b["k"], 2) == (0, 1)} == {2}


@pytest.mark.parametrize("idx,b", c.block_kinds(), ids=lambda v: "block%d" % v if isinstance(v, int) else "")
def test_mbconv_restatement_and_padding_mutation(idx, b):
    sd = c.block_state(idx)
    full = c.encoder_state()
    for size in c.BLOCK_SIZES:
        x = c.block_input(idx, b, size).double()
        want = o.mbconv(full, "_blocks.%d." % idx, b, x)
        assert same(c.mbconv_padded(sd, b, x), want)
        lo, hi = o.same_pad(b["image_size"], b["k"], b["s"])
        if lo != hi:                                        # the stride-2 (0, 1) kind: (1, 0) is another function
            bad = c.mbconv_padded(sd, b, x, pad=(hi, lo))
            assert bad.shape == want.shape
            m = c.border_mask(*want.shape[2:])
            for region in (torch.ones_like(m), m):          # the whole-output gate and the border gate of the GPU file
                moved = float((bad - want)[:, :, region].abs().max())
                assert moved > FACTOR * c.BLOCK_GATE * float(want[:, :, region].abs().max()), (idx, size, moved)


# ---- the cases discriminate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,case", list(enumerate(c.dw_cases())), ids=lambda v: c.dw_case_id(v) if isinstance(v, tuple) else str(v))
def test_depthwise_cases_tell_pad_top_from_pad_left(index, case):
    k, s, _, out = case
    seen = 0
    for pad, ch in c.dw_subcases(index):
        if pad[0] == pad[1]:
            continue
        x, wt, b = c.dw_inputs(case, pad, ch)
        for act in (c.ACT_NONE, c.ACT_SWISH):
            ref, bound = c.dwconv_reference(x, wt, b, k, s, pad, out, act)
            bad, _ = c.dwconv_reference(x, wt, b, k, s, pad[::-1], out, act)
            assert float(((bad - ref).abs() / bound).max()) > FACTOR, (case, pad, ch, act)
        seen += 1
    assert seen == 3


@pytest.mark.parametrize("ch,nsq", [s for s in c.SE_SHAPES if s[0] > 1])           # one channel cannot be rolled
def test_se_cases_tell_a_gate_from_its_neighbour(ch, nsq):
    for tiles in c.SE_TILES:
        for plane in c.SE_PLANES:
            sums, wr, br, we, be = c.se_inputs(ch, nsq, tiles, plane)
            gate, bound = c.se_gate_reference(sums, plane, wr, br, we, be)
            assert float(((torch.roll(gate, 1, dims=1) - gate).abs() / bound).max()) > FACTOR
            if tiles > 1:                                   # the sums do nearly cancel: the mean is 1e-3 of their magnitude
                total, mag = sums.double().sum(-1).abs(), sums.double().abs().sum(-1)
                assert float((total / mag).max()) < 1e-2
            hot, cold = gate[:, c.SE_HOT], gate[:, c.SE_COLD]      # expand biases of +-100: the true gate is 1 / 0 to float32 and beyond
            assert hot.numel() > 0 and float((1 - hot).abs().max()) < 1e-30 and (cold.numel() == 0 or float(cold.max()) < 1e-30)


def test_upsample_concat_cases_tell_nearest_from_bilinear_and_the_operand_order():
    for h, w in ((129, 128), (130, 127)):
        x, skip = c.distinct_planes(40 + h, 2, 3, h, w), c.distinct_planes(41 + h, 2, 2, 2 * h, 2 * w)
        ref = c.upsample2_concat_reference(x, skip)
        scale = float(ref.abs().max())
        # the GPU comparison is bitwise (tolerance 0): 1000 float32 roundings of the largest value stand in for it
        for bad in (c.upsample2_concat_reference(x, skip, mode="bilinear"), c.upsample2_concat_reference(x, skip, up_first=False)):
            assert bad.shape == ref.shape or bad.shape[1] == ref.shape[1]
            assert float((bad - ref).abs().max()) > FACTOR * c.U * scale


def test_padded_dense_cases_tell_the_pads_apart():
    """(0, 1) against (1, 0), under the tolerance of test_gmflow_kernels_gpu.py::test_gconv (atol = rtol = 2e-5)"""
    for out in c.GCONV_PAD_OUT_SIZES:
        for cin in c.GCONV_PAD_CIN:
            x, wt, b = c.gconv_pad_inputs(3, (0, 1), out, cin, 40)
            ref = c.gconv_pad_reference(x, wt, b, 2, (0, 1), out)
            bad = c.gconv_pad_reference(x, wt, b, 2, (1, 0), out)
            assert float(((bad - ref).abs() / (2e-5 + 2e-5 * ref.abs())).max()) > FACTOR


# ---- the wrappers refuse wrong shapes before the library is touched --------------------------------------------------------------
@pytest.fixture
def unet(monkeypatch):
    import ct_hip
    from ct_hip import unet as mod

    def no_lib():
        raise AssertionError("lib() was touched before the shape check")
    monkeypatch.setattr(mod, "lib", no_lib)
    return ct_hip, mod


def z(*shape):
    return torch.zeros(*shape)


def test_dwconv_refuses_wrong_shapes(unet):
    hip, mod = unet
    x = z(2, 6, 8, 9)
    for args in [(x, z(6, 9), z(6), 5, 1), (x, z(6, 25), z(6), 3, 1), (x, z(5, 9), z(6), 3, 1), (x, z(6, 9), z(5), 3, 1), (x, z(54), z(6), 3, 1),
                 (x, z(6, 49), z(6), 7, 1), (x, z(6, 9), z(6), 3, 3), (x, z(6, 9), z(6), 3, 0), (x[0], z(6, 9), z(6), 3, 1)]:
        with pytest.raises(hip.CtHipError, match="dwconv: .*must be"):
            mod.dwconv(*args, (1, 1), (8, 9), want_sums=True)
    with pytest.raises(hip.CtHipError, match="no CPU path"):           # right shapes: on to the device check, still no library
        mod.dwconv(x, z(6, 9), z(6), 3, 1, (1, 1), (8, 9), want_sums=True)


def test_se_gate_refuses_wrong_shapes(unet):
    hip, mod = unet
    good = dict(tile_sums=z(3, 8, 4), w_reduce=z(2, 8), b_reduce=z(2), w_expand=z(8, 2), b_expand=z(8))
    bad = dict(tile_sums=z(3, 8), w_reduce=z(2, 7), b_reduce=z(3), w_expand=z(2, 8), b_expand=z(7))
    for name, t in bad.items():
        args = dict(good)
        args[name] = t
        with pytest.raises(hip.CtHipError, match="se_gate: .*must be"):
            mod.se_gate(args["tile_sums"], 100, args["w_reduce"], args["b_reduce"], args["w_expand"], args["b_expand"])
    with pytest.raises(hip.CtHipError, match="se_gate: w_reduce must be"):
        mod.se_gate(good["tile_sums"], 100, z(16), good["b_reduce"], good["w_expand"], good["b_expand"])
    with pytest.raises(hip.CtHipError, match="se_gate: w_expand must be"):  # a gate's worth of weights for another squeeze width
        mod.se_gate(good["tile_sums"], 100, good["w_reduce"], good["b_reduce"], z(8, 3), good["b_expand"])
    with pytest.raises(hip.CtHipError, match="no CPU path"):
        mod.se_gate(good["tile_sums"], 100, good["w_reduce"], good["b_reduce"], good["w_expand"], good["b_expand"])


def test_scale_planes_refuses_a_gate_of_another_shape(unet):
    hip, mod = unet
    x = z(2, 6, 4, 4)
    for gate in (z(2, 5), z(6, 2), z(12), z(2, 6, 1, 1), z(3, 6)):
        with pytest.raises(hip.CtHipError, match="scale_planes_: gate must be"):
            mod.scale_planes_(x, gate)
    with pytest.raises(hip.CtHipError, match="scale_planes_: x must be"):
        mod.scale_planes_(z(12, 16), z(2, 6))
    with pytest.raises(hip.CtHipError, match="no CPU path"):
        mod.scale_planes_(x, z(2, 6))


def test_gconv2d_pad_refuses_operands_packed_for_other_channels(unet):
    hip, mod = unet
    wt, b = c.rand(1, 40, 5, 3, 3), c.rand(2, 40)
    wp, bp = hip.pack_gconv_weight(wt, b)                   # pure torch: packs on the CPU
    x = z(2, 5, 8, 9)
    with pytest.raises(hip.CtHipError, match="no CPU path"):
        mod.gconv2d_pad(x, wp, bp, 40, 3, 2, (0, 0), (4, 5))
    for xx, cout, k, why in [(z(2, 8, 8, 9), 40, 3, "packed weight"), (x, 65, 3, "packed weight"), (x, 40, 5, "packed weight"),
                             (z(2, 6, 8, 9), 40, 3, "packed for"), (x, 33, 3, "packed for"), (x, 0, 3, "positive")]:
        with pytest.raises(hip.CtHipError, match="gconv2d_pad: .*" + why):
            mod.gconv2d_pad(xx, wp, bp, cout, k, 2, (0, 0), (4, 5))
    with pytest.raises(hip.CtHipError, match="gconv2d_pad: the packed bias must be"):
        mod.gconv2d_pad(x, wp, b, 40, 3, 2, (0, 0), (4, 5))
    w5, b5 = hip.pack_gconv_weight(c.rand(3, 40, 5, 5, 5), b)     # a 5 x 5 packing carries no source: checked up to its zero padding
    with pytest.raises(hip.CtHipError, match="packed weight"):
        mod.gconv2d_pad(z(2, 7, 8, 9), w5, b5, 40, 5, 2, (2, 2), (4, 5))
    with pytest.raises(hip.CtHipError, match="no CPU path"):
        mod.gconv2d_pad(z(2, 6, 8, 9), w5, b5, 40, 5, 2, (2, 2), (4, 5))

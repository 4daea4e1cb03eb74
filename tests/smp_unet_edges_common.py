"""CPU helpers of tests/test_smp_unet_edges_host.py and tests/test_smp_unet_edges_gpu.py: float64 references of the layers of
DMSCT's colour-correction network (csrc/unet.hip, ct_gconv2d_pad_f32) with a forward error bound of the float32 kernel computed
next to each of them, the cases both files share (so that the host file can prove that a case discriminates before the GPU file
relies on it), and the distinct MBConv block kinds of EfficientNet-B2.  Not a test module; no GPU, no product import.

Error model.  u = 2**-24 is the unit roundoff of float32; a chain of n float32 operations on top of exactly represented inputs
is within n * u * (sum of the magnitudes that enter it) of the exact value (first order; the (1 + u)**n - 1 excess is below
1e-5 of the bound for every n here).  Stages compose to first order: a stage's bound is its own rounding term plus the previous
stage's bound times the largest derivative of the stage.
"""
import math

import torch
import torch.nn.functional as F

from oracle import smp_unet as o

U = 2.0 ** -24
TILE_H, TILE_W = 16, 64                      # csrc/unet.hip: kDwTH, kDwTW
SWISH_SLOPE = 1.1                            # max |d/dv v sigmoid(v)| = 1.0998
ACT_NONE, ACT_SWISH = 0, 5


def swish(v):
    return v * torch.sigmoid(v)


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def distinct_planes(seed, n, c, h, w):
    """float32 [n, c, h, w] noise with a different offset and gain in every channel and every image: a kernel that reads the
    wrong plane gets values that are wrong by O(1)"""
    x = rand(seed, n, c, h, w)
    idx = torch.arange(n * c, dtype=torch.float32).reshape(n, c, 1, 1)
    return x * (1.0 + 0.37 * torch.cos(1.7 * idx)) + 0.9 * torch.sin(0.61 * idx + 0.3)


# ---- depthwise convolution ------------------------------------------------------------------------------------------------
def pad_explicit(x, kh, kw, stride, pad_top_left, out_size):
    """zero padding as the kernels define it: `pad_top_left` zeros in front, and behind whatever the output size still reads
    (the implicit zero fill) -- or a crop where the output size does not reach the last rows / columns"""
    top, left = pad_top_left
    rows, cols = (out_size[0] - 1) * stride + kh, (out_size[1] - 1) * stride + kw
    h, w = x.shape[2:]
    x = F.pad(x, (left, max(0, cols - (w + left)), top, max(0, rows - (h + top))))
    return x[:, :, :rows, :cols]


def dwconv_reference(x, weight, bias, k, stride, pad_top_left, out_size, act):
    """float64 depthwise convolution (weight [C, k*k], bias [C]) (+ swish), and the bound of the float32 kernel's error:
    K*K fmas on top of the bias: |err_pre| <= (K*K + 1) u (|w| (*) |x| + |b|); after swish 1.1 err_pre + 8 u |ref| (expf, the
    addition and the division: 2 u + u + u, doubled)."""
    c = x.shape[1]
    xp = pad_explicit(x.double(), k, k, stride, pad_top_left, out_size)
    w4 = weight.double().reshape(c, 1, k, k)
    pre = F.conv2d(xp, w4, bias.double(), stride=stride, groups=c)
    mag = F.conv2d(xp.abs(), w4.abs(), bias.double().abs(), stride=stride, groups=c)
    err = (k * k + 1) * U * mag
    assert tuple(pre.shape[2:]) == tuple(out_size)
    if act == ACT_SWISH:
        ref = swish(pre)
        return ref, SWISH_SLOPE * err + 8 * U * ref.abs()
    return pre, err


def dw_input_sizes(k, stride, out_size):
    """input sizes that give `out_size`: stride 1 the output's own size; stride 2 the even and the odd one"""
    ho, wo = out_size
    if stride == 1:
        return [(ho, wo)]
    return [(2 * ho, 2 * wo), (2 * ho - 1, 2 * wo - 1)]


DW_OUT_SIZES = [(16, 64), (17, 65), (15, 63), (1, 1), (33, 129)]
DW_PADS = [(1, 1), (0, 0), (2, 2), (0, 1), (2, 0), (1, 2)]       # the network's three, then three with pad_top != pad_left
DW_CHANNELS = [1, 7, 96]


def dw_cases():
    """(k, stride, (h, w), out_size): all four kernels, every output size, both input parities at stride 2"""
    return [(k, s, hw, out) for k in (3, 5) for s in (1, 2) for out in DW_OUT_SIZES for hw in dw_input_sizes(k, s, out)]


def dw_case_id(case):
    k, s, (h, w), (ho, wo) = case
    return "k%ds%d-%dx%d-to-%dx%d" % (k, s, h, w, ho, wo)


def dw_subcases(case_index):
    """the (pad, channels) pairs of one geometry: every pad, the channel count rotating so that every (pad, channels) pair
    occurs across the geometries"""
    return [(pad, DW_CHANNELS[(case_index + j) % 3]) for j, pad in enumerate(DW_PADS)]


def dw_inputs(case, pad, c, n=2):
    k, s, (h, w), out = case
    seed = 1000 * k + 100 * s + 7 * h + 3 * w + 11 * pad[0] + 13 * pad[1] + c
    x = distinct_planes(seed, n, c, h, w)
    weight = rand(seed + 1, c, k * k) / k + 0.05 * torch.arange(k * k, dtype=torch.float32) / (k * k)     # no two taps alike
    bias = rand(seed + 2, c)
    return x, weight, bias


def tile_sums_reference(out32):
    """float64 sums of the DEVICE's float32 outputs over the 16 x 64 tiles, [n, c, tiles] (tile = ty * tiles_x + tx), and the
    kernel's bound 12 u sum|v|: 4 additions in the thread, 6 shuffle steps, 2 wave combinations"""
    n, c, ho, wo = out32.shape
    ty, tx = (ho + TILE_H - 1) // TILE_H, (wo + TILE_W - 1) // TILE_W
    v = F.pad(out32.double(), (0, tx * TILE_W - wo, 0, ty * TILE_H - ho)).reshape(n, c, ty, TILE_H, tx, TILE_W)
    return v.sum((3, 5)).reshape(n, c, ty * tx), 12 * U * v.abs().sum((3, 5)).reshape(n, c, ty * tx)


# ---- squeeze-and-excitation gate ----------------------------------------------------------------------------------------------
def se_gate_reference(tile_sums32, plane, w_reduce, b_reduce, w_expand, b_expand):
    """float64 gate [N, C] from the given float32 tile sums, and the bound of csrc/unet.hip's se_scale_kernel:
      mean    3 u |mean|          (tile sums added in float64; 1 / plane is rounded to float32, the product once more)
      reduce  (ceil(C / 64) + 8) u (sum|w mean| + |b|) + sum|w| err_mean    (a lane's fmas, 6 shuffle steps, the bias)
      swish   1.1 err + 8 u |sq|
      expand  (NSQ + 1) u (sum|w sq| + |b|) + sum|w| err_sq                 (NSQ fmas on top of the bias)
      sigmoid err / 4 + 8 u |gate|                                          (largest slope 1/4)
    The biases enter the magnitudes exactly as in the depthwise bound: the addition that brings them in rounds at their size."""
    c, nsq = w_expand.shape
    wr, br, we, be = w_reduce.double(), b_reduce.double(), w_expand.double(), b_expand.double()
    mean = tile_sums32.double().sum(-1) / plane                                   # [N, C]
    e_mean = 3 * U * mean.abs()
    pre = mean @ wr.t() + br
    e_pre = (math.ceil(c / 64) + 8) * U * (mean.abs() @ wr.abs().t() + br.abs()) + e_mean @ wr.abs().t()
    sq = swish(pre)
    e_sq = SWISH_SLOPE * e_pre + 8 * U * sq.abs()
    z = sq @ we.t() + be
    e_z = (nsq + 1) * U * (sq.abs() @ we.abs().t() + be.abs()) + e_sq @ we.abs().t()
    gate = torch.sigmoid(z)
    return gate, 0.25 * e_z + 8 * U * gate.abs()


SE_SHAPES = [(1, 1), (63, 3), (64, 4), (65, 5), (255, 1), (256, 8), (257, 22), (720, 30), (2112, 88)]
SE_TILES = [1, 35]
SE_PLANES = [3, 35 * 1024 - 5]
SE_SATURATED = 100.0
SE_HOT, SE_COLD = slice(3, None, 10), slice(8, None, 10)      # channels whose expand bias is +100 / -100 (none when C <= 3)


def se_inputs(c, nsq, tiles, plane, n=3):
    """tile sums of mixed sign whose total nearly cancels (the last tile takes back all but a 1e-3 part of the others), weights
    of the network's scale, and expand biases of +-100 on every fifth channel from the fourth on: those gates saturate"""
    seed = 31 * c + 7 * nsq + tiles + plane % 97
    sums = rand(seed, n, c, tiles) * plane
    if tiles > 1:
        sums[:, :, -1] = -sums[:, :, :-1].double().sum(-1).float() * (1 - 1e-3)
    else:
        sums = sums * 0.3
    w_reduce, b_reduce = rand(seed + 1, nsq, c) / c ** 0.5, rand(seed + 2, nsq) * 0.1
    w_expand, b_expand = rand(seed + 3, c, nsq) / nsq ** 0.5, rand(seed + 4, c) * 0.1
    b_expand[SE_HOT] = SE_SATURATED
    b_expand[SE_COLD] = -SE_SATURATED
    return sums, w_reduce, b_reduce, w_expand, b_expand


# ---- the decoder's front and the padded dense convolution ----------------------------------------------------------------------
def upsample2_concat_reference(x, skip=None, up_first=True, mode="nearest"):
    """cat([nearest-x2(x), skip], 1) by indexing (no interpolation call).  up_first / mode: the mutations of the host file."""
    if mode == "nearest":
        up = x[:, :, torch.arange(2 * x.shape[2]) // 2][:, :, :, torch.arange(2 * x.shape[3]) // 2]
    else:
        up = F.interpolate(x, scale_factor=2, mode=mode, align_corners=False)
    if skip is None:
        return up
    return torch.cat([up, skip] if up_first else [skip, up], 1)


def gconv_pad_reference(x, weight, bias, stride, pad_top_left, out_size, act=ACT_NONE):
    """float64 dense convolution with explicit (top, left) padding and output size (+ swish)"""
    kh, kw = weight.shape[2:]
    ref = F.conv2d(pad_explicit(x.double(), kh, kw, stride, pad_top_left, out_size), weight.double(),
                   None if bias is None else bias.double(), stride=stride)
    assert tuple(ref.shape[2:]) == tuple(out_size)
    return swish(ref) if act == ACT_SWISH else ref


GCONV_PAD_OUT_SIZES = [(4, 32), (5, 33), (3, 31), (1, 1)]
GCONV_PAD_GEOMS = [(3, (0, 0)), (3, (1, 1)), (3, (0, 1)), (5, (2, 2))]        # (kernel, (pad_top, pad_left)), all stride 2
GCONV_PAD_CIN = [3, 5]
GCONV_PAD_COUT = [32, 40, 65]


def gconv_pad_inputs(k, pad, out_size, cin, cout, n=2):
    """an even height and an odd width (H != W) that give `out_size` at stride 2"""
    ho, wo = out_size
    h, w = 2 * ho, 2 * wo - 1
    seed = 500 * k + 50 * pad[0] + 5 * pad[1] + 17 * ho + cin + 3 * cout
    x = distinct_planes(seed, n, cin, h, w)
    weight, bias = rand(seed + 1, cout, cin, k, k) / (cin * k * k) ** 0.5, rand(seed + 2, cout)
    return x, weight, bias


# ---- MBConv blocks ---------------------------------------------------------------------------------------------------------------
def block_kinds():
    """[(block index, table entry)]: the first block of each distinct (k, s, e, cin, cout) of EfficientNet-B2"""
    seen, kinds = set(), []
    for idx, b in enumerate(o.block_table()):
        key = (b["k"], b["s"], b["e"], b["cin"], b["cout"])
        if key not in seen:
            seen.add(key)
            kinds.append((idx, b))
    return kinds


BLOCK_KIND_INDICES = (0, 1, 2, 3, 5, 6, 8, 9, 12, 13, 16, 17, 21, 22)
BLOCK_SIZES = [(20, 36), (19, 37)]
BLOCK_GATE = 4e-6                            # tests/test_smp_unet_gpu.py::test_encoder_decoder_head_vs_restatement, per scale

_STATE = {}


def encoder_state(seed=5):
    """oracle.smp_unet.random_state of the whole encoder in float64, made once"""
    if seed not in _STATE:
        _STATE[seed] = o.random_state(o.encoder_param_shapes(), seed, torch.float64)
    return _STATE[seed]


def block_state(idx, seed=5):
    """the entries of block `idx`, with the `_blocks.<idx>.` prefix taken off: a state dict of one MBConvBlock"""
    prefix = "_blocks.%d." % idx
    return {k[len(prefix):]: v for k, v in encoder_state(seed).items() if k.startswith(prefix)}


def block_input(idx, b, size, n=2):
    return distinct_planes(900 + idx, n, b["cin"], size[0], size[1]) * 0.7


def mbconv_padded(sd, b, x, pad=None):
    """oracle.smp_unet.mbconv restated with the depthwise padding as an argument ((lo, hi); None = same_pad of the block's
    nominal size): what the host file mutates.  `sd` is a block_state (no prefix)."""
    lo, hi = o.same_pad(b["image_size"], b["k"], b["s"]) if pad is None else pad
    inp = x
    if b["e"] != 1:
        x = swish(o._bn(sd, "_bn0", F.conv2d(x, sd["_expand_conv.weight"])))
    x = F.conv2d(F.pad(x, (lo, hi, lo, hi)), sd["_depthwise_conv.weight"], None, stride=b["s"], groups=x.shape[1])
    x = swish(o._bn(sd, "_bn1", x))
    sq = x.mean((2, 3), keepdim=True)
    sq = swish(F.conv2d(sq, sd["_se_reduce.weight"], sd["_se_reduce.bias"]))
    sq = F.conv2d(sq, sd["_se_expand.weight"], sd["_se_expand.bias"])
    x = torch.sigmoid(sq) * x
    x = o._bn(sd, "_bn2", F.conv2d(x, sd["_project_conv.weight"]))
    if b["s"] == 1 and b["cin"] == b["cout"]:
        x = x + inp
    return x


def border_mask(h, w, width=2):
    """True on the outermost `width` rows and columns"""
    m = torch.ones(h, w, dtype=torch.bool)
    if h > 2 * width and w > 2 * width:
        m[width:h - width, width:w - width] = False
    return m


def rel_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())

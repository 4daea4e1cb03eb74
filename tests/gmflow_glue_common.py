"""Seeded case builders for the GMFlow glue kernels (csrc/gmflow.hip: instance norm, elementwise steps, bilinear resize, flow warp,
convex upsampling, forward-backward check; csrc/linear_tokens.hip: LayerNorm(128)) at the sizes DMSCT runs them and at their edges.

Everything here is torch on the CPU plus oracle/gmflow.py; nothing touches ct_hip.  tests/test_gmflow_glue_host.py proves on the
CPU that every case meets the conditions its device check relies on, tests/test_gmflow_glue_gpu.py holds the kernels to the cases.

The gate of a continuous output: with y64 the oracle on x.double(), y32 the same call on the float32 x (the reference's
arithmetic) and y the device result,   max|y - y64| <= max(2 max|y32 - y64|, g)   over the whole tensor, g the fixed gate
the kernel's small test already uses (2e-5; flow_warp 1e-4).  Two float32 evaluations of one expression with different rounding
orders sit within 2x of each other's distance from exact.  A case is only admitted if that gate is at most
1e-3 of max|y64| (gate_cap_ok): data that breaks this is the wrong data."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import gmflow as og

G_CONT, G_WARP = 2e-5, 1e-4
CAP = 1e-3
ULP = 2.0 ** -23
HALF_ULP = 2.0 ** -24


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gate(y32, y64, g):
    """(gate, floor): floor = the float32 reference's own distance from float64"""
    floor = (y32.double() - y64).abs().max().item()
    return max(2.0 * floor, g), floor


def gate_cap_ok(case):
    """(ok, gate, scale): the gate of a case is at most 1e-3 of its output range max|y64|.  Where the whole output is zero by
    construction (a constant flow of one image width; a one-hot mask whose tap lies outside a 1 x 1 image) there is no output
    range: the case names the range of what the kernel samples (`scale`) instead."""
    gt, _ = gate(case.y32, case.y64, case.g)
    scale = case.y64.abs().max().item()
    if getattr(case, "scale", None) is not None and scale <= 1e-12 * case.scale:
        scale = case.scale
    return gt <= CAP * scale, gt, scale


def _grid(h, w, dtype=torch.float32):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return xx, yy


# ---- flow_warp ----------------------------------------------------------------------------------------------------------------
WARP_SHAPES = [(2, 5, 68, 120), (1, 16, 136, 240), (1, 3, 544, 960), (1, 3, 2, 2), (1, 2, 3, 257), (2, 129, 17, 33)]
HUGE_FLOWS = (1e4, -1e4, 3e9, -3e9, 1e30, -1e30)


def const_flows(h, w):
    return [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (w - 1, h - 1), (w, 0), (0, -h), (2.5, -1.5)]


def smooth_image(n, c, h, w, seed):
    """smooth plus noise: one sine wave of 0.5 .. 2.5 periods across the frame per plane, plus 0.1 N(0,1)"""
    g = gen(seed)
    xx, yy = _grid(h, w)
    kx, ky = (0.5 + 2.0 * torch.rand(n, c, 1, 1, generator=g) for _ in range(2))
    ph = 2 * math.pi * torch.rand(n, c, 1, 1, generator=g)
    return torch.sin(2 * math.pi * (kx * xx / w + ky * yy / h) + ph) + 0.1 * torch.randn(n, c, h, w, generator=g)


def smooth_flow(n, h, w, seed):
    """a smooth field of amplitude 5 .. 10 % of the width, plus 0.3 N(0,1)"""
    g = gen(seed)
    xx, yy = _grid(h, w)
    amp = (0.05 + 0.05 * torch.rand(n, 1, 1, generator=g)) * w
    p = 2 * math.pi * torch.rand(4, n, 1, 1, generator=g)
    fx = amp * torch.sin(2 * math.pi * yy / h + p[0]) * torch.cos(math.pi * xx / w + p[1])
    fy = amp * torch.cos(2 * math.pi * xx / w + p[2]) * torch.sin(math.pi * yy / h + p[3])
    return torch.stack([fx, fy], 1) + 0.3 * torch.randn(n, 2, h, w, generator=g)


def source_points(flow):
    """float64 source point (x + flow_x, y + flow_y) of every pixel"""
    n, _, h, w = flow.shape
    xx, yy = _grid(h, w, torch.float64)
    return xx + flow[:, 0].double(), yy + flow[:, 1].double()


def outside_masks(flow):
    """per pixel: source left of / right of / above / below the image [0, w-1] x [0, h-1]"""
    n, _, h, w = flow.shape
    sx, sy = source_points(flow)
    return sx < 0, sx > w - 1, sy < 0, sy > h - 1


def far_outside(flow, by=1.5):
    """source at least `by` pixels outside: no bilinear tap can lie inside the image, the warp is exactly 0 there"""
    n, _, h, w = flow.shape
    sx, sy = source_points(flow)
    return (sx <= -by) | (sx >= w - 1 + by) | (sy <= -by) | (sy >= h - 1 + by)


def outside_flow(n, h, w, seed, corners=(0, 1, 2, 3)):
    """40 % of the pixels are sent to a source point 0.2 .. 4 px outside the image, in equal parts through the four sides and the
    corners listed (so partial taps on every border and pixels with no tap at all); the others follow smooth_flow, pulled back
    inside.  Images with fewer than 8 pixels cannot feed eight groups: there the chosen pixels go through the corners only."""
    g = gen(seed)
    xx, yy = _grid(h, w)
    base = smooth_flow(n, h, w, seed + 1)
    sx = (xx + base[:, 0]).clamp(0, w - 1)
    sy = (yy + base[:, 1]).clamp(0, h - 1)
    hw = h * w
    k = max(int(round(0.4 * hw)), 2)
    groups = [("c", c) for c in corners] + ([("s", s) for s in range(4)] if hw >= 8 else [])
    for i in range(n):
        perm = torch.randperm(hw, generator=g)[:k]
        d = 0.2 + 3.8 * torch.rand(2, k, generator=g)                        # how far outside
        ins = torch.rand(2, k, generator=g)                                    # where along a side
        fx, fy = sx[i].reshape(-1), sy[i].reshape(-1)
        for j, (kind, which) in enumerate(groups):
            sel = perm[j::len(groups)]
            dx, dy, ix, iy = d[0, j::len(groups)], d[1, j::len(groups)], ins[0, j::len(groups)] * (w - 1), ins[1, j::len(groups)] * (h - 1)
            if kind == "c":                                                    # 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right
                fx[sel] = -dx if which % 2 == 0 else w - 1 + dx
                fy[sel] = -dy if which // 2 == 0 else h - 1 + dy
            else:                                                              # 0 left, 1 right, 2 top, 3 bottom
                fx[sel] = (-dx, w - 1 + dx, ix, ix)[which]
                fy[sel] = (iy, iy, -dy, h - 1 + dy)[which]
        sx[i], sy[i] = fx.view(h, w), fy.view(h, w)
    return torch.stack([sx - xx, sy - yy], 1).contiguous()


def huge_flow(n, h, w, seed, rot=0):
    """smooth_flow with a quarter of the pixels given one finite huge component: +-1e4, +-3e9 (beyond int32) or +-1e30, in turn on x
    and y; returns (flow, mask of those pixels)"""
    g = gen(seed)
    flow = smooth_flow(n, h, w, seed + 1)
    hw = h * w
    k = max(hw // 4, 1)
    mask = torch.zeros(n, hw, dtype=torch.bool)
    for i in range(n):
        perm = torch.randperm(hw, generator=g)[:k]
        j = torch.arange(k) + rot
        vals = torch.tensor(HUGE_FLOWS, dtype=torch.float32)[j % 6]
        comp = (j // 6) % 2
        fl = flow[i].reshape(2, hw)
        fl[comp, perm] = vals
        mask[i, perm] = True
    return flow, mask.view(n, h, w)


def warp_case_names(shape):
    n, c, h, w = shape
    names = ["smooth", "outside"] + ["const%d" % i for i in range(9)]
    if h * w < 8:
        names.append("outside_corners")
    return names + ["huge%d" % r for r in range(12 if h * w < 24 else 1)]


def warp_case(shape, name):
    """flow_warp case: img, flow, y64, y32, g, zero (pixels whose output must be exactly 0.0), huge (mask or None)"""
    n, c, h, w = shape
    seed = 1000 + 7 * WARP_SHAPES.index(shape)
    img = smooth_image(n, c, h, w, seed)
    huge = None
    if name == "smooth":
        flow = smooth_flow(n, h, w, seed + 1)
    elif name == "outside":
        # a 2 x 2 image has four pixels: 20 .. 60 % of them is one or two, so two opposite corners (all four sides) -- the other
        # two corners are the case "outside_corners", where every pixel leaves
        flow = outside_flow(n, h, w, seed + 2, corners=(0, 3) if h * w < 8 else (0, 1, 2, 3))
    elif name == "outside_corners":
        xx, yy = _grid(h, w)
        flow = torch.stack([torch.where(xx == 0, -1.25, 2.5) + 0 * yy, torch.where(yy == 0, -0.75, 1.75) + 0 * xx], 0)[None].repeat(n, 1, 1, 1).contiguous()
    elif name.startswith("const"):
        fx, fy = const_flows(h, w)[int(name[5:])]
        flow = torch.empty(n, 2, h, w)
        flow[:, 0], flow[:, 1] = float(fx), float(fy)
    else:
        flow, huge = huge_flow(n, h, w, seed + 3, rot=int(name[4:]))
    y64 = og.flow_warp(img.double(), flow.double())
    y32 = og.flow_warp(img, flow)
    zero = far_outside(flow)
    return SimpleNamespace(name="warp %s %s" % ("x".join(map(str, shape)), name), img=img, flow=flow, y64=y64, y32=y32, g=G_WARP,
                           zero=zero, huge=huge, scale=img.abs().max().item())


# ---- bilinear_resize ----------------------------------------------------------------------------------------------------------
# (n, c, (h, w), (ho, wo), mul0, mul1)
RESIZE_CASES = {
    "68x120_to_544x960": (1, 2, (68, 120), (544, 960), 8.0, 8.0),
    "136x240_to_272x480": (2, 2, (136, 240), (272, 480), 2.0, 2.0),
    "1080x1920_to_480x896": (1, 3, (1080, 1920), (480, 896), 1.0, 1.0),
    "544x960_to_1080x1920": (2, 2, (544, 960), (1080, 1920), 1920 / 960, 1080 / 544),
    "same_9x14_n3c2": (3, 2, (9, 14), (9, 14), 1.75, -0.625),
    "1x1_to_5x7_n2c3": (2, 3, (1, 1), (5, 7), 1.75, -0.625),
    "5x7_to_1x1_n3c2": (3, 2, (5, 7), (1, 1), 1.75, -0.625),
    "2x3_to_1x9_n2c3": (2, 3, (2, 3), (1, 9), 1.75, -0.625),
    "2x3_to_1x9_n3c2": (3, 2, (2, 3), (1, 9), 1.75, -0.625),
    "11x17_to_21x33_n3c2": (3, 2, (11, 17), (21, 33), 1.75, -0.625),
    "11x17_to_21x33_n2c3": (2, 3, (11, 17), (21, 33), 1.75, -0.625),
}


def resize_ref(x, size, mul0, mul1):
    """F.interpolate(bilinear, align_corners=True) times mul0 on channel 0 and mul1 on every other channel of each image"""
    y = F.interpolate(x, size=list(size), mode="bilinear", align_corners=True)
    return torch.cat([y[:, :1] * mul0, y[:, 1:] * mul1], 1)


def resize_case(name):
    n, c, (h, w), size, mul0, mul1 = RESIZE_CASES[name]
    seed = 2000 + sorted(RESIZE_CASES).index(name)
    x = smooth_image(n, c, h, w, seed) + 0.9 * torch.randn(n, c, h, w, generator=gen(seed + 500))
    return SimpleNamespace(name="resize " + name, x=x, size=size, mul0=mul0, mul1=mul1, y64=resize_ref(x.double(), size, mul0, mul1),
                           y32=resize_ref(x, size, mul0, mul1), g=G_CONT)


# ---- convex_upsample ----------------------------------------------------------------------------------------------------------
# (b, h, w, factor) -> mask kinds
CONVEX_BIG_KINDS = ["randn", "equal", "pm80"]
CONVEX_ALL_KINDS = CONVEX_BIG_KINDS + ["tap60_%d" % t for t in range(9)] + ["tap120_%d" % t for t in range(9)]
CONVEX_CASES = {(1, 68, 120, 8): CONVEX_BIG_KINDS + ["tap60_7"], (2, 136, 240, 4): CONVEX_BIG_KINDS + ["tap60_7"],
                (1, 1, 1, 4): CONVEX_ALL_KINDS, (2, 3, 5, 2): CONVEX_ALL_KINDS,
                (2, 3, 5, 1): CONVEX_ALL_KINDS, (1, 4, 3, 8): CONVEX_ALL_KINDS}


def neighbour(flow, t):
    """flow[y + t // 3 - 1][x + t % 3 - 1] with zeros outside the image (F.unfold's padding), and the mask of taps inside"""
    b, c, h, w = flow.shape
    dy, dx = t // 3 - 1, t % 3 - 1
    pad = F.pad(flow, (1, 1, 1, 1))
    inside = F.pad(torch.ones(1, 1, h, w, dtype=torch.bool), (1, 1, 1, 1))
    return pad[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], inside[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def convex_case(cfg, kind):
    b, h, w, f = cfg
    seed = 3000 + 11 * sorted(CONVEX_CASES).index(cfg)
    g = gen(seed)
    flow = smooth_flow(b, h, w, seed + 1) + 1.5
    shape = (b, 9 * f * f, h, w)
    tap = None
    if kind == "randn":
        mask = torch.randn(shape, generator=g)
    elif kind == "equal":
        mask = torch.full(shape, 0.375)
    elif kind == "pm80":
        mask = torch.where(torch.rand(shape, generator=g) < 0.5, -80.0, 80.0)
    else:
        level, tap = float(kind[3:kind.index("_")]), int(kind.split("_")[1])
        mask = torch.zeros(b, 9, f * f, h, w)
        mask[:, tap] = level
        mask = mask.view(shape).contiguous()
    y64 = og.upsample_flow_with_mask(flow.double(), mask.double(), f)
    y32 = og.upsample_flow_with_mask(flow, mask, f)
    return SimpleNamespace(name="convex %dx%dx%d f%d %s" % (b, h, w, f, kind), flow=flow, mask=mask, factor=f, y64=y64, y32=y32, g=G_CONT,
                           tap=tap, kind=kind, scale=f * flow.abs().max().item())


def up_nearest(x, f):
    return x.repeat_interleave(f, dim=2).repeat_interleave(f, dim=3)


# ---- fb_check -----------------------------------------------------------------------------------------------------------------
FB_SHAPES = [(2, 2, 68, 120), (1, 2, 136, 240), (1, 2, 2, 2), (3, 2, 5, 300)]


def fb_flows(shape):
    """fwd = a per-image constant vector of a few pixels + 0.05 x a smooth field, bwd = -fwd + 0.4 N(0,1): pixels that warp out of
    the image are occluded through the zero padding, the noise decides the others.  Four pixels cannot be drawn: the 2 x 2 frame
    has one pixel per mask whose flow leaves the image (3 px), the others rest."""
    n, _, h, w = shape
    if h * w < 8:
        fwd, bwd = torch.zeros(shape), torch.zeros(shape)
        fwd[:, 0, 0, 0] = -3.0
        bwd[:, 0, 1, 1] = 3.0
        return fwd, bwd
    seed = 4000 + 13 * FB_SHAPES.index(shape)
    g = gen(seed)
    const = torch.tensor([[3.0, -2.0], [-4.5, 1.25], [2.0, 0.75]])[:n].view(n, 2, 1, 1)
    if h < 8:
        const = const * torch.tensor([1.0, 0.25]).view(1, 2, 1, 1)          # five rows: keep the vertical part below a row
    fwd = const + 0.05 * smooth_flow(n, h, w, seed + 1)
    bwd = -fwd + 0.4 * torch.randn(shape, generator=g)
    return fwd.contiguous(), bwd.contiguous()


def fb_reference(fwd, bwd, alpha=0.01, beta=0.5):
    """float64: (fwd_occ, bwd_occ, fwd_band, bwd_band); band = pixels whose margin |diff| - (alpha mag + beta) is within
    1e-4 max(1, mag) of zero, where float32 arithmetic may decide either way"""
    f, b = fwd.double(), bwd.double()
    mag = torch.norm(f, dim=1) + torch.norm(b, dim=1)
    thr = alpha * mag + beta
    out = []
    for a, other in ((f, b), (b, f)):
        margin = torch.norm(a + og.flow_warp(other, a), dim=1) - thr
        out.append(((margin > 0).double(), margin.abs() <= 1e-4 * mag.clamp(min=1.0)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- instance_norm --------------------------------------------------------------------------------------------------------------
# name -> x shape [N, C, H, W]; the split path runs when planes < 1024 and plane >= 16384
INORM_SHAPES = {"p%d" % p: (2, 3, 1, p) for p in (1, 2, 63, 64, 255, 256, 257, 1000)}
INORM_SHAPES.update({"p%d" % p: (1, 3, 1, p) for p in (16383, 16384, 16385)})
INORM_SHAPES.update({"128x128x1023": (1, 1023, 128, 128), "128x128x1024": (1, 1024, 128, 128), "half_res": (1, 4, 272, 480)})
INORM_SPECIAL_SHAPES = ["p1", "p2", "p257", "p1000", "p16383", "p16385", "half_res"]       # constant / tiny-spread / offset data
INORM_EPS = 1e-5


def inorm_plain(x):
    """InstanceNorm2d(affine=False, eps=1e-5): og._inorm; torch refuses a 1-pixel plane, whose statement is the same formula"""
    if x.shape[2] * x.shape[3] > 1:
        return og._inorm(x)
    mean = x.mean(dim=(2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - mean) / torch.sqrt(var + INORM_EPS)


def inorm_modes(y, skip):
    """the three forms of backbone.py:34-39 from IN(x): mode 0, 1 (relu), 2 (relu(skip + relu))"""
    return [y, F.relu(y), F.relu(skip.to(y.dtype) + F.relu(y))]


def inorm_data(name, kind):
    shape = INORM_SHAPES[name]
    seed = 5000 + 17 * sorted(INORM_SHAPES).index(name)
    g = gen(seed)
    skip = torch.randn(shape, generator=g)
    n, c = shape[:2]
    if kind == "randn":
        x = torch.randn(shape, generator=g) * 3 + 1
    elif kind == "constant":
        x = (torch.randn(n, c, 1, 1, generator=g) * 3 + 1).expand(shape).contiguous()
    elif kind == "tiny":
        x = torch.randn(shape, generator=g) * 1e-4
    else:                                                                      # "offset": mean 1e3, standard deviation 1e-2
        x = torch.randn(shape, generator=g) * 1e-2 + 1e3
    return x, skip


def inorm_case(name, kind="randn"):
    x, skip = inorm_data(name, kind)
    return SimpleNamespace(name="inorm %s %s" % (name, kind), x=x, skip=skip, y64=inorm_plain(x.double()), y32=inorm_plain(x), g=G_CONT)


def inorm_offset_bound(x, y64):
    """mean 1e3, spread 1e-2: the kernel, like torch, subtracts the mean ROUNDED to float32, an error of up to 2^-24 |mean| rstd in
    the output that the float32 reference may or may not share (luck), so the floor of the gate is no measure here; the contract
    is  |y - y64| <= 2^-24 |mean| rstd + 8 * 2^-24 max|y64|"""
    xd = x.double()
    mean = xd.mean(dim=(2, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(dim=(2, 3), keepdim=True) + INORM_EPS)
    return HALF_ULP * mean.abs() * rstd + 8 * HALF_ULP * y64.abs().max()


# ---- eltwise --------------------------------------------------------------------------------------------------------------------
ELT_LENGTHS = [1, 255, 256, 257, 4099]
IMG_MEAN, IMG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def eltwise_operands(n, seed=6000):
    g = gen(seed + n)
    a, b, c = (torch.randn(n, generator=g) * 2 for _ in range(3))
    return a, b, c, torch.sigmoid(torch.randn(n, generator=g) * 2)


def normalize_img_ref(img):
    """utils.py:26-34 (oracle/gmflow.py: unimatch_flow_bidir's first line)"""
    mean = torch.tensor(IMG_MEAN, dtype=img.dtype).view(1, 3, 1, 1)
    std = torch.tensor(IMG_STD, dtype=img.dtype).view(1, 3, 1, 1)
    return (img / 255.0 - mean) / std


def normalize_case(plane):
    img = torch.rand(2, 3, 1, plane, generator=gen(6100 + plane)) * 255
    return SimpleNamespace(name="eltwise normalize_img plane %d" % plane, x=img, plane=plane, y64=normalize_img_ref(img.double()),
                           y32=normalize_img_ref(img), g=G_CONT)


def tanh_relu_ref(x, split):
    """unimatch.py:320-323: tanh on the first `split` channels, relu on the others"""
    return torch.cat([torch.tanh(x[:, :split]), torch.relu(x[:, split:])], 1)


def tanh_relu_case(chans, split, plane):
    x = torch.randn(2, chans, 1, plane, generator=gen(6200 + chans + split)) * 2
    return SimpleNamespace(name="eltwise tanh|relu chans %d split %d plane %d" % (chans, split, plane), x=x, chans=chans, split=split,
                           plane=plane, y64=tanh_relu_ref(x.double(), split), y32=tanh_relu_ref(x, split), g=G_CONT)


# ---- layernorm128 ---------------------------------------------------------------------------------------------------------------
LN_TOKENS = [1, 3, 4, 5, 4099]
LN_PARTIALS = [1, 2, 5]
LN_EPS = 1e-5


def ln_params(seed=7000):
    g = gen(seed)
    return torch.randn(128, generator=g), torch.randn(128, generator=g)


def ln_ref(x, gamma, beta, res):
    y = F.layer_norm(x, (128,), gamma.to(x.dtype), beta.to(x.dtype), eps=LN_EPS)
    return y if res is None else res.to(x.dtype) + y


def ln_case(tokens, partials=1, residual=False, kind="randn"):
    g = gen(7100 + 31 * tokens + partials)
    gamma, beta = ln_params()
    if kind == "randn":
        x = torch.randn(partials, tokens, 128, generator=g) * 2 + 0.5
    elif kind == "constant":
        x = (torch.randn(partials, tokens, 1, generator=g) * 2 + 0.5).expand(partials, tokens, 128).contiguous()
    else:                                                                      # "offset": rows of 1e3 +- 1e-2
        x = torch.randn(partials, tokens, 128, generator=g) * 1e-2 + 1e3 / partials
    res = torch.randn(tokens, 128, generator=g) if residual else None
    s = x[0].clone()                                                           # the slabs, added in float32 in slab order
    for p in range(1, partials):
        s = s + x[p]
    return SimpleNamespace(name="layernorm T %d P %d %s%s" % (tokens, partials, kind, " +res" if residual else ""),
                           x=x if partials > 1 else x[0].contiguous(), summed=s, gamma=gamma, beta=beta, res=res, partials=partials,
                           y64=ln_ref(s.double(), gamma, beta, res), y32=ln_ref(s, gamma, beta, res), g=G_CONT)


def ln_offset_bound(case):
    """rows of 1e3 +- 1e-2: the mean of 128 float32 values carries up to 128 * 2^-24 |mean| of summation error, times rstd |gamma| in
    the output; the float32 reference's share of it is luck, so the bound comes from the contract, plus 8 ulp of the output range"""
    s = case.summed.double()
    mean = s.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((s - mean) ** 2).mean(dim=-1, keepdim=True) + LN_EPS)
    return 128 * HALF_ULP * mean.abs() * rstd * case.gamma.abs().max().double() + 8 * HALF_ULP * case.y64.abs().max()

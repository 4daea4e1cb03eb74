"""Seeded case builders for the GMFlow STAGES (color-transfer_amd/unimatch/__init__.py: the host code between the kernels -- residual
block, backbone, transformer layer, six-layer transformer, global matching, the two propagations, the net | inp split and the
update block), teacher forced: a case gives ONE stage the input the float64 oracle saw, rounded to float32, so the rounding a
150-layer random-weight network amplifies (tests/test_gmflow_gpu.py: STAGE_BOUNDS of 1e-2 px) never builds up.

Everything here is torch on the CPU plus oracle/gmflow.py; nothing touches ct_hip.  tests/test_gmflow_stages_host.py proves on the
CPU that every case is admitted and that a wrong stage cannot pass it, tests/test_gmflow_stages_gpu.py holds the stages to the cases.

The gate of an output: y64 = the oracle on x.double() with the weights in double, y32 = the same call in float32 (the reference to
the last bit), y = the device result.
  maximum   max|y - y64| <= max(2 max|y32 - y64|, g),  g = 2e-5 max(1, max|y64|)   (the rule of tests/gmflow_glue_common.py; g is
            the atol 2e-5 + rtol 2e-5 that tests/test_gmflow_kernels_gpu.py::close holds the stages' kernels to)
  rms       rms(y - y64) <= R rms(y32 - y64),  R = F64_RATIO[conv_mode][0] of tests/test_gmflow_gpu.py; skipped where the float32
            oracle is exact (rms(y32 - y64) == 0: the one-hot matching case)
The update block alone misses the rms rule on the device while meeting the maximum one (net: ratio 2.05 .. 2.76 in every mode, the
bitwise fmaf chain of the exact mode included: arithmetic, not a wrong stage.  Its six GRU convolutions sum 1920 products per
output; the device kernels add them as one float32 chain (ct_hip/conv.py), and the float32 oracle's convolution sits closer to
float64 than such a chain is expected to).  Its outputs carry `model`, the rms error a chain of that length is expected to have
on the case, evaluated in float64 (update_block_model), and are held to R max(rms(y32 - y64), model).
Nothing in either rule is measured on the code under test.  A case is admitted only if its maximum gate is at most CAP = 1e-3 of
max|y64|."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gmflow as og
from tests.gmflow_common import procedural_state
from tests.gmflow_glue_common import CAP, gen
from tests.test_gmflow_gpu import F64_RATIO

G_REL = 2e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
cached = functools.lru_cache(maxsize=None)


# ---- weights ----------------------------------------------------------------------------------------------------------------
@cached
def state_spec():
    g = np.load(os.path.join(GOLDEN, "gmflow_small.npz"), allow_pickle=False)
    names = [str(s) for s in g["state_names"]]
    shapes = [tuple(int(x) for x in s[:n]) for s, n in zip(g["state_shapes"], g["state_ndim"])]
    return names, shapes


@cached
def state():
    """the procedural float32 state_dict of tests/test_gmflow_gpu.py::build"""
    return procedural_state(*state_spec())


@cached
def state64():
    return {k: v.double() for k, v in state().items()}


def both(fn):
    """(y32, y64) of fn(sd, cast): the same oracle call in float32 and in float64"""
    y32 = fn(state(), lambda t: t)
    y64 = fn(state64(), lambda t: t.double())
    return y32, y64


# ---- the gate ---------------------------------------------------------------------------------------------------------------
def rms(t):
    return t.double().pow(2).mean().sqrt().item()


def gate(y32, y64):
    """(gate, floor, g): floor = the float32 oracle's own distance from float64"""
    floor = (y32.double() - y64).abs().max().item()
    g = G_REL * max(1.0, y64.abs().max().item())
    return max(2.0 * floor, g), floor, g


def admitted(out):
    """(ok, gate, range): the maximum gate of an output is at most CAP of its range"""
    gt, _, _ = gate(out.y32, out.y64)
    scale = out.y64.abs().max().item()
    return gt <= CAP * scale, gt, scale


def ratio_for(conv_mode):
    return F64_RATIO[conv_mode][0]


def measure(name, out, y, conv_mode):
    """one row of the per-stage table: the achieved error of the device result y against the output's two rules"""
    assert tuple(y.shape) == tuple(out.y64.shape), (name, out.label, tuple(y.shape), tuple(out.y64.shape))
    y = y.detach().double().cpu()
    assert torch.isfinite(y).all(), (name, out.label)
    gt, floor, _ = gate(out.y32, out.y64)
    err = (y - out.y64).abs().max().item()
    r_ref, r_dev = rms(out.y32.double() - out.y64), rms(y - out.y64)
    R = ratio_for(conv_mode)
    r_base = max(r_ref, out.model or 0.0)               # the float32 oracle's rms error, or the modelled one of the kernels' arithmetic
    row = SimpleNamespace(name="%s / %s" % (name, out.label), err=err, floor=floor, gate=gt, rms=r_dev, rms_ref=r_ref, model=out.model,
                          ratio=(r_dev / r_base if r_base > 0 else float("nan")), R=R,
                          ok_max=err <= gt, ok_rms=(r_ref == 0.0 or r_dev <= R * r_base))
    print("   %-58s err %.2e  floor %.2e  gate %.2e  rms %.2e / %s%.2e = %5.2f (<= %.1f)%s"
          % (row.name, err, floor, gt, r_dev, "" if out.model is None else "max(model %.2e, float32) " % out.model, r_base, row.ratio, R,
             "" if row.ok_max and row.ok_rms else "   <-- FAILS"))
    return row


def hold(case, ys, conv_mode):
    """print every output's figures, then assert both rules on every output"""
    assert len(ys) == len(case.outs), (case.name, len(ys), len(case.outs))
    print("\n[%s, %s]" % (case.name, conv_mode))
    rows = [measure(case.name, o, y, conv_mode) for o, y in zip(case.outs, ys)]
    bad = [(r.name, "err %.3g > gate %.3g" % (r.err, r.gate) if not r.ok_max else "rms ratio %.3g > %.1f" % (r.ratio, r.R))
           for r in rows if not (r.ok_max and r.ok_rms)]
    assert not bad, bad
    return rows


def out(label, y32, y64, model=None):
    """model: the rms error the stage's documented arithmetic is expected to have on this case (float64 evaluation), or None"""
    return SimpleNamespace(label=label, y32=y32, y64=y64, model=model)


def tokens(x):                                         # [B,C,H,W] -> [B,H*W,C]
    return x.flatten(2).transpose(1, 2).contiguous()


def nchw(t, h, w):                                     # [B,H*W,C] -> [B,C,H,W]
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], h, w).contiguous()


def swap_halves(t):
    return torch.cat(t.chunk(2, dim=0)[::-1], dim=0)


def altered(sd, **changes):
    sd = dict(sd)
    sd.update(changes)
    return sd


# ---- _add_position, _tokens / _nchw: bitwise ----------------------------------------------------------------------------------
POSITION_SHAPES = [((2, 128, 8, 12), 2), ((2, 128, 16, 24), 8)]
TOKEN_SHAPES = [(2, 128, 8, 12), (1, 128, 5, 7), (3, 2, 16, 24)]


def position_case(shape, splits):
    g = gen(100 + shape[2])
    f0, f1 = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    return SimpleNamespace(f0=f0, f1=f1, splits=splits, want=og.feature_add_position(f0, f1, splits, shape[1]))


# ---- _resblock, _backbone -----------------------------------------------------------------------------------------------------
# name -> (prefix, stride, input shape)
RESBLOCK_CASES = {"layer1.0 12x20": ("backbone.layer1.0", 1, (2, 64, 12, 20)), "layer2.0 16x24": ("backbone.layer2.0", 2, (2, 64, 16, 24)),
                  "layer2.0 17x23": ("backbone.layer2.0", 2, (2, 64, 17, 23))}
BACKBONE_SHAPES = [(2, 3, 64, 96), (2, 3, 40, 72)]


def _residual_block_no_inner_relu(sd, pre, x, stride):
    """og.residual_block with relu(IN(conv2)) replaced by IN(conv2): the mode-2 instance norm taken for skip + IN"""
    y = F.relu(og._inorm(F.conv2d(x, sd[pre + ".conv1.weight"], None, stride=stride, padding=1)))
    y = og._inorm(F.conv2d(y, sd[pre + ".conv2.weight"], None, padding=1))
    if pre + ".downsample.0.weight" in sd:
        x = og._inorm(F.conv2d(x, sd[pre + ".downsample.0.weight"], sd[pre + ".downsample.0.bias"], stride=stride))
    return F.relu(x + y)


@cached
def resblock_case(name):
    pre, stride, shape = RESBLOCK_CASES[name]
    x = torch.relu(torch.randn(shape, generator=gen(200 + shape[3])))                 # what a block sees: the output of a relu
    y32, y64 = both(lambda sd, c: og.residual_block(sd, pre, c(x), stride))
    alts = {"inner relu missing": lambda: [_residual_block_no_inner_relu(state64(), pre, x.double(), stride)]}
    if stride == 2:
        # the 3x3 and the 1x1 convolution read DIFFERENT phases of the shared space-to-depth image: the 1x1 fed phase (1, 1)
        # the 3x3 and the 1x1 convolution read different phases of the shared space-to-depth image: the 1x1 fed phase (1, 1)
        alts["downsample reads phase (1, 1)"] = lambda: [_resblock_wrong_phase(pre, x.double())]
    return SimpleNamespace(name="resblock " + name, prefix=pre, stride=stride, x=x, outs=[out("y", y32, y64)], alts=alts)


def _resblock_wrong_phase(pre, x):
    """float64 residual block whose skip convolution samples x[1::2, 1::2] (zero beyond the frame) instead of x[0::2, 0::2];
    the sum before the last relu is not clamped in between, so this is the block's pre-activation with the skip exchanged"""
    sd = state64()
    y = F.relu(og._inorm(F.conv2d(x, sd[pre + ".conv1.weight"], None, stride=2, padding=1)))
    y = F.relu(og._inorm(F.conv2d(y, sd[pre + ".conv2.weight"], None, padding=1)))
    xs = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]
    skip = og._inorm(F.conv2d(xs, sd[pre + ".downsample.0.weight"], sd[pre + ".downsample.0.bias"], stride=2))
    return F.relu(skip + y)


@cached
def backbone_case(shape):
    x = torch.randn(shape, generator=gen(300 + shape[2]))                             # a normalised image
    y32, y64 = both(lambda sd, c: og.cnn_encoder(sd, c(x)))
    labels = ("stride 1", "stride 2")

    def no_conv2_bias():
        sd = state64()
        return og.cnn_encoder(altered(sd, **{"backbone.conv2.bias": 0 * sd["backbone.conv2.bias"]}), x.double())

    def stride2_wrong_phase():                             # the stride-2 trident output = the stride-1 one at [::2, ::2], here [1::2, 1::2]
        a = y64[0]
        return [a, F.pad(a, (0, 1, 0, 1))[:, :, 1::2, 1::2][:, :, :y64[1].shape[2], :y64[1].shape[3]]]
    alts = {"conv2 bias missing": no_conv2_bias, "stride-2 output samples phase (1, 1)": stride2_wrong_phase}
    return SimpleNamespace(name="backbone %dx%d" % shape[2:], x=x, outs=[out(l, a, b) for l, a, b in zip(labels, y32, y64)], alts=alts)


# ---- _tlayer ------------------------------------------------------------------------------------------------------------------
# (h, w, splits, token batch); 32x32 x 4 = 4096 tokens: the resident-weight kernels' threshold (ct_hip/linears.py), 32x56 x 2 = 3584
TLAYER_GEOMS = [(8, 12, 2, 4), (16, 24, 8, 4), (8, 16, 8, 4), (8, 12, 2, 2), (32, 32, 8, 4), (32, 56, 8, 2)]
TLAYER_SMALL = TLAYER_GEOMS[:3]
TLAYER_KINDS = ("self_attn", "cross_attn_ffn")
L1 = "transformer.layers.1"


def window_mask(h, w, splits, dtype):
    return og.shift_window_mask(h, w, h // splits, w // splits).to(dtype)


@cached
def tlayer_input(geom):
    """float32 input of layer 1: N(0,1) features with their position, through layer 0 of the float64 oracle"""
    h, w, splits, nb = geom
    f = torch.randn(nb, 128, h, w, generator=gen(400 + 7 * TLAYER_GEOMS.index(geom)))
    f0, f1 = og.feature_add_position(*f.double().chunk(2, dim=0), splits, 128)
    c0 = torch.cat((tokens(f0), tokens(f1)), dim=0)
    sd, mask = state64(), window_mask(h, w, splits, torch.float64)
    s = og.transformer_layer(sd, "transformer.layers.0.self_attn", c0, c0, h, w, mask, False, splits, ffn=False)
    c0 = og.transformer_layer(sd, "transformer.layers.0.cross_attn_ffn", s, swap_halves(c0), h, w, mask, False, splits, ffn=True)
    return c0.float().contiguous()


@cached
def tlayer_case(geom, kind, shift):
    """source / target as _transformer passes them to _tlayer: self_attn gets the layer's input twice, cross_attn_ffn the float64
    self-attention output (rounded) and the layer's INPUT with kv_swap; the oracle's target is the exchanged concat"""
    h, w, splits, nb = geom
    c_in = tlayer_input(geom)
    ffn = kind == "cross_attn_ffn"
    pre = L1 + "." + kind
    if ffn:
        mask64 = window_mask(h, w, splits, torch.float64)
        source = og.transformer_layer(state64(), L1 + ".self_attn", c_in.double(), c_in.double(), h, w, mask64, shift, splits, ffn=False)
        source = source.float().contiguous()
    else:
        source = c_in

    def run(sd, c, with_shift=shift, zero_mask=False, exchange=ffn, pre=pre):
        mask = window_mask(h, w, splits, c(c_in).dtype)
        target = swap_halves(c(c_in)) if exchange else c(c_in)
        return og.transformer_layer(sd, pre, c(source), target, h, w, mask * 0 if zero_mask else mask, with_shift, splits, ffn)
    y32, y64 = both(run)
    dbl = lambda t: t.double()
    sd64 = state64()
    alts = {"k_proj and v_proj weights exchanged": lambda: [run(altered(sd64, **{pre + ".k_proj.weight": sd64[pre + ".v_proj.weight"],
                                                                                 pre + ".v_proj.weight": sd64[pre + ".k_proj.weight"]}), dbl)]}
    if shift:
        alts["shift off"] = lambda: [run(sd64, dbl, with_shift=False)]
        alts["mask zeroed"] = lambda: [run(sd64, dbl, zero_mask=True)]
    if ffn:
        alts["batch halves of the target not exchanged"] = lambda: [run(sd64, dbl, exchange=False)]
    return SimpleNamespace(name="tlayer %s %dx%d/%d B%d shift %d" % (kind, h, w, splits, nb, shift), geom=geom, kind=kind, shift=shift,
                           source=source, target=c_in, outs=[out("tokens", y32, y64)], alts=alts)


# ---- _transformer -------------------------------------------------------------------------------------------------------------
TRANSFORMER_CASES = [((1, 128, 16, 24), 8), ((2, 128, 8, 12), 2)]


def _transformer_stale_target(sd, f0, f1, splits):
    """og.feature_transformer whose exchanged concat is built once and never refreshed after a layer"""
    b, c, h, w = f0.shape
    mask = window_mask(h, w, splits, f0.dtype)
    c0, c1 = torch.cat((tokens(f0), tokens(f1)), dim=0), torch.cat((tokens(f1), tokens(f0)), dim=0)
    for i in range(6):
        pre = "transformer.layers.%d" % i
        c0 = og.transformer_layer(sd, pre + ".self_attn", c0, c0, h, w, mask, i % 2 == 1, splits, ffn=False)
        c0 = og.transformer_layer(sd, pre + ".cross_attn_ffn", c0, c1, h, w, mask, i % 2 == 1, splits, ffn=True)
    return [nchw(t, h, w) for t in c0.chunk(2, dim=0)]


@cached
def transformer_case(shape, splits):
    g = gen(500 + shape[2])
    f0, f1 = og.feature_add_position(torch.randn(shape, generator=g), torch.randn(shape, generator=g), splits, 128)
    f0, f1 = f0.contiguous(), f1.contiguous()
    y32, y64 = both(lambda sd, c: og.feature_transformer(sd, c(f0), c(f1), splits))
    alts = {"exchanged concat never refreshed": lambda: _transformer_stale_target(state64(), f0.double(), f1.double(), splits)}
    return SimpleNamespace(name="transformer %dx%dx%d/%d" % (shape[0], shape[2], shape[3], splits), f0=f0, f1=f1, splits=splits,
                           outs=[out("t0", y32[0], y64[0]), out("t1", y32[1], y64[1])], alts=alts)


# ---- global matching ------------------------------------------------------------------------------------------------------------
MATCH_KINDS = ("randn", "matched x1", "matched x3")
MATCH_SHAPE = (2, 128, 8, 12)


@cached
def match_case(kind, bidir):
    g = gen(600 + MATCH_KINDS.index(kind))
    f0 = torch.randn(MATCH_SHAPE, generator=g)
    if kind == "randn":
        f1 = torch.randn(MATCH_SHAPE, generator=g)
    else:                                                  # f1 = f0 moved by (1, 2) + noise: peaked rows, largest logit 16 / 136
        f0 = f0 * float(kind[-1])
        f1 = torch.roll(f0, shifts=(1, 2), dims=(2, 3)) + 0.1 * torch.randn(MATCH_SHAPE, generator=g)
    y32, y64 = both(lambda sd, c: og.global_correlation_softmax_bidir(c(f0), c(f1), bidir))
    logit = (torch.matmul(tokens(f0).double(), tokens(f1).double().transpose(1, 2)) / 128 ** 0.5).max().item()
    alts = {"frames exchanged": lambda: [og.global_correlation_softmax_bidir(f1.double(), f0.double(), bidir)]}
    return SimpleNamespace(name="global match %s bidir %d" % (kind, bidir), f0=f0, f1=f1, bidir=bidir, logit=logit,
                           outs=[out("flow", y32, y64)], alts=alts)


# ---- propagation ----------------------------------------------------------------------------------------------------------------
PROP_SHAPE = (2, 128, 16, 24)


@cached
def prop_case(radius):
    g = gen(700 + radius)
    f0, flow = torch.randn(PROP_SHAPE, generator=g), 3 * torch.randn(PROP_SHAPE[0], 2, *PROP_SHAPE[2:], generator=g)
    y32, y64 = both(lambda sd, c: og.self_attn_propagation(sd, c(f0), c(flow), radius))
    sd = state64()
    if radius <= 0:                                        # k = k_proj(x) instead of the reference's k_proj(q_proj(x))
        def alt():
            b, c, h, w = f0.shape
            t = tokens(f0.double())
            q = F.linear(t, sd["feature_flow_attn.q_proj.weight"], sd["feature_flow_attn.q_proj.bias"])
            k = F.linear(t, sd["feature_flow_attn.k_proj.weight"], sd["feature_flow_attn.k_proj.bias"])
            p = torch.softmax(torch.matmul(q, k.transpose(1, 2)) / c ** 0.5, dim=-1)
            return [nchw(torch.matmul(p, tokens(flow.double())), h, w)]
        alts = {"quirk k_proj(q_proj(x)) dropped": alt}
    else:
        def alt():
            q = F.linear(tokens(f0.double()), sd["feature_flow_attn.q_proj.weight"], sd["feature_flow_attn.q_proj.bias"])
            return [og.self_attn_propagation(altered(sd, **{"feature_flow_attn.q_proj.weight": torch.eye(128, dtype=torch.float64),
                                                            "feature_flow_attn.q_proj.bias": torch.zeros(128, dtype=torch.float64)}),
                                             nchw(q, *f0.shape[2:]), flow.double(), radius)]
        alts = {"quirk k_proj(q_proj(x)) added": alt}
    return SimpleNamespace(name="propagation %s" % ("global" if radius <= 0 else "local r%d" % radius), f0=f0, flow=flow, radius=radius,
                           outs=[out("flow", y32, y64)], alts=alts)


# ---- refine_proj: net | inp -----------------------------------------------------------------------------------------------------
def _net_inp(sd, f0, exchanged=False):
    proj = F.conv2d(f0, sd["refine_proj.weight"], sd["refine_proj.bias"])            # unimatch.py:318-323, the oracle's two lines
    net, inp = torch.chunk(proj, 2, dim=1)
    return [torch.relu(net), torch.tanh(inp)] if exchanged else [torch.tanh(net), torch.relu(inp)]


@cached
def refine_state_case():
    f0 = torch.randn(PROP_SHAPE, generator=gen(800))
    y32, y64 = both(lambda sd, c: _net_inp(sd, c(f0)))
    alts = {"tanh and relu exchanged": lambda: _net_inp(state64(), f0.double(), exchanged=True)}
    return SimpleNamespace(name="refine_proj net | inp", f0=f0, outs=[out("net", y32[0], y64[0]), out("inp", y32[1], y64[1])], alts=alts)


# ---- _refine_iter ---------------------------------------------------------------------------------------------------------------
UPDATE_SHAPES = [(2, 16, 24), (1, 5, 6)]
UPDATE_ALTS = ("convz and convr weights exchanged", "h and q exchanged in the blend", "flow missing from x", "bias doubled")


def update_block(sd, net, inp, corr, flow, want_mask, alt=None):
    """og.basic_update_block (bit for bit with alt=None: tests/test_gmflow_stages_host.py) with the named alterations"""
    p = "refine."
    if alt == UPDATE_ALTS[0]:
        sd = altered(sd, **{p + "gru.conv%s%s.%s" % (a, s, k): sd[p + "gru.conv%s%s.%s" % (b, s, k)]
                            for a, b in (("z", "r"), ("r", "z")) for s in "12" for k in ("weight", "bias")})
    if alt == UPDATE_ALTS[3]:
        sd = altered(sd, **{k: 2 * v for k, v in sd.items() if k.startswith(p + "gru.") and k.endswith(".bias")})
    cor = F.relu(og._c(sd, p + "encoder.convc1", corr, 0))
    cor = F.relu(og._c(sd, p + "encoder.convc2", cor, 1))
    flo = F.relu(og._c(sd, p + "encoder.convf1", flow, 3))
    flo = F.relu(og._c(sd, p + "encoder.convf2", flo, 1))
    mot = F.relu(og._c(sd, p + "encoder.conv", torch.cat([cor, flo], dim=1), 1))
    x = torch.cat([inp, mot, 0 * flow if alt == UPDATE_ALTS[2] else flow], dim=1)
    h = net
    for suf, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(og._c(sd, p + "gru.convz" + suf, hx, pad))
        r = torch.sigmoid(og._c(sd, p + "gru.convr" + suf, hx, pad))
        q = torch.tanh(og._c(sd, p + "gru.convq" + suf, torch.cat([r * h, x], dim=1), pad))
        h = (1 - z) * q + z * h if alt == UPDATE_ALTS[1] else (1 - z) * h + z * q
    delta = og._c(sd, p + "flow_head.conv2", F.relu(og._c(sd, p + "flow_head.conv1", h, 1)), 1)
    mask = og._c(sd, p + "mask.2", F.relu(og._c(sd, p + "mask.0", h, 1)), 0) if want_mask else None
    return h, mask, delta


U32 = 2.0 ** -24                                       # unit roundoff of float32


def _conv_chain(sd, name, x, vx, pad):
    """(y, var y) of a convolution accumulated as ONE float32 chain per output, in any order (the documented arithmetic of the
    device convolutions: ct_hip/conv.py, "exact" = bitwise an fmaf chain over cin kh kw products; the split forms accumulate their
    pieces in float32 the same way).  Each of the K additions rounds the partial sum s_k it produces by a relative error of at most
    u = 2^-24, taken as independent and uniform: variance u^2/3 s_k^2.  Whatever the order, with uncorrelated terms
    E s_k^2 <= sum_j t_j^2 + S^2 (t_j = x_j w_j the products, S the finished sum), so
        var y = conv(var x, w^2) + u^2/3 K (conv(x^2, w^2) + y^2),   K = the taps inside the frame."""
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    y = F.conv2d(x, w, b, padding=pad)
    k = F.conv2d(torch.ones_like(x[:1, :1]), torch.ones_like(w[:1, :1]), padding=pad) * w.shape[1]
    return y, F.conv2d(vx, w * w, None, padding=pad) + U32 ** 2 / 3 * k * (F.conv2d(x * x, w * w, None, padding=pad) + y * y)


def _rounded(y, v, n=1):
    """n further float32 roundings of a stored elementwise result"""
    return v + n * U32 ** 2 / 3 * y * y


def update_block_model(sd, net, inp, corr, flow, want_mask):
    """rms of the error a float32 implementation of og.basic_update_block built from such chains is expected to have, per output
    (net, mask, delta), evaluated on the case in float64: the variances of _conv_chain carried through the block to first order
    (relu: the sign's indicator; sigmoid' = s (1 - s); tanh' = 1 - t^2; products and the blend by their partial derivatives; errors
    of different operands taken as independent), one rounding per stored elementwise result.  Inputs are exact."""
    p = "refine."
    zero = torch.zeros_like

    def crelu(name, x, vx, pad):
        y, v = _conv_chain(sd, name, x, vx, pad)
        return F.relu(y), v * (y > 0)
    cor, vcor = crelu(p + "encoder.convc1", corr, zero(corr), 0)
    cor, vcor = crelu(p + "encoder.convc2", cor, vcor, 1)
    flo, vflo = crelu(p + "encoder.convf1", flow, zero(flow), 3)
    flo, vflo = crelu(p + "encoder.convf2", flo, vflo, 1)
    mot, vmot = crelu(p + "encoder.conv", torch.cat([cor, flo], dim=1), torch.cat([vcor, vflo], dim=1), 1)
    x, vx = torch.cat([inp, mot, flow], dim=1), torch.cat([zero(inp), vmot, zero(flow)], dim=1)
    h, vh = net, zero(net)
    for suf, pad in (("1", (0, 2)), ("2", (2, 0))):
        hx, vhx = torch.cat([h, x], dim=1), torch.cat([vh, vx], dim=1)
        z, vz = _conv_chain(sd, p + "gru.convz" + suf, hx, vhx, pad)
        z = torch.sigmoid(z)
        vz = _rounded(z, vz * (z * (1 - z)) ** 2)
        r, vr = _conv_chain(sd, p + "gru.convr" + suf, hx, vhx, pad)
        r = torch.sigmoid(r)
        vr = _rounded(r, vr * (r * (1 - r)) ** 2)
        rh, vrh = r * h, _rounded(r * h, r * r * vh + h * h * vr)
        q, vq = _conv_chain(sd, p + "gru.convq" + suf, torch.cat([rh, x], dim=1), torch.cat([vrh, vx], dim=1), pad)
        q = torch.tanh(q)
        vq = _rounded(q, vq * (1 - q * q) ** 2)
        hn = (1 - z) * h + z * q
        h, vh = hn, _rounded(hn, (q - h) ** 2 * vz + (1 - z) ** 2 * vh + z * z * vq, 3)
    d, vd = crelu(p + "flow_head.conv1", h, vh, 1)
    d, vd = _conv_chain(sd, p + "flow_head.conv2", d, vd, 1)
    res = [vh, None, vd]
    if want_mask:
        m, vm = crelu(p + "mask.0", h, vh, 1)
        res[1] = _conv_chain(sd, p + "mask.2", m, vm, 0)[1]
    return [None if v is None else v.mean().sqrt().item() for v in res]


def _update_outs(y32, y64, model):
    return [out(l, a, b, m) for l, a, b, m in zip(("net", "mask", "delta"), y32, y64, model) if b is not None]


@cached
def update_case(shape, want_mask, convz1_scale=1.0):
    """one iteration (outs) and the next one through the same buffers (outs2): a fresh correlation, the flow advanced by the float64
    oracle's delta, the same loop-invariant net and inp.  convz1_scale: the oracle's gru.convz1.weight times this"""
    b, h, w = shape
    g = gen(900 + 10 * UPDATE_SHAPES.index(shape))
    net, inp = torch.tanh(torch.randn(b, 128, h, w, generator=g)), torch.relu(torch.randn(b, 128, h, w, generator=g))
    corr, flow = torch.randn(b, 81, h, w, generator=g), 3 * torch.randn(b, 2, h, w, generator=g)
    corr2 = torch.randn(b, 81, h, w, generator=g)
    key = "refine.gru.convz1.weight"

    def scaled(sd):
        return sd if convz1_scale == 1.0 else altered(sd, **{key: sd[key] * convz1_scale})
    y32, y64 = both(lambda sd, c: og.basic_update_block(scaled(sd), c(net), c(inp), c(corr), c(flow), want_mask))
    flow2 = (flow.double() + y64[2]).float()
    z32, z64 = both(lambda sd, c: og.basic_update_block(scaled(sd), c(net), c(inp), c(corr2), c(flow2), want_mask))
    dbl = [t.double() for t in (net, inp, corr, flow)]
    ymodel = update_block_model(scaled(state64()), *dbl, want_mask)
    zmodel = update_block_model(scaled(state64()), net.double(), inp.double(), corr2.double(), flow2.double(), want_mask)
    alts = {a: (lambda a=a: [t for t in update_block(scaled(state64()), *dbl, want_mask, alt=a) if t is not None]) for a in UPDATE_ALTS}
    return SimpleNamespace(name="update block %dx%dx%d mask %d%s" % (b, h, w, want_mask, "" if convz1_scale == 1.0 else " convz1 x %g" % convz1_scale),
                           net=net, inp=inp, corr=corr, flow=flow, corr2=corr2, flow2=flow2, want_mask=want_mask,
                           outs=_update_outs(y32, y64, ymodel), outs2=_update_outs(z32, z64, zmodel), alts=alts)


def second_iteration(case):
    return SimpleNamespace(name=case.name + ", second iteration", outs=case.outs2)


# ---- every case, for the host tests -------------------------------------------------------------------------------------------
def all_cases():
    """(id, zero-argument builder) of every stage case the device tests use"""
    cases = [("resblock " + n, functools.partial(resblock_case, n)) for n in RESBLOCK_CASES]
    cases += [("backbone %dx%d" % s[2:], functools.partial(backbone_case, s)) for s in BACKBONE_SHAPES]
    cases += [("tlayer %s %s shift %d" % (k, "x".join(map(str, gm)), s), functools.partial(tlayer_case, gm, k, s))
              for gm in TLAYER_GEOMS for k in TLAYER_KINDS for s in (False, True)]
    cases += [("transformer %dx%dx%d" % (s[0], s[2], s[3]), functools.partial(transformer_case, s, k)) for s, k in TRANSFORMER_CASES]
    cases += [("match %s bidir %d" % (k, b), functools.partial(match_case, k, b)) for k in MATCH_KINDS for b in (True, False)]
    cases += [("propagation r%d" % r, functools.partial(prop_case, r)) for r in (-1, 1)]
    cases += [("refine_proj", refine_state_case)]
    cases += [("update %s mask %d" % ("x".join(map(str, s)), m), functools.partial(update_case, s, m)) for s in UPDATE_SHAPES for m in (True, False)]
    cases += [("update 2x16x24 mask 1 convz1 x 0.5", functools.partial(update_case, UPDATE_SHAPES[0], True, 0.5))]
    return cases

"""The GMFlow stages of color-transfer_amd/unimatch/__init__.py, ONE stage at a time on the device, each fed the float32 input the
float64 oracle saw (tests/gmflow_stages_common.py: cases, gate, admission; tests/test_gmflow_stages_host.py: every case discriminates).
Each test prints, per output: achieved max error, the float32 oracle's own error (floor), the gate, and the rms ratio."""
# One MI355X run (130 tests, 4.5 s), worst case of each stage per convolution mode: max error / floor / gate / rms ratio (<= 2.0).
# Nothing asserted is taken from this table: the gates come from the float32 oracle and the formats (gmflow_stages_common.py).
#   stage / output                    split (both 3x3 forms)               exact
#   resblock layer1.0 12x20           1.4e-06 1.5e-06 1.4e-04  1.10        3.2e-06 1.5e-06 1.4e-04  1.85
#   resblock layer2.0 16x24 (s2d)     3.5e-06 1.6e-06 1.3e-04  1.77        4.5e-06 1.6e-06 1.3e-04  1.92
#   resblock layer2.0 17x23           3.4e-06 1.3e-06 1.4e-04  1.86        3.3e-06 1.3e-06 1.4e-04  1.95
#   backbone (both outputs)           2.8e-05 1.7e-05 2.5e-04  1.48        2.8e-05 1.7e-05 2.5e-04  1.76
#   tlayer self_attn                  2.2e-06 2.7e-06 2.3e-04  0.90        2.6e-06 2.7e-06 2.3e-04  1.06
#   tlayer cross_attn_ffn             5.3e-06 2.6e-06 2.2e-04  1.65        7.4e-06 2.6e-06 2.2e-04  1.93
#   transformer (six layers)          9.8e-06 7.6e-06 3.3e-04  1.37        1.1e-05 7.6e-06 3.3e-04  1.60
#   global match randn                1.3e-06 1.5e-06 1.3e-04  1.01        (no convolution or linear layer)
#   global match matched x1           3.5e-06 3.8e-06 2.0e-04  1.31
#   global match matched x3           0       0       2.0e-04  -           (one-hot: the float32 oracle is exact, g alone)
#   propagation global                7.7e-08 8.4e-08 2.0e-05  0.90        7.2e-08 8.4e-08 2.0e-05  0.89
#   propagation local r1              4.7e-07 6.9e-07 7.3e-05  0.78        5.1e-07 6.9e-07 7.3e-05  0.86
#   refine_proj net                   7.9e-07 1.1e-06 2.0e-05  0.90        1.1e-06 1.1e-06 2.0e-05  1.08
#   refine_proj inp                   1.9e-06 1.7e-06 1.3e-04  0.95        2.5e-06 1.7e-06 1.3e-04  1.33
#   update block net                  4.1e-06 1.3e-06 2.0e-05  2.76 [0.26] 3.3e-06 1.3e-06 2.0e-05  2.36 [0.23]
#   update block mask                 3.8e-06 1.6e-06 6.5e-05  2.59 [0.27] 3.6e-06 1.6e-06 6.5e-05  2.43 [0.27]
#   update block delta                2.3e-07 5.7e-07 2.0e-05  1.76 [0.14] 1.7e-07 5.7e-07 2.0e-05  1.64 [0.13]
# The update block is the one stage over 2.0 against the float32 oracle's rms error (in every mode, the bitwise fmaf chain of the
# exact mode included) while a factor 5 inside the maximum gate: the arithmetic of a 1920-term float32 chain, not a wrong stage.
# Its rms rule takes the larger of the oracle's rms error and the modelled one of such chains, evaluated on the case in float64
# (gmflow_stages_common.update_block_model); the ratio against that is the figure in brackets.
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import gmflow_stages_common as C   # noqa: E402


@pytest.fixture(scope="module")
def hip():
    import ct_hip
    ct_hip.lib()
    return ct_hip


@pytest.fixture(scope="module")
def model(hip):
    from unimatch import GMFlow
    names, shapes = C.state_spec()
    m = GMFlow()
    assert list(m.state_dict().keys()) == names and [tuple(v.shape) for v in m.state_dict().values()] == shapes
    m.load_state_dict(C.state(), strict=True)
    return m.cuda()


def dev(t):
    return t.cuda().contiguous()


# ---- bitwise stages -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,splits", C.POSITION_SHAPES)
def test_add_position_is_the_oracle_bit_for_bit(model, shape, splits):
    """the same float32 table (tests/test_gmflow_stages_host.py), one float32 add per element"""
    case = C.position_case(shape, splits)
    got = model._add_position(dev(case.f0), dev(case.f1), splits)
    for a, b in zip(got, case.want):
        assert a.dtype == torch.float32 and torch.equal(a.cpu(), b)


@pytest.mark.parametrize("shape", C.TOKEN_SHAPES)
def test_tokens_and_nchw_are_the_permutation(hip, shape):
    import unimatch
    b, c, h, w = shape
    x = torch.randn(shape, generator=C.gen(50 + h))
    t = unimatch._tokens(dev(x))
    assert tuple(t.shape) == (b, h * w, c) and t.is_contiguous() and torch.equal(t.cpu(), C.tokens(x))
    back = unimatch._nchw(t, h, w)
    assert tuple(back.shape) == shape and back.is_contiguous() and torch.equal(back.cpu(), x)
    tok = torch.randn(b, h * w, c, generator=C.gen(51 + h))                       # and from the token side
    n = unimatch._nchw(dev(tok), h, w)
    assert torch.equal(n.cpu(), C.nchw(tok, h, w)) and torch.equal(unimatch._tokens(n).cpu(), tok)
    assert torch.equal(hip.tokens_to_nchw(hip.nchw_to_tokens(dev(x)), h, w).cpu(), x)


# ---- backbone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.RESBLOCK_CASES))
def test_resblock(model, hip, name, conv_mode):
    case = C.resblock_case(name)
    layer, idx = case.prefix.split(".")[1:]
    blk = getattr(model.backbone, layer)[int(idx)]
    x = dev(case.x)
    if case.stride == 2:                             # the shared space-to-depth image: taken at 16 x 24 (split mode), refused at 17 x 23
        assert blk.downsample is not None and blk.stride == 2
        assert hip.s2d_ok(x) == (conv_mode == "split" and case.x.shape[2] % 2 == 0 and case.x.shape[3] % 8 == 0)
    else:
        assert blk.downsample is None
    C.hold(case, [model._resblock(blk, x)], conv_mode)


@pytest.mark.parametrize("shape", C.BACKBONE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backbone(model, hip, shape, conv_mode):
    case = C.backbone_case(shape)
    stem = torch.empty(shape[0], 64, shape[2] // 2, shape[3] // 2, device="cuda")
    assert hip.s2d_ok(stem) == (conv_mode == "split" and shape == C.BACKBONE_SHAPES[0])       # 32 x 48 taken, 20 x 36 refused
    C.hold(case, model._backbone(dev(case.x)), conv_mode)


# ---- transformer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("kind", C.TLAYER_KINDS)
@pytest.mark.parametrize("geom", C.TLAYER_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_tlayer(model, geom, kind, shift, conv_mode):
    h, w, splits, nb = geom
    case = C.tlayer_case(geom, kind, shift)
    layer = getattr(model.transformer.layers[1], kind)
    for p in (layer.q_proj.weight, layer.k_proj.weight):
        if hasattr(p, "_ct_lin_ws16_multi"):
            del p._ct_lin_ws16_multi
    source = dev(case.source)
    if kind == "self_attn":
        y = model._tlayer(layer, source, source, h, w, shift, splits)
        first = layer.q_proj.weight                  # the multi-projection packs q | k | v, cached on the first weight
    else:
        y = model._tlayer(layer, source, dev(case.target), h, w, shift, splits, kv_swap=True)
        first = layer.k_proj.weight                  # k | v of the target
    # which kernels ran: from 4096 tokens on the resident-weight family (multi-projection, LayerNorm epilogue, partial slabs)
    assert hasattr(first, "_ct_lin_ws16_multi") == (conv_mode == "split" and nb * h * w >= 4096), (nb * h * w, conv_mode)
    C.hold(case, [y], conv_mode)


@pytest.mark.parametrize("shape,splits", C.TRANSFORMER_CASES)
def test_transformer(model, shape, splits, conv_mode):
    import unimatch
    case = C.transformer_case(shape, splits)
    h, w = shape[2:]
    t0, t1 = model._transformer(unimatch._tokens(dev(case.f0)), unimatch._tokens(dev(case.f1)), h, w, splits)
    C.hold(case, [C.nchw(t0.cpu(), h, w), C.nchw(t1.cpu(), h, w)], conv_mode)


# ---- matching and propagation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidir", [True, False])
@pytest.mark.parametrize("kind", C.MATCH_KINDS)
def test_global_match(model, hip, kind, bidir):
    """attention over the coordinate table; no convolution or linear layer: the arithmetic does not depend on the convolution mode"""
    case = C.match_case(kind, bidir)
    h, w = case.f0.shape[2:]
    y = model._global_match(dev(C.tokens(case.f0)), dev(C.tokens(case.f1)), h, w, bidir)
    C.hold(case, [y], hip.conv_mode())


@pytest.mark.parametrize("radius", [-1, 1])
def test_propagation(model, radius, conv_mode):
    case = C.prop_case(radius)
    h, w = case.f0.shape[2:]
    C.hold(case, [model._propagate(dev(C.tokens(case.f0)), dev(case.flow), h, w, radius)], conv_mode)


# ---- refinement -------------------------------------------------------------------------------------------------------------------
def test_refine_state_splits_net_and_inp(model, hip, conv_mode):
    case = C.refine_state_case()
    h, w = case.f0.shape[2:]
    net, xbuf, pre = model._refine_state(dev(C.tokens(case.f0)), h, w)
    assert tuple(xbuf.shape) == (case.f0.shape[0], 256, h, w) and net.is_contiguous()
    assert (pre is not None) == (conv_mode == "split")
    C.hold(case, [net, xbuf[:, :128]], conv_mode)


def run_update(model, case, use_pre, iterations=1):
    """the loop of _unimatch around _refine_iter: one x buffer, one set of invariants, net and inp loop invariant.  The motion and
    flow channels of the buffer start at 1e3 (torch.empty in _refine_state): an iteration that does not write them shows.
    Returns (outputs per iteration, whether every iteration left net, inp and the flow channels as they have to be)"""
    net = dev(case.net)
    xbuf = torch.full((net.shape[0], 256) + tuple(net.shape[2:]), 1e3, dtype=torch.float32, device="cuda")
    xbuf[:, :128] = dev(case.inp)
    pre = model._gru_invariants(net, xbuf[:, :128]) if use_pre else None
    res, intact = [], True
    for corr, flow in ((case.corr, case.flow), (case.corr2, case.flow2))[:iterations]:
        h, mask, delta = model._refine_iter(net, xbuf, dev(corr), dev(flow), want_mask=case.want_mask, pre=pre)
        assert (mask is not None) == case.want_mask
        intact = intact and torch.equal(xbuf[:, 254:].cpu(), flow) and torch.equal(xbuf[:, :128].cpu(), case.inp) and torch.equal(net.cpu(), case.net)
        res.append([t.clone() for t in (h, mask, delta) if t is not None])
    return res, intact


@pytest.mark.parametrize("want_mask", [True, False])
@pytest.mark.parametrize("shape", C.UPDATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_refine_iter(model, hip, shape, want_mask, conv_mode):
    """the path _unimatch takes for this mode and width: split mode and w % 4 == 0 -> the invariant blocks convolved once, the GRU's
    elementwise steps in the convolution epilogues; otherwise (exact mode; w = 6) the reference's form.  Two consecutive iterations."""
    case = C.update_case(shape, want_mask)
    use_pre = conv_mode == "split" and shape[2] % 4 == 0
    assert hip.conv_ws16()
    (first, second), intact = run_update(model, case, use_pre, iterations=2)
    C.hold(case, first, conv_mode)
    C.hold(C.second_iteration(case), second, conv_mode)
    assert intact


@pytest.mark.parametrize("want_mask", [True, False])
def test_refine_iter_without_fused_post_ops(model, hip, want_mask):
    """split mode with the bf16 form of the tile kernel: r * h and the gate are separate elementwise launches"""
    case = C.update_case(C.UPDATE_SHAPES[0], want_mask)
    hip.set_conv_ws16(False)
    try:
        assert hip.conv_mode() == "split" and not hip.conv_ws16()
        (first, second), intact = run_update(model, case, True, iterations=2)
    finally:
        hip.set_conv_ws16(True)
    C.hold(case, first, "split")
    C.hold(C.second_iteration(case), second, "split")
    assert intact


def test_refine_iter_follows_an_in_place_weight_update(model, hip, conv_mode):
    """_gru_packed is keyed by the parameters' versions: after convz1.weight.mul_(0.5) the split weights are cut and packed again"""
    shape = C.UPDATE_SHAPES[0]
    use_pre = conv_mode == "split"
    before = C.update_case(shape, True)
    C.hold(before, run_update(model, before, use_pre)[0][0], conv_mode)          # packs the current weights
    w = model.refine.gru.convz1.weight
    with torch.no_grad():
        w.mul_(0.5)
    try:
        after = C.update_case(shape, True, 0.5)
        C.hold(after, run_update(model, after, use_pre)[0][0], conv_mode)
    finally:
        with torch.no_grad():
            w.mul_(2.0)                                                          # exact: a power of two
    assert torch.equal(w.cpu(), C.state()["refine.gru.convz1.weight"])
    C.hold(before, run_update(model, before, use_pre)[0][0], conv_mode)

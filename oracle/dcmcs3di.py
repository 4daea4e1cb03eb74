"""DCMCS3DI forward, CPU oracle: a functional float64 restatement of the reference's
methods/dcmcs3di.py:53-66, pasmnet/backbone.py:14-15, pasmnet/attention.py:33-48,
pasmnet/utils.py:28-40,123-125 that works from a plain state_dict (no module classes).
TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

`forward` evaluates a whole image pair; `forward_band` evaluates a band of output rows of a pair that is too large
for `forward` (1920 x 1080: one [H,W,W] float64 attention map would be 32 GB) from the same stages."""
import torch
import torch.nn.functional as F

# Rows of context a row of `pre_clamp` depends on.  The network is convolutional down the rows (every 3x3 convolution
# reaches one row up and one down) and attends along a row only:
#   after the attention: transfer[0] is 1x1, then transfer_layers ResBs (2 rows each) and two 3x3 convolutions
#   before it:           extraction[0] (1 row), extraction_layers ResBs, the matcher head (one ResB); query / key / value are 1x1


def attention_margin(transfer_layers=6):
    """output rows [y0, y1) read the attention's results on rows [y0 - m, y1 + m)"""
    return 2 * transfer_layers + 2


def band_margin(extraction_layers=18, transfer_layers=6):
    """output rows [y0, y1) read input rows [y0 - m, y1 + m): 53 at full depth"""
    return 1 + 2 * extraction_layers + 2 + attention_margin(transfer_layers)


def _conv(sd, name, x, pad):
    return F.conv2d(x, sd[name + ".weight"].double(), sd[name + ".bias"].double(), padding=pad)


def _resb(sd, name, x):
    t = F.leaky_relu(_conv(sd, name + ".body.0", x, 1), 0.01)
    return x + _conv(sd, name + ".body.2", t, 1)


def _warp(img, att):
    return torch.matmul(att, img.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


def extraction_stage(sd, x, extraction_layers=18):
    """features of one view (dcmcs3di.py:54-55)"""
    x = _conv(sd, "extraction.0", x, 1)
    for i in range(1, extraction_layers + 1):
        x = _resb(sd, "extraction.%d" % i, x)
    return x


def head_stage(sd, fea):
    """the matcher's shared residual block (attention.py:35-36)"""
    return _resb(sd, "matcher.head", fea)


def attention_stage(sd, fea_right, hl, hr, right, rows=None):
    """Parallax attention of the rows `rows` (a slice; default: all) of head features hl / hr: costs, softmaxes, column sums,
    valid mask of the left view, warped value features and warped right image.  Every tensor of the result holds those rows only."""
    if rows is not None:
        fea_right, hl, hr, right = (t[:, :, rows] for t in (fea_right, hl, hr, right))
    c = hl.shape[1]
    # cost_right2left = Q(left) K(right) / c ; cost_left2right = Q(right) K(left) / c
    Q = _conv(sd, "matcher.query", hl, 0).permute(0, 2, 3, 1)
    K = _conv(sd, "matcher.key", hr, 0).permute(0, 2, 1, 3)
    cost_r2l = torch.matmul(Q, K) / c
    Q = _conv(sd, "matcher.query", hr, 0).permute(0, 2, 3, 1)
    K = _conv(sd, "matcher.key", hl, 0).permute(0, 2, 1, 3)
    cost_l2r = torch.matmul(Q, K) / c
    att_r2l = F.softmax(cost_r2l, dim=-1)
    att_l2r = F.softmax(cost_l2r, dim=-1)
    colsum = att_l2r.sum(dim=-2)
    valid_left = (colsum > 0.1).unsqueeze(1)
    fea_warped = _warp(_conv(sd, "matcher.value", fea_right, 0), att_r2l)
    return dict(cost_r2l=cost_r2l, cost_l2r=cost_l2r, att_r2l=att_r2l, att_l2r=att_l2r, colsum=colsum, valid_left=valid_left,
                fea_warped=fea_warped, warped_rgb=_warp(right, att_r2l))


def transfer_stage(sd, fea_left, fea_warped, valid, transfer_layers=6):
    """the colour-transfer branch (dcmcs3di.py:59,47-51) up to the pre-clamp output"""
    x = torch.cat([fea_left, fea_warped, valid.double()], dim=1)
    x = _conv(sd, "transfer.0", x, 0)
    for i in range(1, transfer_layers + 1):
        x = _resb(sd, "transfer.%d" % i, x)
    x = _conv(sd, "transfer.%d" % (transfer_layers + 1), x, 1)
    return _conv(sd, "transfer.%d" % (transfer_layers + 2), x, 1)


def forward(sd, left, right, extraction_layers=18, transfer_layers=6, valid_override=None):
    """Returns a dict with the same intermediates the goldens hold. sd: name -> tensor.
    valid_override: a boolean [B,1,H,W] mask used in place of `colsum > 0.1` (the threshold is discontinuous: a test that
    wants to compare the arithmetic behind it feeds both sides the same mask); adds `pre_clamp_override` to the result."""
    left, right = left.double(), right.double()
    fea_left, fea_right = extraction_stage(sd, left, extraction_layers), extraction_stage(sd, right, extraction_layers)
    att = attention_stage(sd, fea_right, head_stage(sd, fea_left), head_stage(sd, fea_right), right)
    pre = transfer_stage(sd, fea_left, att["fea_warped"], att["valid_left"], transfer_layers)
    extra = {} if valid_override is None else \
        {"pre_clamp_override": transfer_stage(sd, fea_left, att["fea_warped"], valid_override, transfer_layers)}
    return dict(extra, fea_left=fea_left, fea_right=fea_right, pre_clamp=pre, corrected=pre.clamp(0, 1), **att)


def band_transfer(sd, state, valid_override, transfer_layers=6):
    """`pre_clamp_override` of a band from the state `forward_band(..., return_state=True)` returned: the transfer branch alone,
    under valid_override (boolean [B,1,H,W], whole image) -- no extraction, no attention.  Rows y0..y1 only."""
    a0, a1, y0, y1 = state["a0"], state["a1"], state["y0"], state["y1"]
    pre = transfer_stage(sd, state["fea_left"], state["fea_warped"], valid_override[:, :, a0:a1], transfer_layers)
    return pre[:, :, y0 - a0:y1 - a0]


def forward_band(sd, left, right, y0, y1, extraction_layers=18, transfer_layers=6, valid_override=None, keep_maps=True,
                 return_state=False):
    """Rows [y0, y1) of what `forward` returns, from a crop of the input rows they depend on: rows [y0 - 53, y1 + 53) (full
    depth; band_margin) through extraction and the matcher head, costs and softmaxes only for rows [y0 - 14, y1 + 14)
    (attention_margin), the transfer branch on those.  Where a crop ends at the image's edge the zero padding is the real one;
    where it is an artificial cut, the margin keeps the wrong padding out of the rows returned.
    Same keys as `forward`, every tensor holding rows y0..y1 of the full width; `pre_clamp_override` when valid_override (boolean
    [B,1,H,W], whole image) is given.  keep_maps=False leaves the four [B,rows,W,W] maps out.  return_state=True returns
    (result, state) with `state` what band_transfer needs to re-run the transfer branch under another mask."""
    left, right = left.double(), right.double()
    H = left.shape[2]
    if not 0 <= y0 < y1 <= H:
        raise ValueError("band rows [%d, %d) outside the image's %d rows" % (y0, y1, H))
    m_att, m_all = attention_margin(transfer_layers), band_margin(extraction_layers, transfer_layers)
    c0, c1 = max(0, y0 - m_all), min(H, y1 + m_all)          # crop rows
    a0, a1 = max(0, y0 - m_att), min(H, y1 + m_att)          # attention rows
    left_c, right_c = left[:, :, c0:c1], right[:, :, c0:c1]
    fea_left, fea_right = extraction_stage(sd, left_c, extraction_layers), extraction_stage(sd, right_c, extraction_layers)
    rows = slice(a0 - c0, a1 - c0)
    att = attention_stage(sd, fea_right, head_stage(sd, fea_left), head_stage(sd, fea_right), right_c, rows=rows)
    state = dict(a0=a0, a1=a1, y0=y0, y1=y1, fea_left=fea_left[:, :, rows].contiguous(), fea_warped=att["fea_warped"])
    pre = transfer_stage(sd, state["fea_left"], att["fea_warped"], att["valid_left"], transfer_layers)
    band_c, band_a = slice(y0 - c0, y1 - c0), slice(y0 - a0, y1 - a0)
    out = dict(fea_left=fea_left[:, :, band_c].contiguous(), fea_right=fea_right[:, :, band_c].contiguous())
    for k in ("cost_r2l", "cost_l2r", "att_r2l", "att_l2r", "colsum"):             # [B, rows, ...]
        if keep_maps or k == "colsum":
            out[k] = att[k][:, band_a].clone()
    for k in ("valid_left", "fea_warped", "warped_rgb"):                            # [B, C, rows, W]
        out[k] = att[k][:, :, band_a].clone()
    out["pre_clamp"] = pre[:, :, band_a].clone()
    out["corrected"] = out["pre_clamp"].clamp(0, 1)
    if valid_override is not None:
        out["pre_clamp_override"] = band_transfer(sd, state, valid_override, transfer_layers).clone()
    return (out, state) if return_state else out

#!/usr/bin/env python
"""The convolution dispatch of ct_hip.conv (_conv_entry, and the way conv2d / gconv2d / conv2d_rows call it) against a verbatim
copy of the decision logic it replaced (the single-file binding: _split_ok, _ws16_ok, the branches of _conv_split and of the three
front doors with every launch replaced by the name of its entry).  No GPU, no library: tensors are descriptors with a shape, an
address and a batch stride.  Every cell of

    (kh, kw) x cin x W % 4 x which tensor is an unaligned view x x2 x res_pre x post-op x conv_mode x ws16 x wino x H W vs 2^32 bytes

must choose the same entry in both; prints the cell count.     usage: python tools/check_conv_dispatch.py"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "color-transfer_amd")]
import torch  # noqa: E402
import ct_hip  # noqa: E402
from ct_hip import conv  # noqa: E402
from ct_hip.packing import SplitOperands  # noqa: E402


class T:
    """what the decisions read of a tensor: dense NCHW float32 on the device, at `ptr`"""
    is_cuda, dtype = True, torch.float32

    def __init__(self, n, c, h, w, ptr=1 << 20):
        self.shape, self.ptr = (n, c, h, w), ptr

    def data_ptr(self):
        return self.ptr

    def stride(self, i):
        n, c, h, w = self.shape
        return (c * h * w, h * w, w, 1)[i]

    def __getitem__(self, i):
        return self

    def is_contiguous(self):
        return True


def cat(*ts):                                       # torch.cat(ts, 1): a fresh, aligned tensor
    return T(ts[0].shape[0], sum(t.shape[1] for t in ts), ts[0].shape[2], ts[0].shape[3])


# ---- the replaced logic, verbatim but for the launches ------------------------------------------------------------
def old_ws16_ok(x, split, kh, kw):
    return ct_hip.conv_ws16() and (kh, kw) == (3, 3) and 32 < x.shape[1] <= 64 and len(split) > 2 and split[2] is not None


def old_split_ok(x, out, residual, kh, kw, stride, ph, pw):
    if ct_hip.conv_mode() != "split" or stride != 1 or (kh, kw) not in ((3, 3), (1, 1), (1, 5), (5, 1)) or (ph, pw) != (kh // 2, kw // 2):
        return False
    if x.shape[3] % 4:
        return False
    for t in (x, out, residual):
        if t is not None and (t.data_ptr() % 16 or t.stride(0) % 4):
            return False
    return True


def old_conv_split(x, split, kh, kw, x2=None, res_pre=False, post=None):
    f16 = 0
    if ct_hip.conv_ws16() and len(split) > 2 and split[2] is not None:
        f16 = 1
    n, cin1, h, w = x.shape
    post_op, p1, p2 = (0, None, None) if post is None else post
    if post_op and not f16:
        return "error: post-op"
    if x2 is None and not res_pre and not post_op and old_ws16_ok(x, split, kh, kw):
        if ct_hip.conv_wino() and len(split) > 3 and split[3] is not None and h * w * 256 < (1 << 32):
            return "wino16"
        return "ws16"
    return "split"


def old_conv2d(x, split, cout, ksize, residual, out, x2, x3=None):
    if x2 is not None:
        c1, c2 = x.shape[1], x.shape[1] + x2.shape[1]
        ok = (split is not None and c1 % 16 == 0 and (x3 is None or c2 % 16 == 0) and
              all(t is None or (t.is_cuda and t.dtype == torch.float32 and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and
                                t[0].is_contiguous()) for t in (x2, x3)))
        if ok and old_split_ok(x, out, residual, ksize, ksize, 1, ksize // 2, ksize // 2):
            return old_conv_split(x, split, ksize, ksize, x2=x2)
        x = cat(*[t for t in (x, x2, x3) if t is not None])
        pre = "cat+"
    else:
        pre = ""
    if split is not None and old_split_ok(x, out, residual, ksize, ksize, 1, ksize // 2, ksize // 2):
        return pre + old_conv_split(x, split, ksize, ksize)
    return pre + "exact"


def old_conv2d_rows(x, split, ksize):
    if split is None or not x.is_cuda or x.dtype != torch.float32 or not old_split_ok(x, None, None, ksize, ksize, 1, ksize // 2, ksize // 2):
        return "none"
    return "rows"


def old_gconv2d(x, split, bias, cout, kh, kw, out, x2, residual, addend, post):
    stride, ph, pw = 1, kh // 2, kw // 2
    if addend is not None:
        n, c1, h, w = x.shape
        ok = (split is not None and bias is not None and
              old_split_ok(x, out, addend, kh, kw, stride, ph, pw) and
              (x2 is None or (c1 % 16 == 0 and x2.data_ptr() % 16 == 0 and x2.stride(0) % 4 == 0)))
        if not ok:
            return "error: addend"
        if post is not None and not ct_hip.conv_ws16():
            return "error: post-op operands"
        return old_conv_split(x, split, kh, kw, x2=x2, res_pre=True, post=post)
    pre = ""
    if x2 is not None:
        n, c1, h, w = x.shape
        if (split is not None and bias is not None and c1 % 16 == 0 and x2.data_ptr() % 16 == 0 and x2.stride(0) % 4 == 0 and
                old_split_ok(x, out if out is not None else x, None, kh, kw, stride, ph, pw)):
            return old_conv_split(x, split, kh, kw, x2=x2)
        x = cat(x, x2)
        pre = "cat+"
    if split is not None and bias is not None and (cout > 4 or residual is not None) and old_split_ok(x, out, residual, kh, kw, stride, ph, pw):
        return pre + old_conv_split(x, split, kh, kw)
    return pre + "gconv"


# ---- the same questions put to the dispatch, the way the front doors put them ------------------------------------
def new_conv2d(x, ops, cout, ksize, residual, out, x2, x3=None):
    pre = ""
    if x2 is not None:
        entry = conv._conv_entry(x, out, residual, ksize, ksize, ops, x2=x2, x3=x3)
        if entry != "exact":
            return entry
        x, pre = cat(*[t for t in (x, x2, x3) if t is not None]), "cat+"
    return pre + conv._conv_entry(x, out, residual, ksize, ksize, ops)


def new_conv2d_rows(x, ops, ksize):
    return "rows" if conv._conv_entry(x, None, None, ksize, ksize, ops, rows=True) == "rows" else "none"


def new_gconv2d(x, ops, bias, cout, kh, kw, out, x2, residual, addend, post):
    ops = ops if bias is not None else None
    pad = (kh // 2, kw // 2)
    if addend is not None:
        entry = conv._conv_entry(x, out, addend, kh, kw, ops, x2=x2, res_pre=True, post=post, stride=1, padding=pad)
        if entry == "exact":
            return "error: addend"
        if post is not None and not ct_hip.conv_ws16():
            return "error: post-op operands"
        return entry
    pre = ""
    if x2 is not None:
        entry = conv._conv_entry(x, out if out is not None else x, None, kh, kw, ops, x2=x2, stride=1, padding=pad)
        if entry != "exact":
            return entry
        x, pre = cat(x, x2), "cat+"
    entry = conv._conv_entry(x, out, residual, kh, kw, ops if (cout > 4 or residual is not None) else None, stride=1, padding=pad)
    return pre + ("gconv" if entry == "exact" else entry)


def operands(cin, kh, kw):
    """which images a packed weight of this shape carries (ct_hip.packing._split_operands), as placeholders"""
    if kh * kw > 9:
        return None                                 # pack_gconv_weight attaches none to a 7x7
    f16 = ("f16", 0) if (kh, kw) in ((3, 3), (1, 1), (1, 5), (5, 1), (2, 2)) else None
    wino = ("wino", 0) if (kh, kw) == (3, 3) and 32 < cin <= 64 else None
    return SplitOperands("bf16", "bias", f16, wino)


def main():
    cells = mismatches = 0
    for mode, ws16, wino in itertools.product(("split", "exact"), (True, False), (True, False)):
        ct_hip.set_conv_mode(mode)
        ct_hip.set_conv_ws16(ws16)
        ct_hip.set_conv_wino(wino)
        for (kh, kw), cin, wmod, skew, with_x2, res_pre, post_on, big in itertools.product(
                ((1, 1), (3, 3), (1, 5), (5, 1), (7, 7)), (3, 16, 32, 33, 64, 128, 129), (0, 2), (None, "x", "out", "residual", "x2"),
                (False, True), (False, True), (False, True), (False, True)):
            cells += 1
            h = 4096 if big else 8
            w = (4096 if big else 32) + wmod        # big: H W 256 >= 2^32
            ptr = {k: (1 << 20) + (4 if skew == k else 0) for k in ("x", "out", "residual", "x2")}      # a view that starts one float in
            cout = 64
            x = T(1, cin, h, w, ptr["x"])
            x2 = T(1, 16, h, w, ptr["x2"]) if with_x2 else None
            out = T(1, cout, h, w, ptr["out"])
            res = T(1, cout, h, w, ptr["residual"])
            post = (1, "p1", None) if post_on else None
            ops = operands(cin + (16 if with_x2 else 0), kh, kw)
            old_ops = None if ops is None else tuple(ops)
            # the dispatch itself against the chain _split_ok -> x2 test -> _conv_split it stands for
            if (old_ops is not None and old_split_ok(x, out, res, kh, kw, 1, kh // 2, kw // 2) and
                    (x2 is None or (cin % 16 == 0 and x2.data_ptr() % 16 == 0 and x2.stride(0) % 4 == 0))):
                want = old_conv_split(x, old_ops, kh, kw, x2=x2, res_pre=res_pre, post=post)
                want = "split" if want == "error: post-op" else want            # the launcher raises that, after the choice
            else:
                want = "exact"
            got = [conv._conv_entry(x, out, res, kh, kw, ops, x2=x2, res_pre=res_pre, post=post)]
            want = [want]
            # the front doors (res_pre / post exist in gconv2d only; conv2d and conv2d_rows take square kernels)
            want.append(old_gconv2d(x, old_ops, "b", cout, kh, kw, out, x2, None, res if res_pre else None, post if res_pre else None))
            got.append(new_gconv2d(x, ops, "b", cout, kh, kw, out, x2, None, res if res_pre else None, post if res_pre else None))
            if not with_x2:
                want.append(old_gconv2d(x, old_ops, "b", 2 if post_on else cout, kh, kw, out, None, res if res_pre else None, None, None))
                got.append(new_gconv2d(x, ops, "b", 2 if post_on else cout, kh, kw, out, None, res if res_pre else None, None, None))
            if kh == kw:
                want.append(old_conv2d(x, old_ops, cout, kh, res if res_pre else None, out, x2))
                got.append(new_conv2d(x, ops, cout, kh, res if res_pre else None, out, x2))
                want.append(old_conv2d_rows(x, old_ops, kh))
                got.append(new_conv2d_rows(x, ops, kh))
            if got != want:
                mismatches += 1
                print("MISMATCH", dict(mode=mode, ws16=ws16, wino=wino, k=(kh, kw), cin=cin, w=w, h=h, skew=skew, x2=with_x2, res_pre=res_pre,
                                       post=post_on), "old", want, "new", got)
    ct_hip.set_conv_mode("split")
    ct_hip.set_conv_ws16(True)
    ct_hip.set_conv_wino(True)
    print("%d cells, %d mismatches" % (cells, mismatches))
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())

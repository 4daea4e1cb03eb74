"""Restatement of regress_disp's contract (pasmnet/utils.py:55-105) for the disparity tests, written as per-row scans.

  disp_ini[i] = i - sum_j att[i][j] j                      (float64 here)
  fill: valid pixels keep disp_ini; an invalid pixel k steps right of the last valid pixel p of its row holds disp_ini[p]
        divided k times by D = float32(1 + 1e-4); a pixel left of the row's first valid pixel f holds disp_ini[f] divided
        (f - x) times; a row without a valid pixel is 0.

`fill(..., np.float32)` divides in float32, one correctly rounded division per step in the reference's order, so it is the
bitwise contract; `fill(..., np.float64)` is the float64 restatement (same D).  The golden (tests/golden/disparity.npz, from
the reference itself) pins both.  Each step is applied to all rows at once: pixels are grouped by their distance to their
source pixel and step t reads the results of step t - 1.
"""
import numpy as np

D32 = np.float32(1) + np.float32(1e-4)


def expected_index(att):
    """float64 i - sum_j att[..., i, j] j over the last axis"""
    att = np.asarray(att, dtype=np.float64)
    w = att.shape[-1]
    j = np.arange(w, dtype=np.float64)
    return j - att @ j


def onehot_index(cols):
    """disp_ini of a one-hot attention stored as its column indices [rows, W]: exact integers"""
    cols = np.asarray(cols, dtype=np.int64)
    return (np.arange(cols.shape[-1])[None, :] - cols).astype(np.float64)


def fill(disp_ini, valid, dtype=np.float32):
    """the occlusion fill on [..., W] rows; valid: bool / 0-1 of the same shape; result in `dtype`"""
    shape = np.shape(disp_ini)
    w = shape[-1]
    x = np.asarray(disp_ini, dtype=dtype).reshape(-1, w)
    v = (np.asarray(valid).reshape(-1, w) > 0.5)
    d = dtype(D32)
    out = np.where(v, x, dtype(0)).astype(dtype)
    idx = np.arange(w)[None, :]
    last = np.maximum.accumulate(np.where(v, idx, -1), axis=1)          # last valid pixel at or left of x
    anyv = v.any(axis=1)
    first = np.where(anyv, v.argmax(axis=1), w)[:, None]                # first valid pixel of the row
    k_left = np.where(~v & (last >= 0), idx - last, 0)                  # steps from the source, first loop
    k_right = np.where(~v & (idx < first) & anyv[:, None], first - idx, 0)   # steps from the source, second loop
    for k, step in ((k_left, -1), (k_right, 1)):
        r, c = np.nonzero(k)
        if r.size == 0:
            continue
        t = k[r, c]
        order = np.argsort(t, kind="stable")
        r, c, t = r[order], c[order], t[order]
        bounds = np.searchsorted(t, np.arange(1, t[-1] + 2))
        for s in range(t[-1]):
            rs, cs = r[bounds[s]:bounds[s + 1]], c[bounds[s]:bounds[s + 1]]
            out[rs, cs] = out[rs, cs + step] / d
    return out.reshape(shape)


def regress_disp(att, valid, dtype=np.float32):
    """the whole contract on an att [..., W, W] and a mask [..., W] (float64 index, fill in dtype)"""
    return fill(expected_index(att), valid, dtype)

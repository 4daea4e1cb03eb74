"""Drop-in for the reference's pasmnet/utils.py:55-105 `regress_disp` (the disparity of a matching attention map), on the GPU.

`regress_disp(att, valid_mask)`: same signature and shapes as the reference -- att [B,H,W,W] (att_right2left), valid_mask
[B,1,H,W] (bool or 0/1 float) -> disparity [B,1,H,W] float32.  One HBM-bound pass over att plus a per-row occlusion fill
(csrc/disparity.hip, ct_pam_regress_disp_f32); the fill is bitwise the reference's two partial-convolution loops given the
same unfilled disparity.  There is no CPU path: CPU tensors raise ct_hip.CtHipError.  Without a materialised attention map,
DCMCS3DI.disparity gives the same quantity from the streaming attention at any width.
"""
import ct_hip


def regress_disp(att, valid_mask):
    return ct_hip.regress_disp(att, valid_mask)

"""ctypes binding of libct_hip.so (C ABI: include/ct_hip.h) + thin torch-tensor helpers.

PyTorch is used here only as the device allocator / stream provider: every function
takes CUDA (= HIP on ROCm) tensors, passes raw device pointers and the current HIP stream
to the library and returns without synchronising.

There is NO CPU fallback: importing works anywhere (so that `-m "not gpu"` tests can
check the exported symbols), but the first compute call without the library or without a
GPU raises.

One module per kernel family; `_core` loads the library and holds what they share.  Every module registers its entries in
`_core.SIGNATURES` on import, and all of them are imported here, before anything can call lib().  This file only re-exports:
the public surface, and the few private names that tests and tools reach for.
"""
from ._core import (ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SWISH, ACT_TANH, CT_ABI_VERSION,
                    CT_LAB_STATS_STRIDE, CT_RGB_STATS_STRIDE, CT_WS_IDT, CT_WS_LAB_STATS, CT_WS_MK_U8, CT_WS_REINHARD, CT_WS_REINHARD_PERSIST,
                    CT_WS_REINHARD_PSNR, CT_WS_RGB_MEANCOV, CtHipError, LIB_PATH, SIGNATURES, check, device_status, lib,
                    workspace, _stream)
from .linear import (CT_LAB_EXACT, CT_LAB_TABLE, CT_PIPE_T_NT, CT_PIPE_T_PLAIN, affine3x3, lab_mode, lab_stats, mk, mk_coef,
                     profile_events, reinhard, reinhard_apply, reinhard_persist, reinhard_persist_supported, reinhard_pipeline,
                     reinhard_pipeline_chunk, reinhard_psnr, reinhard_takes_persist, rgb_meancov, set_lab_mode,
                     set_reinhard_pipeline, upload_records)
from .metrics import (CT_WS_FSIM, DISTORTIONS, ICID_INTENTS, icid_intent, distort_u8, fft2d_, frame_fsim, frame_fsim_hwc, frame_icid, frame_icid_hwc, frame_psnr, frame_ssim,
                      frame_ssim_hwc, regrain,
                      _fsim_stages, _fsim_tables)
from .idt import IdtDebug, idt, idt_u8
from .grading import acg_u8, regrain_u8
from .resize_pack import CT_PACK_CHW, CT_PACK_HWC, PACK_LAYOUTS, bicubic_resize, bilinear_resize, pack_u8, resize_geometry
from .packing import (ConvSource, SplitOperands, pack_conv_weight, pack_conv_weight_split, pack_conv_weight_split16,
                      pack_conv_weight_wino16, pack_gconv_weight, pack_linear_weight_split, pack_linear_weight_ws16)
from .gmflow import (convex_upsample, eltwise, fb_check, flow_warp, instance_norm, local_attn_prop, local_corr_flow,
                     local_corr_softmax)
from .conv import (conv2d, conv2d_rows, conv_mode, conv_scratch_prepare, conv_stream_k_state, conv_wino, conv_ws16, gconv2d,
                   s2d_ok, set_conv_mode, set_conv_stream_k, set_conv_wino, set_conv_wino_form, set_conv_ws16, space_to_depth2,
                   _conv_scratch, _conv_split, _sk_cache)
from .linears import layernorm128, linear_layernorm128, linear_tokens, linear_tokens_multi, set_linear_ws16
from .attention import (attention_tokens, nchw_to_rows, nchw_to_tokens, pam_attend, pam_streaming, pam_streaming_rows, pam_valid,
                        pam_valid_rows, tokens_to_nchw)
from .unet import dwconv, gconv2d_pad, scale_planes_, se_gate, upsample2_concat
from .disparity import attention_rows64_index, pam_disp_fill, regress_disp
from .views import (CT_VIEW_ABMSE, CT_VIEW_GRAY, CT_VIEW_LABMSE, CT_VIEW_RGBMSE, abmse_view, chess_mix, flow_to_image, gray_view, labmse_view,
                    rgbmse_view, rgbssim_view)
from .png import INFLATE_STATUS, PNG_MAX_WIDTH, PNG_ROWS_PER_CHUNK, inflate, png_decode, png_deflate, png_geometry
from .augment import AUGMENT_KINDS, AUGMENT_MAX_OPS, AUGMENT_SAMPLE, augment_table, augment_u8, frame_losses
from .pam_losses import PAM_SWEEP_MAX_W, masked_l1_sums, pam_cycle_l1, pam_map_sweep
from .warp import CT_WARP_AUTO, CT_WARP_GLOBAL, CT_WARP_STAGED, WARP_MAX_SIDE, WARP_PATHS, invert3x3, warp_maps, warp_perspective
from .yuv import YUV_MATRICES, YUV_RANGES, YUV_SITINGS, rgb_to_yuv420, yuv420_frame_bytes, yuv420_to_rgb
from . import _core


def __getattr__(name):
    # `_lib` is rebound by the first lib() call: forward the live value (a by-value import would stay None).  The other rebound
    # module globals (the convolution / linear switches) are read through their accessors: conv_mode(), conv_ws16(), ...
    if name == "_lib":
        return _core._lib
    raise AttributeError("module %r has no attribute %r" % (__name__, name))

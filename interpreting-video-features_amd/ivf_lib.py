"""ctypes binding of libivf_hip.so (include/ivf_hip.h).

The HIP library IS the product: if it is missing or a call fails this module
raises -- there is no CPU or PyTorch fallback anywhere in the package.
PyTorch is used only for device memory and streams.
"""
import collections
import ctypes
import os
from ctypes import (POINTER, Structure, byref, c_char, c_char_p, c_float, c_int,
                    c_size_t, c_void_p)

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libivf_hip.so")


class IvfError(RuntimeError):
    pass


MATH_FP32, MATH_BF16X3, MATH_BF16X6, MATH_BF16ACT = 0, 1, 2, 3
CONV_AUTO, CONV_IGEMM_BASE, CONV_PIX4, CONV_HALO_BASE = 0, 1, 15, 16      # IVF_CONV_* (kernel variant ids)
# IVF_CAM_* (kind ids of the Grad-CAM family, csrc/cam_ops.hip) and the chunk of its per-channel passes
CAM_KINDS = {"gradcam": 0, "gradcam++": 1, "xgradcam": 2, "hirescam": 3, "layercam": 4}
CAM_CHUNK = 128
MATH_MODES = {"fp32": MATH_FP32, "bf16x3": MATH_BF16X3, "bf16x6": MATH_BF16X6, "bf16act": MATH_BF16ACT}


class ConvDesc(Structure):
    _fields_ = [(n, c_int) for n in (
        "B", "Ti", "Hi", "Wi", "Cin", "in_ld", "in_coff", "To", "Ho", "Wo", "Cout", "out_ld",
        "out_coff", "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "relu", "accumulate",
        "mask_ld", "mask_coff", "d2s", "dT", "dH", "dW", "dC", "bsT", "bsH", "bsW", "math", "variant",
        "K0", "in2_ld", "in2_coff")] + [("in2", c_void_p)] + [(n, c_int) for n in ("N0", "out2_ld", "out2_coff")] + \
        [("out2", c_void_p), ("gate_out", c_void_p), ("gate_out2", c_void_p), ("gate_in", c_void_p)] + \
        [(n, c_int) for n in ("gate_out_ld", "gate_out_coff", "gate_out2_ld", "gate_in_ld", "gate_in_coff")]


class BwdGeom(Structure):
    _fields_ = [(n, c_int) for n in ("d2s", "kT", "kH", "kW", "pT", "pH", "pW", "rows")]


class PoolDesc(Structure):
    _fields_ = [(n, c_int) for n in (
        "B", "Ti", "Hi", "Wi", "C", "in_ld", "in_coff", "To", "Ho", "Wo", "out_ld", "out_coff",
        "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "gate_nonpos", "act_bf16")]


class I3DConfig(Structure):
    _fields_ = [(n, c_int) for n in (
        "B", "C", "T", "H", "W", "num_classes", "stem_stride_t", "pool4a_stride_t",
        "pool5a_stride_t", "head_kt", "head_kh", "head_kw", "softmax", "math")]


class TFCLSTMConfig(Structure):
    _fields_ = [(n, c_int) for n in ("B", "C", "T", "H", "W", "layers")] + [("units", c_int * 8)] + \
        [(n, c_int) for n in ("kh", "kw", "stride", "padding", "recurrent_hard_sigmoid", "only_last", "num_classes")]


class CLSTMConfig(Structure):
    _fields_ = [(n, c_int) for n in (
        "B", "C", "T", "H", "W", "hidden", "layers", "kernel", "stride", "num_classes",
        "softmax", "batch_norm", "out_step", "n_out_steps")] + [("out_steps", c_int * 16)]


_P = c_void_p
_I = c_int
_F = c_float
_U = ctypes.c_uint

_SIGS = {
    "ivf_version": (c_int, []),
    "ivf_freeze_fwd": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_freeze_bwd_workspace_bytes": (c_size_t, [_I, _I]),
    "ivf_freeze_bwd": (c_int, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "ivf_submask_pairs": (c_int, [_P, _I, _F, _P, _P, _P, _P]),
    "ivf_reverse_fwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_submask_pairs_batched": (c_int, [_P, _I, _I, _F, _P, _P, _P]),
    "ivf_reverse_fwd_batched": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_reverse_bwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "ivf_tv_norm": (c_int, [_P, _I, _I, _F, _F, _P, _P, _P]),
    "ivf_mask_reg": (c_int, [_P, _I, _I, _F, _F, _P, _P, _P, _P]),
    "ivf_adam_step": (c_int, [_P, _P, _P, _P, _I, _I, _F, _F, _F, _F, _P]),
    "ivf_search_step": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P]),
    "ivf_sigmoid": (c_int, [_P, _P, _I, _P]),
    "ivf_rank_frames": (c_int, [_P, _I, _I, _P, _P]),
    "ivf_init_central_select": (c_int, [_P, _P, _P, _I, _I, _I, c_float, _P, _P, _P, _P]),
    "ivf_blob_count": (c_int, [_I, _I]),
    "ivf_blob_stage": (c_int, [_P, _I, _I, _I, _I, _I, _I, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_blob_select": (c_int, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P, _P]),
    # csrc/stmask_ops.hip (maskType 'spacetime', documented extension)
    "ivf_stmask_axis_weights": (c_int, [_I, _I, _F, _P]),
    "ivf_stmask_expand_fwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_stmask_expand_bwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_stfreeze_fwd": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_stfreeze_bwd": (c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_stmask_reg": (c_int, [_P, _I, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P]),
    "ivf_stmask_step": (c_int, [_P] * 9 + [_I] * 5 + [_F] * 4 + [_P]),
    "ivf_stsearch_workspace_bytes": (c_size_t, [_I] * 6),
    # one-box search (maskType 'stcombi', documented extension)
    "ivf_box_count": (ctypes.c_longlong, [_I] * 6),
    "ivf_box_stage": (c_int, [_P] + [_I] * 5 + [_P, _P] + [_I] * 5 + [ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_box_select": (c_int, [_P, _P, _P] + [_I] * 7 + [_F] * 4 + [_P] * 5),
    "ivf_box_drop": (c_int, [_P, _P] + [_I] * 7 + [_P, _P]),
    # csrc/rise_ops.hip (RISE random-mask saliency, documented extension)
    "ivf_rise_masks": (c_int, [_U, _U] + [_I] * 5 + [_P, _P]),
    "ivf_rise_stage": (c_int, [_P] + [_I] * 5 + [_P, _P] + [_I] * 4 + [_U, _U, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_rise_reduce": (c_int, [_P, _P, _I, _I, _U, _U] + [_I] * 3 + [_P] * 4),
    # csrc/shapley_ops.hip (Shapley value sampling, documented extension)
    "ivf_shap_ranks": (c_int, [_U] + [_I] * 6 + [_P, _P]),
    "ivf_shap_stage": (c_int, [_P] + [_I] * 5 + [_P, _P] + [_I] * 4 + [_P, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_shap_reduce": (c_int, [_P, _P] + [_I] * 5 + [_P] * 5),
    # csrc/curve_ops.hip (deletion / insertion curves, documented extension)
    "ivf_curve_ranks": (c_int, [_P] + [_I] * 7 + [_P, _P]),
    "ivf_curve_stage": (c_int, [_P] + [_I] * 5 + [_P, _P] + [_I] * 3 + [_P, _I, _I, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_curve_reduce": (c_int, [_P] + [_I] * 5 + [_P] * 3),
    # csrc/linsur_ops.hip (KernelSHAP and LIME, documented extension)
    "ivf_kshap_rows": (c_int, [_U] + [_I] * 6 + [_P] * 4),
    "ivf_lime_rows": (c_int, [_U, _U] + [_I] * 5 + [_P, _P]),
    "ivf_lin_stage": (c_int, [_P] + [_I] * 5 + [_P, _P] + [_I] * 4 + [_P, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_lin_moments": (c_int, [_P] * 4 + [_I] * 3 + [_P] * 8),
    "ivf_lin_workspace_bytes": (c_size_t, [_I]),
    "ivf_lin_solve": (c_int, [_I] + [_P] * 7 + [_I] * 3 + [ctypes.c_double] + [_P] * 6),
    "ivf_lin_fit": (c_int, [_P] * 9 + [_I] * 3 + [_P, _P]),
    # csrc/scorecam_ops.hip (Score-CAM, documented extension)
    "ivf_scorecam_normalise": (c_int, [_P, _I, _I, _I] + [_P] * 5),
    "ivf_scorecam_stage": (c_int, [_P] + [_I] * 5 + [_P, _P] + [_I] * 3 + [_P, _I, _I, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_scorecam_reduce": (c_int, [_P] * 3 + [_I] * 4 + [_P] * 3),
    # csrc/ig_ops.hip (Integrated Gradients, documented extension)
    "ivf_ig_stage": (c_int, [_P, _I, _P, _F, _P] + [_I] * 5 + [ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_ig_accumulate": (c_int, [_P, _I, _P, _I, ctypes.c_longlong, _I, _P] + [_I] * 4 + [_P]),
    "ivf_ig_finish": (c_int, [_P, _I, _P, _F, _P] + [_I] * 4 + [_P] * 5),
    "ivf_ig_workspace_bytes": (c_size_t, [_I] * 5),
    # csrc/smoothgrad_ops.hip (SmoothGrad / SmoothGrad^2 / VarGrad, documented extension)
    "ivf_sg_noise": (c_int, [_U] + [_I] * 5 + [_P, _P]),
    "ivf_sg_range": (c_int, [_P] + [_I] * 4 + [_F, _P, _P]),
    "ivf_sg_stage": (c_int, [_P, _P] + [_I] * 5 + [_U, ctypes.c_longlong, _I, _P, _I, _P]),
    "ivf_sg_accumulate": (c_int, [_P, _I, _I, ctypes.c_longlong, _I, _P, _P] + [_I] * 4 + [_P]),
    "ivf_sg_finish": (c_int, [_P, _P] + [_I] * 5 + [_P] * 7),
    "ivf_sg_workspace_bytes": (c_size_t, [_I] * 5),
    "ivf_clip_ingest_u8": (c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_conv3d": (c_int, [POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P]),
    "ivf_bn_fold": (c_int, [_P, _P, _P, _P, _F, _P, _P, _I, _P]),
    "ivf_conv3d_pack_fwd_elems": (c_size_t, [_I] * 6),
    "ivf_conv3d_pack_fwd": (c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_conv3d_pack_fwd_rows": (c_int, [_P, _P] + [_I] * 9 + [_P]),
    "ivf_conv3d_pack_bwd_elems": (c_size_t, [_I] * 12),
    "ivf_conv3d_pack_bwd": (c_int, [_P, _P, _P] + [_I] * 13 + [POINTER(BwdGeom), _P]),
    "ivf_conv3d_pack_bwd_fused1x1_elems": (c_size_t, [_I, _I, _I]),
    "ivf_conv3d_pack_bwd_fused1x1": (c_int, [_P, _P, _P] + [_I] * 6 + [_P]),
    "ivf_maxpool3d_fwd": (c_int, [POINTER(PoolDesc), _P, _P, _P, _P]),
    "ivf_maxpool3d_bwd": (c_int, [POINTER(PoolDesc), _P, _P, _P, _P, _I, _P]),
    "ivf_head_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_head_bwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_head_fwd_bf16": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_head_bwd_bf16": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_gradcam_reduce": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ivf_gradcam_reduce_bf16": (c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    # csrc/cam_ops.hip (Grad-CAM++ / XGrad-CAM / HiResCAM / LayerCAM, documented extension)
    "ivf_cam_ws_bytes": (c_size_t, [_I, _I, _I]),
    "ivf_cam_reduce": (c_int, [_P, _P, _I, POINTER(c_int), _P, _P, _P, _I, _I, _I, _P]),
    "ivf_cam_reduce_bf16": (c_int, [_P, _P, _I, POINTER(c_int), _P, _P, _P, _I, _I, _I, _P]),
    "ivf_cam_resize_normalise": (c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "ivf_argmax": (c_int, [_P, _I, _I, _P, _P]),
    "ivf_i3d_create": (c_int, [POINTER(I3DConfig), POINTER(c_void_p)]),
    "ivf_i3d_destroy": (None, [_P]),
    "ivf_i3d_set_overlap": (_I, [_P, _I]),
    "ivf_i3d_weights_bytes": (c_size_t, [_P]),
    "ivf_i3d_workspace_bytes": (c_size_t, [_P]),
    "ivf_i3d_bind": (c_int, [_P, _P, _P]),
    "ivf_i3d_num_convs": (c_int, [_P]),
    "ivf_i3d_conv_info": (c_int, [_P, _I, c_char_p] + [POINTER(c_int)] * 6),
    "ivf_i3d_load_conv": (c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _P]),
    "ivf_i3d_forward": (c_int, [_P, _P, _I, _P, _P, _P]),
    "ivf_i3d_forward_staged": (c_int, [_P, _I, _P, _P, _P]),
    "ivf_i3d_input_buffer": (c_void_p, [_P]),
    "ivf_i3d_input_grad_buffer": (c_void_p, [_P]),
    "ivf_i3d_backward": (c_int, [_P, _I, _P, _P, _P, _P, _P]),
    "ivf_i3d_endpoint": (c_int, [_P, c_char_p, POINTER(c_void_p)] + [POINTER(c_int)] * 5),
    "ivf_i3d_act_elem_bytes": (c_int, [_P]),
    "ivf_i3d_search": (c_int, [_P, _P, _I, _P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _I, _I, _I, _P, _P]),
    "ivf_i3d_perturbed_forward": (c_int, [_P, _P, _I, _P, _I, _P, _P]),
    "ivf_i3d_stsearch": (c_int, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I] + [_F] * 7 + [_I, _I, _P, _P, _P]),
    "ivf_i3d_stperturbed_forward": (c_int, [_P, _P, _I, _P, _P, _P]),
    "ivf_i3d_blob_scores": (c_int, [_P, _P, _I, _P, _I, _I, _P, _P]),
    "ivf_i3d_ig": (c_int, [_P, _P, _I, _P, _I, _P, _F, _P, _P, _I] + [_P] * 7),
    "ivf_i3d_ig_path_scores": (c_int, [_P, _P, _I, _P, _I, _P, _F, _P, _I, _P, _P]),
    "ivf_i3d_box_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 5 + [_P, _P]),
    "ivf_i3d_rise_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 4 + [_U, _U, _P, _P]),
    "ivf_i3d_shap_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 4 + [_P, _P, _P]),
    "ivf_i3d_lin_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 4 + [_P, _P, _P]),
    "ivf_i3d_curve_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 3 + [_P, _I, _I, _P, _P]),
    "ivf_i3d_scorecam_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 3 + [_P, _I, _I, _P, _P]),
    "ivf_i3d_smoothgrad": (c_int, [_P, _P, _I, _P, _I, _F, _U] + [_P] * 10),
    "ivf_i3d_gradcam": (c_int, [_P, _P, _I, _P, _I, _I, _I, _P, _P, _P]),
    "ivf_i3d_gradcam_layer": (c_int, [_P, _P, _I, _P, c_char_p, _I, _I, _I, _P, _P, _P]),
    "ivf_i3d_cam_layer": (c_int, [_P, _P, _I, _P, c_char_p, _I, POINTER(c_int), _I, _I, _I, _P, _P, _P]),
    "ivf_i3d_cam_raw": (c_int, [_P, _P, _I, _P, c_char_p, _I, POINTER(c_int)] + [_P] * 6),
    "ivf_i3d_conv_flops_per_clip": (ctypes.c_double, [_P]),
    "ivf_conv3d_variants": (c_int, [POINTER(ConvDesc), POINTER(c_int), _I]),
    "ivf_conv3d_default_variant": (c_int, [POINTER(ConvDesc)]),
    "ivf_i3d_num_conv_ops": (c_int, [_P]),
    "ivf_i3d_autotune": (c_int, [_P, _I, _I, _P]),
    "ivf_i3d_get_tuning": (c_int, [_P, POINTER(c_int)]),
    "ivf_i3d_set_tuning": (c_int, [_P, POINTER(c_int)]),
    "ivf_viz_blend": (c_int, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "ivf_viz_dots": (c_int, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "ivf_profile_enable": (c_int, [_I, _I]),
    "ivf_profile_disable": (c_int, []),
    "ivf_profile_collect": (c_int, [POINTER(ctypes.c_double), POINTER(ctypes.c_longlong),
                                    POINTER(ctypes.c_double)]),
    "ivf_profile_class_name": (c_char_p, [_I]),
    "ivf_profile_collect_sites": (c_int, [POINTER(ctypes.c_double), POINTER(ctypes.c_longlong),
                                          POINTER(ctypes.c_double), POINTER(c_int), _I]),
    "ivf_i3d_num_sites": (c_int, [_P]),
    "ivf_i3d_site_name": (c_int, [_P, _I, c_char_p]),
    # csrc/convlstm.hip
    "ivf_clstm_create": (c_int, [POINTER(CLSTMConfig), POINTER(c_void_p)]),
    "ivf_clstm_destroy": (None, [_P]),
    "ivf_clstm_weights_bytes": (c_size_t, [_P]),
    "ivf_clstm_workspace_bytes": (c_size_t, [_P]),
    "ivf_clstm_bind": (c_int, [_P, _P, _P]),
    "ivf_clstm_load_cell": (c_int, [_P, _I] + [_P] * 12 + [_P]),
    "ivf_clstm_load_head": (c_int, [_P, _P, _P, _P, _P, _P, _P, _F, _P]),
    "ivf_clstm_forward": (c_int, [_P, _P, _I, _P, _P, _P]),
    "ivf_clstm_backward": (c_int, [_P, _I, _P, _P, _P, _P, _P]),
    "ivf_clstm_search": (c_int, [_P, _P, _I, _P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _I, _I, _I, _P, _P]),
    "ivf_clstm_perturbed_forward": (c_int, [_P, _P, _I, _P, _I, _P, _P]),
    "ivf_clstm_stsearch": (c_int, [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I] + [_F] * 7 + [_I, _I, _P, _P, _P]),
    "ivf_clstm_stperturbed_forward": (c_int, [_P, _P, _I, _P, _P, _P]),
    "ivf_clstm_blob_scores": (c_int, [_P, _P, _I, _P, _I, _I, _P, _P]),
    "ivf_clstm_ig": (c_int, [_P, _P, _I, _P, _I, _P, _F, _P, _P, _I] + [_P] * 7),
    "ivf_clstm_ig_path_scores": (c_int, [_P, _P, _I, _P, _I, _P, _F, _P, _I, _P, _P]),
    "ivf_clstm_box_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 5 + [_P, _P]),
    "ivf_clstm_rise_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 4 + [_U, _U, _P, _P]),
    "ivf_clstm_shap_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 4 + [_P, _P, _P]),
    "ivf_clstm_lin_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 4 + [_P, _P, _P]),
    "ivf_clstm_curve_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 3 + [_P, _I, _I, _P, _P]),
    "ivf_clstm_scorecam_scores": (c_int, [_P, _P, _I, _P, _P, _P] + [_I] * 3 + [_P, _I, _I, _P, _P]),
    "ivf_clstm_smoothgrad": (c_int, [_P, _P, _I, _P, _I, _F, _U] + [_P] * 10),
    "ivf_clstm_gradcam_reduce": (c_int, [_P, _P, POINTER(c_int), _I, _P, _P, _I, _I, _I, _I, _P]),
    "ivf_clstm_set_cam_steps": (c_int, [_P, POINTER(c_int), _I]),
    "ivf_clstm_gradcam": (c_int, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    "ivf_clstm_gradcam_raw": (c_int, [_P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P]),
    "ivf_clstm_cam_reduce": (c_int, [_P, _P, POINTER(c_int), _I, _I, POINTER(c_int), _P, _P, _I, _I, _I, _I, _P]),
    "ivf_clstm_cam": (c_int, [_P, _P, _I, _P, _I, _I, POINTER(c_int), _I, _I, _I, _P, _P, _P]),
    "ivf_clstm_cam_raw": (c_int, [_P, _P, _I, _P, _I, _I, POINTER(c_int)] + [_P] * 6),
    "ivf_clstm_layer_buffers": (c_int, [_P, _I, POINTER(c_void_p), POINTER(c_void_p)] + [POINTER(c_int)] * 3),
    # csrc/tf_clstm.hip (documented extension)
    "ivf_tfclstm_create": (c_int, [POINTER(TFCLSTMConfig), POINTER(c_void_p)]),
    "ivf_tfclstm_destroy": (None, [_P]),
    "ivf_tfclstm_weights_bytes": (c_size_t, [_P]),
    "ivf_tfclstm_workspace_bytes": (c_size_t, [_P]),
    "ivf_tfclstm_bind": (c_int, [_P, _P, _P]),
    "ivf_tfclstm_layer_dims": (c_int, [_P, _I] + [POINTER(c_int)] * 5),
    "ivf_tfclstm_fc_inputs": (c_int, [_P]),
    "ivf_tfclstm_layer_buffers": (c_int, [_P, _I] + [POINTER(c_void_p)] * 3),
    "ivf_tfclstm_load_layer": (c_int, [_P, _I, _P, _P, _P, _P]),
    "ivf_tfclstm_load_head": (c_int, [_P, _P, _P, _P]),
    "ivf_tfclstm_forward": (c_int, [_P, _P, _I, _P, _P, _P]),
    "ivf_tfclstm_backward": (c_int, [_P, _I, _P, _P, _P, _P]),
    "ivf_tfclstm_perturbed_forward": (c_int, [_P, _P, _I, _P, _P, _P]),
    "ivf_tfclstm_search": (c_int, [_P, _P, _I, _P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _I, _I, _P, _P]),
    "ivf_tfclstm_gradcam": (c_int, [_P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P]),
}

_lib = None


def lib():
    """Load libivf_hip.so once; raise loudly if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IvfError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                "(or `make -C interpreting-video-features_amd/csrc`). There is no fallback path.")
        L = ctypes.CDLL(LIB_PATH)
        L.ivf_last_error.restype = c_char_p
        L.ivf_last_error.argtypes = []
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return ["ivf_last_error"] + list(_SIGS)


def check(rc):
    if rc != 0:
        raise IvfError(f"libivf_hip error {rc}: {lib().ivf_last_error().decode()}")


_recent = collections.deque(maxlen=64)


def cam_kind_ids(kinds):
    """ctypes int array of the ids of a sequence of Grad-CAM family kind names; an unknown name raises."""
    kinds = [kinds] if isinstance(kinds, str) else list(kinds)
    for k in kinds:
        if k not in CAM_KINDS:
            raise IvfError(f"unknown CAM kind {k!r}: one of {', '.join(CAM_KINDS)}")
    return kinds, (c_int * max(len(kinds), 1))(*[CAM_KINDS[k] for k in kinds])


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor stays referenced for the next 64 pointers taken: a
    temporary passed as `ptr(x.cuda())` would otherwise hand its block back to the caching allocator before the other
    arguments of the same call are built, and a tensor created for one of them could be placed on it and overwrite it
    before the kernel runs."""
    if t is None:
        return None
    _recent.append(t)
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(*tensors):
    if not torch.cuda.is_available():
        raise IvfError("no HIP device visible: the saliency path runs on the MI355X only "
                       "(there is no CPU fallback)")
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise IvfError("tensor must live on the GPU (call .cuda() first)")


def f32c(t):
    """contiguous fp32 view/copy on the same device"""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()

"""ctypes binding of libbasedet_hip.so (the C ABI declared in include/basedet_hip.h).

The product path has NO CPU fallback: if the shared library is missing, or a kernel is asked to run on a
tensor that is not on a HIP device, this module raises.  torch is only the memory carrier (data_ptr / stream).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BASEDET_HIP_LIB") or os.path.join(_HERE, "lib", "libbasedet_hip.so")   # override: A/B of two builds

BD_MAX_SEGS = 8
ABI_VERSION = 118              # bd_version() of the library this binding matches (118: bd_affine_jitter_normalize of image_affine.hip; 117: bd_centernet_boxes_to_image; 116: the bd_center_head_out_* entries of center_head.hip; 115: the bd_centernet_* entries of centernet.hip; 114: the GroupNorm partials of bd_conv2d_fwd_gnstats / bd_groupnorm_fwd hold (mean, M2), not (sum, sum of squares); 113: the bd_deform_conv_* entries of deform_conv.hip;101: the liveness-map fields; 102: the EMA entries; 103: raw-image input; 104: the *_ld entries; 105: bd_iou_ltrb_fwd_bwd, bd_loss_grid_cap; 106: the Adam / Nesterov entries of optim.hip; 107: the forward liveness maps; 108: the stem backward entries of stem_bwd.hip; 109: the bd_bn_* entries of batchnorm.hip; 110: bd_bn_apply_act_fwd, bd_stem_conv7x7_raw_fwd; 111: bd_bn_apply_fwd removed, bd_bn_apply_act_fwd serves its callers; 112: one entry per operator -- the *_ld, _general, _batched and _joint twins and the giou forwarder folded into the base names, which take their arguments)
EPI_RELU, EPI_ADD_BEFORE, EPI_ADD_AFTER, EPI_MASK, EPI_SPARSE = 1, 2, 4, 8, 16


class BasedetHipError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("R", C.c_int32), ("S", C.c_int32),
        ("stride", C.c_int32), ("pad", C.c_int32), ("nseg", C.c_int32),
        ("Hi", C.c_int32 * BD_MAX_SEGS), ("Wi", C.c_int32 * BD_MAX_SEGS),
        ("Ho", C.c_int32 * BD_MAX_SEGS), ("Wo", C.c_int32 * BD_MAX_SEGS),
        ("in_off", C.c_int32 * BD_MAX_SEGS), ("out_off", C.c_int32 * BD_MAX_SEGS),
        ("in_pix_per_img", C.c_int32), ("out_pix_per_img", C.c_int32),
        ("route", C.c_int32 * 4), ("sr_seed", C.c_uint32),        # per-call kernel routing / e5m2 rounding seed (0 = the library's choice)
        ("gskip", C.c_int32), ("gskip_ws", C.c_void_p), ("gskip_ws_bytes", C.c_size_t),   # gradient-skip hint + dgrad scratch (0 = dense)
        # liveness maps of g (read) and dx (written), and the promise that dx holds +0 outside the dx map's last list (0 = none)
        ("gskip_gmap", C.c_void_p), ("gskip_gmap_bytes", C.c_size_t), ("gskip_dxmap", C.c_void_p), ("gskip_dxmap_bytes", C.c_size_t),
        ("gskip_dx_clean", C.c_int32),
        # forward liveness map of the output (bd_fwd_live_maps) and the promise that y holds +0 outside the previous call's list (0 = dense)
        ("fwd_map", C.c_void_p), ("fwd_map_bytes", C.c_size_t), ("fwd_clean", C.c_int32),
    ]


class PackDesc(C.Structure):
    _fields_ = [("w", C.c_void_p), ("row_scale", C.c_void_p), ("w_fwd", C.c_void_p), ("w_dgrad", C.c_void_p),
                ("Cout", C.c_int32), ("RS", C.c_int32), ("Cin", C.c_int32), ("block_start", C.c_int32)]


class ImageDesc(C.Structure):
    """bd_image_desc: one image of a packed raw batch (bd_resize_pad_normalize)."""
    _fields_ = [("offset", C.c_int64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("dst_h", C.c_int32), ("dst_w", C.c_int32),
                ("flip", C.c_int32), ("reserved_", C.c_int32 * 1)]


AFFINE_BRIGHTNESS, AFFINE_CONTRAST, AFFINE_SATURATION, AFFINE_LIGHTING = 1, 2, 4, 8          # bd_affine_desc.stages


class AffineDesc(C.Structure):
    """bd_affine_desc: one image of a packed raw batch and what CenterNet's training pipeline does to it (bd_affine_jitter_normalize);
    inv = the row-major 2 x 3 map from an output pixel to the source image."""
    _fields_ = [("offset", C.c_int64), ("src_h", C.c_int32), ("src_w", C.c_int32), ("inv", C.c_double * 6), ("flip", C.c_int32),
                ("stages", C.c_uint32), ("alpha_brightness", C.c_float), ("alpha_contrast", C.c_float), ("alpha_saturation", C.c_float),
                ("delta", C.c_float * 3)]


_P, _I, _L, _F, _Z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_D = C.POINTER(ConvDesc)

# name -> (restype, argtypes); must list every symbol include/basedet_hip.h declares
SIGNATURES = {
    "bd_last_error_string": (C.c_char_p, []),
    "bd_version": (_I, []),
    "bd_conv_last_kernel": (C.c_char_p, []),
    "bd_probe_mfma_rate": (_I, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), _P]),
    "bd_probe_kernel_clock": (_I, [C.c_char_p, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bd_conv2d_fwd": (_I, [_D, _P, _P, _P, _P, _P, _I, _P]),
    "bd_conv2d_dgrad": (_I, [_D, _P, _P, _P, _P, _P, _I, _P]),
    "bd_conv2d_dgrad_gskip_bytes": (_Z, [_D]),
    "bd_conv2d_gskip_map_bytes": (_Z, [_D, _I]),
    "bd_gskip_map_scan": (_I, [_D, _I, _P, _P, _Z, _P]),
    "bd_fwd_live_map_bytes": (_Z, [_D]),
    "bd_fwd_live_maps": (_I, [_D, _P, _I, _I, C.POINTER(C.c_void_p), _Z, _I, _P]),
    "bd_conv2d_fwd_bits": (_I, [_D, _P, _P, _P, _P, _P, _P, _I, _P]),
    "bd_conv2d_fwd_ex": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "bd_conv2d_dgrad_ex": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "bd_conv2d_dgrad_bits": (_I, [_D, _P, _P, _P, _P, _P, _I, _P]),
    "bd_conv2d_wgrad_workspace_bytes": (_Z, [_D]),
    "bd_conv2d_wgrad": (_I, [_D, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "bd_conv2d_wgrad_bias_workspace_bytes": (_Z, [_D]),
    "bd_conv2d_wgrad_bias": (_I, [_D, _P, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "bd_fpn_deconv_pack": (_I, [_P, _I, _P, _P, _P]),
    "bd_fpn_deconv_fwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "bd_fpn_deconv_dgrad": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "bd_fpn_deconv_wgrad_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "bd_fpn_deconv_wgrad": (_I, [_P, _P, _P, _I, _P, _Z, _I, _I, _I, _I, _I, _I, _P]),
    # (..., N, H, W, Cin, Cout, ld, modulated, kernel_size, stride, padding, dilation, deformable_groups, stream)
    "bd_deform_conv_fwd": (_I, [_P, _P, _P, _P, _P] + [_I] * 12 + [_P]),
    "bd_deform_conv_wgrad_workspace_bytes": (_Z, [_I] * 5),
    "bd_deform_conv_wgrad": (_I, [_P, _P, _P, _P, _P, _I, _P, _Z] + [_I] * 12 + [_P]),
    "bd_deform_conv_bwd_data_workspace_bytes": (_Z, [_I] * 5),
    "bd_deform_conv_bwd_data": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _Z] + [_I] * 12 + [_P]),
    "bd_wgrad_queue_create": (_I, [_P]),
    "bd_wgrad_queue_destroy": (_I, [_P]),
    "bd_wgrad_queue_pending": (_I, [_P]),
    "bd_conv2d_wgrad_queued": (_I, [_P, _D, _P, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "bd_wgrad_queue_flush": (_I, [_P, _P]),
    "bd_stem_conv7x7_fwd": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "bd_stem_conv7x7_raw_fwd": (_I, [_I, _I, _I, _P, _P, _P, _P]),
    "bd_stem_pool_fwd": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "bd_stem_weight_pack": (_I, [_P, _P, _P, _P]),
    "bd_maxpool3x3s2_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "bd_stem_conv7x7_wgrad_workspace_bytes": (_Z, [_I, _I, _I]),
    "bd_stem_conv7x7_wgrad": (_I, [_I, _I, _I, _P, _P, _P, _P, _I, _P, _Z, _P]),
    "bd_weight_pack": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "bd_weight_pack_blocks": (_I, [_I, _I, _I]),
    "bd_weight_pack_multi": (_I, [_P, _I, _I, _P]),
    "bd_colsum_workspace_bytes": (_Z, [_I]),
    "bd_colsum_bf16": (_I, [_P, _I, _L, _L, _L, _I, _P, _I, _P, _Z, _P]),
    "bd_pad_normalize": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "bd_bottleneck_fwd_supported": (_I, [_I, _I, _I, _I, _I, _I, _I]),
    "bd_bottleneck_fwd": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "bd_h2d_create": (_I, [C.POINTER(C.c_void_p), _I, _I]),
    "bd_h2d_threads": (_I, [_P]),
    "bd_h2d_submit": (_I, [_P, _P, _I, _L, _P, _L, _P]),
    "bd_h2d_destroy": (_I, [_P]),
    "bd_pad_normalize_nchw": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "bd_resize_pad_normalize": (_I, [_P, _L, C.POINTER(ImageDesc), _I, _I, _I, _P, _P, _P, _P]),
    "bd_resize_bilinear_normalize": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "bd_affine_jitter_workspace_bytes": (_Z, [_I, _I, _I]),
    "bd_affine_jitter_normalize": (_I, [_P, _L, C.POINTER(AffineDesc), _I, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_maxpool3x3s2_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "bd_upsample2x_add_fwd": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _P]),
    "bd_upsample2x_add_bwd": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _I, _P]),
    "bd_relu_bf16": (_I, [_P, _P, _L, _P]),
    "bd_relu_bwd_bf16": (_I, [_P, _P, _P, _P, _L, _P]),
    "bd_add_bf16": (_I, [_P, _P, _P, _L, _P]),
    "bd_anchors_generate": (_I, [_I, _I, _I, _F, _P, _I, _P, _P]),
    "bd_points_generate": (_I, [_I, _I, _I, _F, _I, _P, _P]),
    "bd_box_pairwise": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "bd_box_encode": (_I, [_P, _P, _L, _P, _P, _P, _P]),
    "bd_box_decode": (_I, [_P, _P, _L, _P, _P, _P, _P]),
    "bd_retina_assign_encode": (_I, [_P, _I, _P, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_fcos_assign": (_I, [_P, _I, _P, _P, _P, _I, _F, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "bd_ota_assign_workspace_bytes": (_Z, [_I, _I]),
    "bd_ota_assign": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _F, _F, _F, _F, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_ota_sinkhorn_workspace_bytes": (_Z, [_I, _I, _I]),
    "bd_ota_assign_sinkhorn": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _F, _F, _F, _F, _I, _F, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_freeanchor_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "bd_freeanchor_loss_fwd_bwd": (_I, [_P, _I, _P, _I, _I, _P, _I, _I, _P, _P, _I, _I, _P, _P, _F, _I, _F, _F, _F, _F, _P, _P, _P, _P, _Z, _P]),
    "bd_atss_assign_workspace_bytes": (_Z, [_I, _I]),
    "bd_atss_assign": (_I, [_P, _I, _P, _P, _I, _I, _F, _P, _P, _I, _I, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_nms_workspace_bytes": (_Z, [_I]),
    "bd_batched_nms": (_I, [_P, _P, _P, _I, _F, _I, _P, _P, _P, _Z, _P]),
    "bd_focal_loss_fwd_bwd": (_I, [_P, _P, _L, _I, _I, _F, _F, _P, _I, _F, _P, _P, _I, _P]),
    "bd_smooth_l1_fwd_bwd": (_I, [_P, _P, _P, _L, _I, _I, _F, _P, _I, _F, _P, _P, _P]),
    "bd_loss_grid_cap": (_I, []),
    "bd_iou_ltrb_fwd_bwd": (_I, [_P, _P, _P, _P, _L, _I, _P, _F, _P, _P, _P]),
    "bd_bce_logits_fwd_bwd": (_I, [_P, _I, _I, _P, _P, _L, _P, _P, _P, _P]),
    "bd_groupnorm_workspace_bytes": (_Z, [_I, _I, _I, _L]),
    "bd_groupnorm_fwd": (_I, [_P, _P, _P, _I, _I, _P, _P, _L, _I, _F, _I, _P, _P, _P, _Z, _P]),
    "bd_conv2d_fwd_gnstats_bytes": (_Z, [_D]),
    "bd_conv2d_fwd_gnstats": (_I, [_D, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_groupnorm_fwd_parts": (_I, [_D, _P, _P, _P, _P, _F, _I, _P, _P, _P]),
    "bd_groupnorm_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _L, _I, _I, _P, _P, _P, _I, _P, _Z, _P]),
    "bd_bn_workspace_bytes": (_Z, [_L, _I]),
    "bd_bn_stats_fwd": (_I, [_P, _I, _L, _L, _L, _I, _F, _F, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_bn_apply_act_fwd": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _L, _L, _P, _L, _L, _I, _L, _I, _I, _P]),
    "bd_bn_bwd_reduce": (_I, [_P, _L, _L, _P, _L, _L, _P, _P, _I, _L, _I, _P, _P, _P, _Z, _P]),
    "bd_bn_bwd_apply": (_I, [_P, _L, _L, _P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _L, _I, _P]),
    # conv -> BN -> SiLU (added without an ABI break, as the bd_yolox_* entries were)
    "bd_bn_silu_fwd": (_I, [_P, _L, _L, _P, _P, _P, _P, _P, _L, _L, _I, _L, _I, _P]),
    "bd_bn_silu_bwd_reduce": (_I, [_P, _L, _L, _P, _L, _L, _P, _P, _P, _P, _I, _L, _I, _P, _P, _P, _Z, _P]),
    "bd_bn_silu_bwd_apply": (_I, [_P, _L, _L, _P, _L, _L, _P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _I, _L, _I, _P]),
    "bd_fcos_offsets_fwd": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _L, _P, _P]),
    "bd_fcos_offsets_workspace_bytes": (_Z, []),
    "bd_fcos_offsets_bwd": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _L, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_rpn_assign_encode": (_I, [_P, _I, _P, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_sample_labels": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "bd_segment_topk": (_I, [_P, _I, _I, _L, _I, _I, _I, _I, _P, _P, _I, _F, _I, _P, _P, _P, _P]),
    "bd_nms_batched_workspace_bytes": (_Z, [_I, _I]),
    "bd_nms_batched": (_I, [_P, _P, _P, _I, _I, _F, _I, _I, _P, _P, _P, _Z, _P]),
    "bd_rpn_proposals_workspace_bytes": (_Z, [_I, _I, _P, _I, _I, _I]),
    "bd_rpn_proposals": (_I, [_P, _I, _I, _I, _I, _I, _L, _I, _P, _P, _P, _P, _I, _P, _P, _I, _F, _I, _P, _P, _P, _Z, _I, _P]),
    "bd_rcnn_sample_targets": (_I, [_P, _P, _I, _P, _P, _I, _I, _P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    "bd_roi_align_fwd": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "bd_conv1x1_thin_bwd_workspace_bytes": (_Z, []),
    "bd_conv1x1_thin_fwd": (_I, [_P, _P, _P, _L, _I, _I, _P, _P]),
    "bd_conv1x1_thin_bwd": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _P, _I, _P, _Z, _P]),
    "bd_roi_align_bwd": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "bd_roi_align_bwd_bf16_workspace_bytes": (_Z, [_I, _I, _P, _P, _I]),
    "bd_roi_align_bwd_bf16": (_I, [_P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "bd_roi_pool_fwd": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "bd_roi_pool_bwd_bf16_workspace_bytes": (_Z, [_I, _I, _P, _P, _I]),
    "bd_roi_pool_bwd_bf16": (_I, [_P, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "bd_subsample2x_fwd": (_I, [_P, _L, _L, _I, _I, _P, _L, _L, _I, _I, _P]),
    "bd_subsample2x_bwd_add": (_I, [_P, _L, _L, _P, _L, _L, _I, _I, _I, _I, _P]),
    "bd_f32_to_bf16": (_I, [_P, _P, _L, _P]),
    "bd_f32_to_bf16_add": (_I, [_P, _P, _L, _P]),
    "bd_rpn_loss_fwd_bwd": (_I, [_P, _I, _I, _I, _I, _P, _P, _L, _F, _P, _P, _P, _P]),
    "bd_rcnn_loss_fwd_bwd": (_I, [_P, _I, _I, _I, _P, _P, _I, _F, _P, _P, _P, _P]),
    "bd_det_scores": (_I, [_P, _I, _P, _I, _I, _L, _I, _P, _P]),
    "bd_det_select_workspace_bytes": (_Z, [_I, _I, _L, _I, _I]),
    "bd_det_select": (_I, [_P, _I, _P, _I, _I, _I, _L, _I, _I, _P, _P, _I, _F, _P, _P, _P, _P, _Z, _P]),
    "bd_centernet_targets_workspace_bytes": (_Z, [_I]),
    # (gt_boxes, num_gt, N, Gmax, K, H, W, T, box_scale, min_overlap (double), score_map, wh, reg, reg_mask, index, num_pos, ws, ws_bytes, stream)
    "bd_centernet_targets": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _F, C.c_double, _P, _P, _P, _P, _P, _P, _P, _Z, _P]),
    "bd_centernet_focal_fwd_bwd": (_I, [_P, _P, _L, _I, _I, _P, _F, _F, _P, _P, _P]),
    "bd_centernet_l1_fwd_bwd": (_I, [_P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P]),
    "bd_centernet_decode_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "bd_centernet_decode": (_I, [_P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    # (feat, w_cls, b_cls, w_wh, b_wh, w_reg, b_reg, M, C, K, cls_ld, logits, wr, stream)
    "bd_centernet_boxes_to_image": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "bd_center_head_out_fwd": (_I, [_P] * 7 + [_L, _I, _I, _I, _P, _P, _P]),
    "bd_center_head_out_bwd_workspace_bytes": (_Z, [_L, _I, _I]),
    # (feat, d_logits, d_wr, w_cls, w_wh, w_reg, M, C, K, cls_ld, d_feat, dw_cls, db_cls, dw_wh, db_wh, dw_reg, db_reg, accumulate, ws, ws_bytes, stream)
    "bd_center_head_out_bwd": (_I, [_P] * 6 + [_L, _I, _I, _I] + [_P] * 7 + [_I, _P, _Z, _P]),
    "bd_yolox_assign_workspace_bytes": (_Z, [_I, _I]),
    # (points, P, lvl_start, strides, L, cls, K, ld, box_obj, gt_boxes, num_gt, N, Gmax, matched, iou_t, stats, ws, ws_bytes, stream)
    "bd_yolox_assign": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "bd_yolox_loss_workspace_bytes": (_Z, []),
    # (points, P, lvl_start, strides, L, cls, K, ld, box_obj, gt_boxes, N, Gmax, matched, iou_t, stats, use_l1, grad_scale, loss_out, d_cls,
    #  d_box_obj, ws, ws_bytes, stream)
    "bd_yolox_loss_fwd_bwd": (_I, [_P, _I, _P, _P, _I, _P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _I, _F, _P, _P, _P, _P, _Z, _P]),
    # (topk_idx, topk_score, topk_cnt, B, L, k, lvl_start, strides, K, points, P, box_obj, boxes, scores, labels, stream)
    "bd_yolox_candidates": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    # CSPDarknet / YOLOPAFPN glue (yolox_neck.hip; added without an ABI break, as the bd_yolox_* entries were)
    "bd_spp_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "bd_spp_bwd": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    # (a, b, M, Ca, Cb, up, N, H, W, out, stream)
    "bd_cat2_fwd": (_I, [_P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P]),
    # (g, M, Ca, Cb, up, N, H, W, d_a, acc_a, d_b, acc_b, stream)
    "bd_cat2_bwd": (_I, [_P, _L, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P]),
    "bd_focus_fwd": (_I, [_P, _I, _I, _I, _P, _P]),
    "bd_rcnn_predict": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "bd_det_candidates": (_I, [_I, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _L, _I, _I, _P, _P, _P, _L, _P, _P, _P, _P]),
    "bd_det_finalize": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    "bd_sgd_momentum_step": (_I, [_P, _P, _P, _L, _F, _F, _F, _F, _P]),
    "bd_ema_update": (_I, [_P, _P, _L, _F, _F, _P]),
    "bd_sgd_momentum_ema_step": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _P]),
    "bd_swap_f32": (_I, [_P, _P, _L, _P]),
    # (w, m, v, g[, e], n, lr, beta1, 1 - beta1, beta2, 1 - beta2, bc1, bc2, eps, wd, grad_scale, decoupled[, ema_m, 1 - ema_m], stream)
    "bd_adam_step": (_I, [_P, _P, _P, _P, _L] + [_F] * 10 + [_I, _P]),
    "bd_adam_ema_step": (_I, [_P, _P, _P, _P, _P, _L] + [_F] * 10 + [_I, _F, _F, _P]),
    "bd_sgd_nesterov_step": (_I, [_P, _P, _P, _L, _F, _F, _F, _F, _P]),
    "bd_sgd_nesterov_ema_step": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _P]),
    "bd_clip_grad_value": (_I, [_P, _L, _F, _F, _F, _P]),
    "bd_clip_grad_norm_workspace_bytes": (_Z, []),
    "bd_clip_grad_norm": (_I, [_P, _L, _F, _F, _F, _P, _P, _Z, _P]),
    "bd_quantize_fp8": (_I, [_P, _L, _F, _P, _P]),
    "bd_weight_pack_fp8": (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _P]),
    "bd_conv2d_fwd_fp8": (_I, [_D, _P, _P, _P, _P, _P, _P, _I, _P]),
    "bd_conv2d_fwd_fp8_ex": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "bd_quantize_bf8": (_I, [_P, _L, _F, _P, C.c_uint32, _P]),
    "bd_absmax_bf16": (_I, [_P, _L, _P, _P]),
    "bd_weight_pack_fp8_t": (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _P]),
    "bd_conv2d_dgrad_fp8": (_I, [_D, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "bd_conv2d_wgrad_fp8_workspace_bytes": (_Z, [_D]),
    "bd_conv2d_wgrad_fp8": (_I, [_D, _P, _P, _F, _P, _P, _I, _P, _Z, _P]),
    "bd_conv1x1_fp8": (_I, [_D, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "bd_sigmoid_focal_loss_elem": (_I, [_P, _P, _L, _F, _F, _P, _P, _P, _P]),
    "bd_bce_elem": (_I, [_P, _P, _L, _I, _P, _P, _P, _P]),
    "bd_smooth_l1_elem": (_I, [_P, _P, _L, _F, _P, _P, _P, _P]),
    "bd_iou_loss_ltrb": (_I, [_P, _P, _L, _I, _F, _P, _P, _P, _P, _P]),
    "bd_iou_to_loss": (_I, [_P, _L, _I, _F, _P, _P]),
    "bd_matcher_matrix": (_I, [_P, _I, _L, _P, _P, _I, _I, _P, _P, _P, _P]),
    "bd_assign_roi_levels": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "bd_roi_pool_max_fwd": (_I, [_P, _I, _I, _I, _I, _P, _I, _F, _I, _I, _P, _P]),
    "bd_comm_unique_id": (_I, [_P]),
    "bd_comm_init": (_I, [C.POINTER(C.c_void_p), _P, _I, _I, _I]),
    "bd_comm_rank": (_I, [_P]),
    "bd_comm_world": (_I, [_P]),
    "bd_comm_stream": (_P, [_P]),
    "bd_comm_bcast": (_I, [_P, _P, _Z, _I, _I, _P]),
    "bd_comm_allreduce": (_I, [_P, _P, _Z, _I, _I, _P]),
    "bd_comm_allreduce_async": (_I, [_P, _P, _Z, _I, _I, C.POINTER(C.c_void_p), _I]),
    "bd_comm_allreduce_async_bf16": (_I, [_P, _P, _P, _Z, _I, C.POINTER(C.c_void_p), _I]),
    "bd_comm_wait": (_I, [_P, _P]),
    "bd_comm_destroy": (_I, [_P]),
}

_lib = None


def load():
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BasedetHipError(
            f"{LIB_PATH} is missing: build it with `python -m basedet_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the basedet_amd operator path.")
    lib = C.CDLL(LIB_PATH)
    lib.bd_version.restype = C.c_int
    check_version(int(lib.bd_version()))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:      # entries added without an ABI break (the bd_yolox_* entries of yolox.hip) keep bd_version() as it is
            raise BasedetHipError(f"{LIB_PATH} does not export {name}: rebuild it with `python -m basedet_amd.build`") from None
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check_version(have):
    """A library built from another header lays bd_conv_desc out differently: refuse it instead of handing it a struct it misreads."""
    if have != ABI_VERSION:
        raise BasedetHipError(f"{LIB_PATH} reports bd_version() = {have}, this binding needs {ABI_VERSION}: rebuild it with "
                              "`python -m basedet_amd.build`")


def check(rc, what=""):
    if rc != 0:
        msg = load().bd_last_error_string()
        raise BasedetHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL). Refuses host tensors: no CPU fallback."""
    if t is None:
        return C.c_void_p(0)
    if not t.is_cuda:
        raise BasedetHipError("basedet_amd kernels need tensors on a HIP device (got a CPU tensor); there is no CPU fallback")
    if not t.is_contiguous():
        raise BasedetHipError("basedet_amd kernels need contiguous tensors")
    return C.c_void_p(t.data_ptr())


def f32arr(vals):
    return (C.c_float * len(vals))(*[float(v) for v in vals])


def i32arr(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])

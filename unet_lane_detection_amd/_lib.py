"""ctypes binding of libunet_hip.so (C ABI: include/unet_hip.h).

There is no fallback: if the library is missing or does not load, importing a
product path raises.  (The oracle under oracle/ is test infrastructure and is
never reached from here.)
"""
from __future__ import annotations

import ctypes as C
import os

# torch bundles its own libamdhip64; it must be the first HIP runtime in the process, or a second copy pulled in through
# libunet_hip.so's RPATH-less dependency fails to see the device.
import torch

from .build import LIB, build_library, is_stale

UNET_MAX_DEPTH = 6


class UnetConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32),
        ("out_channels", C.c_int32),
        ("depth", C.c_int32),
        ("features", C.c_int32 * UNET_MAX_DEPTH),
        ("device", C.c_int32),
        ("input_mean", C.c_float * 3),
        ("input_std", C.c_float * 3),
    ]


class LossConfig(C.Structure):
    """unet_loss_config of include/unet_hip.h"""
    _fields_ = [
        ("mode", C.c_int),
        ("bce_weight", C.c_float),
        ("focal_weight", C.c_float),
        ("dice_weight", C.c_float),
        ("pos_weight", C.c_float),
        ("alpha", C.c_float),
        ("gamma", C.c_float),
        ("smooth", C.c_float),
    ]


UNET_MAX_CLASSES = 8


class ClassLossConfig(C.Structure):
    """unet_class_loss_config of include/unet_hip.h"""
    _fields_ = [
        ("ce_weight", C.c_float),
        ("dice_weight", C.c_float),
        ("smooth", C.c_float),
        ("class_weight", C.c_float * UNET_MAX_CLASSES),
        ("ignore_index", C.c_int),
    ]


class LaneViewStyle(C.Structure):
    """unet_lane_view_style of include/unet_hip.h"""
    _fields_ = [
        ("alpha", C.c_float),
        ("beta", C.c_float),
        ("gamma", C.c_float),
        ("area", C.c_uint8 * 3),
        ("marking", C.c_uint8 * 3),
        ("reserved", C.c_uint8 * 2),
        ("thickness", C.c_int),
        ("layers", C.c_uint),
    ]


class CorrectConfigStruct(C.Structure):
    """unet_correct_config of include/unet_hip.h"""
    _fields_ = [
        ("white_balance", C.c_int),
        ("max_gain", C.c_int),
        ("lo_bp", C.c_int),
        ("hi_bp", C.c_int),
        ("clahe", C.c_int),
        ("grid_x", C.c_int),
        ("grid_y", C.c_int),
        ("clip_q8", C.c_int),
        ("only_flagged", C.c_int),
        ("dark_limit", C.c_int),
        ("bright_limit", C.c_int),
        ("tone", C.c_uint8 * 256),
    ]


STATUS = {0: "UNET_OK", 1: "UNET_ERR_INVALID_ARG", 2: "UNET_ERR_SHAPE", 3: "UNET_ERR_STATE", 4: "UNET_ERR_HIP",
          5: "UNET_ERR_NOMEM", 6: "UNET_ERR_UNKNOWN_PARAM", 7: "UNET_ERR_RANGE"}
UNET_ERR_HIP = 4     # a HIP runtime call or a kernel-side check failed
UNET_ERR_RANGE = 7   # f16x3 tier: an activation left the fp16 range (include/unet_hip.h); re-run on the fp32 tier

# name -> (restype, argtypes); every symbol include/unet_hip.h declares
SIGNATURES = {
    "unet_create": (C.c_int, [C.POINTER(UnetConfig), C.POINTER(C.c_void_p)]),
    "unet_load_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "unet_finalize": (C.c_int, [C.c_void_p]),
    "unet_num_params": (C.c_int, [C.c_void_p]),
    "unet_param_name": (C.c_char_p, [C.c_void_p, C.c_int]),
    "unet_param_numel": (C.c_size_t, [C.c_void_p, C.c_int]),
    "unet_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "unet_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "unet_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_float, C.c_void_p]),
    "unet_forward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_float, C.c_void_p]),
    "unet_forward_u8_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_float, C.c_void_p]),
    "unet_forward_u8_x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_float, C.c_void_p]),
    "unet_forward_f32_x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_float, C.c_void_p]),
    "unet_op_conv3x3_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_conv3x3_x3_head": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "unet_op_upconv2x2_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_conv3x3_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_upconv2x2_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_conv_first_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_maxpool2x2_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "unet_op_head1x1_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "unet_op_split_planes_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p]),
    "unet_op_conv3x3_bf16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "unet_op_conv3x3_bf16_head": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                            C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_upconv2x2_bf16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_conv_first_bf16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "unet_op_maxpool2x2_bf16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "unet_op_head1x1_bf16": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                       C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_i8_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "unet_i8_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "unet_i8_finalize": (C.c_int, [C.c_void_p]),
    "unet_i8_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_float, C.c_void_p]),
    "unet_i8_out_channels": (C.c_int, [C.c_void_p]),
    "unet_i8_forward_classes_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_i8_run_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                   C.c_void_p]),
    "unet_i8_read_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "unet_i8_set_hybrid": (C.c_int, [C.c_void_p, C.c_int]),
    "unet_i8_tensor_dtype": (C.c_int, [C.c_void_p, C.c_char_p]),
    "unet_i8_read_tensor_f16": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]),
    "unet_i8_destroy": (C.c_int, [C.c_void_p]),
    "unet_i8_last_error": (C.c_char_p, [C.c_void_p]),
    "unet_num_range_tensors": (C.c_int, [C.c_void_p]),
    "unet_forward_u8_ranges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_forward_classes_u8_ranges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p]),
    "unet_op_histogram_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "unet_forward_u8_histograms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p]),
    "unet_forward_classes_u8_histograms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                     C.c_int, C.c_void_p, C.c_void_p]),
    "unet_prob_mae_accumulate": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "unet_destroy": (C.c_int, [C.c_void_p]),
    "unet_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "unet_profile_count": (C.c_int, [C.c_void_p]),
    "unet_profile_get": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "unet_train_param_numel": (C.c_size_t, [C.c_void_p]),
    "unet_train_buffer_numel": (C.c_size_t, [C.c_void_p]),
    "unet_train_layout": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "unet_train_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_train_set_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]),
    "unet_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "unet_train_forward_backward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_train_forward_backward_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_train_adam_step": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                       C.c_int, C.c_float, C.c_void_p]),
    "unet_train_adam_step_rec": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                           C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "unet_grad_work_bytes": (C.c_size_t, []),
    "unet_grad_accumulate_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "unet_train_debug_snapshot": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "unet_op_wgrad3x3": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p]),
    "unet_op_wgrad3x3_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p]),
    "unet_op_train_conv3x3_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "unet_op_upconv_bwd_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "unet_op_upconv_fwd_train_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_train_repack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "unet_set_train_x3": (C.c_int, [C.c_int]),
    "unet_set_train_side": (C.c_int, [C.c_int]),
    "unet_train_set_comm_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "unet_train_grad_split": (C.c_size_t, [C.c_void_p]),
    "unet_dice_metric": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p,
                                   C.c_void_p]),
    "unet_train_eval_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_train_eval_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_seg_metrics_accumulate": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_int,
                                              C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "unet_train_set_loss_cfg": (C.c_int, [C.c_void_p, C.POINTER(LossConfig)]),
    "unet_seg_metrics_accumulate_cfg": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_float,
                                                  C.POINTER(LossConfig), C.c_void_p, C.c_void_p]),
    "unet_op_loss_grad": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(LossConfig), C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "unet_mask_positive_counts": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_device_error": (C.c_int, [C.c_void_p]),
    "unet_device_error_on": (C.c_int, [C.c_void_p, C.c_void_p]),
    "unet_device_status_to": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_debug_set_error_block": (C.c_int, [C.c_void_p, C.c_int, C.c_uint]),
    "unet_debug_act_scale": (C.c_float, [C.c_float, C.c_float]),
    "unet_last_error": (C.c_char_p, [C.c_void_p]),
    "unet_op_last_error": (C.c_char_p, []),
    "unet_version": (C.c_char_p, []),
    "unet_set_winograd": (C.c_int, [C.c_int]),
    "unet_set_bf16_persistent": (C.c_int, [C.c_int]),
    "unet_set_x3_upconv_r512": (C.c_int, [C.c_int]),
    "unet_set_x3_cross_fp8": (C.c_int, [C.c_int]),
    "unet_set_x3_compose": (C.c_int, [C.c_int]),
    "unet_set_x3_dec_form": (C.c_int, [C.c_int]),
    "unet_set_x3_compose_deep": (C.c_int, [C.c_int]),
    "unet_op_updeep_window_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                  C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_updeep_conv3x3_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_void_p, C.c_void_p]),
    "unet_host_pack_updeep_x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "unet_host_plan_updeep_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "unet_set_x3_fuse_first": (C.c_int, [C.c_int]),
    "unet_host_plan_enc1_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "unet_op_enc1_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_upcat_conv3x3_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_host_compose_upcat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_host_plan_conv3x3_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "unet_host_plan_upconv2x2_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "unet_host_plan_dec_step_x3": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "unet_host_pack_x3": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "unet_ipm_prestage_u8": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_resize_u8": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    "unet_augment_u8": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_augment_u8_labels": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_augment_param_bytes": (C.c_size_t, []),
    "unet_resize_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "unet_overlay_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_ensemble_combine": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_float), C.c_size_t,
                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_score_sweep_accumulate": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_float),
                                              C.c_int, C.c_void_p, C.c_void_p]),
    "unet_set_sweep_combine": (C.c_int, [C.c_int]),
    "unet_hsv_lanes_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_lane_center_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                            C.c_int, C.c_void_p, C.c_void_p]),
    "unet_lane_fit_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_label_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_label_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "unet_keep_components_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p]),
    "unet_lane_view_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                          C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                          C.POINTER(LaneViewStyle), C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_lane_view_style_bytes": (C.c_size_t, []),
    "unet_frame_stats_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p]),
    "unet_prob_stats_f32_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
    "unet_correct_config_bytes": (C.c_size_t, []),
    "unet_correct_work_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "unet_correct_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(CorrectConfigStruct), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                        C.c_void_p]),
    "unet_fill_polygons_u8_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_conv3x3": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_upconv2x2": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_conv1x1": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                  C.c_void_p, C.c_void_p]),
    "unet_op_maxpool2x2": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_head1x1": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                  C.c_void_p, C.c_void_p]),
    # the fp32 tier on the network's own paths (tests/test_f32_ops_gpu.py)
    "unet_op_conv3x3_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "unet_op_upconv2x2_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_conv1x1_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_maxpool2x2_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p]),
    "unet_op_head1x1_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_op_pack_input_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "unet_host_plan_conv_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    # multi-class segmentation (csrc/multiclass_kernels.h)
    "unet_forward_classes_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_forward_classes_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_train_set_class_loss": (C.c_int, [C.c_void_p, C.POINTER(ClassLossConfig)]),
    "unet_train_forward_backward_labels_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_train_forward_backward_labels_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_confusion_work_bytes": (C.c_size_t, []),
    "unet_confusion_accumulate": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "unet_op_headk": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "unet_op_headk_x3_planes": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "unet_class_loss_work_bytes": (C.c_size_t, []),
    "unet_class_loss_grad": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t,
                                       C.POINTER(ClassLossConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "unet_class_labels_f32": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]),
    "unet_op_headk_backward": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


def load(build_if_missing: bool = True) -> C.CDLL:
    """Load (building first if the .so is absent and hipcc is available)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("UNET_HIP_LIB", LIB)   # override: A/B timing builds of the same ABI
    if path == LIB and is_stale():
        # content hash of the sources differs from the one the .so was built from (or there is no .so)
        if not build_if_missing:
            raise RuntimeError(f"{LIB} is missing or older than its sources; run `python -m unet_lane_detection_amd.build`")
        build_library()
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class UnetError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__(f"{where}: {STATUS.get(code, code)}" + (f" ({detail})" if detail else ""))


def check(code, where, handle=None):
    if code != 0:
        # without a handle: the calling thread's last failure in a handle-less entry point (unet_op_*, metrics, camera)
        msg = load().unet_last_error(handle) if handle else load().unet_op_last_error()
        detail = msg.decode() if msg else ""
        raise UnetError(code, where, detail)


def ptr(t):
    """a tensor's device address as the ABI's void*; None is the null pointer"""
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def stream(device):
    """torch's current stream on `device` as the ABI's void* stream"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, device, *args):
    """Call the handle-less entry point `name(int device, ..., void* stream)` on torch's current stream of `device` and
    raise UnetError on a failure.  Tensors among `args` pass as their device addresses, everything else unchanged."""
    argv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]   # None is already null
    check(getattr(load(), name)(device.index, *argv, stream(device)), name)

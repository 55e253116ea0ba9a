"""ctypes binding of libdib_hip.so (C ABI: include/dib.h).

There is deliberately NO fallback: if the HIP library is missing or fails to load, importing
any compute entry point raises.  The CPU oracle under oracle/ is test infrastructure and is
never imported from this package.
"""
import ctypes
import os

# torch must be imported BEFORE libdib_hip.so is opened: the wheel bundles its own HIP runtime
# (same SONAME as /opt/rocm's); whichever is loaded first serves the whole process, and the
# streams / device pointers we are handed belong to torch's.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# DIB_HIP_LIB: another build of the same library (diagnostic builds of scratch/: stamps, timelines); never set in production
LIB_PATH = os.environ.get("DIB_HIP_LIB") or os.path.join(_HERE, "libdib_hip.so")

DIB_F16, DIB_F32 = 0, 1
DIB_ACC_BITEXACT, DIB_ACC_FP32, DIB_ACC_FMA16, DIB_ACC_FAST16 = 0, 1, 2, 3
DIB_EINVAL, DIB_ESHAPE, DIB_EHIP, DIB_ENOT128, DIB_ECAPTURE, DIB_ETIMEOUT = -1, -2, -3, -4, -5, -6
DIB_STEP_PSFS_COMPLETE, DIB_STEP_LARGE_WINDOW = 1, 2
DIB_COMPACT_LARGE_WINDOW, DIB_WINDOW_LARGE, DIB_COMPACT_VRUNS = 8, 0x100, 16
DIB_EPILOGUE_QUANTIZE, DIB_EPILOGUE_PAD = 1, 2
DIB_WARP_NHWC, DIB_WARP_NCHW = 0, 1

_lib = None

_c_int_p = ctypes.POINTER(ctypes.c_int)
_c_void_pp = ctypes.POINTER(ctypes.c_void_p)


class AugmixImage(ctypes.Structure):
    """include/dib.h dib_augmix_image: one image's AugMix plan for dib_augmix."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("buf_offset", ctypes.c_ulonglong), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("flip", ctypes.c_int), ("n_ops", ctypes.c_int * 3), ("op", (ctypes.c_int * 3) * 3),
                ("iparam", (ctypes.c_int * 3) * 3), ("affine", ((ctypes.c_double * 6) * 3) * 3), ("ws", ctypes.c_float * 3),
                ("m", ctypes.c_float), ("one_minus_m", ctypes.c_float)]


_c_augmix_p = ctypes.POINTER(AugmixImage)


class OverlayBox(ctypes.Structure):
    """include/dib.h dib_overlay_box: one outline of dib_overlay_rgb8 (rgb = R | G << 8 | B << 16 of the output)."""
    _fields_ = [("x0", ctypes.c_int), ("y0", ctypes.c_int), ("x1", ctypes.c_int), ("y1", ctypes.c_int), ("rgb", ctypes.c_uint)]

_SIGNATURES = {
    "dib_abi_version": (ctypes.c_int, []),
    "dib_last_error": (ctypes.c_char_p, []),
    "dib_tap_table_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "dib_tap_tables_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "dib_psf_compact": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "dib_psf_compact_list": (ctypes.c_int, [_c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "dib_sparse_blur": (ctypes.c_int, [_c_void_pp, _c_void_pp, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p]),
    "dib_blur_step": (ctypes.c_int, [_c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     _c_void_pp, _c_void_pp, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "dib_blur_step_packed": (ctypes.c_int, [_c_void_pp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "dib_blur_step_release": (ctypes.c_int, []),
    "dib_blur_step_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "dib_blur_step_ws": (ctypes.c_int, [_c_void_pp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        _c_void_pp, _c_void_pp, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int,
                                        ctypes.c_void_p]),
    "dib_device_status": (ctypes.c_int, [ctypes.c_int]),
    "dib_normalize_pad": (ctypes.c_int, [_c_void_pp, ctypes.c_int, _c_int_p, _c_int_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                         ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]),
    "dib_normalize_resize_pad": (ctypes.c_int, [_c_void_pp, ctypes.c_int, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_normalize_resize_crop": (ctypes.c_int, [_c_void_pp, ctypes.c_int, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_sparse_blur_normalized": (ctypes.c_int, [_c_void_pp, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_expand_boxes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p]),
    "dib_clamp_boxes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_psf_rasterize_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dib_psf_rasterize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "dib_roi_align_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "dib_roi_align_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "dib_roi_align_nhwc_forward": (ctypes.c_int, [_c_void_pp, _c_int_p, _c_int_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_roi_align_nhwc_backward": (ctypes.c_int, [ctypes.c_void_p, _c_int_p, _c_int_p, ctypes.POINTER(ctypes.c_float),
                                                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_void_pp, ctypes.c_void_p]),
    "dib_nms_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "dib_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p]),
    "dib_nms_batched": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_box_match": (ctypes.c_int, [ctypes.c_void_p, _c_int_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_box_encode_matched": (ctypes.c_int, [ctypes.c_void_p, _c_int_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "dib_box_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_bias_act_transpose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_topk_levels": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "dib_det_candidates": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_float] * 9 +
                           [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_box_pool": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                    ctypes.c_void_p]),
    "dib_box_labels": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _c_int_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "dib_coco_box_iou": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "dib_bias_act_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_void_p]),
    "dib_bias_act_mask_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "dib_relu_mask_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    "dib_add_relu_mask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    "dib_scatter_add_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_fpn_topdown_merge_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_stem_pool_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_stem_pool_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_void_p]),
    "dib_fold_bn_multi": (ctypes.c_int, [_c_void_pp, _c_void_pp, _c_void_pp, _c_void_pp, _c_void_pp, _c_int_p, _c_int_p, ctypes.c_int,
                                         ctypes.c_float, _c_void_pp, _c_void_pp, _c_void_pp, ctypes.c_void_p]),
    "dib_scale_rows_multi": (ctypes.c_int, [_c_void_pp, _c_void_pp, _c_int_p, _c_int_p, ctypes.c_int, _c_void_pp, ctypes.c_void_p]),
    "dib_post_ops": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_double, ctypes.c_ulonglong, ctypes.c_double, ctypes.c_void_p]),
    "dib_jpeg_roundtrip": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_void_p]),
    "dib_bn_mode_one_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int]),
    "dib_bn_mode_one_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_bn_acclimate_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_augmix_buffer_bytes": (ctypes.c_ulonglong, [_c_augmix_p]),
    "dib_augmix_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_ulonglong]),
    "dib_augmix": (ctypes.c_int, [_c_augmix_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dib_squint_warp_forward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_squint_warp_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_overlay_rgb8": (ctypes.c_int, [_c_void_pp, ctypes.c_int, _c_int_p, _c_int_p, ctypes.c_int, ctypes.c_void_p, _c_int_p, _c_void_pp,
                                        ctypes.c_void_p]),
    "dib_deblur_pyramid": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_void_pp, ctypes.c_void_p]),
    "dib_deblur_shuffle_concat": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_deblur_finish": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]),
    # IEEE Half forms: the deblurrer under --deblur_precision half (the only Half member of the epilogue family is bias_act)
    "dib_bias_act_f16_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_void_p]),
    "dib_deblur_pyramid_f16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_void_pp, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "dib_deblur_shuffle_concat_f16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "dib_deblur_finish_f16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p]),
    # --deconvolve_first: Richardson-Lucy with the blur's own tap table (models/deconvolve.py)
    "dib_rl_deconvolve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]),
    # the total-variation factor x * g and the regularised iteration (models/deconvolve.py: tv_lambda, tv_beta)
    "dib_tv_weight": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_void_p]),
    "dib_rl_deconvolve_tv": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                            ctypes.c_float, ctypes.c_float, ctypes.c_void_p]),
    # restoration quality: mse, PSNR and SSIM of one image against another (quality.py)
    "dib_image_quality_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dib_image_quality": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # ... of one or two candidates against one sharp image, with a per-cell accumulator on the device (quality.RestorationMeter)
    "dib_restoration_quality_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dib_restoration_quality": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, _c_void_pp, _c_int_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    # the DeepDeblur trainer (models/deblur_train.py): patch gather, epilogue backward with the bias gradient, L1 loss of a level
    "dib_deblur_patches": (ctypes.c_int, [_c_void_pp, ctypes.c_int, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.POINTER(ctypes.c_uint),
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    # ... with dataCommon's saturation change and add_noise in the same launch (--change_saturation, --patch_noise_sigma)
    "dib_deblur_patches_augment": (ctypes.c_int, [_c_void_pp, ctypes.c_int, _c_int_p, _c_int_p, _c_int_p, _c_int_p, ctypes.POINTER(ctypes.c_uint),
                                                  ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint),
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_bias_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int]),
    "dib_bias_grad_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # their Half forms: the trainer under --amp
    "dib_bias_act_mask_f16_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    "dib_bias_grad_f16_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong, ctypes.c_int]),
    "dib_bias_grad_f16_nhwc": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_l1_pyramid_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong]),
    "dib_l1_pyramid_loss": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    # the trainer's adversarial loss (models/deblur_adversarial.py): LeakyReLU with a sign mask, its backward, BCE against a constant label
    "dib_leaky_relu_mask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_leaky_relu_mask_f16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    "dib_leaky_relu_mask_backward": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong,
                                                    ctypes.c_void_p]),
    "dib_leaky_relu_mask_backward_f16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_longlong,
                                                        ctypes.c_void_p]),
    "dib_adv_bce_loss_workspace_bytes": (ctypes.c_size_t, [ctypes.c_longlong]),
    "dib_adv_bce_loss": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    # test hook, not part of the drop-in boundary
    "dib_sparse_blur_generic": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p]),
}

# The trunk's epilogue family (csrc/dib_eltwise_vec.h): an fp32 and a bf16 entry point per member, with one argument list.  LANE:
# elements per 16-byte lane vector by activation dtype (channel and element counts are multiples of it, one sign-mask byte each).
LANE = {torch.float32: 4, torch.bfloat16: 8}
_FAMILY = {"bias_act": "dib_bias_act%s_nhwc", "bias_act_mask": "dib_bias_act_mask%s_nhwc", "relu_mask_backward": "dib_relu_mask_backward%s",
           "add_relu_mask": "dib_add_relu_mask%s", "scatter_add": "dib_scatter_add%s_nhwc", "topdown_merge": "dib_fpn_topdown_merge%s_nhwc",
           "stem_pool_forward": "dib_stem_pool_forward%s", "stem_pool_backward": "dib_stem_pool_backward%s"}
_SIGNATURES.update({pattern % "_bf16": _SIGNATURES[pattern % ""] for pattern in _FAMILY.values()})
_family = {}      # (member, dtype) -> entry point, resolved once: the lookup sits on every launch's host path

EXPORTS = tuple(k for k in _SIGNATURES if k != "dib_sparse_blur_generic")


class DibError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libdib_hip: %s (code %d)" % (text, code))
        self.code = code


class DibStepTimeout(DibError):
    """DIB_ETIMEOUT: an EARLIER blur step on this device gave up waiting inside its launch (include/dib.h, "Device status"); its
    images are incomplete, nothing was launched by the call that reports it, and the device is on two launches per step from here."""


def lib():
    """Loads libdib_hip.so once.  Raises if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise ImportError("%s not found: build it with `make -C detectinblur_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        if l.dib_abi_version() != 7:
            raise ImportError("libdib_hip.so ABI version mismatch")
        _lib = l
    return _lib


def family(member, dtype):
    """The entry point of a member of the epilogue family (a key of _FAMILY) for activations of `dtype`; KeyError for any other dtype."""
    if not _family:
        _family.update({(m, dt): getattr(lib(), p % sfx) for m, p in _FAMILY.items() for dt, sfx in ((torch.float32, ""), (torch.bfloat16, "_bf16"))})
    return _family[member, dtype]


def check(code):
    if code != 0:
        text = lib().dib_last_error().decode("utf-8", "replace")
        raise (DibStepTimeout if code == DIB_ETIMEOUT else DibError)(code, text)


_raw_stream = None


def stream_of(tensor):
    """hipStream_t (as an int) of torch's current stream on the tensor's device.  torch's raw accessor is ~30x cheaper than building
    a torch.cuda.Stream object (8 us of host time per call: measured in round 4), which is most of a small launch."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream:
        idx = tensor.device.index
        return _raw_stream(idx if idx is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(tensor.device).cuda_stream


_INT_ARRAYS, _PTR_ARRAYS = {}, {}      # ctypes array TYPES by length (building the type is most of a small array's cost)


def int_array(values):
    n = len(values)
    t = _INT_ARRAYS.get(n)
    if t is None:
        t = _INT_ARRAYS[n] = ctypes.c_int * n
    return t(*values)


def ptr_array(values):
    n = len(values)
    t = _PTR_ARRAYS.get(n)
    if t is None:
        t = _PTR_ARRAYS[n] = ctypes.c_void_p * n
    return t(*values)

"""ctypes binding of libmrcnn_hip.so (the C-ABI declared in include/mrcnn_hip.h).

This is the only way the product path reaches the GPU: there is no eager/PyTorch fallback.  If the
library is missing or a call returns a non-zero status a ``HipPathError`` is raised.
PyTorch is used by the callers only as the owner of device memory and of the current HIP stream.
"""
import ctypes as C
import os
import threading

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libmrcnn_hip.so")


class HipPathError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad_t", "pad_l", "OH", "OW",
        "act", "res_mode", "out_mode", "cmod")] + [
        ("out_n_stride", C.c_int64), ("out_h_stride", C.c_int64), ("out_w_stride", C.c_int64)]


class ConvProblem(C.Structure):
    """mrcnn_conv_problem (include/mrcnn_hip.h): one convolution of a mrcnn_conv2d_fwd_multi launch."""
    _fields_ = [("d", ConvDesc)] + [(n, C.c_void_p) for n in ("x", "w", "bias", "scale", "shift", "res", "out", "z_out")]


class WgradProblem(C.Structure):
    """mrcnn_wgrad_problem (include/mrcnn_hip.h)."""
    _fields_ = [("d", ConvDesc), ("x", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p), ("accumulate", C.c_int32)]


class RoiAlignDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("R", C.c_int32), ("P", C.c_int32), ("C", C.c_int32),
                ("H", C.c_int32 * 4), ("W", C.c_int32 * 4), ("image_area", C.c_float)]


class ProposalDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("A", C.c_int32), ("pre_nms_limit", C.c_int32),
                ("proposal_count", C.c_int32), ("nms_threshold", C.c_float), ("std_dev", C.c_float * 4)]


class DetTargetDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "R", "G", "T", "MH", "MW", "mask_h", "mask_w",
                                          "positive_count")] + [
        ("negative_ratio_r", C.c_float), ("bbox_std_dev", C.c_float * 4), ("use_mini_mask", C.c_int32)]


class RpnTargetDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("A", C.c_int32), ("G", C.c_int32), ("n_train", C.c_int32),
                ("bbox_std_dev", C.c_double * 4)]


class WinoGroup(C.Structure):
    """mrcnn_wino_group (include/mrcnn_hip.h): a group of Winograd tiles of one map."""
    _fields_ = [("oth", C.c_int), ("otw", C.c_int), ("th_n", C.c_int), ("tw_n", C.c_int), ("oh0", C.c_int), ("ow0", C.c_int)]


class BwdEpilogue(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("out", "z", "scale", "mean", "rstd", "dgamma", "dbeta", "dbias")] + [
        ("act", C.c_int32), ("dy", C.c_void_p)]


class ConvPlan(C.Structure):
    """mrcnn_conv_plan (include/mrcnn_hip.h): what a float32 convolution launch would do, from mrcnn_conv2d_fwd_plan."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "bm", "bn", "ksplit", "ksteps", "grid", "reduce", "mt_full", "tail_ksplit",
                                          "tail_ksteps", "slab_bytes")]


CONV_KERNELS = ("TILE", "BLDS", "GLDS", "BLDS_SPLITK", "BLDS_TAIL", "SK", "SK16", "SK64")      # MRCNN_CONV_*, by value
CONV_REDUCTIONS = ("NONE", "SCALAR", "VEC", "BWD")                                            # MRCNN_CONV_RED_*


class BwdEpilogueH16(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("out", "z", "scale", "mean", "rstd", "dgamma", "dbeta", "dbias")] + [
        ("act", C.c_int32), ("dy", C.c_void_p), ("grad_multiplier", C.c_float)]


class H16Plan(C.Structure):
    """mrcnn_h16_plan (include/mrcnn_hip.h): what a 16-bit forward / data-gradient launch would do, from mrcnn_conv2d_fwd_h16_plan."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "zout", "grid", "threads", "ptiles", "mtile0", "rem_grid", "rem_mtile0", "ep_vec", "dense",
                                          "fused_ep", "reserved")] + [("trace", C.c_uint64)]


class H16WgradPlan(C.Structure):
    """mrcnn_h16_wgrad_plan: what a 16-bit weight-gradient launch would do, from mrcnn_conv2d_wgrad_h16_plan."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "splits", "chunk", "nk", "itiles", "ntiles", "grid", "reduce", "reduce_grid", "xcd_order")] + [
        (n, C.c_int64) for n in ("table_bytes", "slab_bytes", "workspace_bytes")]


class WgradPlan(C.Structure):
    """mrcnn_wgrad_plan: what a float32 weight-gradient launch would do, from mrcnn_conv2d_wgrad_plan."""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "bi", "bn", "fast", "splits", "chunk", "grid", "table_grid", "reduce", "reduce_grid", "lds_bytes",
                                          "reserved")] + [(n, C.c_int64) for n in ("slab_bytes", "table_bytes", "workspace_bytes")]


WGRAD_MULTI_MAX = 16                                                                          # MRCNN_WGRAD_MULTI_MAX


class WgradMultiPlan(C.Structure):
    """mrcnn_wgrad_multi_plan: what mrcnn_conv2d_wgrad_multi would launch, from mrcnn_conv2d_wgrad_multi_plan."""
    _fields_ = [(n, C.c_int32) for n in ("n", "grid", "reduce_grid", "reserved")] + [
        ("splits", C.c_int32 * WGRAD_MULTI_MAX), ("chunk", C.c_int32 * WGRAD_MULTI_MAX),
        ("first", C.c_int32 * (WGRAD_MULTI_MAX + 1)), ("rfirst", C.c_int32 * (WGRAD_MULTI_MAX + 1)),
        ("slab_offset", C.c_int64 * WGRAD_MULTI_MAX), ("slab_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


WGRAD_KERNELS = ("TILE", "BLDS", "BLDS_TABLE", "GLDS")                                        # MRCNN_WGRAD_*, by value
WGRAD_REDUCTIONS = ("NONE", "SCALAR", "VEC")                                                  # MRCNN_WGRAD_RED_*
H16_KERNELS = ("S64", "T128", "RING", "BIG", "WAVE128", "PHASE", "PHASE_DECONV", "SLAB")       # MRCNN_H16_*, by value
H16_WGRAD_KERNELS = ("TABLE", "PHASE")                                                        # MRCNN_H16_WGRAD_*
H16_REDUCTIONS = ("SCALAR", "VEC")                                                            # MRCNN_H16_RED_*


class DetectionDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("R", C.c_int32), ("C", C.c_int32), ("max_instances", C.c_int32),
                ("min_confidence", C.c_float), ("nms_threshold", C.c_float), ("bbox_std_dev", C.c_float * 4)]


class LossDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "A", "T", "C", "mask_h", "mask_w", "max_rpn_pos",
                                          "mask_loss_dice")] + [("w", C.c_float * 5)]


class DrawDesc(C.Structure):
    """mrcnn_draw_desc (include/mrcnn_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "scale", "n_planes", "n_items", "n_texts", "n_glyphs", "n_colours", "shaded", "pad")]


class FitsChain(C.Structure):
    """mrcnn_fits_chain (include/mrcnn_hip.h): the read_fits flags of mrcnn_fits_to_image / mrcnn_fits_tiles_to_image."""
    _fields_ = [(n, C.c_int32) for n in ("zscale", "biascontrast", "normalize", "out_kind")] + [
        ("zscale_contrasts", C.c_double * 3), ("bias", C.c_double), ("contrast", C.c_double)]


ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
RES_NONE, RES_SAME, RES_UP2 = 0, 1, 2
OUT_NHWC, OUT_DECONV2 = 0, 1

_P = C.c_void_p
_SIGNATURES = {
    "mrcnn_conv2d_fwd": (C.c_int, [C.POINTER(ConvDesc)] + [_P] * 9),
    "mrcnn_conv2d_fwd_ws": (C.c_int, [C.POINTER(ConvDesc)] + [_P] * 9 + [C.c_size_t, _P]),
    "mrcnn_conv2d_fwd_workspace": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "mrcnn_conv2d_fwd_plan": (C.c_int, [C.POINTER(ConvDesc)] + [_P] * 9 + [C.c_size_t, C.POINTER(BwdEpilogue), C.POINTER(ConvPlan)]),
    "mrcnn_conv2d_fwd_multi_workspace": (C.c_size_t, [C.POINTER(ConvProblem), C.c_int]),
    "mrcnn_conv2d_fwd_multi": (C.c_int, [C.POINTER(ConvProblem), C.c_int, _P, C.c_size_t, _P]),
    "mrcnn_conv2d_wgrad_multi_workspace": (C.c_size_t, [C.POINTER(WgradProblem), C.c_int]),
    "mrcnn_conv2d_wgrad_multi": (C.c_int, [C.POINTER(WgradProblem), C.c_int, _P, C.c_size_t, _P]),
    "mrcnn_conv2d_wgrad": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, C.c_size_t, C.c_int, _P]),
    "mrcnn_conv2d_wgrad_workspace": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "mrcnn_conv2d_wgrad_plan": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, C.c_size_t, C.POINTER(WgradPlan)]),
    "mrcnn_conv2d_wgrad_multi_plan": (C.c_int, [C.POINTER(WgradProblem), C.c_int, _P, C.c_size_t, C.POINTER(WgradMultiPlan)]),
    "mrcnn_weight_flip_transpose": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_weight_flip_transpose_batched": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P]),
    "mrcnn_bn_fold": (C.c_int, [_P, _P, _P, _P, C.c_float, _P, _P, _P, C.c_int64, _P]),
    "mrcnn_epilogue_bwd": (C.c_int, [_P] * 11 + [C.c_int64, C.c_int, C.c_int, _P]),
    "mrcnn_maxpool3x3s2_fwd": (C.c_int, [_P, _P, _P] + [C.c_int] * 8 + [_P]),
    "mrcnn_maxpool3x3s2_bwd": (C.c_int, [_P, _P, _P] + [C.c_int] * 6 + [_P]),
    "mrcnn_subsample2_fwd": (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P]),
    "mrcnn_subsample2_bwd_acc": (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P]),
    "mrcnn_upsample2_bwd": (C.c_int, [_P, _P] + [C.c_int] * 5 + [_P]),
    "mrcnn_pixel_unshuffle2": (C.c_int, [_P, _P] + [C.c_int] * 4 + [_P]),
    "mrcnn_mask_out_bwd": (C.c_int, [_P] * 8 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_copy2d": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_size_t, C.c_size_t, _P]),
    "mrcnn_fill_zero": (C.c_int, [_P, C.c_size_t, _P]),
    "mrcnn_unpack_mask_bits": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_augment_warp_u8": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P]),
    "mrcnn_augment_warp_mask_bits": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P]),
    "mrcnn_mask_bits_stats_check": (C.c_int, [C.c_int] * 4),
    "mrcnn_mask_bits_stats_workspace": (C.c_size_t, [C.c_int]),
    "mrcnn_mask_bits_stats": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    "mrcnn_mask_bits_gather_check": (C.c_int, [C.c_int] * 5),
    "mrcnn_mask_bits_gather": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "mrcnn_mask_bits_zoom_check": (C.c_int, [C.c_int] * 9),
    "mrcnn_mask_bits_zoom": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       _P, _P]),
    "mrcnn_tile_adjacency": (C.c_int, [_P, C.c_int64, _P, C.c_int, _P, C.c_int, _P, _P]),
    "mrcnn_tile_union": (C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    "mrcnn_source_params": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P, C.c_int, _P, _P, _P, C.c_int64, C.c_double,
                                      C.c_int, _P, _P]),
    "mrcnn_mask_planes_pack": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "mrcnn_mask_pair_stats": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "mrcnn_mask_union": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "mrcnn_mask_cross_stats": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    "mrcnn_mask_plane_sums": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]),
    # box_host / piece_offsets_host are HOST tables (numpy int32)
    "mrcnn_mask_components_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t]),
    "mrcnn_mask_components_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_mask_components_count": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P]),
    "mrcnn_mask_components_emit": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "mrcnn_mask_row_extents": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "mrcnn_voc_match": (C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    # caps is a HOST table (4 x int32)
    "mrcnn_ap_sweep_caps": (C.c_int, [_P]),
    "mrcnn_ap_sweep": (C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P]),
    "mrcnn_unmold_masks_workspace": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "mrcnn_unmold_masks": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P,
                                     C.c_size_t, _P]),
    "mrcnn_fits_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "mrcnn_fits_to_rgb": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    # tiles_host is a HOST table (numpy, a 32-byte record per tile: ops.FITS_TILE_DTYPE)
    "mrcnn_outline_check": (C.c_int, [_P, C.c_int, C.c_int64, _P]),
    "mrcnn_outline_workspace": (C.c_size_t, [_P, C.c_int, C.c_int64, _P]),
    "mrcnn_outline_count": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int, _P, C.c_size_t, _P, _P, _P]),
    "mrcnn_outline_emit": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int, _P, _P, C.c_size_t, _P, C.c_size_t, _P, _P, C.c_int64, _P, C.c_int64,
                                     _P, _P, C.c_int64, _P]),
    # items_host / texts_host / glyphs_host are HOST tables (numpy: draw.ITEM_DTYPE, draw.TEXT_DTYPE, uint64)
    "mrcnn_draw_check": (C.c_int, [C.POINTER(DrawDesc), _P, _P, _P]),
    "mrcnn_draw_overlay": (C.c_int, [C.POINTER(DrawDesc)] + [_P] * 13),
    "mrcnn_fits_tiles_check": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "mrcnn_fits_tiles_workspace": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int]),
    "mrcnn_fits_tiles_to_rgb": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_double), _P, C.c_size_t, _P,
                                          C.c_size_t, _P]),
    "mrcnn_fits_image_check": (C.c_int, [C.POINTER(FitsChain), C.c_int, C.c_int]),
    "mrcnn_fits_to_image": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(FitsChain), _P, C.c_size_t, _P, C.c_size_t, _P]),
    "mrcnn_fits_tiles_to_image": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.POINTER(FitsChain), _P, C.c_size_t, _P,
                                            C.c_size_t, _P]),
    "mrcnn_mosaic_overview_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double]),
    "mrcnn_mosaic_overview_workspace": (C.c_size_t, [C.c_int, C.c_int]),
    "mrcnn_mosaic_overview": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _P, C.c_size_t, _P, C.c_size_t, _P]),
    "mrcnn_sources_to_planes_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mrcnn_sources_to_planes": (C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "mrcnn_catalog_check": (C.c_int, [C.c_int]),
    "mrcnn_catalog_count": (C.c_int, [_P, _P, C.c_int, C.c_double, C.c_double, _P, _P, _P]),
    "mrcnn_catalog_fill": (C.c_int, [_P] * 6 + [C.c_int, C.c_double, C.c_double, _P, C.c_longlong, _P, _P, _P]),
    "mrcnn_catalog_window_flags": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, _P, _P]),
    "mrcnn_catalog_nan_fill": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "mrcnn_mold_image_u8": (C.c_int, [_P] + [C.c_int] * 9 + [C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    "mrcnn_resize_image_u8": (C.c_int, [_P] + [C.c_int] * 9 + [_P, _P, C.c_size_t, _P]),
    "mrcnn_mold_image_f32_workspace_bytes": (C.c_size_t, []),
    "mrcnn_mold_image_f32": (C.c_int, [_P] + [C.c_int] * 9 + [C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    "mrcnn_add_inplace": (C.c_int, [_P, _P, C.c_int64, _P]),
    "mrcnn_softmax_rows": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "mrcnn_roialign_fwd": (C.c_int, [C.POINTER(RoiAlignDesc)] + [_P] * 8),
    "mrcnn_roialign_bwd": (C.c_int, [C.POINTER(RoiAlignDesc)] + [_P] * 7),
    "mrcnn_roialign_bwd_gather": (C.c_int, [C.POINTER(RoiAlignDesc)] + [_P] * 7),
    "mrcnn_roialign_fwd_h16": (C.c_int, [C.POINTER(RoiAlignDesc), C.c_int] + [_P] * 7),
    "mrcnn_roialign_bwd_h16": (C.c_int, [C.POINTER(RoiAlignDesc), C.c_int, _P, _P, C.c_float] + [_P] * 5),
    "mrcnn_proposal_workspace": (C.c_size_t, [C.POINTER(ProposalDesc)]),
    "mrcnn_proposal_status_offset": (C.c_size_t, [C.POINTER(ProposalDesc), _P, C.POINTER(C.c_size_t)]),
    "mrcnn_proposal_fwd": (C.c_int, [C.POINTER(ProposalDesc)] + [_P] * 8 + [C.c_size_t, _P]),
    "mrcnn_detection_targets": (C.c_int, [C.POINTER(DetTargetDesc)] + [_P] * 12),
    "mrcnn_conv2d_fwd_h16": (C.c_int, [C.POINTER(ConvDesc), C.c_int] + [_P] * 8),
    "mrcnn_conv2d_fwd_h16_res": (C.c_int, [C.POINTER(ConvDesc), C.c_int] + [_P] * 9),
    "mrcnn_conv2d_fwd_h16_supported": (C.c_int, [C.POINTER(ConvDesc), C.c_int]),
    "mrcnn_conv2d_dgrad_ep_h16": (C.c_int, [C.POINTER(ConvDesc), C.c_int, _P, _P, _P, _P, C.POINTER(BwdEpilogueH16), _P]),
    "mrcnn_conv2d_fwd_h16_plan": (C.c_int, [C.POINTER(ConvDesc), C.c_int] + [_P] * 8 + [C.POINTER(BwdEpilogueH16), C.POINTER(H16Plan)]),
    "mrcnn_conv2d_dgrad_ep": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, C.POINTER(BwdEpilogue), _P, C.c_size_t, _P]),
    "mrcnn_conv2d_wgrad_h16_workspace": (C.c_size_t, [C.POINTER(ConvDesc)]),
    "mrcnn_conv2d_wgrad_h16": (C.c_int, [C.POINTER(ConvDesc), C.c_int, _P, _P, _P, _P, C.c_size_t, C.c_int, C.c_float, _P]),
    "mrcnn_conv2d_wgrad_h16_plan": (C.c_int, [C.POINTER(ConvDesc), C.c_int, _P, _P, _P, _P, C.c_size_t, C.POINTER(H16WgradPlan)]),
    "mrcnn_mask_out_fwd_h16": (C.c_int, [C.c_int, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, _P]),
    "mrcnn_mask_out_bwd_h16": (C.c_int, [C.c_int] + [_P] * 8 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "mrcnn_weights_to_h16": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_weights_to_h16_batched": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_cast_to_h16": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "mrcnn_epilogue_bwd_h16": (C.c_int, [C.c_int] + [_P] * 10 + [C.c_int64, C.c_int, C.c_int, C.c_float, _P]),
    "mrcnn_epilogue_bwd_h16_dy": (C.c_int, [C.c_int] + [_P] * 11 + [C.c_int64, C.c_int, C.c_int, C.c_float, _P]),
    "mrcnn_cast_from_h16": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "mrcnn_axpy_from_h16": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_float, _P]),
    "mrcnn_rpn_targets_workspace": (C.c_size_t, [C.POINTER(RpnTargetDesc)]),
    "mrcnn_rpn_targets": (C.c_int, [C.POINTER(RpnTargetDesc)] + [_P] * 7 + [C.c_size_t, _P]),
    "mrcnn_detection_workspace": (C.c_size_t, [C.POINTER(DetectionDesc)]),
    "mrcnn_detection_fwd": (C.c_int, [C.POINTER(DetectionDesc)] + [_P] * 6 + [C.c_size_t, _P]),
    "mrcnn_losses_workspace": (C.c_size_t, [C.POINTER(LossDesc)]),
    "mrcnn_losses_fwd_bwd": (C.c_int, [C.POINTER(LossDesc)] + [_P] * 18 + [C.c_size_t, _P]),
    "mrcnn_losses_fwd_bwd_weighted": (C.c_int, [C.POINTER(LossDesc)] + [_P] * 19 + [C.c_size_t, _P]),
    "mrcnn_grad_prepare": (C.c_int, [_P, _P, C.c_float, _P, C.c_int64, _P, _P]),
    "mrcnn_sumsq": (C.c_int, [_P, C.c_int64, _P, _P]),
    "mrcnn_sgd_momentum": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, C.c_float, _P, C.c_int64, _P]),
    "mrcnn_sgd_momentum_guarded": (C.c_int, [_P, _P, _P, _P, C.c_float, C.c_float, C.c_float, _P, C.c_int64, _P, _P]),
    "mrcnn_winograd_buffer_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mrcnn_winograd_weights": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_gemm_batched_f32": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_winograd_gemm": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_winograd_group_floats": (C.c_size_t, [C.POINTER(WinoGroup), C.c_int, C.c_int]),
    "mrcnn_winograd_input_g": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WinoGroup), _P]),
    "mrcnn_winograd_weights_g": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_winograd_output_g": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WinoGroup), _P]),
    "mrcnn_winograd_chain": (C.c_int, [_P] * 6 + [C.c_int] * 6 + [_P]),
    "mrcnn_winograd_output_bwd_rows": (C.c_int, [C.POINTER(WinoGroup), C.c_int, C.c_int]),
    "mrcnn_winograd_output_bwd_g": (C.c_int, [_P] * 8 + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WinoGroup), _P]),
    "mrcnn_winograd_output_bwd_zmask_g": (C.c_int, [_P] * 8 + [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WinoGroup), _P]),
    "mrcnn_winograd_output_bwd_sums": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    "mrcnn_winograd_bwd_chain": (C.c_int, [_P] * 10 + [C.c_int] * 5 + [_P]),
    "mrcnn_winograd_dy_g": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(WinoGroup), _P]),
    "mrcnn_winograd_dw_g": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_deconv2x2_gemm": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_deconv2x2_mask_gemm": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "mrcnn_allreduce_load": (C.c_int, [C.c_char_p]),
    "mrcnn_allreduce_unique_id": (C.c_int, [_P]),
    "mrcnn_allreduce_init": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int]),
    "mrcnn_allreduce_scratch": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "mrcnn_allreduce_grad": (C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int, _P, C.c_size_t, _P]),
    "mrcnn_allreduce_direct_plan": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P]),
    "mrcnn_allreduce_direct_simulate": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.c_int64, C.c_int64, _P]),
    "mrcnn_allreduce_destroy": (C.c_int, [_P]),
    "mrcnn_allreduce_last_error": (C.c_char_p, []),
    "mrcnn_tuning_set": (C.c_int, [C.c_char_p, C.c_longlong]),
    "mrcnn_hip_version": (C.c_char_p, []),
}

_lib = None
_proxy = None
_tape = None          # a list while a step is being recorded (engine.step_taped), else None
_tape_owner = None    # the thread that opened it: calls from any other thread (loaders, another engine) are not part of the step

# entry points that launch nothing (pure queries / process state): never recorded
# (mrcnn_allreduce_grad is appended by its caller, parallel.RcclComm.reduce: the other mrcnn_allreduce_* calls are set-up)
_NO_RECORD = ("_workspace", "_fwd_plan", "_h16_plan", "_wgrad_plan", "_wgrad_multi_plan", "_tiles_check", "_outline_check", "_draw_check", "_components_check", "_catalog_check", "_overview_check", "_planes_check", "_stats_check", "_gather_check", "_supported", "_status_offset", "_version", "mrcnn_allreduce_", "_scratch", "_floats", "_bwd_rows")


class _LibProxy(object):
    """What lib() hands out: the ctypes library with every launching entry point wrapped so that, while a tape is open,
    the call (function, arguments) is appended to it after it ran.  Replaying the tape issues exactly the same launches
    without re-running the Python that built their arguments (descriptors, workspace look-ups, shape logic): a step's
    ~700-1000 launches cost 14-21 ms of Python when issued from the engine and ~2-3 ms from the tape."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if any(k in name for k in _NO_RECORD):
            f = real
        else:
            def f(*args, _real=real):
                rc = _real(*args)
                t = _tape
                if t is not None and not rc and _tape_owner == threading.get_ident():
                    t.append((_real, args))     # (a refusal -- MRCNN_ERR_UNSUPPORTED: the caller falls back -- launched nothing)
                return rc
        setattr(self, name, f)              # next look-up skips __getattr__
        return f


def tape_begin():
    global _tape, _tape_owner
    assert _tape is None, "a launch tape is already being recorded"
    _tape, _tape_owner = [], threading.get_ident()
    return _tape


def tape_end():
    global _tape, _tape_owner
    t, _tape, _tape_owner = _tape, None, None
    return t


def tape_replay(tape):
    """Issue the recorded calls again.  C entry points return a status (0 = ok); torch stream / event methods return None."""
    for f, a in tape:
        rc = f(*a)
        if rc:
            raise HipPathError("replayed launch %s failed with status %r" % (getattr(f, "__name__", f), rc))


def ev_record(stream):
    """A new event recorded on `stream` (torch objects); part of the tape while one is open."""
    import torch
    ev = torch.cuda.Event()
    ev.record(stream)
    if _tape is not None:
        _tape.append((ev.record, (stream,)))
    return ev


def ev_wait(stream, ev):
    stream.wait_event(ev)
    if _tape is not None:
        _tape.append((stream.wait_event, (ev,)))


def stream_wait(a, b):
    """a waits for everything enqueued on b so far."""
    a.wait_stream(b)
    if _tape is not None:
        _tape.append((a.wait_stream, (b,)))


def exported_symbols():
    """Names every build of the library must export (mirrors include/mrcnn_hip.h)."""
    return sorted(_SIGNATURES)


def lib():
    """Load (once) and return the kernel library (behind the recording proxy); never falls back to anything else."""
    global _lib, _proxy
    if _lib is None:
        why = ""
        if not os.path.exists(LIB_PATH):
            # not built yet (fresh checkout on a box with the toolchain): build once, in-tree; still no fallback.
            # build() takes a file lock and links to a temporary name, so the ranks of a torchrun job that all arrive
            # here together neither compile twice nor load a half-written library.
            try:
                from . import build as _build
                _build.build(verbose=False)
            except Exception as e:
                why = " Building it here failed: %s" % (e,)
        if not os.path.exists(LIB_PATH):
            raise HipPathError(
                "libmrcnn_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'`; there is no CPU fallback for the hot path.%s" % (LIB_PATH, why))
        # torch first: its wheel carries its own HIP runtime, and the streams / device pointers we are handed belong
        # to that one.  Loaded before torch, this library would pull in the system runtime instead and every launch
        # on a torch stream would fail (seen as status -2 from the first kernel when build() and smoke() share a process).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)   # AttributeError here == symbol missing == broken build
            fn.restype = res
            fn.argtypes = args
        _lib = l
        _proxy = _LibProxy(l)
    return _proxy


def check(status, what):
    if status != 0:
        raise HipPathError("%s failed with status %d" % (what, status))


def ptr(t):
    """Device (or host) address of a torch tensor / None."""
    return None if t is None else t.data_ptr()


_dev_index = None


def set_device_index(index):
    """Device whose current stream the launches go to (set by the engine; default: torch's current device
    at the first launch)."""
    global _dev_index
    _dev_index = int(index)


def current_stream():
    """Raw hipStream_t of torch's current stream on the engine's device (the C-level getter: the Python
    `torch.cuda.current_stream()` object costs ~7 us per call, two per launch)."""
    import torch
    global _dev_index
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_dev_index)

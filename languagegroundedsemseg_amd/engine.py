"""ctypes binding of the C-ABI in include/lgs_engine.h (liblgs_engine.so).

This is the only place the product path touches native code, and it FAILS LOUDLY: if the
library is missing or a call returns non-zero a RuntimeError is raised -- there is no CPU or
PyTorch fallback anywhere in this package.
"""
import ctypes
import os

from . import build as _build

LGS_F32, LGS_BF16 = 0, 1
LGS_SUPCON_COS, LGS_SUPCON_L2 = 0, 1     # `distance` of lgs_supcon_forward / lgs_supcon_backward
LGS_AUG_MAX_SCENES = 32                  # scenes per call of the lgs_aug_* / lgs_elastic_* / lgs_color_* entry points
LGS_AUG_F32X3, LGS_AUG_I32X4 = 0, 1      # `form` of lgs_aug_bounds
LGS_INSTSHIFT_MAX_TAIL, LGS_INSTSHIFT_MAX_CAP = 256, 65536     # tail labels / seg_cap of lgs_instance_shift
LGS_PASTE_MAX_SLOTS = 1024               # (scene, instance) slots per call of lgs_paste_instances
LGS_PASTE_SLOT_COLS, LGS_PASTE_SCENE_COLS = 6, 4
LGS_COLOR_AUTOCONTRAST, LGS_COLOR_TRANSLATION, LGS_COLOR_JITTER = 1, 2, 4     # lgs_color_scene.flags
ABI_VERSION = 18     # LGS_ABI_VERSION of include/lgs_engine.h


class PackDesc(ctypes.Structure):
    """lgs_pack_desc (include/lgs_engine.h): layout of one packed weight image"""
    _fields_ = [("weight", ctypes.c_void_p), ("packed", ctypes.c_void_p), ("bytes", ctypes.c_int64), ("total", ctypes.c_int64),
                ("K", ctypes.c_int), ("cin_w", ctypes.c_int), ("cout_w", ctypes.c_int), ("transposed", ctypes.c_int),
                ("mirror", ctypes.c_int), ("g_real", ctypes.c_int), ("o_real", ctypes.c_int), ("ncp", ctypes.c_int),
                ("nbp", ctypes.c_int), ("dtype", ctypes.c_int)]

class ConvPlanView(ctypes.Structure):
    """lgs_conv_plan_view: one view of a synthetic kernel map, by plain integers"""
    _fields_ = [("n_pad", ctypes.c_int64), ("n_in", ctypes.c_int64), ("n_out", ctypes.c_int64), ("KS", ctypes.c_int), ("K", ctypes.c_int),
                ("has_nbr", ctypes.c_int), ("has_tile_k", ctypes.c_int), ("has_out_row", ctypes.c_int)]


class ConvPlanQuery(ctypes.Structure):
    """lgs_conv_plan_query"""
    _fields_ = [("fwd", ConvPlanView), ("bwd", ConvPlanView), ("ks", ctypes.c_int), ("op", ctypes.c_int), ("transposed", ctypes.c_int),
                ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("dtype", ctypes.c_int), ("epilogue", ctypes.c_int)]


class ConvPlanRegion(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("bytes", ctypes.c_int64)]


class ConvPlanInfo(ctypes.Structure):
    """lgs_conv_plan_info: what lgs_debug_conv_plan answers (no GPU needed)"""
    _fields_ = [(n, ctypes.c_int) for n in ("path", "tile_id", "sc", "wb", "tm", "nc", "nb_total", "ncp", "nbp", "gc", "wld")] + \
               [("total", ctypes.c_int64)] + \
               [(n, ctypes.c_int) for n in ("pad_input", "scratch_out", "packed_ext_ok", "split", "bn_rows", "can_accumulate")] + \
               [("grid_x", ctypes.c_int64), ("grid_y", ctypes.c_int), ("grid_z", ctypes.c_int)] + \
               [(n, ConvPlanRegion) for n in ("packed", "padded_in", "scratch", "bias", "partials")] + \
               [("bytes_total", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64),
                ("q_bn_partial_rows", ctypes.c_int), ("q_can_accumulate", ctypes.c_int), ("pack_desc", PackDesc)]


class ConvGatherInstance(ctypes.Structure):
    """lgs_conv_gather_instance: what lgs_debug_conv_gather_instance answers (no GPU needed)"""
    _fields_ = [(n, ctypes.c_int) for n in ("tile_id", "scl", "row1", "bn", "onebuf", "rb", "ncb", "wm", "wn", "sc", "d")] + \
               [("site", ctypes.c_char * 160)]


class WgradPlanQuery(ctypes.Structure):
    """lgs_wgrad_plan_query"""
    _fields_ = [("fwd", ConvPlanView), ("bwd", ConvPlanView)] + \
               [(n, ctypes.c_int) for n in ("ks", "transposed", "cin", "cout", "dtype", "in_row_stride")]


class WgradPlanInfo(ctypes.Structure):
    """lgs_wgrad_plan_info: what lgs_debug_wgrad_plan answers (no GPU needed)"""
    _fields_ = [(n, ctypes.c_int) for n in ("path", "bwd_view", "in_place", "pad_in", "pad_gout", "all_cus", "f32_kernel", "t0", "t1",
                                            "pad_a", "pad_b", "slots")] + \
               [("span", ctypes.c_int64)] + \
               [(n, ctypes.c_int) for n in ("n_ranges", "kpw", "tasks_a", "tasks_b", "cpl", "n_chunks", "xcd_map", "ntile")] + \
               [("grid_x", ctypes.c_int64), ("grid_y", ctypes.c_int), ("grid_z", ctypes.c_int), ("lds_bytes", ctypes.c_int),
                ("reduce_blocks", ctypes.c_int64)] + \
               [(n, ConvPlanRegion) for n in ("partials", "padded_in", "padded_gout", "ww_count", "ww_offset", "ww_total", "ww_pair_in",
                                              "ww_pair_out")] + \
               [("bytes_total", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64), ("supports_stride", ctypes.c_int)]


class NormPlanQuery(ctypes.Structure):
    """lgs_norm_plan_query"""
    _fields_ = [(n, ctypes.c_int) for n in ("direction", "c", "dtype", "conv_partial_rows", "resident_cap")] + [("n", ctypes.c_int64)]


class NormPlanInfo(ctypes.Structure):
    """lgs_norm_plan_info: what lgs_debug_norm_plan answers (no GPU needed)"""
    _fields_ = [("path", ctypes.c_int), ("from_partials", ctypes.c_int), ("reduce_grid", ctypes.c_int), ("rows_per_block", ctypes.c_int64)] + \
               [(n, ctypes.c_int) for n in ("partial_rpb", "fold_rows", "fold_grid", "apply_grid")] + \
               [(n, ConvPlanRegion) for n in ("partials", "sums", "spill")] + \
               [("bytes_total", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)]


class NormPairPlanInfo(ctypes.Structure):
    """lgs_norm_pair_plan_info: what lgs_bn_pair_plan / lgs_debug_norm_pair_plan answer"""
    _fields_ = [(n, ctypes.c_int) for n in ("path", "single_path", "launches", "reduce_grid")] + [("rows_per_block", ctypes.c_int64)] + \
               [(n, ctypes.c_int) for n in ("fold_rows", "fold_grid", "apply_grid")] + \
               [(n, ConvPlanRegion) for n in ("partials_a", "partials_b", "sums_a", "sums_b")] + \
               [("bytes_total", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)]


class InstNormPlanQuery(ctypes.Structure):
    """lgs_instnorm_plan_query"""
    _fields_ = [(n, ctypes.c_int) for n in ("direction", "c", "dtype")] + [(n, ctypes.c_int64) for n in ("n_fine", "n_seg", "n_items")]


class InstNormPlanInfo(ctypes.Structure):
    """lgs_instnorm_plan_info: what lgs_debug_instnorm_plan answers (no GPU needed)"""
    _fields_ = [(n, ctypes.c_int) for n in ("vec", "lanes_log2", "rows_per_apply_block")] + \
               [(n, ctypes.c_int64) for n in ("reduce_grid", "combine_grid", "apply_grid")] + \
               [(n, ConvPlanRegion) for n in ("partials", "sums")] + \
               [("bytes_total", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)]


class SegPlanQuery(ctypes.Structure):
    """lgs_seg_plan_query"""
    _fields_ = [(n, ctypes.c_int) for n in ("family", "c", "dtype", "single_pass", "vec_ok")] + \
               [(n, ctypes.c_int64) for n in ("n_fine", "n_coarse", "n_items")]


class SegPlanInfo(ctypes.Structure):
    """lgs_seg_plan_info: what lgs_debug_seg_plan answers (no GPU needed)"""
    _fields_ = [(n, ctypes.c_int) for n in ("vec", "lanes_log2", "combine_lanes_log2")] + \
               [(n, ctypes.c_int64) for n in ("reduce_grid", "combine_grid", "bcast_grid", "max_bwd_grid")] + \
               [(n, ConvPlanRegion) for n in ("partials", "partial_argmax")] + \
               [("bytes_total", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)]


class KmapRelationQuery(ctypes.Structure):
    """lgs_kmap_relation_query"""
    _fields_ = [(n, ctypes.c_int) for n in ("entry", "ks", "dilation", "link", "tensor_stride", "out_sorted", "in_origin", "out_origin")]


class KmapRelationInfo(ctypes.Structure):
    """lgs_kmap_relation_info: what lgs_debug_kmap_relation answers (no GPU needed)"""
    _fields_ = [(n, ctypes.c_int) for n in ("rc", "relation", "K", "strided", "bwd_mirror", "transposed_ok")] + \
               [("pairs_only", ctypes.c_int * 2), ("served_by_old_entry", ctypes.c_int)]


class ColorScene(ctypes.Structure):
    """lgs_color_scene: one scene's record of lgs_color_augment"""
    _fields_ = [("flags", ctypes.c_int32), ("seed", ctypes.c_int32), ("blend", ctypes.c_float), ("translation", ctypes.c_float * 3),
                ("jitter_std", ctypes.c_float), ("reserved", ctypes.c_float)]


class BnParams(ctypes.Structure):
    """lgs_bn_params"""
    _fields_ = [("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p), ("running_mean", ctypes.c_void_p), ("running_var", ctypes.c_void_p),
                ("num_batches_tracked", ctypes.c_void_p), ("eps", ctypes.c_float), ("momentum", ctypes.c_float)]


class BlockFwd(ctypes.Structure):
    """lgs_block_fwd (include/lgs_engine.h)"""
    _fields_ = [("km3", ctypes.c_void_p), ("km1", ctypes.c_void_p),
                ("dtype", ctypes.c_int), ("relu_final", ctypes.c_int), ("cin", ctypes.c_int), ("planes", ctypes.c_int),
                ("n", ctypes.c_int64), ("x", ctypes.c_void_p),
                ("w1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("wd", ctypes.c_void_p),
                ("pk1", ctypes.c_void_p), ("pk2", ctypes.c_void_p), ("pkd", ctypes.c_void_p),
                ("pm1", ctypes.c_int), ("pm2", ctypes.c_int), ("pmd", ctypes.c_int),
                ("n1", BnParams), ("n2", BnParams), ("nd", BnParams),
                ("o1", ctypes.c_void_p), ("y1", ctypes.c_void_p), ("o2", ctypes.c_void_p), ("od", ctypes.c_void_p),
                ("res", ctypes.c_void_p), ("y2", ctypes.c_void_p),
                ("st1", ctypes.c_void_p), ("st2", ctypes.c_void_p), ("std_", ctypes.c_void_p),
                ("conv_ws", ctypes.c_void_p), ("bn_ws", ctypes.c_void_p)]


class BlockBwd(ctypes.Structure):
    """lgs_block_bwd (include/lgs_engine.h)"""
    _fields_ = [("km3", ctypes.c_void_p), ("km1", ctypes.c_void_p),
                ("dtype", ctypes.c_int), ("relu_final", ctypes.c_int), ("cin", ctypes.c_int), ("planes", ctypes.c_int),
                ("want_gin", ctypes.c_int), ("x_row_stride", ctypes.c_int),
                ("n", ctypes.c_int64), ("dy_row_stride", ctypes.c_int64), ("dy", ctypes.c_void_p),
                ("x", ctypes.c_void_p), ("o1", ctypes.c_void_p), ("y1", ctypes.c_void_p), ("o2", ctypes.c_void_p),
                ("y2", ctypes.c_void_p), ("od", ctypes.c_void_p),
                ("st1", ctypes.c_void_p), ("st2", ctypes.c_void_p), ("std_", ctypes.c_void_p),
                ("w1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("wd", ctypes.c_void_p),
                ("pk1", ctypes.c_void_p), ("pk2", ctypes.c_void_p), ("pkd", ctypes.c_void_p),
                ("pm1", ctypes.c_int), ("pm2", ctypes.c_int), ("pmd", ctypes.c_int),
                ("gamma1", ctypes.c_void_p), ("beta1", ctypes.c_void_p), ("gamma2", ctypes.c_void_p), ("beta2", ctypes.c_void_p),
                ("gammad", ctypes.c_void_p), ("betad", ctypes.c_void_p),
                ("dx2", ctypes.c_void_p), ("dres", ctypes.c_void_p), ("dy1", ctypes.c_void_p), ("dx1", ctypes.c_void_p),
                ("dxd", ctypes.c_void_p), ("gind", ctypes.c_void_p),
                ("gw1", ctypes.c_void_p), ("gw2", ctypes.c_void_p), ("gwd", ctypes.c_void_p),
                ("dgamma1", ctypes.c_void_p), ("dbeta1", ctypes.c_void_p), ("dgamma2", ctypes.c_void_p), ("dbeta2", ctypes.c_void_p),
                ("dgammad", ctypes.c_void_p), ("dbetad", ctypes.c_void_p),
                ("conv_ws", ctypes.c_void_p), ("bn_ws", ctypes.c_void_p),
                ("wgrad_stream", ctypes.c_void_p), ("wgrad_ws", ctypes.c_void_p), ("fork_event", ctypes.c_void_p),
                ("ev_w1", ctypes.c_void_p), ("ev_w2", ctypes.c_void_p), ("ev_wd", ctypes.c_void_p)]


# struct-module packers of lgs_block_fwd / lgs_block_bwd (native alignment), derived from the ctypes layouts above
import struct as _struct
_FORMAT_OF = {ctypes.c_void_p: "P", ctypes.c_int: "i", ctypes.c_int64: "q", ctypes.c_float: "f"}


def struct_format(cls):
    """struct-module format characters of a ctypes.Structure, nested structures flattened member by member"""
    return "".join(_FORMAT_OF[t] if t in _FORMAT_OF else struct_format(t) for _, t in cls._fields_)


BLOCK_FWD_PACK = _struct.Struct("@" + struct_format(BlockFwd))
BLOCK_BWD_PACK = _struct.Struct("@" + struct_format(BlockBwd))
assert BLOCK_FWD_PACK.size == ctypes.sizeof(BlockFwd) and BLOCK_BWD_PACK.size == ctypes.sizeof(BlockBwd)

_lib = None

# every symbol include/lgs_engine.h declares; tests check the built library exports all of them
EXPORTS = [
    "lgs_abi_version", "lgs_last_error",
    "lgs_tuning_set", "lgs_tuning_get", "lgs_tuning_describe", "lgs_debug_dispatch_counts", "lgs_debug_conv_plan", "lgs_debug_conv_gather_instance",
    "lgs_debug_conv_gather_residency", "lgs_debug_wgrad_plan",
    "lgs_debug_norm_plan", "lgs_debug_instnorm_plan", "lgs_debug_seg_plan", "lgs_debug_kmap_relation",
    "lgs_manager_create", "lgs_manager_destroy", "lgs_manager_insert", "lgs_manager_stride2", "lgs_manager_check",
    "lgs_manager_parent_of", "lgs_manager_map_size", "lgs_manager_get_coords", "lgs_manager_nearest", "lgs_manager_kernel_map",
    "lgs_manager_kernel_map_ex",
    "lgs_kmap_export", "lgs_debug_kmap_tables",
    "lgs_manager_origin", "lgs_manager_segment_map", "lgs_segmap_size", "lgs_seg_workspace_bytes", "lgs_seg_reduce",
    "lgs_seg_broadcast", "lgs_seg_max_backward",
    "lgs_in_workspace_bytes", "lgs_in_forward", "lgs_in_backward",
    "lgs_conv_workspace_bytes", "lgs_conv_bn_partial_rows", "lgs_conv_forward", "lgs_conv_dgrad", "lgs_conv_wgrad",
    "lgs_conv_wgrad_supports_stride", "lgs_conv_dgrad_can_accumulate", "lgs_conv_dgrad_accumulate",
    "lgs_conv_pack_desc", "lgs_pack_weights_batch",
    "lgs_bn_workspace_bytes", "lgs_bn_forward", "lgs_bn_backward",
    "lgs_bn_pair_workspace_bytes", "lgs_bn_pair_plan", "lgs_debug_norm_pair_plan", "lgs_bn_forward_pair", "lgs_bn_backward_pair",
    "lgs_block_workspace_bytes", "lgs_block_forward", "lgs_block_backward",
    "lgs_bn_stats", "lgs_bn_sync_combine", "lgs_bn_apply", "lgs_bn_backward_reduce", "lgs_bn_backward_apply",
    "lgs_clip_similarity", "lgs_clip_workspace_bytes",
    "lgs_clip_loss_workspace_bytes", "lgs_clip_loss_forward", "lgs_clip_loss_backward",
    "lgs_clip_anchor_grad_workspace_bytes", "lgs_clip_loss_backward_anchors",
    "lgs_ce_forward_backward", "lgs_ce_forward_backward_rows", "lgs_split_stats",
    "lgs_ce_count_valid", "lgs_focal_forward_backward", "lgs_ce_weight_sum", "lgs_seg_metrics",
    "lgs_ap_workspace_bytes", "lgs_average_precision",
    "lgs_inst_overlap_workspace_bytes", "lgs_inst_overlap",
    "lgs_instance_info_workspace_bytes", "lgs_instance_info", "lgs_offset_loss_forward", "lgs_offset_loss_backward",
    "lgs_supcon_sample", "lgs_supcon_forward", "lgs_supcon_backward",
    "lgs_comm_unique_id", "lgs_comm_create", "lgs_comm_create_ipc", "lgs_comm_ipc_open", "lgs_comm_destroy", "lgs_comm_world", "lgs_bn_sync_workspace_bytes",
    "lgs_bn_forward_sync", "lgs_bn_backward_sync",
    "lgs_voxelize", "lgs_label_vote", "lgs_cluster_workspace_bytes", "lgs_cluster", "lgs_sgd_step",
    "lgs_aug_bounds", "lgs_elastic_workspace_bytes", "lgs_elastic_distort", "lgs_voxelize_batched", "lgs_coords_flip_shift",
    "lgs_color_augment", "lgs_aug_status", "lgs_debug_philox",
    "lgs_paste_workspace_bytes", "lgs_paste_instances",
    "lgs_dropout_workspace_bytes", "lgs_dropout_select",
    "lgs_instance_shift_workspace_bytes", "lgs_instance_shift",
    "lgs_fps_workspace_bytes", "lgs_fps_segments",
]


def lib_path():
    return _build.LIB_PATH


def lib():
    """Load (once) the engine. Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "liblgs_engine.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or languagegroundedsemseg_amd.build.build()). There is no fallback path." % path)
    L = ctypes.CDLL(path)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    pi, pi64, pvp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_void_p)
    cf = ctypes.c_float
    L.lgs_abi_version.restype = ci
    L.lgs_abi_version.argtypes = []
    L.lgs_last_error.restype = ctypes.c_char_p
    L.lgs_last_error.argtypes = []
    sig = {
        "lgs_block_forward": [vp, vp],        # (const lgs_block_fwd *, stream): the host packs the struct with struct.pack_into
        "lgs_block_backward": [vp, vp],
        "lgs_tuning_set": [ctypes.c_char_p, i64],
        "lgs_tuning_get": [ctypes.c_char_p, pi64],
        "lgs_manager_create": [ci, pvp],
        "lgs_manager_destroy": [vp],
        "lgs_manager_insert": [vp, vp, i64, vp, vp, vp, pi, pi64],
        "lgs_manager_stride2": [vp, ci, vp, pi, pi64],
        "lgs_manager_check": [vp, pi],
        "lgs_manager_parent_of": [vp, ci, pi],
        "lgs_manager_map_size": [vp, ci, pi64, pi],
        "lgs_manager_get_coords": [vp, ci, vp, vp],
        "lgs_manager_nearest": [vp, ci, vp, i64, vp, ci, ci, ctypes.POINTER(ctypes.c_double), ctypes.c_double, vp, vp, vp],
        "lgs_manager_kernel_map": [vp, ci, ci, ci, vp, pvp],
        "lgs_manager_kernel_map_ex": [vp, ci, ci, ci, ci, vp, pvp],
        "lgs_kmap_export": [vp, vp, vp, vp, vp, pi64],
        "lgs_debug_kmap_tables": [vp, ci, vp, vp, vp, vp, pi64, pi, pi],
        "lgs_manager_origin": [vp, vp, pi, pi64],
        "lgs_manager_segment_map": [vp, ci, ci, vp, pvp],
        "lgs_segmap_size": [vp, pi64, pi64],
        "lgs_seg_reduce": [vp, ci, vp, vp, i64, ci, vp, vp, ci, vp, vp],
        "lgs_seg_broadcast": [vp, ci, vp, ci, vp, i64, vp, i64, ci, vp],
        "lgs_seg_max_backward": [vp, vp, vp, ci, vp, ci, vp],
        "lgs_in_forward": [vp, vp, ci, vp, vp, cf, vp, vp, ci, vp, vp],
        "lgs_in_backward": [vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp],
        "lgs_conv_forward": [vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, ci, ci, vp],
        "lgs_conv_pack_desc": [vp, ci, ci, ci, ci, ci, ctypes.POINTER(PackDesc)],
        "lgs_pack_weights_batch": [vp, ci, i64, vp],
        "lgs_debug_conv_plan": [ctypes.POINTER(ConvPlanQuery), ctypes.POINTER(ConvPlanInfo)],
        "lgs_debug_conv_gather_instance": [ctypes.POINTER(ConvPlanQuery), ci, ctypes.POINTER(ConvGatherInstance)],
        "lgs_debug_conv_gather_residency": [ci, ci, ci, pi],
        "lgs_debug_wgrad_plan": [ctypes.POINTER(WgradPlanQuery), ctypes.POINTER(WgradPlanInfo)],
        "lgs_debug_norm_plan": [ctypes.POINTER(NormPlanQuery), ctypes.POINTER(NormPlanInfo)],
        "lgs_debug_instnorm_plan": [ctypes.POINTER(InstNormPlanQuery), ctypes.POINTER(InstNormPlanInfo)],
        "lgs_debug_seg_plan": [ctypes.POINTER(SegPlanQuery), ctypes.POINTER(SegPlanInfo)],
        "lgs_debug_kmap_relation": [ctypes.POINTER(KmapRelationQuery), ctypes.POINTER(KmapRelationInfo)],
        "lgs_conv_bn_partial_rows": [vp, ci, ci, ci],
        "lgs_conv_dgrad": [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, ci, vp],
        "lgs_sgd_step": [vp, vp, vp, vp, i64, cf, cf, cf, cf, ci, vp],
        "lgs_cluster": [vp, vp, vp, i64, cf, ci, vp, ctypes.POINTER(ctypes.c_int32), vp, vp],
        "lgs_voxelize": [vp, i64, ctypes.POINTER(ctypes.c_double), ci, vp, vp],
        "lgs_label_vote": [vp, i64, vp, vp, i64, i64, vp, vp],
        "lgs_conv_wgrad": [vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp],
        "lgs_conv_wgrad_supports_stride": [vp, ci, ci, ci, ci, ci],
        "lgs_conv_dgrad_can_accumulate": [vp, ci, ci, ci, ci],
        "lgs_conv_dgrad_accumulate": [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, ci, vp],
        "lgs_bn_forward": [vp, i64, ci, vp, vp, cf, cf, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, ci, vp, i64, vp],
        "lgs_bn_backward": [vp, vp, vp, i64, i64, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, i64, vp],
        "lgs_bn_pair_plan": [ci, i64, ci, ci, ctypes.POINTER(NormPairPlanInfo)],
        "lgs_debug_norm_pair_plan": [ctypes.POINTER(NormPlanQuery), ctypes.POINTER(NormPairPlanInfo)],
        "lgs_bn_forward_pair": [vp, ctypes.POINTER(BnParams), vp, vp, ctypes.POINTER(BnParams), vp, i64, ci, ci, vp, i64, vp, ci, vp, vp],
        "lgs_bn_backward_pair": [vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, i64, i64, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, i64, vp],
        "lgs_bn_stats": [vp, i64, ci, vp, ci, vp, vp, ci, vp, vp],
        "lgs_bn_apply": [vp, i64, ci, vp, vp, vp, vp, ci, vp, ci, i64, vp],
        "lgs_bn_backward_reduce": [vp, vp, vp, i64, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, i64, i64, vp],
        "lgs_bn_sync_combine": [vp, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp],
        "lgs_bn_backward_apply": [vp, vp, vp, i64, ci, vp, vp, vp, vp, cf, vp, ci, vp, vp, ci, i64, i64, vp],
        "lgs_clip_similarity": [vp, i64, ci, vp, ci, vp, vp, ci, vp, vp],
        "lgs_ce_forward_backward": [vp, i64, ci, vp, i64, vp, vp, vp, ci, vp],
        "lgs_ce_forward_backward_rows": [vp, i64, ci, vp, i64, vp, vp, vp, vp, ci, vp],
        "lgs_split_stats": [vp, vp, i64, vp, ci, i64, vp, ci, vp],
        "lgs_ce_count_valid": [vp, i64, ci, i64, vp, vp],
        "lgs_focal_forward_backward": [vp, i64, ci, vp, i64, vp, cf, vp, vp, vp, vp, ci, vp],
        "lgs_ce_weight_sum": [vp, i64, ci, i64, vp, vp, ci, vp],
        "lgs_seg_metrics": [vp, i64, ci, vp, i64, vp, vp, vp, ci, vp],
        "lgs_average_precision": [vp, i64, ci, vp, i64, ci, vp, ci, vp, vp],
        "lgs_inst_overlap": [vp, vp, vp, ci, i64, vp, i64, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp],
        "lgs_instance_info": [vp, vp, vp, i64, pi64, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "lgs_offset_loss_forward": [vp, vp, vp, vp, i64, cf, ci, vp, ci, vp, vp, vp, vp],
        "lgs_offset_loss_backward": [vp, vp, vp, vp, i64, cf, ci, vp, vp, vp, vp, vp],
        "lgs_supcon_sample": [vp, i64, ci, i64, vp, vp, vp, vp, vp, ci, ci, i64, vp, vp, vp],
        "lgs_supcon_forward": [vp, i64, ci, vp, vp, ci, vp, ci, i64, ci, ci, vp, vp, vp, vp, ci, vp],
        "lgs_supcon_backward": [vp, i64, ci, vp, vp, ci, vp, ci, i64, ci, ci, vp, vp, vp, vp, vp, ci, vp],
        "lgs_aug_bounds": [vp, i64, ci, vp, ci, vp, vp],
        "lgs_elastic_distort": [vp, i64, vp, ci, vp, ctypes.c_double, ctypes.c_double, i64, vp, ci, ci, vp, i64, vp, vp, vp, vp],
        "lgs_voxelize_batched": [vp, i64, vp, ci, ctypes.POINTER(ctypes.c_double), ci, vp, vp],
        "lgs_coords_flip_shift": [vp, i64, vp, ci, vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), vp],
        "lgs_color_augment": [vp, i64, vp, ci, vp, ctypes.POINTER(ColorScene), cf, ci, i64, vp, vp],
        "lgs_aug_status": [vp, pi, vp],
        "lgs_debug_philox": [vp, i64, i64, vp, vp],
        "lgs_paste_instances": [vp, vp, vp, i64, ci, vp, vp, vp, i64, vp, vp, ci, i64, vp, vp, vp, i64, vp, ci, i64, i64, vp, vp, vp, vp,
                                vp, vp, vp],
        "lgs_dropout_select": [vp, i64, ci, ci, ctypes.c_double, i64, ctypes.POINTER(ctypes.c_int32), vp, vp, vp, vp, vp, vp],
        "lgs_instance_shift": [vp, vp, vp, vp, i64, vp, ci, vp, pi64, ci, ctypes.c_double, ctypes.c_double, i64, ctypes.POINTER(ctypes.c_int32),
                               vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp],
        "lgs_fps_segments": [vp, i64, vp, vp, i64, vp, ci, ctypes.c_double, ci, ci, vp, vp, vp, vp, vp],
        "lgs_comm_unique_id": [vp],
        "lgs_comm_create": [vp, ci, ci, ci, ctypes.POINTER(vp)],
        "lgs_comm_create_ipc": [ci, ci, ci, ctypes.POINTER(vp), vp],
        "lgs_comm_ipc_open": [vp, vp],
        "lgs_comm_destroy": [vp],
        "lgs_comm_world": [vp],
        "lgs_bn_forward_sync": [vp, vp, i64, ci, vp, vp, cf, cf, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, i64, vp],
        "lgs_bn_backward_sync": [vp, vp, vp, vp, i64, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, i64, i64, vp],
        "lgs_clip_loss_forward": [vp, i64, ci, vp, ci, vp, vp, ci, i64, vp, vp, vp, vp, vp, vp, ci, vp, vp],
        "lgs_clip_loss_backward": [vp, i64, ci, vp, ci, vp, vp, ci, i64, vp, vp, vp, vp, vp, vp, ci, vp],
        "lgs_clip_loss_backward_anchors": [vp, i64, ci, ci, vp, vp, ci, i64, vp, vp, vp, vp, ci, vp, vp],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.restype = ci
        f.argtypes = args
    L.lgs_tuning_describe.restype = i64
    L.lgs_tuning_describe.argtypes = [ctypes.c_char_p, i64]
    L.lgs_debug_dispatch_counts.restype = i64
    L.lgs_debug_dispatch_counts.argtypes = [ctypes.c_char_p, i64, ci]
    L.lgs_block_workspace_bytes.restype = i64
    L.lgs_block_workspace_bytes.argtypes = [vp, vp, ci, ci, ci]
    L.lgs_seg_workspace_bytes.restype = i64
    L.lgs_seg_workspace_bytes.argtypes = [vp, ci]
    L.lgs_in_workspace_bytes.restype = i64
    L.lgs_in_workspace_bytes.argtypes = [vp, ci]
    L.lgs_elastic_workspace_bytes.restype = i64
    L.lgs_elastic_workspace_bytes.argtypes = [ci, i64]
    L.lgs_paste_workspace_bytes.restype = i64
    L.lgs_paste_workspace_bytes.argtypes = [ci, ci, i64, i64]
    L.lgs_dropout_workspace_bytes.restype = i64
    L.lgs_dropout_workspace_bytes.argtypes = [i64, ci]
    L.lgs_instance_shift_workspace_bytes.restype = i64
    L.lgs_instance_shift_workspace_bytes.argtypes = [i64, ci, ci]
    L.lgs_fps_workspace_bytes.restype = i64
    L.lgs_fps_workspace_bytes.argtypes = [i64, i64]
    L.lgs_cluster_workspace_bytes.restype = i64
    L.lgs_cluster_workspace_bytes.argtypes = [i64]
    L.lgs_conv_workspace_bytes.restype = i64
    L.lgs_conv_workspace_bytes.argtypes = [vp, ci, ci, ci, ci]
    L.lgs_bn_workspace_bytes.restype = i64
    L.lgs_bn_workspace_bytes.argtypes = [i64, ci]
    L.lgs_bn_pair_workspace_bytes.restype = i64
    L.lgs_bn_pair_workspace_bytes.argtypes = [i64, ci]
    L.lgs_bn_sync_workspace_bytes.restype = i64
    L.lgs_bn_sync_workspace_bytes.argtypes = [i64, ci, ci]
    L.lgs_ap_workspace_bytes.restype = i64
    L.lgs_ap_workspace_bytes.argtypes = [i64, ci]
    L.lgs_inst_overlap_workspace_bytes.restype = i64
    L.lgs_inst_overlap_workspace_bytes.argtypes = [i64, i64, ci, ci]
    L.lgs_instance_info_workspace_bytes.restype = i64
    L.lgs_instance_info_workspace_bytes.argtypes = [i64, ci]
    L.lgs_clip_workspace_bytes.restype = i64
    L.lgs_clip_workspace_bytes.argtypes = [ci, ci, ci]
    L.lgs_clip_loss_workspace_bytes.restype = i64
    L.lgs_clip_loss_workspace_bytes.argtypes = [ci, ci, ci]
    L.lgs_clip_anchor_grad_workspace_bytes.restype = i64
    L.lgs_clip_anchor_grad_workspace_bytes.argtypes = [i64, ci, ci, ci]
    if L.lgs_abi_version() != ABI_VERSION:
        raise RuntimeError("liblgs_engine.so ABI version mismatch")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().lgs_last_error()
        raise RuntimeError("lgs_engine: " + (msg.decode(errors="replace") if msg else "error %d" % rc))


# ---- tuning table / dispatch counters (include/lgs_engine.h, csrc/lgs_tuning.hip)
TUNING_EPOCH = 0      # bumped by every tuning_set(): host-side caches of knob-dependent answers (pack descriptors) key on it


def tuning_set(name, value):
    global TUNING_EPOCH
    check(lib().lgs_tuning_set(name.encode(), int(value)))
    TUNING_EPOCH += 1


def tuning_get(name):
    v = ctypes.c_int64()
    check(lib().lgs_tuning_get(name.encode(), ctypes.byref(v)))
    return int(v.value)


class tuning:
    """with engine.tuning(WW_MIN_ROWS=0): ...   -- set knobs for a block (tests), restore afterwards"""

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        self.prev = {k: tuning_get(k) for k in self.knobs}
        for k, v in self.knobs.items():
            tuning_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            tuning_set(k, v)


def tuning_table():
    """-> [(name, default, value, doc)]"""
    L = lib()
    n = L.lgs_tuning_describe(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    L.lgs_tuning_describe(buf, n)
    rows = []
    for line in buf.value.decode().splitlines():
        name, d, v, doc = line.split("\t", 3)
        rows.append((name, int(d), int(v), doc))
    return rows


def dispatch_counts(reset=False):
    """-> {launch site: launches since the last reset}"""
    L = lib()
    cap = 1 << 19
    buf = ctypes.create_string_buffer(cap)
    L.lgs_debug_dispatch_counts(buf, cap, 1 if reset else 0)
    out = {}
    for line in buf.value.decode().splitlines():
        c, name = line.split("\t", 1)
        out[name] = int(c)
    return out

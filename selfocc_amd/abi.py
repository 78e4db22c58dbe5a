"""ctypes mirror of include/selfocc_hip.h (the C ABI of libselfocc_hip.so).

Field order and types must match the header exactly; tests/test_abi.py checks
``sizeof`` of every struct against the sizes the compiled library reports through
its exported symbols being callable with these layouts.
"""
import ctypes as C

ABI_VERSION = 35

# enums ---------------------------------------------------------------------------
RAYS_EXPLICIT, RAYS_PIXEL_GRID = 0, 1
SAMPLE_AT_START, SAMPLE_AT_MID = 0, 1
BKGD_NONE, BKGD_CONST, BKGD_PER_RAY = 0, 1, 2
JITTER_NONE, JITTER_SINGLE, JITTER_PER_BIN, JITTER_EDGES = 0, 1, 2, 3
FLAG_DEPTH_DIV_NORM, FLAG_CLAMP_RGB, FLAG_EXACT, FLAG_NO_SKIP, FLAG_NO_FACE_SAFE, FLAG_NO_AHEAD, FLAG_RAY_PER_LANE = 1, 2, 4, 8, 16, 32, 64
MSDA_PLAIN, MSDA_FUSED, MSDA_CROSS = 0, 1, 2
# selfocc_msda_plan: indices into its SO_MSDA_PLAN_INTS outputs
MSDA_PLAN_LOG2_GROUP, MSDA_PLAN_BANDED, MSDA_PLAN_COUNT_HERE, MSDA_PLAN_BIN_VIS, MSDA_PLAN_BANDS, MSDA_PLAN_ROWS, MSDA_PLAN_INTS = 0, 1, 2, 3, 4, 12, 20
VALUE_PIXEL_MAJOR, VALUE_HEAD_MAJOR = 0, 1
DTYPE_F32, DTYPE_BF16 = 0, 1
LINEAR_RELU, LINEAR_BF16X1 = 1, 2
LBL_F32, LBL_U8, LBL_I32, LBL_I64 = 0, 1, 2, 3
MAP_LINEAR, MAP_UPSCALE = 0, 1
SH_RELU, SH_SIGMOID = 0, 1
GRAD_ANALYTIC, GRAD_NUMERICAL = 0, 1

_f, _i, _p = C.c_float, C.c_int32, C.c_void_p


class SoAxis(C.Structure):
    _fields_ = [("size0", _f), ("size1", _f), ("range0", _f), ("range1", _f),
                ("off0", _f), ("off1", _f), ("start", _f), ("tot_len", _i)]


class SoUpscaleAxis(C.Structure):
    _fields_ = [("unit", _f), ("inc", _f), ("c", _f), ("c2", _f)]


class SoMapping(C.Structure):
    _fields_ = [("h", SoAxis), ("w", SoAxis), ("d", SoAxis),
                ("kind", _i), ("_pad", _i * 3), ("uh", SoUpscaleAxis), ("uw", SoUpscaleAxis), ("ud", SoUpscaleAxis)]


class SoRenderArgs(C.Structure):
    _fields_ = [
        ("map", SoMapping),
        ("sdf_vol", _p), ("feat_vol", _p),
        ("feat_dtype", _i), ("feat_stride", _i), ("n_rgb", _i), ("n_sem", _i),
        ("ray_mode", _i), ("n_rays", _i),
        ("origins", _p), ("dirs", _p), ("dir_norm", _p), ("img2lidar", _p),
        ("n_cams", _i), ("nx", _i), ("ny", _i),
        ("sx", _f), ("sy", _f), ("ox", _f), ("oy", _f),
        ("aabb", _f * 6), ("near_plane", _f),
        ("n_samples", _i), ("sample_pos", _i), ("jitter_mode", _i),
        ("t_rand", _p),
        ("inv_s", _f),
        ("bkgd_mode", _i), ("bkgd", _f * 3),
        ("bkgd_rays", _p),
        ("flags", _i),
        ("depth", _p), ("acc", _p), ("rgb", _p), ("sem", _p), ("max_depth", _p),
        ("nears", _p), ("fars", _p),
        ("weights", _p), ("ts", _p), ("deltas", _p), ("sdf", _p), ("grad", _p),
        ("sdf_brick", _p),
        ("inv_s_dev", _p),
        ("sh_deg", _i), ("sh_act", _i),
    ]


class SoRenderBwdArgs(C.Structure):
    _fields_ = [
        ("fwd", SoRenderArgs),
        ("g_depth", _p), ("g_acc", _p), ("g_rgb", _p), ("g_sem", _p),
        ("g_weights", _p), ("g_sdf", _p), ("g_grad", _p),
        ("g_sdf_vol", _p), ("g_feat_vol", _p), ("g_inv_s", _p),
        ("scatter_ws", _p), ("scatter_ws_bytes", C.c_uint64),
    ]


class SoRenderMedianArgs(C.Structure):
    _fields_ = [("fwd", SoRenderArgs), ("median_depth", _p), ("median_index", _p)]


class SoRenderNormalArgs(C.Structure):
    _fields_ = [("fwd", SoRenderArgs), ("normal_vis", _p)]


class SoRenderUpsampleArgs(C.Structure):
    _fields_ = [("fwd", SoRenderArgs), ("n_importance", _i), ("n_steps", _i), ("base_variance", _f),
                ("u_rand", _p), ("edges", _p)]


class SoMsdaArgs(C.Structure):
    _fields_ = [
        ("form", _i), ("bs", _i), ("nv", _i), ("nq", _i), ("heads", _i), ("d", _i), ("L", _i), ("P", _i),
        ("value_layout", _i), ("value_dtype", _i), ("value_stride", _i), ("ref_kind", _i),
        ("ol_stride", _i), ("g_value_stride", _i),
        ("value", _p), ("shapes", _p), ("starts", _p), ("host_shapes", _p),
        ("loc", _p), ("attw", _p), ("ref", _p), ("vis", _p), ("off_raw", _p), ("logits", _p),
        ("out", _p),
        ("g_out", _p), ("g_value", _p), ("g_loc", _p), ("g_attw", _p), ("g_off", _p), ("g_logits", _p),
        ("workspace", _p), ("workspace_bytes", C.c_uint64),
    ]


class SoQueryArgs(C.Structure):
    _fields_ = [
        ("map", SoMapping),
        ("sdf_vol", _p), ("feat_vol", _p),
        ("feat_dtype", _i), ("feat_stride", _i), ("n_rgb", _i), ("n_sem", _i),
        ("xyz", _p), ("n", _i),
        ("sdf", _p), ("sem_logits", _p), ("sem_argmax", _p),
    ]


class SoFieldGradArgs(C.Structure):
    _fields_ = [("q", SoQueryArgs), ("grad", _p), ("mode", _i), ("delta", _f)]


class SoOccArgs(C.Structure):
    _fields_ = [
        ("grid", _p), ("logits", _p),
        ("H", _i), ("W", _i), ("D", _i), ("C", _i),
        ("coords", _p),
        ("n0", _i), ("n1", _i), ("n2", _i),
        ("crop", _i * 6),
        ("thresh", _f), ("density", _i),
        ("lut", _p),
        ("sampled", _p), ("occ", _p), ("sem", _p),
    ]


class SoReprojArgs(C.Structure):
    _fields_ = [
        ("weights", _p), ("ts", _p), ("deltas", _p),
        ("pix", _p), ("curr_rgb", _p),
        ("T_prev", _p), ("T_next", _p),
        ("img_prev", _p), ("img_next", _p),
        ("R", _i), ("S", _i), ("Hi", _i), ("Wi", _i),
        ("img_h", _f), ("img_w", _f),
        ("l1", _p), ("rgb_combine", _p), ("any_valid", _p),
        ("wnorm", _p),
    ]


class SoReprojCArgs(C.Structure):
    _fields_ = [
        ("weights", _p), ("ts", _p), ("deltas", _p),
        ("pix", _p), ("curr", _p),
        ("T_prev", _p), ("T_next", _p),
        ("img_prev", _p), ("img_next", _p),
        ("R", _i), ("S", _i), ("Hi", _i), ("Wi", _i), ("C", _i), ("img_stride", _i),
        ("img_h", _f), ("img_w", _f),
        ("l1", _p), ("combine", _p), ("any_valid", _p),
        ("wnorm", _p),
    ]


class SoReprojPickArgs(C.Structure):
    _fields_ = [
        ("weights", _p), ("ts", _p), ("deltas", _p),
        ("values", _p),
        ("pix", _p),
        ("T_prev", _p), ("T_next", _p),
        ("R", _i), ("S", _i),
        ("img_h", _f), ("img_w", _f),
        ("pick_index", _p), ("pick_value", _p),
    ]


class SoDepthMetricArgs(C.Structure):
    _fields_ = [
        ("pred", _p), ("loc", _p), ("gt", _p), ("mask", _p),
        ("N", _i), ("h", _i), ("w", _i), ("n", _i),
        ("n_types", _i), ("raw_row", _i), ("median_row", _i), ("_pad", _i),
        ("abs_rel", _p), ("sq_rel", _p), ("rmse", _p), ("rmse_log", _p),
        ("a1", _p), ("a2", _p), ("a3", _p), ("scaling", _p),
        ("count", _p), ("errors", _p), ("sampled", _p), ("medians", _p),
        ("ws", _p), ("ws_bytes", C.c_uint64),
    ]


class SoSscMetricArgs(C.Structure):
    _fields_ = [
        ("H", _i), ("W", _i), ("D", _i), ("pred_dtype", _i),
        ("pred", _p), ("sdf", _p),
        ("thresh", _f), ("crop", _i * 6),
        ("gt_dtype", _i), ("gt", _p),
        ("flip_gt", _i), ("iou_empty", _i), ("iou_ignore", _i), ("n_classes", _i), ("ssc_keep255", _i), ("n_lut", _i),
        ("nonempty", _p), ("nonsurface", _p), ("iou_mask", _p),
        ("sem", _p), ("lut", _p), ("miou_map", _p),
        ("n_miou", _i), ("miou_empty", _i),
        ("coords", _p), ("n_coords", C.c_int64),
        ("iou", _p), ("completion", _p), ("semantic", _p), ("miou", _p), ("bad", _p),
        ("d_range", _p), ("occ", _p), ("ws", _p),
    ]


class SoRowGroups(C.Structure):
    """so_row_groups: passed BY VALUE; group g owns rows row_start[g] .. row_start[g + 1] - 1"""
    _fields_ = [("n_groups", _i), ("row_start", C.c_int64 * 9)]

    @classmethod
    def from_sizes(cls, sizes):
        g = cls()
        g.n_groups = len(sizes)
        if 1 <= len(sizes) <= 8:
            o = 0
            for k, n in enumerate(sizes):
                o += int(n)
                g.row_start[k + 1] = o
        return g


# every symbol include/selfocc_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "selfocc_abi_version": (C.c_int, []),
    "selfocc_last_error": (C.c_char_p, []),
    "selfocc_meter2grid": (C.c_int, [C.POINTER(SoMapping), _p, _i, _i, _p, _p]),
    "selfocc_render_fwd": (C.c_int, [C.POINTER(SoRenderArgs), _p]),
    "selfocc_render_bwd": (C.c_int, [C.POINTER(SoRenderBwdArgs), _p]),
    "selfocc_render_bwd_ws_bytes": (C.c_size_t, [C.POINTER(SoRenderBwdArgs)]),
    "selfocc_render_median": (C.c_int, [C.POINTER(SoRenderMedianArgs), _p]),
    "selfocc_render_normal": (C.c_int, [C.POINTER(SoRenderNormalArgs), _p]),
    "selfocc_render_upsample": (C.c_int, [C.POINTER(SoRenderUpsampleArgs), _p]),
    "selfocc_msda_fwd": (C.c_int, [C.POINTER(SoMsdaArgs), _p]),
    "selfocc_msda_bwd": (C.c_int, [C.POINTER(SoMsdaArgs), _p]),
    "selfocc_msda_ws_bytes": (C.c_size_t, [C.POINTER(SoMsdaArgs)]),
    "selfocc_msda_banded_supported": (C.c_int, [C.POINTER(SoMsdaArgs)]),
    "selfocc_msda_plan": (C.c_int, [C.POINTER(SoMsdaArgs), C.POINTER(C.c_int32)]),
    "selfocc_field_query": (C.c_int, [C.POINTER(SoQueryArgs), _p]),
    "selfocc_field_query_bwd": (C.c_int, [C.POINTER(SoQueryArgs), _p, _p, _p, _p, _p]),
    "selfocc_field_grad": (C.c_int, [C.POINTER(SoFieldGradArgs), _p]),
    "selfocc_field_grad_bwd": (C.c_int, [C.POINTER(SoFieldGradArgs), _p, _p, _p, _p]),
    "selfocc_field_volume_bwd": (C.c_int, [_p] * 3 + [_i] * 4 + [_p, _p, _p, _i, _p, _p, _i] + [_p] * 7 + [_p]),
    "selfocc_field_volume_fwd": (C.c_int, [_p] * 3 + [_i] * 4 + [_p, _p, _i, _p, _p, _i, _p, _p, _i, _i, _p]),
    "selfocc_occ_resample": (C.c_int, [C.POINTER(SoOccArgs), _p]),
    "selfocc_iou_counts": (C.c_int, [_p, _p, _p, C.c_int64, _p, _i, _i, _p, _p]),
    "selfocc_layernorm_fwd": (C.c_int, [_p] * 6 + [C.c_int64, _i, C.c_float, _p]),
    "selfocc_layernorm_bwd_workspace": (C.c_size_t, [C.c_int64, _i]),
    "selfocc_layernorm_bwd": (C.c_int, [_p] * 8 + [C.c_int64, _i, _p, C.c_size_t, _p]),
    "selfocc_layernorm_grouped_supported": (C.c_int, [C.c_int64, _i, SoRowGroups]),
    "selfocc_layernorm_fwd_grouped": (C.c_int, [_p] * 6 + [C.c_int64, _i, C.c_float, SoRowGroups, _p]),
    "selfocc_layernorm_bwd_grouped_workspace": (C.c_size_t, [C.c_int64, _i, SoRowGroups]),
    "selfocc_layernorm_bwd_grouped": (C.c_int, [_p] * 8 + [C.c_int64, _i, SoRowGroups, _p, C.c_size_t, _p]),
    "selfocc_linear_fwd_grouped_supported": (C.c_int, [C.c_int64, _i, _i, SoRowGroups]),
    "selfocc_linear_fwd_grouped": (C.c_int, [_p] * 4 + [_i, _p, _p, C.c_float, _p, _i, _p, _p, _p, C.c_int64, _i, _i, C.c_uint32,
                                             SoRowGroups, C.c_int64, C.c_int64, _p]),
    "selfocc_linear_dgrad_grouped_supported": (C.c_int, [C.c_int64, _i, _i, SoRowGroups]),
    "selfocc_linear_dgrad_grouped_workspace": (C.c_size_t, [_i, _i, SoRowGroups]),
    "selfocc_linear_dgrad_grouped": (C.c_int, [_p] * 3 + [C.c_int64, _i, _i, SoRowGroups, _p, C.c_int64, _p]),
    "selfocc_linear_wgrad_grouped_supported": (C.c_int, [C.c_int64, _i, _i, SoRowGroups]),
    "selfocc_linear_wgrad_grouped_workspace": (C.c_size_t, [C.c_int64, _i, _i, SoRowGroups]),
    "selfocc_linear_wgrad_grouped": (C.c_int, [_p] * 4 + [C.c_int64, _i, _i, SoRowGroups, _p, C.c_size_t, _p]),
    "selfocc_flatten_feats": (C.c_int, [_p, _p, _i, _i, _i, _i, _p, _p, _p, _p]),
    "selfocc_camera_se_supported": (C.c_int, [_i] * 5),
    "selfocc_camera_se_flatten_fwd": (C.c_int, [_p, _p] + [_i] * 5 + [_p] * 7),
    "selfocc_camera_se_flatten_bwd_workspace": (C.c_size_t, [_p] + [_i] * 5),
    "selfocc_camera_se_flatten_bwd": (C.c_int, [_p, _p, _p] + [_i] * 5 + [_p] * 6 + [C.c_size_t, _p]),
    "selfocc_point_sampling": (C.c_int, [_p] * 7 + [_i] * 4 + [C.c_float, C.c_float, _p]),
    "selfocc_linear_wgrad_supported": (C.c_int, [C.c_int64, _i, _i]),
    "selfocc_linear_wgrad_workspace": (C.c_size_t, [C.c_int64, _i, _i]),
    "selfocc_linear_wgrad": (C.c_int, [_p] * 4 + [C.c_int64, _i, _i, _p, C.c_size_t, _p]),
    "selfocc_linear_fwd_supported": (C.c_int, [C.c_int64, _i, _i]),
    "selfocc_linear_fwd": (C.c_int, [_p] * 4 + [_i, _p, _p, C.c_float, _p, _i, _p, _p, _p, C.c_int64, _i, _i, C.c_uint32, _p]),
    "selfocc_linear_fwd_heads": (C.c_int, [_p] * 4 + [C.c_int64, _i, _i, _i, C.c_uint32, _p]),
    "selfocc_linear_dgrad_supported": (C.c_int, [C.c_int64, _i, _i]),
    "selfocc_linear_dgrad_workspace": (C.c_size_t, [_i, _i]),
    "selfocc_linear_dgrad": (C.c_int, [_p] * 3 + [C.c_int64, _i, _i, _p, C.c_int64, _p]),
    "selfocc_linear_dgrad_workspace_flags": (C.c_size_t, [_i, _i, C.c_uint32]),
    "selfocc_linear_dgrad_flags": (C.c_int, [_p] * 3 + [C.c_int64, _i, _i, _p, C.c_int64, C.c_uint32, _p]),
    "selfocc_linear_dgrad_grouped_workspace_flags": (C.c_size_t, [_i, _i, SoRowGroups, C.c_uint32]),
    "selfocc_linear_dgrad_grouped_flags": (C.c_int, [_p] * 3 + [C.c_int64, _i, _i, SoRowGroups, _p, C.c_int64, C.c_uint32, _p]),
    "selfocc_linear_wgrad_workspace_flags": (C.c_size_t, [C.c_int64, _i, _i, C.c_uint32]),
    "selfocc_linear_wgrad_flags": (C.c_int, [_p] * 4 + [C.c_int64, _i, _i, _p, C.c_size_t, C.c_uint32, _p]),
    "selfocc_linear_wgrad_grouped_workspace_flags": (C.c_size_t, [C.c_int64, _i, _i, SoRowGroups, C.c_uint32]),
    "selfocc_linear_wgrad_grouped_flags": (C.c_int, [_p] * 4 + [C.c_int64, _i, _i, SoRowGroups, _p, C.c_size_t, C.c_uint32, _p]),
    "selfocc_second_diff_size": (C.c_size_t, [_i, _i, _i]),
    "selfocc_second_diff_fwd": (C.c_int, [_p, _p, _i, _i, _i, _p]),
    "selfocc_second_diff_bwd": (C.c_int, [_p, _p, _i, _i, _i, _p]),
    "selfocc_eikonal_partials": (C.c_int, [C.c_int64]),
    "selfocc_eikonal_fwd": (C.c_int, [_p, _p, C.c_int64, _p]),
    "selfocc_eikonal_bwd": (C.c_int, [_p, _p, _p, C.c_int64, _p]),
    "selfocc_dropout_add_fwd": (C.c_int, [_p, _p, _p, C.c_int64, C.c_float, C.c_uint64, _p]),
    "selfocc_dropout_bwd": (C.c_int, [_p, _p, C.c_int64, C.c_float, C.c_uint64, _p]),
    "selfocc_ssim_fwd": (C.c_int, [_p] * 4 + [_i] * 4 + [_p, _p]),
    "selfocc_ssim_bwd": (C.c_int, [_p] * 4 + [_i] * 4 + [_p, _p, _p, _p]),
    "selfocc_reproj_fwd": (C.c_int, [C.POINTER(SoReprojArgs), _p]),
    "selfocc_reproj_bwd": (C.c_int, [C.POINTER(SoReprojArgs), _p, _p, _p, _p]),
    "selfocc_reproj_c_fwd": (C.c_int, [C.POINTER(SoReprojCArgs), _p]),
    "selfocc_reproj_c_bwd": (C.c_int, [C.POINTER(SoReprojCArgs), _p, _p, _p, _p]),
    "selfocc_reproj_pick_fwd": (C.c_int, [C.POINTER(SoReprojPickArgs), _p]),
    "selfocc_reproj_pick_bwd": (C.c_int, [_p, _p, _p, _i, _i, _p]),
    "selfocc_depth_metric_ws_bytes": (C.c_size_t, [C.POINTER(SoDepthMetricArgs)]),
    "selfocc_depth_metric": (C.c_int, [C.POINTER(SoDepthMetricArgs), _p]),
    "selfocc_ssc_metric": (C.c_int, [C.POINTER(SoSscMetricArgs), _p]),
    "selfocc_iou_coords": (C.c_int, [C.POINTER(SoSscMetricArgs), _p]),
}

"""The ctypes mirror of include/hgs_rasterizer.h, in one place: every struct, every function prototype, and bind(), which applies
the table to a loaded library.  _load() calls bind() once; nothing else in the project sets a prototype.

Rule for the table (tests/test_abi.py holds every line to the header's declaration): scalars are exact; a pointer to a mirrored
struct is POINTER(mirror); hgs_alloc_fn is _ALLOC_FN; every other pointer or array parameter is c_void_p -- which takes an int
address, None, byref(), a ctypes array or bytes -- or POINTER(scalar) / c_char_p where a call site hands over such an object.
A new entry point is one declaration in the header and one line here.
"""
import ctypes as C

MLP_MAX_TRUNK, MLP_MAX_HEADS = 3, 3   # HGS_MLP_MAX_TRUNK, HGS_MLP_MAX_HEADS


class _Settings(C.Structure):
    _fields_ = [("image_height", C.c_int32), ("image_width", C.c_int32), ("tanfovx", C.c_float),
                ("tanfovy", C.c_float), ("bg", C.c_void_p), ("scale_modifier", C.c_float),
                ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("sh_degree", C.c_int32),
                ("campos", C.c_void_p), ("prefiltered", C.c_int32), ("debug", C.c_int32)]


class _Segment(C.Structure):
    _fields_ = [("P", C.c_int32), ("M", C.c_int32), ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
                ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p)]


class _ForwardArgs(C.Structure):
    _fields_ = [("s", _Settings), ("P", C.c_int32), ("M", C.c_int32), ("means3D", C.c_void_p),
                ("shs", C.c_void_p), ("colors_precomp", C.c_void_p), ("opacities", C.c_void_p),
                ("scales", C.c_void_p), ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p),
                ("out_color", C.c_void_p), ("radii", C.c_void_p), ("binning_capacity_hint", C.c_int64),
                ("grad_accum_to_zero", C.c_void_p), ("clamp_output", C.c_int32), ("expect_no_long_tiles", C.c_int32),
                ("defer_n", C.c_int32), ("backward_checkpoints", C.c_int32), ("scratch", C.c_void_p * 4),
                ("scratch_bytes", C.c_size_t * 4), ("seg2", _Segment), ("visible", C.c_void_p), ("ckpt_slots_hint", C.c_int64),
                ("before_wait", C.c_void_p), ("before_wait_ctx", C.c_void_p)]


class _ForwardState(C.Structure):
    _fields_ = [("geom", C.c_void_p), ("geom_bytes", C.c_size_t), ("binning", C.c_void_p),
                ("binning_bytes", C.c_size_t), ("image", C.c_void_p), ("image_bytes", C.c_size_t),
                ("ckpt", C.c_void_p), ("ckpt_bytes", C.c_size_t), ("num_rendered", C.c_int64), ("binning_capacity", C.c_int64), ("sparse_frame", C.c_int32),
                ("has_long_tiles", C.c_int32), ("n_token", C.c_uint64), ("ckpt_slots", C.c_int64), ("ckpt_slots_used", C.c_int64)]


class _BackwardArgs(C.Structure):
    _fields_ = [("fwd", _ForwardArgs), ("state", _ForwardState), ("dL_dout_color", C.c_void_p),
                ("grad_accum", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("dL_dopacity", C.c_void_p),
                ("dL_dcolors", C.c_void_p), ("dL_dmeans3D", C.c_void_p), ("dL_dcov3D", C.c_void_p),
                ("dL_dsh", C.c_void_p), ("dL_dscales", C.c_void_p), ("dL_drotations", C.c_void_p),
                ("seg2_dL_dopacity", C.c_void_p), ("seg2_dL_dcolors", C.c_void_p), ("seg2_dL_dmeans3D", C.c_void_p),
                ("seg2_dL_dcov3D", C.c_void_p), ("seg2_dL_dsh", C.c_void_p), ("seg2_dL_dscales", C.c_void_p),
                ("seg2_dL_drotations", C.c_void_p), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("add_dL_dopacity", C.c_void_p), ("add_dL_dcolors", C.c_void_p), ("add_dL_dmeans3D", C.c_void_p),
                ("add_dL_dcov3D", C.c_void_p), ("add_dL_dsh", C.c_void_p), ("add_dL_dscales", C.c_void_p),
                ("add_dL_drotations", C.c_void_p), ("wait_before_per_gaussian", C.c_void_p)]


class _Desc(C.Structure):
    _fields_ = [("in_width", C.c_int32), ("n_trunk", C.c_int32), ("trunk_width", C.c_int32 * MLP_MAX_TRUNK), ("n_heads", C.c_int32),
                ("head_width", C.c_int32 * MLP_MAX_HEADS), ("head_act", C.c_int32 * MLP_MAX_HEADS),
                ("trunk_weight", C.c_void_p * MLP_MAX_TRUNK), ("trunk_bias", C.c_void_p * MLP_MAX_TRUNK),
                ("head_weight", C.c_void_p * MLP_MAX_HEADS), ("head_bias", C.c_void_p * MLP_MAX_HEADS)]


class _Grads(C.Structure):
    _fields_ = [("trunk_weight", C.c_void_p * MLP_MAX_TRUNK), ("trunk_bias", C.c_void_p * MLP_MAX_TRUNK),
                ("head_weight", C.c_void_p * MLP_MAX_HEADS), ("head_bias", C.c_void_p * MLP_MAX_HEADS)]


class _AdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64),
                ("one_minus_beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float),
                ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


_ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_size_t)   # hgs_alloc_fn

# the header's name of every mirrored struct
STRUCTS = {"hgs_settings": _Settings, "hgs_segment": _Segment, "hgs_forward_args": _ForwardArgs, "hgs_forward_state": _ForwardState,
           "hgs_backward_args": _BackwardArgs, "hgs_mlp_desc": _Desc, "hgs_mlp_grads": _Grads, "hgs_adam_tensor": _AdamTensor}

i32, i64, u32, sz, f32, p, s = C.c_int32, C.c_int64, C.c_uint32, C.c_size_t, C.c_float, C.c_void_p, C.c_char_p
P = C.POINTER

# name: (restype, argtypes), in the header's order
PROTOTYPES = {
    "hgs_rasterize_forward": (i64, (P(_ForwardArgs), _ALLOC_FN, p, P(_ForwardState), p)),
    "hgs_rasterize_backward": (i32, (P(_BackwardArgs), p)),
    "hgs_forward_poll": (i64, (P(_ForwardState), i32, p)),
    "hgs_maps_forward": (i32, (P(_ForwardArgs), P(_ForwardState), p, p, p)),
    "hgs_maps_backward": (i32, (P(_BackwardArgs), p, p, p)),
    "hgs_maps_finish": (i32, (P(_BackwardArgs), p)),
    "hgs_mark_visible": (i32, (i32, p, p, p, p)),
    "hgs_densification_stats": (i32, (i32,) + (p,) * 7),
    "hgs_knn_points": (i32, (i32, p, i32, p, i32, p, p, p)),
    "hgs_knn_workspace": (sz, (i32, i32)),
    "hgs_knn_points_ws": (i32, (i32, p, i32, p, i32, p, p, p, p)),
    "hgs_smpl_lbsweight_top_k": (i32, (i32, p, i32, p, p, i32, i32, p, p, p)),
    "hgs_smpl_lbsweight_top_k_ws": (i32, (i32, p, i32, p, p, i32, i32, p, p, p, p)),
    "hgs_smpl_lbsmap_top_k": (i32, (i32, p, i32, p, p, i32, i32, p, p, i32) + (p,) * 7),
    "hgs_smpl_lbsmap_top_k_backward": (i32, (i32, i32, p, p, p, p, i32, p, p, p)),
    "hgs_lbs_skin_forward": (i32, (i32, i32) + (p,) * 8),
    "hgs_lbs_skin_backward_workspace": (sz, (i32, i32)),
    "hgs_lbs_skin_backward": (i32, (i32, i32) + (p,) * 14),
    "hgs_dist_cuda2": (i32, (i32, p, p, p)),
    "hgs_dist_cuda2_workspace": (sz, (i32,)),
    "hgs_dist_cuda2_ws": (i32, (i32, p, p, p, p)),
    "hgs_ssim_l1_workspace": (sz, (i32, i32, i32)),
    "hgs_ssim_l1_forward": (i32, (i32, i32, i32) + (p,) * 6),
    "hgs_ssim_l1_backward": (i32, (i32, i32, i32) + (p,) * 7),
    "hgs_masked_loss_workspace": (sz, (i32, i32, i32)),
    "hgs_masked_loss_forward": (i32, (i32, i32, i32, i32) + (p,) * 8),
    "hgs_masked_loss_backward": (i32, (i32, i32, i32, i32) + (p,) * 10),
    "hgs_scene_forward": (i32, (i32, i32) + (p,) * 10),
    "hgs_scene_backward": (i32, (i32, i32) + (p,) * 13),
    "hgs_rotation_6d_to_matrix": (i32, (i32, p, p, p)),
    "hgs_rotation_6d_to_matrix_backward": (i32, (i32, p, p, p, p)),
    "hgs_matrix_to_quaternion": (i32, (i32, p, p, p)),
    "hgs_matrix_to_quaternion_backward": (i32, (i32, p, p, p, p)),
    "hgs_triplane_forward": (i32, (i32, i32, P(i32), P(i64), f32, f32) + (p,) * 6),
    "hgs_triplane_backward": (i32, (i32, i32, P(i32), P(i64), f32, f32, p, P(p), p, p, P(p), p)),
    "hgs_mlp_forward": (i32, (i32, P(_Desc), p, P(p), p)),
    "hgs_mlp_backward": (i32, (i32, P(_Desc), p, P(p), p, P(_Grads), p)),
    "hgs_mlp_tile": (i32, ()),
    "hgs_smpl_workspace": (sz, (i32, i32, i32)),
    "hgs_smpl_forward": (i32, (i32, i32, i32, P(i32)) + (p,) * 8 + (i32,) + (p,) * 10),
    "hgs_smpl_backward": (i32, (i32, i32, i32, P(i32)) + (p,) * 5 + (i32,) + (p,) * 15),
    "hgs_adam_step": (i32, (P(_AdamTensor), i32, p)),
    "hgs_adam_limits": (None, (P(i32), P(i32))),
    "hgs_densify_limits": (None, (P(i32), P(i32))),
    "hgs_densify_plan": (i32, (i32, i32, i32) + (p,) * 5 + (f32, f32, f32, i32, f32, f32) + (p,) * 4),
    "hgs_densify_scatter": (i32, (i32, i32, p, p, p, p, i32, p, p, p, p)),   # `tensors`: hgs_densify_tensor records, see hugs_amd/densify.py
    "hgs_last_error": (s, ()),
    "hgs_abi_version": (i32, ()),
    "hgs_geom_bytes": (sz, (i32, i32, i32)),
    "hgs_image_bytes": (sz, (i32, i32)),
    "hgs_binning_bytes": (sz, (i64, i32, i32)),
    "hgs_ckpt_bytes": (sz, (i64, i32, i32)),
    "hgs_ckpt_bytes_for_slots": (sz, (i64,)),
    "hgs_profile_enable": (None, (u32,)),
    "hgs_profile_set_sampling": (None, (u32,)),
    "hgs_profile_read": (i32, (i32, P(C.c_double), P(i64))),
    "hgs_profile_reset": (None, ()),
    "hgs_stage_name": (s, (i32,)),
    "hgs_copy_bandwidth": (i32, (p, p, sz, p)),
    "hgs_scratch_offset": (sz, (s, i32, i64, i32, i32)),
    "hgs_debug_stat": (i64, (s,)),
    "hgs_reload_switches": (None, ()),
}


def bind(lib):
    """Set restype and argtypes of every declared function on a loaded libhgs_rasterizer.so (a missing symbol raises)."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes

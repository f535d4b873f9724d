"""The Python view of the C ABI of libgs_rasterizer_hip.so (include/*.h), in one place: the struct mirrors, the signature of every
entry point and the header constants Python needs. ``_C.load_library()`` applies the table once, right after dlopen; every int-returning
entry point then raises RuntimeError on a negative return code (GSR_ERR_*, with gsr_last_error()'s text) and returns the value otherwise.
tests/test_abi_declarations.py checks this module against the headers. Importable without the library."""
import ctypes as C

i, i32, i64, u, sz, f, d, vp, P = C.c_int, C.c_int32, C.c_int64, C.c_uint, C.c_size_t, C.c_float, C.c_double, C.c_void_p, C.POINTER

# ---- constants ----------------------------------------------------------------------------------------------------------------------
GSR_NUM_CHANNELS = 3                                                              # gs_rasterizer.h
GSR_BACKWARD_ACCUMULATE, GSR_BACKWARD_POSE_ONLY = 2, 4
GSR_MAX_VIEWS = 12
GSR_DENSIFY_COPY, GSR_DENSIFY_STATE, GSR_DENSIFY_XYZ, GSR_DENSIFY_SCALE = 0, 1, 2, 3  # slam_map.h
GSR_DENSIFY_MAX_TENSORS = 32
GSR_CAMERA_STEPS_MAX = 12
GSR_SLOTS_MAX = 4
GSR_HEXPLANE_MAX_LEVELS = 8                                                       # deformation_field.h
GSR_HEXPLANE_MAX_VIEWS = 12
GSR_KNN_MAX_K, GSR_KNN_MAX_DIM, GSR_BLEND_MAX_K = 32, 32, 8                       # control_nodes.h
GSR_NODE_RADIUS_IS_LOG, GSR_NODE_WEIGHT_IS_LOGIT = 1, 2
GSR_YOLO_MAX_LEVELS, GSR_YOLO_MAX_ANCHORS, GSR_YOLO_REG_MAX, GSR_YOLO_DET_HEAD = 4, 8192, 16, 7  # segmentation.h
GSR_LPIPS_MAX_LEVELS, GSR_LPIPS_NORM_TORCHMETRICS, GSR_LPIPS_NORM_LPIPS = 8, 0, 1  # perceptual.h
GSR_PNG_SEGMENT = 16384                                                           # video_io.h
GSR_JPEG_GREY, GSR_JPEG_444, GSR_JPEG_422, GSR_JPEG_420 = 0, 1, 2, 3
GSR_JPEG_OK, GSR_JPEG_OUT_OF_BYTES, GSR_JPEG_LONG_CODE, GSR_JPEG_INDEX_PAST_63, GSR_JPEG_BAD_RESTART = 0, 1, 2, 3, 4

# ---- types (field names and order as in the headers; every pointer field is a plain address) -----------------------------------
gsr_alloc_fn = C.CFUNCTYPE(vp, vp, sz)


class gsr_raw_inputs(C.Structure):                                                # gs_rasterizer.h
    _fields_ = [("xyz", vp), ("log_scales", vp), ("scale_dim", i), ("raw_rotations", vp), ("logit_opacity", vp), ("features_dc", vp),
                ("features_rest", vp), ("dyn_slot", vp), ("dx", vp), ("ds", vp), ("dr", vp), ("gather", vp), ("flow_dx2", vp),
                ("flow_proj1", vp), ("flow_proj2", vp), ("delta_mode", i), ("delta_stride", i)]


class gsr_raw_grads(C.Structure):
    _fields_ = [("xyz", vp), ("log_scales", vp), ("raw_rotations", vp), ("logit_opacity", vp), ("features_dc", vp), ("features_rest", vp),
                ("dx", vp), ("ds", vp), ("dr", vp), ("dx2", vp)]


class gsr_view(C.Structure):
    _fields_ = [("viewmatrix", vp), ("projmatrix", vp), ("projmatrix_raw", vp), ("cam_pos", vp), ("dx", vp), ("ds", vp), ("dr", vp),
                ("out_color", vp), ("out_depth", vp), ("out_opacity", vp), ("radii", vp), ("n_touched", vp),
                ("geometry_user", vp), ("binning_user", vp), ("image_user", vp),
                ("geom_buffer", vp), ("binning_buffer", vp), ("image_buffer", vp), ("num_rendered", i),
                ("dL_dcolor", vp), ("dL_ddepth", vp), ("dL_dmean2D", vp), ("ddx", vp), ("dds", vp), ("ddr", vp), ("dL_dtau_sum", vp),
                ("flow_dx2", vp), ("flow_proj1", vp), ("flow_proj2", vp), ("ddx2", vp), ("flow_clip", vp)]


class gsr_masked_l1_term(C.Structure):                                            # slam_losses.h
    _fields_ = [("image", vp), ("target", vp), ("mask", vp), ("dL_dimage", vp)]


class gsr_adam_segment(C.Structure):
    _fields_ = [("param", vp), ("grad", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("n", C.c_ulonglong), ("lr", f), ("beta2", f), ("eps", f),
                ("beta1_d", d), ("beta2_d", d), ("step", i)]


class gsr_densify_tensor(C.Structure):                                            # slam_map.h
    _fields_ = [("src", vp), ("dst", vp), ("width", i), ("kind", i)]


class gsr_camera_step(C.Structure):
    _fields_ = [("rot_delta", vp), ("g_rot_delta", vp), ("trans_delta", vp), ("g_trans_delta", vp),
                ("exposure_a", vp), ("g_exposure_a", vp), ("exposure_b", vp), ("g_exposure_b", vp),
                ("exp_avg", vp), ("exp_avg_sq", vp), ("step", vp),
                ("lr_rot", f), ("lr_trans", f), ("lr_exposure", f), ("beta1", f), ("beta2", f), ("eps", f),
                ("R", vp), ("T", vp), ("projmatrix", vp), ("viewmatrix", vp), ("full_proj", vp), ("campos", vp),
                ("converged", vp), ("converged_threshold", f), ("do_pose", i), ("latch", i)]


class gsr_track_loss(C.Structure):
    _fields_ = [("gt_image", vp), ("gt_depth", vp), ("w_rgb", vp), ("w_depth", vp), ("alpha", f), ("opacity_depth_threshold", f),
                ("opacity_weights", i)]


class gsr_keyframe_entry(C.Structure):
    _fields_ = [(n, vp) for n in ("viewmatrix", "full_proj", "campos", "exposure_a", "exposure_b", "gt_image", "gt_depth", "w_rgb", "w_depth")]


class gsr_hexplane_level(C.Structure):                                            # deformation_field.h
    _fields_ = [("planes", vp * 6), ("grad_planes", vp * 6), ("res", i32 * 4)]


class gsr_hexplane_field(C.Structure):
    _fields_ = [("num_levels", i32), ("feat_dim", i32), ("channels_last", i32), ("reserved", i32), ("aabb", vp),
                ("levels", gsr_hexplane_level * GSR_HEXPLANE_MAX_LEVELS)]


class gsr_deform_mlp(C.Structure):
    _fields_ = [("W0", vp), ("b0", vp), ("W1", vp * 3), ("b1", vp * 3), ("W2", vp * 3), ("b2", vp * 3), ("in_dim", i32), ("reserved", i32)]


class gsr_dense_chain_op(C.Structure):                                            # dense_layers.h
    _fields_ = [("X", vp), ("ldx", i32), ("K", i32), ("planes", vp), ("bias", vp), ("relu", i32), ("Y", vp), ("ldy", i32), ("mask", vp),
                ("ldmask", i32), ("dbias", vp)]


class gsr_dense_split_item(C.Structure):
    _fields_ = [("W", vp), ("planes", vp), ("N", i32), ("K", i32), ("ldw", i32), ("k0", i32), ("transposed", i32)]


class gsr_dense_wgrad_item(C.Structure):
    _fields_ = [("G", vp), ("X", vp), ("dW", vp), ("ldg", i32), ("ldx", i32), ("lddw", i32), ("N", i32), ("K", i32)]


class gsr_trunk(C.Structure):
    _fields_ = [("E", i32), ("n_head_outputs", i32), ("planes", vp * 10), ("bias", vp * 9)]


class gsr_node_blend(C.Structure):                                                # control_nodes.h
    _fields_ = [("n", i64), ("m", i32), ("K", i32), ("local_frame", i32), ("rot_as_residual", i32), ("node_stride", i32), ("flags", i32),
                ("x", vp), ("motion_mask", vp), ("nodes", vp), ("node_radius", vp), ("node_weight", vp), ("node_trans", vp), ("node_rot", vp),
                ("node_scale", vp), ("node_frame", vp), ("node_local_rotation", vp), ("attr_stride", i32), ("grad_stride", i32)]


class gsr_multi_add_item(C.Structure):
    _fields_ = [("dst", vp), ("src", vp * 4), ("count", i32)]


# ---- entry points: name -> (restype, argtypes), per header in prototype order ---------------------------------------------------------
FUNCTIONS = {
    # gs_rasterizer.h
    "gsr_forward": (i, [gsr_alloc_fn, vp, gsr_alloc_fn, vp, gsr_alloc_fn, vp, i, i, i, vp, i, i] + [vp] * 5 + [f] + [vp] * 5 + [f, f, i] + [vp] * 5 + [i, vp]),
    "gsr_backward": (i, [i, i, i, i, vp, i, i, vp, vp, vp, vp, f] + [vp] * 6 + [f, f] + [vp] * 17 + [i, vp]),
    "gsr_backward_fused": (i, [i, i, i, i, vp, i, i, vp, vp, vp, vp, f] + [vp] * 6 + [f, f] + [vp] * 18 + [i, vp]),
    "gsr_forward_raw": (i, [gsr_alloc_fn, vp, gsr_alloc_fn, vp, gsr_alloc_fn, vp, i, i, i, vp, i, i, P(gsr_raw_inputs), f, vp, vp, vp, f, f] + [vp] * 5 + [i, vp]),
    "gsr_backward_raw": (i, [i, i, i, i, vp, i, i, P(gsr_raw_inputs), f, vp, vp, vp, vp, f, f] + [vp] * 7 + [P(gsr_raw_grads), vp, i, vp]),
    "gsr_forward_views": (i, [i, P(gsr_view), gsr_alloc_fn, gsr_alloc_fn, gsr_alloc_fn, i, i, i, vp, i, i, P(gsr_raw_inputs), f, f, f, i, vp]),
    "gsr_views_scratch_size": (sz, [i, i, i, i]),
    "gsr_backward_views": (i, [i, P(gsr_view), i, i, i, vp, i, i, P(gsr_raw_inputs), f, f, f, P(gsr_raw_grads), vp, i, vp]),
    "gsr_mark_visible": (i, [i] + [vp] * 5),
    "gsr_geometry_buffer_size": (sz, [i]),
    "gsr_image_buffer_size": (sz, [i, i, i]),
    "gsr_binning_buffer_size": (sz, [i]),
    "gsr_debug_read_state": (i, [i, i, i, i] + [vp] * 16),
    "gsr_debug_wave_reduce10": (i, [vp, vp, vp]),
    "gsr_debug_item_block": (i, [u, u, u, i]),
    "gsr_set_option": (i, [C.c_char_p, i]),
    "gsr_forward_status": (i, [P(u), P(u)]),
    "gsr_forward_status_views": (i, [P(u)]),
    "gsr_last_error": (C.c_char_p, []),
    "gsr_profile_enable": (i, [i]),
    "gsr_profile_read": (i, [P(C.c_char_p), P(f), P(i), i]),
    "gsr_profile_reset": (None, []),
    "gsr_version": (C.c_char_p, []),
    # simple_knn.h
    "gsr_knn_workspace_size": (sz, [i]),
    "gsr_knn_mean_dist2": (i, [i, vp, vp, vp, vp]),
    # slam_losses.h
    "gsr_l1_loss_workspace_size": (sz, []),
    "gsr_l1_loss_forward": (i, [i, i] + [vp] * 8 + [f, vp, f, vp, vp, vp]),
    "gsr_l1_loss_backward": (i, [i, i] + [vp] * 8 + [f, vp, f] + [vp] * 6),
    "gsr_masked_l1_forward": (i, [i, P(gsr_masked_l1_term), i, i, i, i, f, vp, vp, vp]),
    "gsr_masked_l1_backward": (i, [i, P(gsr_masked_l1_term), i, i, i, i, f, vp, vp]),
    "gsr_ssim_workspace_size": (sz, [i, i, i]),
    "gsr_ssim_forward": (i, [i, i, i] + [vp] * 6),
    "gsr_ssim_backward": (i, [i, i, i] + [vp] * 7),
    "gsr_adam_step": (i, [i, P(gsr_adam_segment), vp]),
    "gsr_adam_coefficients": (None, [d, d, d, i, P(f)]),
    "gsr_adam_step_scheduled": (i, [i, P(gsr_adam_segment), vp, vp]),
    "gsr_adam_step_device_count": (i, [i, P(gsr_adam_segment), P(vp), vp, vp]),
    "gsr_densification_stats": (i, [i] + [vp] * 6),
    # slam_map.h
    "gsr_seed_workspace_size": (sz, [i]),
    "gsr_seed_from_rgbd": (i, [i, vp, i, i, vp, vp, vp, vp, f, f, f, f, vp, vp, f, i] + [vp] * 7),
    "gsr_densify_select": (i, [i, vp, vp, vp, i, vp, f, f, f, f, vp, vp]),
    "gsr_densify_apply": (i, [i, vp, vp] + [i] * 5 + [P(gsr_densify_tensor), vp, vp, i, vp, vp, vp]),
    "gsr_camera_step_launch": (i, [P(gsr_camera_step), vp]),
    "gsr_camera_steps_launch": (i, [i, P(gsr_camera_step), vp]),
    "gsr_track_workspace_size": (sz, [i, i]),
    "gsr_track_step": (i, [gsr_alloc_fn, vp, gsr_alloc_fn, vp, gsr_alloc_fn, vp, i, i, i, vp, i, i, P(gsr_raw_inputs), f, vp, f, f] + [vp] * 5 +
                       [P(gsr_track_loss), P(gsr_camera_step), vp, vp, vp]),
    "gsr_schedule_advance": (i, [vp, vp, i, i, vp, vp]),
    "gsr_slot_gather": (i, [i, P(gsr_keyframe_entry), vp, P(gsr_keyframe_entry), i, vp]),
    "gsr_edge_mask": (i, [vp, i, i, f, f, vp, vp, vp, vp]),
    "gsr_mono_keyframe_depth_workspace_size": (sz, [i, i]),
    "gsr_mono_keyframe_depth": (i, [vp, vp, vp, i, i, f, vp, vp, vp, vp, vp]),
    "gsr_kabsch_rotations": (i, [i, vp, vp, vp]),
    "gsr_isotropic_loss_workspace_size": (sz, [i]),
    "gsr_isotropic_loss_forward": (i, [i, vp, vp, vp, vp]),
    "gsr_isotropic_loss_backward": (i, [i, vp, vp, vp, vp]),
    "gsr_arap_forward": (i, [i, i, i, i] + [vp] * 6),
    "gsr_arap_backward": (i, [i, i, i, i] + [vp] * 8),
    "gsr_elastic_forward": (i, [i, i, i, i, vp, vp, vp, vp]),
    "gsr_elastic_backward": (i, [i, i, i, i] + [vp] * 6),
    # deformation_field.h
    "gsr_hexplane_forward": (i, [P(gsr_hexplane_field), i64, vp, i64, vp, i64, vp, vp]),
    "gsr_hexplane_backward": (i, [P(gsr_hexplane_field), i64, vp, i64, vp, i64, vp, vp, vp, sz, vp]),
    "gsr_hexplane_backward_workspace_size": (sz, [P(gsr_hexplane_field), i64]),
    "gsr_hexplane_forward_views": (i, [P(gsr_hexplane_field), i64, vp, i64, i, P(f), vp, vp]),
    "gsr_hexplane_backward_views_workspace_size": (sz, [P(gsr_hexplane_field), i64, i]),
    "gsr_hexplane_backward_views": (i, [P(gsr_hexplane_field), i64, vp, i64, i, P(f)] + [vp] * 4 + [sz, vp]),
    "gsr_row_mask_workspace_size": (sz, [i, i64]),
    "gsr_row_mask": (i, [i, i64, i] + [vp] * 6),
    "gsr_linear_wgrad_workspace_size": (sz, [i64, i, i]),
    "gsr_linear_wgrad": (i, [i64, i, i, vp, i64, vp, i64, vp, vp, vp, vp]),
    "gsr_deform_mlp_forward": (i, [P(gsr_deform_mlp), i64, vp, vp, vp]),
    "gsr_deform_mlp_grad_count": (sz, [i]),
    "gsr_deform_mlp_workspace_size": (sz, [i]),
    "gsr_deform_mlp_backward": (i, [P(gsr_deform_mlp), i64] + [vp] * 6),
    "gsr_deform_mlp_backward_rows": (i, [P(gsr_deform_mlp), i64] + [vp] * 8),
    # dense_layers.h
    "gsr_dense_planes_size": (sz, [i, i]),
    "gsr_dense_split": (i, [i, i, vp, i, i, i, vp, vp]),
    "gsr_dense_forward": (i, [i, i, i, vp, i, vp, i, vp, vp, i, vp, i, vp]),
    "gsr_dense_backward_input_workspace_size": (sz, [i, i]),
    "gsr_dense_backward_input": (i, [i, i, i, vp, i, vp, vp, i, vp, i, vp, vp, vp]),
    "gsr_dense_chain_workspace_size": (sz, [i, i, i]),
    "gsr_dense_chain": (i, [i, i, i, P(gsr_dense_chain_op), vp, vp]),
    "gsr_dense_split_many": (i, [i, P(gsr_dense_split_item), vp]),
    "gsr_dense_wgrad_workspace_size": (sz, [i, i, i]),
    "gsr_dense_wgrad": (i, [i, i, i, vp, i, vp, i, vp, i, vp, i, vp, vp]),
    "gsr_dense_wgrad_many_workspace_size": (sz, [i, i, P(gsr_dense_wgrad_item)]),
    "gsr_dense_wgrad_many": (i, [i, i, P(gsr_dense_wgrad_item), vp, vp]),
    "gsr_trunk_forward": (i, [P(gsr_trunk), i, vp, P(vp), P(i), vp, vp]),
    # control_nodes.h
    "gsr_knn_points": (i, [i64, i64, i, i] + [vp] * 5),
    "gsr_knn_points_batch": (i, [i64, i64, i64, i, i] + [vp] * 5),
    "gsr_node_blend_forward": (i, [P(gsr_node_blend)] + [vp] * 7),
    "gsr_node_blend_workspace_size": (sz, [i64, i32]),
    "gsr_node_blend_backward": (i, [P(gsr_node_blend)] + [vp] * 15),
    "gsr_node_blend_forward_batch": (i, [P(gsr_node_blend), i] + [vp] * 7),
    "gsr_node_blend_workspace_size_batch": (sz, [i64, i32, i]),
    "gsr_node_blend_backward_batch": (i, [P(gsr_node_blend), i] + [vp] * 15),
    "gsr_node_embedding_workspace_size": (sz, [i, i, i, i]),
    "gsr_node_embedding": (i, [i, i, i, i, vp, i, vp, vp, vp, vp]),
    "gsr_relu_backward_bias_workspace_size": (sz, [i, i]),
    "gsr_relu_backward_bias": (i, [i, i] + [vp] * 6),
    "gsr_index_csr_workspace_size": (sz, [i, i, i]),
    "gsr_index_csr": (i, [i, i, i, vp, vp, vp]),
    "gsr_segment_sum": (i, [i] * 5 + [vp] * 5),
    "gsr_multi_add": (i, [i, P(gsr_multi_add_item), vp]),
    # frame_io.h
    "gsr_frame_prepare": (i, [i, i, vp, vp, vp, vp, f, vp, vp, vp]),
    "gsr_frame_export": (i, [i, i, i, vp, i64, vp, i64, vp, f, f, vp, vp, vp, vp]),
    # video_io.h
    "gsr_jpeg_workspace_size": (sz, [i, i, i]),
    "gsr_jpeg_encode": (i, [i, i, i, vp, vp, vp, i64, vp, vp, vp, sz, vp]),
    "gsr_jpeg_decode_workspace_size": (sz, [i, i, i, i, i]),
    "gsr_jpeg_decode": (i, [i, i, i, i, i, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "gsr_png_workspace_size": (sz, [i, i, i, i]),
    "gsr_png_stream_bound": (sz, [i, i, i]),
    "gsr_png_encode": (i, [i, i, i, i, i, vp, vp, i64, vp, vp, sz, vp]),
    # stereo_depth.h
    "gsr_stereo_workspace_size": (sz, [i, i, i]),
    "gsr_stereo_depth": (i, [i] * 7 + [f] + [vp] * 12 + [sz, vp]),
    # multiview_depth.h
    "gsr_sweep_workspace_size": (sz, [i, i, i]),
    "gsr_sweep_depth": (i, [i] * 3 + [f] * 6 + [i] * 4 + [vp] * 8 + [sz, vp]),
    # optical_flow.h
    "gsr_raft_corr_pyramid": (i, [i, i, i, vp, vp, P(vp), P(vp), vp]),
    "gsr_raft_corr_lookup": (i, [i, i, i, P(vp), vp, vp, vp]),
    "gsr_raft_upsample": (i, [i, i, i, vp, vp] + [i] * 5 + [vp, vp]),
    "gsr_gma_attention": (i, [i, i, i, i, vp, vp, f, vp, vp]),
    "gsr_gma_aggregate": (i, [i, i, i, i, vp, vp, vp, f, vp, vp]),
    # segmentation.h
    "gsr_yolo_workspace_size": (sz, [i]),
    "gsr_yolo_detect": (i, [i, P(i), P(f), P(vp), P(vp), i, i, P(i), i, f, f, i, vp, vp, i, vp, vp]),
    "gsr_yolo_masks": (i, [i, vp, vp, i, vp, i, i, i, i, vp, vp, vp]),
    # perceptual.h
    "gsr_lpips_prepare": (i, [i, i, i, vp, vp, vp, vp]),
    "gsr_lpips_workspace_size": (sz, [i, i, P(i)]),
    "gsr_lpips_distance": (i, [i, i, P(i), P(vp), P(vp), i, vp, vp, vp, vp]),
    # motion_segmentation.h
    "gsr_flow_rigid_fit_workspace_size": (sz, [i, i]),
    "gsr_flow_rigid_fit": (i, [i, i, f, f, f, f] + [vp] * 5 + [i] + [f] * 5 + [vp] * 6 + [sz, vp]),
    "gsr_motion_mask_clean_workspace_size": (sz, [i, i]),
    "gsr_motion_mask_clean": (i, [i, i, vp, i, i, i] + [vp] * 5 + [sz, vp]),
    # visual_odometry.h
    "gsr_odometry_pyramid_size": (sz, [i, i, i]),
    "gsr_odometry_pyramid": (i, [i, i, i, vp, vp, vp, f, f, vp, sz, vp]),
    "gsr_odometry_align_workspace_size": (sz, [i, i, i]),
    "gsr_odometry_align": (i, [i, i, i, f, f, f, f, vp, vp, vp, P(i)] + [f] * 7 + [vp] * 4 + [sz, vp]),
    "gsr_odometry_align_rgbd_workspace_size": (sz, [i, i, i]),
    "gsr_odometry_align_rgbd": (i, [i, i, i, f, f, f, f, vp, vp, vp, P(i), i] + [f] * 13 + [vp] * 4 + [sz, vp]),
    # relocalisation.h
    "gsr_reloc_encode_workspace_size": (sz, [i, i]),
    "gsr_reloc_encode": (i, [i, i, vp, vp, vp, i, i, i, vp, f, vp, vp, sz, vp]),
    "gsr_reloc_search": (i, [i, i, vp, vp, i, i, vp, vp, vp]),
    "gsr_reloc_score": (i, [i, i] + [vp] * 6 + [i, f, vp, vp]),
    # loop_closure.h
    "gsr_pose_graph_workspace_size": (sz, [i, i]),
    "gsr_pose_graph_solve": (i, [i, i, vp, vp, vp, vp, vp, i, i, d, d, vp, vp, vp, sz, vp]),
    "gsr_map_correct": (i, [i, vp, vp, vp, i, vp, i, vp, vp, vp]),
    # feature_matching.h
    "gsr_feat_slots": (i, [i, i, i, i]),
    "gsr_feat_extract_workspace_size": (sz, [i, i]),
    "gsr_feat_extract": (i, [i, i, vp, vp, i, i, i] + [vp] * 5 + [sz, vp]),
    "gsr_feat_match_workspace_size": (sz, [i, i]),
    "gsr_feat_match": (i, [i, vp, vp, i, vp, vp, i, i, vp, vp, sz, vp]),
    "gsr_feat_pose_workspace_size": (sz, [i, i]),
    "gsr_feat_pose": (i, [i, i, i, vp, vp, i] + [vp] * 5 + [u, i, f, f, f, i, i, i, f, f, f] + [vp] * 4 + [sz, vp]),
    "gsr_feat_pose_pnp_workspace_size": (sz, [i, i]),
    "gsr_feat_pose_pnp": (i, [i, i, i, vp, vp, i] + [vp] * 4 + [u, i, f, f, i, i, i, f, f, f] + [vp] * 4 + [sz, vp]),
}

# Exported by the library (csrc/gs_capi.hip) but not part of include/*.h: the view-slot inspector, and the readers of the
# instrumented dev builds (-DGSR_TIMELINE / -DGSR_FWD_TIMING, tools/) -- declared when the loaded library has them.
DEV_FUNCTIONS = {
    "gsr_debug_view_slots": (i, [P(u), i]),
    "gsr_debug_spans": (i, [vp, i, i]),
    "gsr_debug_fwd_timing": (i, [vp, i]),
    "gsr_debug_pre_timing": (i, [vp, i, i]),
    "gsr_debug_geo_timing": (i, [vp, i]),
    "gsr_debug_bwd_timing": (i, [vp, i]),
}


def declare(lib):
    """Apply the table to a freshly loaded library. Every int-returning entry point gets the one error path of the binding."""
    def check(rc, func, _args):
        if rc < 0:
            raise RuntimeError(f"{func.__name__} failed (code {rc}): {lib.gsr_last_error().decode(errors='replace')}")
        return rc

    dev = {k: v for k, v in DEV_FUNCTIONS.items() if hasattr(lib, k)}
    for name, (restype, argtypes) in {**FUNCTIONS, **dev}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
        if restype is i:
            fn.errcheck = check
    return lib

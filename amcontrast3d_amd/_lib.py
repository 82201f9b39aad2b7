"""ctypes binding of libamc3d_hip.so (C-ABI: include/amc3d.h).

There is NO fallback: if the shared library is missing or a symbol is absent,
importing the operators raises.  The product path never routes through oracle/.
"""
import ctypes
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.environ.get("AMC3D_LIB") or os.path.join(_CSRC, "libamc3d_hip.so")  # AMC3D_LIB: diagnostic builds

_vp, _i, _f, _sz, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_long
_ll = ctypes.c_longlong

# name -> (restype, argtypes); must list every symbol include/amc3d.h declares
SIGNATURES = {
    "amc3d_version": (ctypes.c_char_p, []),
    "amc3d_last_error": (ctypes.c_char_p, []),
    "amc3d_stream_create_dedicated": (_i, [ctypes.POINTER(ctypes.c_void_p)]),
    "amc3d_stream_create_masked": (_i, [_vp, _i, _i]),
    "amc3d_reserve_scratch": (_i, [_i, _vp, _vp]),
    "amc3d_stream_destroy": (_i, [_vp]),
    "amc3d_grid_search_workspace_bytes": (_sz, [_i, _i, _i]),
    "amc3d_grid_search_pays": (_i, [_i, _i, _i]),
    "amc3d_ball_query": (_i, [_i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_group_points": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_group_points_grad": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_gather_points": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_gather_points_grad": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_fps_workspace_bytes": (_sz, [_i, _i]),
    "amc3d_furthest_point_sampling": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_three_nn": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_three_interpolate": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_three_interpolate_add": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_three_interpolate_grad": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_three_interpolate_grad_route": (_i, [_i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "amc3d_three_interpolate_grad_write": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_three_interpolate_grad_lds": (_i, [_i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_knnquery_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "amc3d_knnquery_uses_grid": (_i, [_i, _i, _i, _i]),
    "amc3d_knnquery": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    "amc3d_knn_prefix": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    "amc3d_knn_batch_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "amc3d_knn_batch": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _sz, _i, _vp]),
    "amc3d_knn_features_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "amc3d_knn_features": (_i, [_i] * 7 + [_vp, _l, _l, _vp, _l, _l, _vp, _vp, _i, _vp, _sz, _vp]),
    "amc3d_knn_group_dp": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "amc3d_pointops_ballquery": (_i, [_i, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_furthestsampling": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_grouping_forward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_grouping_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_interpolation_forward": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_interpolation_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_subtraction_forward": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_subtraction_backward": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_aggregation_forward": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_aggregation_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointops_scatter_csr": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_vote_labels": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_posmask": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_ambiguity_workspace_bytes": (_sz, [_i]),
    "amc3d_ambiguity": (_i, [_i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_loss_rows_supported": (_i, [_i]),
    "amc3d_loss_rows": (_i, [_i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_contrast_csr_workspace_bytes": (_sz, [_i]),
    "amc3d_contrast_csr": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_contrast_backward_csr_supported": (_i, [_i]),
    "amc3d_contrast_backward_rows_supported": (_i, [_i]),
    "amc3d_contrast_backward_csr": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp,
                                         _vp, _vp]),
    "amc3d_contrast_mutual_workspace_bytes": (_sz, [_i]),
    "amc3d_contrast_mutual": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_contrast_backward_mutual_workspace_bytes": (_sz, [_i]),
    "amc3d_contrast_backward_mutual": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz,
                                            _vp, _vp]),
    "amc3d_contrast_stages_forward_cm": (_i, [_i, _vp, _f, _f, _f, _f, _vp, _vp]),
    "amc3d_contrast_stages_backward_cm_workspace_bytes": (_sz, [_i, _vp]),
    "amc3d_contrast_stages_backward_cm": (_i, [_i, _vp, _f, _f, _f, _f, _vp, _vp, _sz, _vp]),
    "amc3d_contrast_variant_forward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp,
                                            _vp, _vp]),
    "amc3d_contrast_variant_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _vp, _vp,
                                             _vp, _vp, _vp, _vp]),
    "amc3d_adamw_chunk": (_i, []),
    "amc3d_adamw_step": (_i, [_vp, _vp, _i, ctypes.c_double, ctypes.c_double, _f, _f, _vp, _vp, _vp]),
    "amc3d_select_anchors_ints": (_sz, [_i]),
    "amc3d_select_anchors": (_i, [_i, _vp, _vp, _sz, _vp]),
    "amc3d_contrast_forward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_contrast_forward_cm": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_contrast_backward": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_grouped_conv_supported": (_i, [_i, _i]),
    "amc3d_transpose_cn": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    "amc3d_grouped_conv_forward": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_grouped_conv_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "amc3d_grouped_conv_backward": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_confusion_update": (_i, [_i, _i, _l, _vp, _vp, _ll, _i, _vp, _vp, _vp]),
    "amc3d_cross_entropy_workspace_bytes": (_sz, [_i, _l]),
    "amc3d_cross_entropy_forward": (_i, [_i, _i, _l, _vp, _vp, _ll, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_cross_entropy_backward": (_i, [_i, _i, _l, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_point_loss_softmax_forward": (_i, [_i, _i, _l, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _i, _f, _i, _f, _vp, _f, _i, _vp, _vp,
                                              _vp, _sz, _vp]),
    "amc3d_point_loss_softmax_backward": (_i, [_i, _i, _l, _vp, _vp, _vp, _i, _ll, _i, _vp, _vp, _i, _f, _i, _f, _vp, _f, _i, _vp, _vp,
                                               _vp, _vp, _vp]),
    "amc3d_point_loss_sigmoid_forward": (_i, [_i, _i, _l, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _vp, _vp, _sz, _vp]),
    "amc3d_point_loss_sigmoid_backward": (_i, [_i, _i, _l, _vp, _vp, _vp, _vp, _f, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "amc3d_pointwise_conv_forward": (_i, [_i, _i, _i, _l, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointwise_conv_forward_workspace_bytes": (_sz, [_i, _i, _i, _l, _i]),
    "amc3d_pointwise_conv_forward_ws": (_i, [_i, _i, _i, _l, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_pointwise_conv_workspace_bytes": (_sz, [_i, _i, _i, _l]),
    "amc3d_pointwise_conv_backward": (_i, [_i, _i, _i, _l, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_pointwise_conv_forward_strided": (_i, [_i, _i, _i, _l, _vp, _vp, _l, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_pointwise_conv_forward_rows": (_i, [_i, _i, _i, _l, _vp, _vp, _l, _vp, _vp, _sz, _vp]),
    "amc3d_pointwise_conv_backward_strided": (_i, [_i, _i, _i, _l, _vp, _vp, _l, _vp, _vp, _i, _vp, _l, _vp, _sz, _vp]),
    "amc3d_gemm_tile_for": (_i, [_i, _i, _i, _i]),
    "amc3d_gemm_probe": (_i, [_i, _i, _i, _i, _i, _l, _l, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_bn_residual_forward": (_i, [_i, _i, _l, _f, _f] + [_vp] * 11 + [_vp, _sz, _vp]),
    "amc3d_bn_residual_backward": (_i, [_i, _i, _l] + [_vp] * 11 + [_vp, _sz, _vp]),
    "amc3d_split_columns": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_join_columns": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_masked_refine_workspace_ints": (_sz, [_i]),
    "amc3d_masked_refine_forward": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_masked_refine_backward": (_i, [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_bn_sigmoid_forward": (_i, [_i, _i, _l, _f, _f] + [_vp] * 10 + [_vp, _sz, _vp]),
    "amc3d_bn_sigmoid_backward": (_i, [_i, _i, _l] + [_vp] * 10 + [_vp, _sz, _vp]),
    "amc3d_bias_grad": (_i, [_i, _i, _l, _vp, _vp, _vp]),
    "amc3d_pointwise_conv_cloud_term_forward": (_i, [_i, _i, _i, _l, _vp, _vp, _l, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_cloud_term_grad": (_i, [_i, _i, _l, _vp, _vp, _vp]),
    "amc3d_sa_residual_forward": (_i, [_i, _i, _i, _i, _i] + [_vp] * 8),
    "amc3d_sa_residual_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "amc3d_sa_residual_backward": (_i, [_i, _i, _i, _i, _i] + [_vp] * 11 + [_sz, _vp]),
    "amc3d_index_duplicates_workspace_bytes": (_sz, [_i, _i]),
    "amc3d_index_duplicates": (_i, [_i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_augment_workspace_bytes": (_sz, [_i]),
    "amc3d_augment_clouds": (_i, [_i, _i, _i, _f, _f] + [_vp] * 10 + [_sz, _vp]),
    "amc3d_transform_max_ops": (_i, []),
    "amc3d_transform_max_phases": (_i, []),
    "amc3d_transform_program_bytes": (_i, []),
    "amc3d_transform_workspace_bytes": (_sz, [_i, _ll, _i]),
    "amc3d_transform_chain": (_i, [_i, _ll, _i, _vp, _vp, _vp, ctypes.POINTER(_vp), _i] + [_vp] * 6 + [_sz, _vp]),
    "amc3d_voxelize_workspace_bytes": (_sz, [_i]),
    "amc3d_voxelize": (_i, [_i, _vp, ctypes.c_double] + [_vp] * 7 + [_sz, _vp]),
    "amc3d_voxel_select": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_crop_nearest_workspace_bytes": (_sz, [_i]),
    "amc3d_crop_nearest": (_i, [_i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_voxelize_f64": (_i, [_i, _vp, ctypes.c_double] + [_vp] * 7 + [_sz, _vp]),
    "amc3d_crop_nearest_f64_workspace_bytes": (_sz, [_i]),
    "amc3d_crop_nearest_f64": (_i, [_i, _vp, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_scannet_stats_workspace_bytes": (_sz, [_i]),
    "amc3d_scannet_room_stats": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_scannet_transform_rooms": (_i, [_i, _ll] + [_vp] * 9 + [_vp]),
    "amc3d_scannet_crop_tail": (_i, [_i, _i] + [_vp] * 10 + [_vp]),
    "amc3d_s3dis_voxelize_workspace_bytes": (_sz, [_i, _ll]),
    "amc3d_s3dis_voxelize_rooms": (_i, [_i, _ll, _i, _vp, _vp, _vp, ctypes.c_double] + [_vp] * 8 + [_vp, _sz, _vp]),
    "amc3d_s3dis_crop_workspace_bytes": (_sz, [_i]),
    "amc3d_s3dis_select_crop": (_i, [_i, _i, _i, _i] + [_vp] * 13 + [_vp, _sz, _vp]),
    "amc3d_s3dis_crop_tail": (_i, [_i, _i, _i, _i] + [_vp] * 12 + [_vp]),
    "amc3d_scannet_voxelize_workspace_bytes": (_sz, [_i, _ll]),
    "amc3d_scannet_voxelize_rooms": (_i, [_i, _ll, _vp, _vp, ctypes.c_double] + [_vp] * 8 + [_vp, _sz, _vp]),
    "amc3d_scannet_crop_workspace_bytes": (_sz, [_i]),
    "amc3d_scannet_select_crop": (_i, [_i, _i, _i, _i] + [_vp] * 13 + [_vp, _sz, _vp]),
    "amc3d_scannet_crop_tail_workspace_bytes": (_sz, [_i]),
    "amc3d_scannet_crop_tail_rooms": (_i, [_i, _i, _i, _i] + [_vp] * 12 + [_vp, _sz, _vp]),
    "amc3d_room_parts": (_i, [_i, _i, _i] + [_vp] * 6 + [_vp]),
    "amc3d_part_batch_workspace_bytes": (_sz, [_i]),
    "amc3d_part_batch": (_i, [_i] * 6 + [_vp] * 12 + [_sz, _vp]),
    "amc3d_vote_parts": (_i, [_i, _i, _i, _i] + [_vp] * 8 + [_vp]),
    "amc3d_s3dis_part_batch_workspace_bytes": (_sz, [_i]),
    "amc3d_s3dis_part_batch": (_i, [_i] * 7 + [_vp] * 14 + [_sz, _vp]),
    "amc3d_room_representatives": (_i, [_i, _i] + [_vp] * 7 + [_vp]),
    "amc3d_expand_parts": (_i, [_i, _i, _i] + [_vp] * 6 + [_vp]),
    "amc3d_local_aggregation_supported": (_i, [_i, _i]),
    "amc3d_group_moments_bytes": (_sz, [_i, _i]),
    "amc3d_group_moments": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_local_aggregation_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "amc3d_local_aggregation_forward": (_i, [_i] * 7 + [_f, _f] + [_vp] * 4 + [_l] + [_vp] * 14 + [_i, _vp, _vp, _sz, _vp]),
    "amc3d_local_aggregation_backward": (_i, [_i] * 6 + [_vp] * 7 + [_l] + [_vp] * 10 + [_l] + [_vp] * 2 + [_i, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_local_aggregation_csr_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "amc3d_local_aggregation_workspace_q_offset": (_sz, [_i, _i, _i, _i]),
    "amc3d_local_aggregation_partial_counts": (_i, [_i, _i, _i, _i, _i, _vp]),
    "amc3d_local_aggregation_pool_centroids": (_i, [_i, _i, _i]),
    "amc3d_three_interpolate_grad_csr": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_masked_refine_backward_csr": (_i, [_i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointwise_conv_forward_bf16": (_i, [_i, _i, _i, _l, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_pointwise_conv_workspace_bytes_bf16": (_sz, [_i, _i, _i, _l]),
    "amc3d_pointwise_conv_backward_bf16": (_i, [_i, _i, _i, _l, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_grouped_conv_bn_supported": (_i, [_i, _i]),
    "amc3d_grouped_conv_bn_forward": (_i, [_i] * 7 + [_f, _f] + [_vp] * 4 + [_l] + [_vp] * 12 + [_i, _vp, _vp, _sz, _vp]),
    "amc3d_grouped_conv_bn_backward": (_i, [_i] * 6 + [_vp, _i] + [_vp] * 7 + [_l] + [_vp] * 8 + [_l] + [_vp] * 2 + [_i, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_group_csr_workspace_bytes": (_sz, [_i, _i, _i]),
    "amc3d_group_csr": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_group_moments_csr": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_grouped_conv_bn_csr_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "amc3d_group_csr_dp": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "amc3d_sa_tail_supported": (_i, [_i, _i, _i]),
    "amc3d_sa_tail_pays": (_i, [_i, _i]),
    "amc3d_sa_tail_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "amc3d_sa_tail_forward": (_i, [_i, _i, _i, _i, _i] + [_vp] * 8 + [_f, _f, _i] + [_vp] * 10 + [_sz, _vp]),
    "amc3d_sa_tail_backward": (_i, [_i, _i, _i, _i, _i] + [_vp] * 10 + [_i, _vp, _vp, _vp, _vp, _i] + [_vp] * 5 + [_sz, _vp]),
    "amc3d_bn_workspace_bytes": (_sz, [_i]),
    "amc3d_bn_stats": (_i, [_i, _i, _l, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_bn_forward": (_i, [_i, _i, _l, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_bn_update_running": (_i, [_i, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_bn_act": (_i, [_i, _i, _l, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_bn_max": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_bn_backward": (_i, [_i, _i, _l, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_bn_sums": (_i, [_i, _i, _l, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_bn_forward_synced": (_i, [_i, _i, _l, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_bn_backward_sums": (_i, [_i, _i, _l, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "amc3d_bn_backward_synced": (_i, [_i, _i, _l, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "amc3d_sphere_workspace_bytes": (_sz, [_i]),
    "amc3d_sphere_minima": (_i, [_i] + [_vp] * 4 + [_vp]),
    "amc3d_sphere_schedule": (_i, [_i] * 6 + [ctypes.c_double] + [_vp] * 13 + [_vp, _sz, _vp]),
    "amc3d_sphere_query": (_i, [_i] * 5 + [ctypes.c_double] + [_vp] * 9 + [_vp, _sz, _vp]),
    "amc3d_sphere_tail": (_i, [_i] * 4 + [_vp] * 18 + [_vp]),
    "amc3d_assa_aggregate_forward": (_i, [_i] * 6 + [_vp] * 5 + [_vp]),
    "amc3d_assa_aggregate_backward": (_i, [_i] * 6 + [_vp] * 5 + [_vp]),
    "amc3d_assa_aggregate_backward_csr": (_i, [_i] * 6 + [_vp] * 6 + [_vp]),
}


CONTRAST_MAX_STAGES = 8  # AMC_CONTRAST_MAX_STAGES
KNN_FALLBACK_COUNT_OFFSET = 1024  # AMC_KNN_FALLBACK_COUNT_OFFSET


class ContrastStageDesc(ctypes.Structure):
    """AmcContrastStage of include/amc3d.h"""
    _fields_ = ([(n, _i) for n in ("b", "C", "n", "k", "nbr_stride")]
                + [(n, _vp) for n in ("f_cm", "nbr", "posmask", "a", "sel", "mutual", "rev", "norm", "unit", "stats", "loss_pt",
                                      "mean_cnt", "rec", "grad_cm")])


def build(force=False):
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", _CSRC, "-j8"] + (["-B"] if force else [])
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise RuntimeError("building libamc3d_hip.so failed:\n" + proc.stdout)
    return _SO


_lib = None


def load():
    """Load the shared library and bind every declared symbol (raises if any is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(
            f"{_SO} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C {_CSRC}`); there is no CPU fallback")
    # PyTorch-ROCm bundles its own libamdhip64 / libhsa-runtime64; import it first so this library binds
    # to the SAME runtime instance (loading /opt/rocm's copy first leaves two HIP runtimes in one process
    # and the kernels here then see "no ROCm-capable device")
    import torch  # noqa: F401
    lib = ctypes.CDLL(_SO)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what} failed (hipError {status}): {load().amc3d_last_error().decode()}")

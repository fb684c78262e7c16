"""ctypes binding of libsradsgan_hip.so (the C ABI declared in include/sradsgan_hip.h).

There is deliberately NO fallback: if the shared library is missing or a call fails, the caller gets
an exception.  PyTorch is only used to own device memory and streams; raw pointers cross the ABI.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libsradsgan_hip.so')

_vp, _i, _f, _l, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long, ctypes.c_size_t
_u64 = ctypes.c_ulonglong

# name -> (restype, argtypes); must list every symbol of include/sradsgan_hip.h (tests check this)
SIGNATURES = {
    'srhip_last_error': (ctypes.c_char_p, []),
    'srhip_abi_version': (_i, []),
    'srhip_stream_fork': (_i, [_vp, _vp]),
    'srhip_debug_set': (_i, [_i, _i]),
    'srhip_probe_config': (_i, [_i] * 7),
    'srhip_probe_read': (_i, [_vp, _vp, _i]),
    'srhip_set_conv_math': (_i, [_i]),
    'srhip_get_conv_math': (_i, []),
    'srhip_resample_ksize': (_i, [_i, _i, _i]),
    'srhip_resample_coeffs': (_i, [_i, _i, _i, _vp, _vp]),
    'srhip_resample_pass_u8': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'srhip_u8_to_float': (_i, [_vp, _vp, _l, _vp]),
    'srhip_scene_tiles_u8': (_i, [_vp, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    'srhip_scene_blend_u8': (_i, [_vp, _i, _l, _l, _l] + [_vp] * 6 + [_i] * 8 + [_vp] * 3),
    'srhip_packed_elems': (_sz, [_i] * 5),
    'srhip_pack_entry_bytes': (_i, []),
    'srhip_packed_is_fast': (_i, [_i] * 5),
    'srhip_pack_weights_batched': (_i, [_vp, _i, _vp]),
    'srhip_pack_weight': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'srhip_conv2d_fwd': (_i, [_vp] * 7 + [_i] * 12 + [_f, _i, _vp]),
    'srhip_conv2d_dgrad': (_i, [_vp] * 5 + [_f] + [_i] * 13 + [_vp]),
    'srhip_conv2d_wgrad_workspace': (_sz, [_i] * 9),
    'srhip_conv2d_wgrad_can_accumulate': (_i, [_i] * 4),
    'srhip_conv2d_wgrad_multi_ok': (_i, [_i] * 9),
    'srhip_conv2d_wgrad_multi': (_i, [_i] + [_vp] * 4 + [_i, _vp, _sz] + [_i] * 11 + [_vp]),
    'srhip_pp_guard': (_i, [_i]),
    'srhip_pp_plane_pixels': (_l, [_i] * 3),
    'srhip_pp_from_f32': (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    'srhip_pp_to_f32': (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    'srhip_conv2d_pp_ok': (_i, [_i] * 5),
    'srhip_conv2d_fwd_dual': (_i, [_vp] * 9 + [_i] * 12 + [_f, _i, _vp]),
    'srhip_conv2d_fwd_pp': (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp] + [_i] * 5 + [_f, _i, _vp]),
    'srhip_conv2d_dgrad_pp': (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _f] + [_i] * 5 + [_vp]),
    'srhip_conv2d_dgrad_res3': (_i, [_vp] * 6 + [_i] * 9 + [_vp]),
    'srhip_conv2d_dgrad_pp_res3': (_i, [_vp, _i] + [_vp] * 5 + [_i] * 5 + [_vp]),
    'srhip_conv2d_pp_sign_bytes': (_sz, [_i] * 4),
    'srhip_conv2d_fwd_pp_signs': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz] + [_i] * 5 + [_f, _vp]),
    'srhip_conv2d_dgrad_pp_signs': (_i, [_vp, _i, _vp, _vp, _vp, _sz, _f] + [_i] * 5 + [_vp]),
    'srhip_conv2d_wgrad_pp_ok': (_i, [_i] * 5),
    'srhip_conv2d_wgrad_pp_workspace': (_sz, [_i] * 8),
    'srhip_conv2d_wgrad_pp': (_i, [_i, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _sz] + [_i] * 6 + [_vp]),
    'srhip_conv2d_wgrad_act_ok': (_i, [_i] * 9),
    'srhip_conv2d_wgrad_act': (_i, [_vp] * 3 + [_f] + [_vp] * 3 + [_sz] + [_i] * 11 + [_vp]),
    'srhip_conv2d_head_mask_ok': (_i, [_i] * 9),
    'srhip_conv2d_head_mask_bytes': (_sz, [_i] * 4),
    'srhip_conv2d_fwd_head_mask': (_i, [_vp] * 6 + [_sz] + [_i] * 7 + [_f, _i, _vp]),
    'srhip_conv2d_dgrad_head_mask': (_i, [_vp] * 4 + [_sz, _f] + [_i] * 7 + [_vp]),
    'srhip_conv2d_wgrad_head_mask': (_i, [_vp] * 3 + [_sz, _f] + [_vp] * 3 + [_sz] + [_i] * 7 + [_vp]),
    'srhip_conv2d_wgrad': (_i, [_vp] * 6 + [_i, _vp, _sz] + [_i] * 11 + [_vp]),
    'srhip_colsum_workspace': (_sz, [_l, _i]),
    'srhip_colsum': (_i, [_vp, _vp, _vp, _sz, _l, _i, _i, _vp]),
    'srhip_lrelu_bwd': (_i, [_vp, _vp, _vp, _l, _f, _vp]),
    'srhip_lrelu_mask_bytes': (_sz, [_l]),
    'srhip_lrelu_bwd_bits': (_i, [_vp, _vp, _vp, _vp, _l, _f, _vp]),
    'srhip_maxpool2x2_fwd': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_maxpool2x2_bwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'srhip_maxpool2x2_fwd_idx': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_maxpool2x2_bwd_idx': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'srhip_pixel_shuffle_fwd': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp]),
    'srhip_pixel_shuffle_bwd': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _vp]),
    'srhip_attn_tail_workspace': (_sz, [_i]),
    'srhip_attn_tail_fwd': (_i, [_vp] * 12 + [_sz] + [_i] * 5 + [_vp]),
    'srhip_attn_tail_eval': (_i, [_vp] * 9 + [_sz] + [_i] * 5 + [_vp]),
    'srhip_attn_tail_bwd_workspace': (_sz, [_i] * 3),
    'srhip_attn_tail_bwd_spatial': (_i, [_vp] * 10 + [_i, _vp, _sz] + [_i] * 4 + [_vp]),
    'srhip_attn_tail_mlp_workspace': (_sz, [_i, _i]),
    'srhip_attn_tail_bwd_mlp': (_i, [_vp] * 10 + [_i, _vp, _sz] + [_i] * 3 + [_vp]),
    'srhip_attn_tail_bwd_fused_workspace': (_sz, [_i] * 4),
    'srhip_attn_tail_bwd': (_i, [_vp] * 14 + [_i] + [_vp] * 2 + [_i, _vp, _sz] + [_i] * 5 + [_vp]),
    'srhip_attn_tail_bwd_pp': (_i, [_vp] * 15 + [_i] + [_vp] * 2 + [_i, _vp, _sz] + [_i] * 5 + [_vp]),
    'srhip_attn_tail_bwd_channel': (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    'srhip_attn_var_workspace': (_sz, [_i]),
    'srhip_attn_var_fwd': (_i, [_vp] * 12 + [_sz] + [_i] * 7 + [_vp]),
    'srhip_attn_var_close': (_i, [_vp] * 5 + [_i] * 5 + [_vp]),
    'srhip_attn_var_bwd_workspace': (_sz, [_i] * 4),
    'srhip_attn_var_bwd': (_i, [_vp] * 14 + [_i] + [_vp] * 2 + [_i, _vp, _sz] + [_i] * 7 + [_vp]),
    'srhip_cgam_workspace': (_sz, [_i, _i]),
    'srhip_cgam_fwd': (_i, [_vp] * 5 + [_sz] + [_i] * 3 + [_vp]),
    'srhip_cgam_bwd': (_i, [_vp] * 6 + [_i, _vp, _sz] + [_i] * 3 + [_vp]),
    'srhip_sgam_flash_fwd': (_i, [_vp] * 8 + [_i] * 4 + [_vp]),
    'srhip_sgam_flash_bwd_workspace': (_sz, [_i, _i]),
    'srhip_sgam_flash_bwd': (_i, [_vp] * 11 + [_i, _vp, _sz] + [_i] * 4 + [_vp]),
    'srhip_cbam_pool_hw': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_cbam_unpool_hw': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    'srhip_cbam_pool_c': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_cbam_unpool_c': (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    'srhip_cbam_scale': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_cbam_dot': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_sigmoid_fwd': (_i, [_vp, _vp, _l, _i, _i, _vp]),
    'srhip_sigmoid_bwd': (_i, [_vp, _vp, _vp, _l, _i, _i, _vp]),
    'srhip_sigmoid_bwd_bwd': (_i, [_vp] * 5 + [_l, _i, _i, _vp]),
    'srhip_reduce_workspace': (_sz, []),
    'srhip_l1_mean_fwd': (_i, [_vp] * 4 + [_sz, _l, _vp]),
    'srhip_l1_mean_bwd': (_i, [_vp] * 5 + [_l, _vp]),
    'srhip_mse_mean_fwd': (_i, [_vp] * 4 + [_sz, _l, _vp]),
    'srhip_mse_mean_bwd': (_i, [_vp] * 5 + [_l, _vp]),
    'srhip_smooth_l1_mean_fwd': (_i, [_vp, _vp, _f, _vp, _vp, _sz, _l, _vp]),
    'srhip_smooth_l1_mean_bwd': (_i, [_vp, _vp, _f] + [_vp] * 3 + [_l, _vp]),
    'srhip_mean_fwd': (_i, [_vp] * 3 + [_sz, _l, _vp]),
    'srhip_mean_bwd': (_i, [_vp] * 2 + [_l, _vp]),
    'srhip_gp_norm_penalty_fwd': (_i, [_vp] * 3 + [_sz, _l, _i, _vp]),
    'srhip_gp_norm_penalty_bwd': (_i, [_vp] * 3 + [_l, _i, _vp]),
    'srhip_gp_penalty_fwd': (_i, [_vp] * 3 + [_sz, _l, _i, _i, _i, _vp]),
    'srhip_gp_penalty_bwd': (_i, [_vp] * 3 + [_l, _i, _i, _i, _vp]),
    'srhip_bn_eval_fwd': (_i, [_vp] * 6 + [_l, _i, _f, _f, _i, _vp]),
    'srhip_dp_id_bytes': (_i, []),
    'srhip_dp_unique_id': (_i, [_vp]),
    'srhip_dp_init': (_i, [_vp, _i, _i]),
    'srhip_dp_world': (_i, []),
    'srhip_dp_rank': (_i, []),
    'srhip_dp_allreduce_bucket': (_i, [_vp, _sz, _vp]),
    'srhip_dp_broadcast': (_i, [_vp, _sz, _i, _vp]),
    'srhip_dp_finalize': (_i, []),
    'srhip_bn_workspace': (_sz, [_l, _i]),
    'srhip_bn_train_fwd': (_i, [_vp] * 9 + [_sz, _l, _i, _f, _f, _f, _i, _vp]),
    'srhip_bn_train_bwd': (_i, [_vp] * 10 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_bn_bwd2_workspace': (_sz, [_l, _i]),
    'srhip_bn_train_bwd_bwd': (_i, [_vp] * 11 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_clam_pool_segments': (_i, []),
    'srhip_clam_pool_max_segments': (_i, []),
    'srhip_clam_pool_partial': (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _vp]),
    'srhip_conv2d_fwd_pool': (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _vp] + [_i] * 8 + [_vp]),
    'srhip_attn_tail_fwd_pooled': (_i, [_vp, _vp, _sz, _i] + [_vp] * 10 + [_i] * 5 + [_vp]),
    'srhip_attn_tail_eval_pooled': (_i, [_vp, _vp, _vp, _sz, _i] + [_vp] * 6 + [_i] * 5 + [_vp]),
    'srhip_sum_n': (_i, [_vp, _i, _vp, _l, _vp]),
    'srhip_ca_segments': (_i, []),
    'srhip_ca_pool_sum': (_i, [_vp, _vp] + [_i] * 3 + [_vp]),
    'srhip_ca_mlp_fwd': (_i, [_vp, _i] + [_vp] * 5 + [_i] * 4 + [_vp]),
    'srhip_ca_scale_res': (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
    'srhip_ca_bwd_partial': (_i, [_vp] * 3 + [_i] * 3 + [_vp]),
    'srhip_ca_mlp_bwd_workspace': (_sz, [_i, _i]),
    'srhip_ca_mlp_bwd': (_i, [_vp] * 10 + [_sz] + [_i] * 4 + [_vp]),
    'srhip_ca_bwd_du': (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
    'srhip_ca_mlp_fwd_bias': (_i, [_vp, _i] + [_vp] * 7 + [_i] * 4 + [_vp]),
    'srhip_ca_mlp_bwd_bias': (_i, [_vp] * 12 + [_sz] + [_i] * 4 + [_vp]),
    'srhip_add_bcast_scaled': (_i, [_vp, _vp, _f, _vp, _i, _l, _vp]),
    'srhip_batch_sum_scaled': (_i, [_vp, _f, _vp, _i, _l, _vp]),
    'srhip_scaled_res_fwd': (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _f, _vp, _i, _vp, _i, _l, _i, _vp]),
    'srhip_scaled_res_bwd': (_i, [_vp, _i, _vp, _i, _f, _f, _f, _vp, _i, _vp, _i, _i, _l, _i, _vp]),
    'srhip_lrelu_bwd_strided': (_i, [_vp, _i, _vp, _i, _vp, _i, _f, _l, _i, _vp]),
    'srhip_upsample_nearest_fwd': (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    'srhip_upsample_nearest_bwd': (_i, [_vp, _vp] + [_i] * 5 + [_vp]),
    'srhip_conv2d_dil_workspace': (_sz, [_i] * 7),
    'srhip_conv2d_fwd_dil': (_i, [_vp] * 6 + [_sz] + [_i] * 8 + [_f, _i, _vp]),
    'srhip_conv2d_dgrad_dil': (_i, [_vp] * 4 + [_sz] + [_i] * 9 + [_vp]),
    'srhip_conv2d_wgrad_dil': (_i, [_vp] * 4 + [_i, _vp, _sz] + [_i] * 8 + [_vp]),
    'srhip_prelu_parts': (_i, []),
    'srhip_prelu_fwd': (_i, [_vp, _i, _vp, _i, _vp, _l, _i, _vp]),
    'srhip_prelu_bwd': (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _vp, _l, _i, _vp]),
    'srhip_prelu_slope_reduce': (_i, [_vp, _i, _vp, _i, _vp]),
    'srhip_nl_quad_fwd': (_i, [_vp] * 5 + [_i] * 3 + [_vp]),
    'srhip_nl_quad_bwd': (_i, [_vp] * 10 + [_i] * 3 + [_vp]),
    'srhip_gamma_parts': (_i, []),
    'srhip_gamma_res_fwd': (_i, [_vp] * 4 + [_l, _vp]),
    'srhip_gamma_res_bwd': (_i, [_vp] * 5 + [_l, _vp]),
    'srhip_cat_channels': (_i, [_vp, _vp, _i, _vp, _l, _vp]),
    'srhip_split_channels': (_i, [_vp, _vp, _i, _vp, _l, _vp]),
    'srhip_bn_train_bwd_acc': (_i, [_vp] * 12 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_bn_train_bwd_acc_x': (_i, [_vp] * 12 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_bn_train_bwd_acc_xa': (_i, [_vp] * 13 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_bn_train_bwd_bwd_acc': (_i, [_vp] * 12 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_bn_train_bwd_bwd_acc_x': (_i, [_vp] * 12 + [_sz, _l, _i, _f, _i, _vp]),
    'srhip_gn_workspace': (_sz, [_l, _l, _i]),
    'srhip_gn_fwd': (_i, [_vp] * 7 + [_sz, _l, _l, _i, _i, _i, _f, _f, _i, _vp]),
    'srhip_gn_bwd': (_i, [_vp] * 13 + [_sz, _l, _l, _i, _i, _i, _f, _i, _vp]),
    'srhip_gn_bwd_bwd': (_i, [_vp] * 12 + [_sz, _l, _l, _i, _i, _i, _f, _i, _vp]),
    'srhip_metric_blocks': (_i, []),
    'srhip_quant_sse': (_i, [_vp, _vp, _vp, _i, _l, _vp]),
    'srhip_ssim_u8': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'srhip_metric_finish': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, ctypes.c_double, _vp]),
    'srhip_lpips_stem': (_i, [_vp] * 4 + [_i] * 4 + [_vp]),
    'srhip_maxpool3x3s2_fwd': (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    'srhip_lpips_blocks': (_i, []),
    'srhip_lpips_head': (_i, [_vp] * 4 + [_i] * 5 + [_vp]),
    'srhip_lpips_finish': (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    'srhip_hat_ln_parts': (_i, [_l]),
    'srhip_hat_ln_fwd': (_i, [_vp] * 6 + [_l, _vp]),
    'srhip_hat_ln_bwd': (_i, [_vp] * 10 + [_l, _vp]),
    'srhip_hat_gelu_fwd': (_i, [_vp, _vp, _l, _vp]),
    'srhip_hat_gelu_bwd': (_i, [_vp] * 3 + [_l, _vp]),
    'srhip_hat_attn_fwd': (_i, [_vp] * 4 + [_i] * 6 + [_vp]),
    'srhip_hat_attn_bwd_workspace': (_sz, [_i] * 5),
    'srhip_hat_attn_bwd': (_i, [_vp] * 8 + [_sz] + [_i] * 6 + [_vp]),
    'srhip_hat_ca_fwd': (_i, [_vp] * 7 + [_i, _l, _i, _i, _vp]),
    'srhip_hat_combine_fwd': (_i, [_vp] * 6 + [_f, _i, _l, _i, _vp]),
    'srhip_hat_combine_bwd_workspace': (_sz, [_i] * 3),
    'srhip_hat_combine_bwd': (_i, [_vp] * 14 + [_sz, _f, _i, _l, _i, _i, _vp]),
    'srhip_hatw_ln_parts': (_i, [_l]),
    'srhip_hatw_ln_fwd': (_i, [_vp] * 6 + [_l, _i, _vp]),
    'srhip_hatw_ln_bwd': (_i, [_vp] * 10 + [_l, _i, _vp]),
    'srhip_hatw_attn_fwd': (_i, [_vp] * 4 + [_i] * 8 + [_vp]),
    'srhip_hatw_attn_bwd_workspace': (_sz, [_i] * 7),
    'srhip_hatw_attn_bwd': (_i, [_vp] * 8 + [_sz] + [_i] * 8 + [_vp]),
    'srhip_hatw_ca_fwd': (_i, [_vp] * 7 + [_i, _l, _i, _i, _vp]),
    'srhip_hatw_combine_bwd': (_i, [_vp] * 14 + [_sz, _f, _i, _l, _i, _i, _vp]),
    'srhip_adam_step': (_i, [_vp] * 5 + [_l] + [_f] * 6 + [_vp]),
    'srhip_sn_entry_bytes': (_i, []),
    'srhip_sn_tpart_elems': (_l, [_i, _i]),
    'srhip_sn_dot_parts': (_l, [_i, _i]),
    'srhip_sn_forward_batched': (_i, [_vp, _i, _vp, _i, _i, _vp]),
    'srhip_sn_backward_batched': (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    'srhip_cls_channel_sums_workspace': (_sz, [_i] * 3),
    'srhip_cls_channel_sums': (_i, [_vp, _vp, _vp, _sz] + [_i] * 4 + [_vp]),
    'srhip_cls_preprocess': (_i, [_vp, _vp, _vp, _l, _i, _vp]),
    'srhip_cls_dense_chunks': (_i, [_i]),
    'srhip_cls_dense_fwd': (_i, [_vp] * 5 + [_sz] + [_i] * 5 + [_u64, _u64, _vp]),
    'srhip_cls_dense_wgrad': (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
    'srhip_cls_dense_dgrad': (_i, [_vp] * 4 + [_i] * 5 + [_u64, _u64, _vp]),
    'srhip_cls_softmax_ce_fwd_bwd': (_i, [_vp] * 5 + [_i, _i, _f, _vp]),
    'srhip_cls_confusion': (_i, [_vp] * 4 + [_i, _i, _vp]),
    'srhip_diff_gn_workspace': (_sz, [_l, _l]),
    'srhip_diff_gn_fwd': (_i, [_vp, _l] + [_vp] * 4 + [_l, _vp, _l, _vp, _sz, _l, _l, _i, _f, _i, _vp]),
    'srhip_diff_silu_fwd': (_i, [_vp, _vp, _l, _vp]),
    'srhip_diff_avgpool2x2_fwd': (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    'srhip_diff_attn_fwd': (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    'srhip_diff_randn': (_i, [_vp, _l, _l, _i, _u64, _u64, _vp]),
    'srhip_diff_sampler_step': (_i, [_vp, _l] * 4 + [_l, _i, _f, _f, _f, _i, _u64, _u64, _vp]),
    'srhip_diff_quant_u8': (_i, [_vp, _l, _vp, _l, _i, _f, _f, _vp]),
    'srhip_diff_gn_stats_offset': (_sz, [_l, _l]),
    'srhip_diff_gn_bwd_workspace': (_sz, [_l, _l, _i]),
    'srhip_diff_gn_bwd': (_i, [_vp, _l, _vp, _l] + [_vp] * 5 + [_l, _vp, _l] + [_vp] * 4 + [_l, _vp, _sz, _l, _l, _i, _i, _vp]),
    'srhip_diff_silu_bwd': (_i, [_vp, _vp, _vp, _l, _vp]),
    'srhip_diff_avgpool2x2_bwd': (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    'srhip_diff_attn_fwd_lse': (_i, [_vp, _vp, _vp] + [_i] * 4 + [_vp]),
    'srhip_diff_attn_bwd_workspace': (_sz, [_i, _i, _i]),
    'srhip_diff_attn_bwd': (_i, [_vp] * 6 + [_sz] + [_i] * 4 + [_vp]),
    'srhip_diff_q_sample': (_i, [_vp, _l] * 3 + [_vp] * 3 + [_i, _l, _l, _i, _u64, _u64, _vp]),
    'srhip_augment_u8': (_i, [_vp] * 4 + [_i] * 5 + [ctypes.c_double, _i, _u64, _u64, _vp]),
    'srhip_dihedral_f32': (_i, [_vp] * 4 + [_i] * 5 + [_vp]),
    'srhip_ensemble_merge_f32': (_i, [_vp, _vp, _vp, _i, _vp, _vp] + [_i] * 4 + [_vp]),
    'srhip_blur_u8': (_i, [_vp] * 3 + [_i] * 5 + [_vp]),
    'srhip_blur_f32': (_i, [_vp, _vp, _vp, _i, _vp, _vp] + [_i] * 5 + [_vp]),
    'srhip_degrade_noise_u8': (_i, [_vp] * 4 + [_i] * 5 + [_u64, _u64, _vp]),
}

_lib = None


class HipLibraryError(RuntimeError):
    pass


# arithmetic of the conv contraction unless SRADSGAN_CONV_MATH overrides it (include/sradsgan_hip.h, srhip_set_conv_math)
DEFAULT_CONV_MATH = 'bf16x3'


def lib():
    """Load (once) and return the shared library; raises HipLibraryError when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                'libsradsgan_hip.so is not built (%s). Build it with `make -C sradsgan_amd/csrc` or '
                '`python -c "import __graft_entry__ as g; g.build()"`. There is no CPU fallback.' % LIB_PATH)
        handle = ctypes.CDLL(os.environ.get('SRHIP_LIB', LIB_PATH))     # SRHIP_LIB: same-box A/B of two builds (debug)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        mode = os.environ.get('SRADSGAN_CONV_MATH', DEFAULT_CONV_MATH)
        if mode not in ('fp32', 'bf16x3', 'half'):
            raise HipLibraryError("SRADSGAN_CONV_MATH must be 'fp32', 'bf16x3' or 'half', got %r" % mode)
        handle.srhip_set_conv_math({'fp32': 0, 'bf16x3': 1, 'half': 2}[mode])
        for item in os.environ.get('SRHIP_DEBUG', '').split(','):      # experiment knobs, "key:value,..." (sradsgan_hip.h)
            if item:
                key, value = item.split(':')
                if handle.srhip_debug_set(int(key), int(value)) != 0:
                    raise HipLibraryError('SRHIP_DEBUG: srhip_debug_set refused key %s (%r): unknown or retired key' % (key, item))
        _lib = handle
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().srhip_last_error()
        raise HipLibraryError('%s failed (%d): %s' % (what or 'srhip call', rc, msg.decode() if msg else '?'))

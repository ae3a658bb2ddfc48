"""ctypes binding of libdsdenoise.so (include/dsd.h).  There is NO fallback: if the library is missing or
does not load, importing the engine fails loudly - the product path never routes through a CPU/oracle
implementation."""
from __future__ import annotations

import ctypes as C
import os

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'libdsdenoise.so')

DSD_ABI_VERSION = 8

# every symbol include/dsd.h declares (tests check the .so exports exactly these)
SYMBOLS = [
    'dsd_abi_version', 'dsd_last_error', 'dsd_build_id', 'dsd_create', 'dsd_destroy', 'dsd_load_weights', 'dsd_set_schedule',
    'dsd_get_schedule_table', 'dsd_set_spec_range', 'dsd_prepare', 'dsd_denoise', 'dsd_q_sample',
    'dsd_sample_ddpm', 'dsd_p_sample', 'dsd_sample_plms', 'dsd_norm_spec', 'dsd_denorm_spec',
    'dsd_set_use_graph', 'dsd_set_layer_tile', 'dsd_time_layer_kernel', 'dsd_debug_layer_timeline', 'dsd_device_bytes',
    'dsd_get_layer_tile', 'dsd_set_loop_mode', 'dsd_get_loop_mode', 'dsd_loop_timeouts', 'dsd_debug_loop_timeline', 'dsd_set_noise_seed', 'dsd_philox_normal',
    'dsd_set_split_mode', 'dsd_get_split_mode', 'dsd_debug_layer', 'dsd_loop_launches', 'dsd_p_sample_ex', 'dsd_set_lat_split', 'dsd_get_lat_split', 'dsd_set_conv_mode', 'dsd_get_conv_mode',
    'dsd_check', 'dsd_loop_parked', 'dsd_debug_hold_cus', 'dsd_debug_condproj_groups',
]
# every symbol include/dsf.h declares (the FastSpeech2 conditioner ops)
SYMBOLS_FS2 = ['dsf_padded_frames', 'dsf_packed_floats', 'dsf_pack_weight', 'dsf_conv1d', 'dsf_layer_norm', 'dsf_attention',
               'dsf_ln_bwd_workspace_floats', 'dsf_layer_norm_bwd', 'dsf_attention_bwd_workspace_floats', 'dsf_attention_bwd',
               'dsf_linear_rows_workspace_floats', 'dsf_linear_rows', 'dsf_linear_rows_bwd',
               'dsf_to_channel_major', 'dsf_from_channel_major', 'dsf_positions', 'dsf_input_cm', 'dsf_gather_frames', 'dsf_sum_embed', 'dsf_token_masks', 'dsf_pitch_coarse', 'dsf_q_sample_rows', 'dsf_l1_workspace_floats', 'dsf_l1_mean', 'dsf_l1_mean_bwd', 'dsf_p_sample', 'dsf_denorm_spec',
               'dsf_conv1d_dilated', 'dsf_set_conv_split', 'dsf_wgrad_workspace_floats', 'dsf_conv1d_wgrad', 'dsf_bias_grad',
               'dsf_train_add_step', 'dsf_train_rowsum', 'dsf_train_gate', 'dsf_train_gate_bwd', 'dsf_train_res_skip', 'dsf_train_res_skip_bwd',
               'dsf_channel_affine', 'dsf_group_norm', 'dsf_adamw_step',
               'dsf_batch_norm_train', 'dsf_batch_norm_train_bwd', 'dsf_group_norm_bwd_workspace_floats', 'dsf_group_norm_bwd',
               'dsf_f0_loss_workspace_floats', 'dsf_f0_loss', 'dsf_f0_loss_bwd',
               'dsf_stack_workspace_floats', 'dsf_set_stack_mode', 'dsf_set_stack_conv', 'dsf_get_stack_conv', 'dsf_set_wgrad_dual', 'dsf_debug_trb_timeline', 'dsf_stack_offsets', 'dsf_stack_forward', 'dsf_stack_backward', 'dsf_wgrad2_workspace_floats', 'dsf_conv1d_wgrad2', 'dsf_wgrad_probe', 'dsf_wgrad_probe_read',
               'dsf_fs2_loss_workspace_floats', 'dsf_mel_loss', 'dsf_mel_loss_bwd', 'dsf_dur_loss', 'dsf_dur_loss_bwd', 'dsf_length_regulate',
               'dsf_dropout_grid_elements', 'dsf_dropout', 'dsf_dropout_add_keep', 'dsf_dropout_add_keep_bwd',
               'dsf_cwt2f0', 'dsf_cwt2f0_bwd', 'dsf_cwt_pitch_loss_workspace_floats', 'dsf_cwt_pitch_loss', 'dsf_cwt_pitch_loss_bwd']

# every symbol include/dsv.h declares (the HiFi-GAN / NSF-HiFi-GAN generator ops)
SYMBOLS_VOC = ['dsv_padded_samples', 'dsv_packed_floats', 'dsv_pack_weight', 'dsv_pad_rows', 'dsv_conv1d', 'dsv_conv1d_multi', 'dsv_set_lean', 'dsv_noise_conv', 'dsv_sine_source',
               'dsv_fold_factor', 'dsv_set_fold', 'dsv_conv1d_folded', 'dsv_chain_fold', 'dsv_chain_supported', 'dsv_resblock_chain', 'dsv_resblock_chain_multi', 'dsv_resblock_chain_sum', 'dsv_set_chain_variant', 'dsv_debug_chain_timeline',
               'dsv_pwg_first', 'dsv_pwg_upsample', 'dsv_pwg_layer',
               'dsv_stft_basis_floats', 'dsv_stft_make_basis', 'dsv_stft_frames', 'dsv_stft', 'dsv_istft_samples', 'dsv_istft_workspace_floats', 'dsv_istft',
               'dsv_logmel',
               'dsv_stft_make_adjoint_basis', 'dsv_stft_adjoint_workspace_floats', 'dsv_stft_adjoint', 'dsv_spectral_loss_workspace_floats', 'dsv_spectral_loss',
               'dsv_spectral_loss_backward',
               'dsv_mel_spectrum', 'dsv_mel_head', 'dsv_mel_head_backward', 'dsv_mel_clamp_backward',
               'dsv_pwgd_tile', 'dsv_pwgd_wgrad_split', 'dsv_pwgd_wgrad_workspace_floats', 'dsv_pwgd_edge_workspace_floats', 'dsv_pwgd_layer', 'dsv_pwgd_wgrad',
               'dsv_pwgd_first', 'dsv_pwgd_first_backward', 'dsv_pwgd_last', 'dsv_pwgd_last_backward', 'dsv_pwgd_lsgan_workspace_floats', 'dsv_pwgd_lsgan',
               'dsv_pwgd_lsgan_backward',
               'dsv_pwgt_wgrad_split', 'dsv_pwgt_wgrad_workspace_floats', 'dsv_pwgt_upsample_workspace_floats', 'dsv_pwgt_layer', 'dsv_pwgt_gate_backward',
               'dsv_pwgt_conv_backward', 'dsv_pwgt_wgrad_conv', 'dsv_pwgt_wgrad_out', 'dsv_pwgt_wgrad_relu', 'dsv_pwgt_rowdot', 'dsv_pwgt_last_dgrad',
               'dsv_pwgt_relu_mask', 'dsv_pwgt_upsample_backward', 'dsv_pwgt_convin_wgrad',
               'dsv_hgt_wgrad_split', 'dsv_hgt_act_floats', 'dsv_hgt_wgrad_workspace_floats', 'dsv_hgt_conv_dgrad', 'dsv_hgt_conv_wgrad', 'dsv_hgt_bias_workspace_floats', 'dsv_hgt_bias_grad',
               'dsv_hgt_upsample_dgrad', 'dsv_hgt_tanh_backward', 'dsv_hgt_noise_conv_backward', 'dsv_hgt_source_mix', 'dsv_hgt_source_backward',
               'dsv_hgd_pool_samples', 'dsv_hgd_avgpool', 'dsv_hgd_avgpool_backward',
               'dsv_hgp_height', 'dsv_hgp_folded_samples', 'dsv_hgp_fold', 'dsv_hgp_fold_backward', 'dsv_hgp_edge_workspace_floats', 'dsv_hgp_first',
               'dsv_hgp_first_backward', 'dsv_hgp_post', 'dsv_hgp_post_backward', 'dsv_hgp_dgrad_phase_taps', 'dsv_hgp_dgrad_packed_offset', 'dsv_hgp_conv',
               'dsv_hgp_conv_dgrad', 'dsv_hgp_wgrad_splits', 'dsv_hgp_wgrad_workspace_floats', 'dsv_hgp_conv_wgrad', 'dsv_hgp_l1_blocks',
               'dsv_hgp_l1_partial', 'dsv_hgp_l1_final', 'dsv_hgp_l1_backward',
               'dsv_hgs_out_len', 'dsv_hgs_first_workspace_floats', 'dsv_hgs_first', 'dsv_hgs_first_backward', 'dsv_hgs_packed_floats', 'dsv_hgs_pack',
               'dsv_hgs_gconv', 'dsv_hgs_gconv_dgrad', 'dsv_hgs_wgrad_splits', 'dsv_hgs_wgrad_workspace_floats', 'dsv_hgs_gconv_wgrad',
               'dsv_mt_chunk_floats', 'dsv_mt_table_tensors', 'dsv_mt_table_chunks', 'dsv_mt_set_table_limit', 'dsv_mt_workspace_floats', 'dsv_mt_grad_norm',
               'dsv_radam_scalars', 'dsv_mt_radam_step', 'dsv_mt_adamw_step']

_fp = C.POINTER(C.c_float)
_fpp = C.POINTER(C.c_void_p)


class DsdConfig(C.Structure):
    _fields_ = [('mel_bins', C.c_int32), ('residual_channels', C.c_int32), ('encoder_hidden', C.c_int32),
                ('residual_layers', C.c_int32), ('dilation_cycle_length', C.c_int32)]


class DsdWeights(C.Structure):
    _fields_ = [
        ('input_projection_w', C.c_void_p), ('input_projection_b', C.c_void_p),
        ('mlp0_w', C.c_void_p), ('mlp0_b', C.c_void_p), ('mlp2_w', C.c_void_p), ('mlp2_b', C.c_void_p),
        ('dilated_conv_w', _fpp), ('dilated_conv_b', _fpp),
        ('diffusion_projection_w', _fpp), ('diffusion_projection_b', _fpp),
        ('conditioner_projection_w', _fpp), ('conditioner_projection_b', _fpp),
        ('output_projection_w', _fpp), ('output_projection_b', _fpp),
        ('skip_projection_w', C.c_void_p), ('skip_projection_b', C.c_void_p),
        ('final_projection_w', C.c_void_p), ('final_projection_b', C.c_void_p),
    ]


_lib = None


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load (once) and type the library.  Raises RuntimeError when it is absent - build it with
    `python -m diffsinger_amd.build` (hipcc, gfx950)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(_LIB_PATH):
        raise RuntimeError(f'{_LIB_PATH} not found: the HIP denoiser library is not built '
                           f'(run `python -m diffsinger_amd.build`); there is no CPU fallback')
    # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as /opt/rocm's).  One process must
    # have ONE runtime: import torch first so that our library binds to the runtime torch's tensors live in.
    import torch  # noqa: F401
    lib = C.CDLL(_LIB_PATH)
    h = C.c_void_p
    lib.dsd_abi_version.restype = C.c_int
    lib.dsd_last_error.restype = C.c_char_p
    lib.dsd_build_id.restype = C.c_char_p
    lib.dsd_create.argtypes = [C.POINTER(DsdConfig), C.c_int, C.POINTER(h)]
    lib.dsd_destroy.argtypes = [h]
    lib.dsd_destroy.restype = None
    lib.dsd_load_weights.argtypes = [h, C.POINTER(DsdWeights), C.c_void_p]
    lib.dsd_set_schedule.argtypes = [h, C.POINTER(C.c_double), C.c_int32]
    lib.dsd_get_schedule_table.argtypes = [h, C.c_int32, _fp, C.c_int32]
    lib.dsd_set_spec_range.argtypes = [h, _fp, _fp]
    lib.dsd_prepare.argtypes = [h, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    lib.dsd_denoise.argtypes = [h, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    lib.dsd_q_sample.argtypes = [h, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.dsd_sample_ddpm.argtypes = [h, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.dsd_p_sample.argtypes = [h, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.dsd_sample_plms.argtypes = [h, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.dsd_norm_spec.argtypes = [h, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dsd_denorm_spec.argtypes = [h, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dsd_set_use_graph.argtypes = [h, C.c_int32]
    lib.dsd_set_layer_tile.argtypes = [h, C.c_int32]
    lib.dsd_time_layer_kernel.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, _fp, C.c_void_p]
    lib.dsd_debug_layer_timeline.argtypes = [h, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    lib.dsd_device_bytes.argtypes = [h]
    lib.dsd_device_bytes.restype = C.c_int64
    lib.dsd_get_layer_tile.argtypes = [h]
    lib.dsd_set_loop_mode.argtypes = [h, C.c_int32]
    lib.dsd_get_loop_mode.argtypes = [h]
    lib.dsd_loop_timeouts.argtypes = [h, C.c_void_p]
    lib.dsd_loop_launches.argtypes = [h]
    lib.dsd_check.argtypes = [h]
    lib.dsd_loop_parked.argtypes = [h]
    lib.dsd_debug_hold_cus.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.dsd_debug_condproj_groups.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    lib.dsd_set_lat_split.argtypes = [h, C.c_int32]
    lib.dsd_get_lat_split.argtypes = [h]
    lib.dsd_set_conv_mode.argtypes = [h, C.c_int32, C.c_int32]
    lib.dsd_get_conv_mode.argtypes = [h]
    lib.dsd_p_sample_ex.argtypes = [h, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p]
    lib.dsd_set_split_mode.argtypes = [h, C.c_int32, C.c_void_p]
    lib.dsd_get_split_mode.argtypes = [h]
    lib.dsd_debug_layer.argtypes = [h, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dsd_set_noise_seed.argtypes = [h, C.c_uint64]
    lib.dsd_philox_normal.argtypes = [h, C.c_uint64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    lib.dsd_debug_loop_timeline.argtypes = [h, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.dsf_padded_frames.argtypes = [i32]
    lib.dsf_padded_frames.restype = i32
    lib.dsf_packed_floats.argtypes = [i32, i32, i32]
    lib.dsf_packed_floats.restype = i64
    lib.dsf_pack_weight.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dsf_conv1d.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp]
    lib.dsf_layer_norm.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, i32, vp, vp]
    lib.dsf_attention.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsf_ln_bwd_workspace_floats.argtypes = [i32, i32]
    lib.dsf_ln_bwd_workspace_floats.restype = i64
    lib.dsf_layer_norm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp]
    lib.dsf_attention_bwd_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsf_attention_bwd_workspace_floats.restype = i64
    lib.dsf_attention_bwd.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsf_set_conv_split.argtypes = [i32]
    lib.dsf_linear_rows_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsf_linear_rows_workspace_floats.restype = i64
    lib.dsf_linear_rows.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_linear_rows_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_to_channel_major.argtypes = [vp, i64, i64, i64, vp, i32, i32, i32, vp]
    lib.dsf_from_channel_major.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.dsf_positions.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsf_input_cm.argtypes = [vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dsf_gather_frames.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsf_sum_embed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_token_masks.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.dsf_q_sample_rows.argtypes = [vp, vp, vp, vp, vp, i32, vp, i32, i64, vp]
    lib.dsf_l1_workspace_floats.argtypes = []
    lib.dsf_l1_workspace_floats.restype = i64
    lib.dsf_l1_mean.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.dsf_l1_mean_bwd.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.dsf_pitch_coarse.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, C.c_double, C.c_double, i32, i32, i32, vp]
    lib.dsf_p_sample.argtypes = [vp, vp, vp, i64, f32, f32, f32, f32, f32, vp]
    lib.dsf_denorm_spec.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_conv1d_dilated.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.dsf_wgrad_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsf_wgrad_workspace_floats.restype = i64
    lib.dsf_conv1d_wgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dsf_bias_grad.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    lib.dsf_train_add_step.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_train_rowsum.argtypes = [vp, vp, i32, i32, vp]
    lib.dsf_train_gate.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.dsf_train_gate_bwd.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_train_res_skip.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_train_res_skip_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_adamw_step.argtypes = [vp, vp, vp, vp, i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, i64, vp, vp]
    lib.dsf_channel_affine.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsf_group_norm.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, vp]
    lib.dsf_batch_norm_train.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp]
    lib.dsf_batch_norm_train_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsf_group_norm_bwd_workspace_floats.argtypes = [i32, i32]
    lib.dsf_group_norm_bwd_workspace_floats.restype = i64
    lib.dsf_group_norm_bwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, vp]
    lib.dsf_f0_loss_workspace_floats.argtypes = []
    lib.dsf_f0_loss_workspace_floats.restype = i64
    lib.dsf_f0_loss.argtypes = [vp, i64, i64, i64, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp]
    lib.dsf_f0_loss_bwd.argtypes = [vp, i64, i64, i64, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp]
    lib.dsf_fs2_loss_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsf_fs2_loss_workspace_floats.restype = i64
    lib.dsf_mel_loss.argtypes = [vp, i64, i64, vp, i64, i64, i32, i32, i32, f32, i32, i32, f32, f32, vp, vp, vp, vp]
    lib.dsf_mel_loss_bwd.argtypes = [vp, i64, i64, vp, i64, i64, i32, i32, i32, f32, i32, i32, f32, f32, vp, vp, vp, vp, vp]
    lib.dsf_dur_loss.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp]
    lib.dsf_dur_loss_bwd.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp]
    lib.dsf_length_regulate.argtypes = [vp, vp, f32, vp, f32, vp, vp, vp, i32, i32, i32, vp]
    u32 = C.c_uint32
    lib.dsf_dropout_grid_elements.argtypes = []
    lib.dsf_dropout_grid_elements.restype = i64
    lib.dsf_dropout.argtypes = [vp, vp, i64, vp, u32, u32, f32, vp]
    lib.dsf_dropout_add_keep.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, u32, u32, f32, vp]
    lib.dsf_dropout_add_keep_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, u32, u32, f32, vp]
    lib.dsf_cwt2f0.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, f32, f32, vp]
    lib.dsf_cwt2f0_bwd.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, i32, i32, i32, f32, i32, f32, f32, vp]
    lib.dsf_cwt_pitch_loss_workspace_floats.argtypes = []
    lib.dsf_cwt_pitch_loss_workspace_floats.restype = i64
    lib.dsf_cwt_pitch_loss.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp]
    lib.dsf_cwt_pitch_loss_bwd.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]
    lib.dsv_padded_samples.argtypes = [i32]
    lib.dsv_padded_samples.restype = i32
    lib.dsv_packed_floats.argtypes = [i32, i32, i32]
    lib.dsv_packed_floats.restype = i64
    lib.dsv_pack_weight.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dsv_pad_rows.argtypes = [vp, vp, i64, i32, vp]
    lib.dsv_conv1d.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp, f32, i32, vp]
    lib.dsv_fold_factor.argtypes = [i32, i32, i32, i32]
    lib.dsv_fold_factor.restype = i32
    lib.dsv_set_fold.argtypes = [i32]
    lib.dsv_conv1d_folded.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp, f32, i32, vp]
    lib.dsv_chain_fold.argtypes = [i32]
    lib.dsv_chain_fold.restype = i32
    lib.dsv_chain_supported.argtypes = [i32, i32, i32, vp]
    lib.dsv_chain_supported.restype = i32
    lib.dsv_resblock_chain.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, f32, f32, vp]
    lib.dsv_conv1d_multi.argtypes = [i32, vp, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_set_lean.argtypes = [i32]
    lib.dsv_resblock_chain_multi.argtypes = [vp, vp, vp, C.POINTER(vp), i32, i32, i32, i32, i32, vp, f32, vp]
    lib.dsv_resblock_chain_sum.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, f32, f32, vp]
    lib.dsv_set_chain_variant.argtypes = [i32, i32, i32]
    lib.dsv_debug_chain_timeline.argtypes = [vp]
    lib.dsv_noise_conv.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_sine_source.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, vp]
    lib.dsv_pwg_first.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsv_pwg_upsample.argtypes = [vp, vp, vp, i64, i32, i32, vp]
    lib.dsv_pwg_layer.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dsv_stft_basis_floats.argtypes = [i32, i32]
    lib.dsv_stft_basis_floats.restype = i64
    lib.dsv_stft_make_basis.argtypes = [i32, i32, vp, vp, vp]
    lib.dsv_stft_frames.argtypes = [i64, i32, i32, i32, i32]
    lib.dsv_stft_frames.restype = i64
    lib.dsv_stft.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_istft_samples.argtypes = [i64, i32, i32, i32]
    lib.dsv_istft_samples.restype = i64
    lib.dsv_istft_workspace_floats.argtypes = [i32, i64, i32]
    lib.dsv_istft_workspace_floats.restype = i64
    lib.dsv_istft.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_logmel.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, f32, i32, vp]
    lib.dsv_stft_make_adjoint_basis.argtypes = [i32, i32, vp, vp]
    lib.dsv_stft_adjoint_workspace_floats.argtypes = [i32, i64, i32]
    lib.dsv_stft_adjoint_workspace_floats.restype = i64
    lib.dsv_stft_adjoint.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_spectral_loss_workspace_floats.argtypes = [i64]
    lib.dsv_spectral_loss_workspace_floats.restype = i64
    lib.dsv_spectral_loss.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.dsv_spectral_loss_backward.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    lib.dsv_mel_spectrum.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_mel_head.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, i32, vp]
    lib.dsv_mel_head_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, i32, vp]
    lib.dsv_mel_clamp_backward.argtypes = [vp, vp, vp, i64, vp]
    lib.dsv_pwgd_tile.argtypes = []
    lib.dsv_pwgd_tile.restype = i32
    lib.dsv_pwgd_wgrad_split.argtypes = []
    lib.dsv_pwgd_wgrad_split.restype = i32
    lib.dsv_pwgd_wgrad_workspace_floats.argtypes = [i32, i32]
    lib.dsv_pwgd_wgrad_workspace_floats.restype = i64
    lib.dsv_pwgd_edge_workspace_floats.argtypes = [i32, i32]
    lib.dsv_pwgd_edge_workspace_floats.restype = i64
    lib.dsv_pwgd_layer.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, vp]
    lib.dsv_pwgd_wgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsv_pwgd_first.argtypes = [vp, vp, vp, vp, i32, i32, f32, vp]
    lib.dsv_pwgd_first_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    lib.dsv_pwgd_last.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.dsv_pwgd_last_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]
    lib.dsv_pwgd_lsgan_workspace_floats.argtypes = [i64]
    lib.dsv_pwgd_lsgan_workspace_floats.restype = i64
    lib.dsv_pwgd_lsgan.argtypes = [vp, f32, vp, vp, i64, vp]
    lib.dsv_pwgd_lsgan_backward.argtypes = [vp, f32, vp, vp, i64, vp]
    lib.dsv_pwgt_wgrad_split.argtypes = []
    lib.dsv_pwgt_wgrad_split.restype = i32
    lib.dsv_pwgt_wgrad_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsv_pwgt_wgrad_workspace_floats.restype = i64
    lib.dsv_pwgt_upsample_workspace_floats.argtypes = [i64, i32]
    lib.dsv_pwgt_upsample_workspace_floats.restype = i64
    lib.dsv_pwgt_layer.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dsv_pwgt_gate_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    lib.dsv_pwgt_conv_backward.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dsv_pwgt_wgrad_conv.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsv_pwgt_wgrad_out.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    lib.dsv_pwgt_wgrad_relu.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    lib.dsv_pwgt_rowdot.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_pwgt_last_dgrad.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsv_pwgt_relu_mask.argtypes = [vp, vp, vp, f32, i64, i32, vp]
    lib.dsv_pwgt_upsample_backward.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]
    lib.dsv_pwgt_convin_wgrad.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsv_hgt_wgrad_split.argtypes = []
    lib.dsv_hgt_wgrad_split.restype = i32
    lib.dsv_hgt_act_floats.argtypes = [i32, i32, i32]
    lib.dsv_hgt_act_floats.restype = i64
    lib.dsv_hgt_wgrad_workspace_floats.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.dsv_hgt_wgrad_workspace_floats.restype = i64
    lib.dsv_hgt_conv_dgrad.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, f32, vp]
    lib.dsv_hgt_conv_wgrad.argtypes = [vp, vp, vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgt_bias_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsv_hgt_bias_workspace_floats.restype = i64
    lib.dsv_hgt_bias_grad.argtypes = [vp, vp, i64, vp, i32, i32, i32, vp]
    lib.dsv_hgt_upsample_dgrad.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, vp]
    lib.dsv_hgt_tanh_backward.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.dsv_hgt_noise_conv_backward.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_hgt_source_mix.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, f32, f32, vp]
    lib.dsv_hgt_source_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.dsv_hgd_pool_samples.argtypes = [i32]
    lib.dsv_hgd_pool_samples.restype = i32
    lib.dsv_hgd_avgpool.argtypes = [vp, vp, i64, i32, i64, vp]
    lib.dsv_hgd_avgpool_backward.argtypes = [vp, vp, i64, i32, i64, vp]
    lib.dsv_hgp_height.argtypes = [i32, i32]
    lib.dsv_hgp_height.restype = i32
    lib.dsv_hgp_folded_samples.argtypes = [i32, i32]
    lib.dsv_hgp_folded_samples.restype = i64
    lib.dsv_hgp_fold.argtypes = [vp, vp, i32, i32, i64, i32, vp]
    lib.dsv_hgp_fold_backward.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.dsv_hgp_edge_workspace_floats.argtypes = [i32, i32, i32, i32, i32]
    lib.dsv_hgp_edge_workspace_floats.restype = i64
    lib.dsv_hgp_first.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgp_first_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dsv_hgp_post.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
    lib.dsv_hgp_post_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgp_dgrad_phase_taps.argtypes = [i32, i32]
    lib.dsv_hgp_dgrad_phase_taps.restype = i32
    lib.dsv_hgp_dgrad_packed_offset.argtypes = [i32, i32, i32, i32]
    lib.dsv_hgp_dgrad_packed_offset.restype = i64
    lib.dsv_hgp_conv.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgp_conv_dgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgp_wgrad_splits.argtypes = [i32, i32, i32, i32, i32]
    lib.dsv_hgp_wgrad_splits.restype = i32
    lib.dsv_hgp_wgrad_workspace_floats.argtypes = [i32, i32, i32, i32, i32]
    lib.dsv_hgp_wgrad_workspace_floats.restype = i64
    lib.dsv_hgp_conv_wgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.dsv_hgp_l1_blocks.argtypes = [i64]
    lib.dsv_hgp_l1_blocks.restype = i32
    lib.dsv_hgp_l1_partial.argtypes = [vp, vp, vp, i64, vp]
    lib.dsv_hgp_l1_final.argtypes = [vp, i32, vp, vp]
    lib.dsv_hgp_l1_backward.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    lib.dsv_hgs_out_len.argtypes = [i32, i32]
    lib.dsv_hgs_out_len.restype = i32
    lib.dsv_hgs_first_workspace_floats.argtypes = [i32, i32, i32]
    lib.dsv_hgs_first_workspace_floats.restype = i64
    lib.dsv_hgs_first.argtypes = [vp, vp, vp, vp, i32, i32, i32, i64, f32, vp]
    lib.dsv_hgs_first_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i64, vp]
    lib.dsv_hgs_packed_floats.argtypes = [i32, i32, i32, i32, i32]
    lib.dsv_hgs_packed_floats.restype = i64
    lib.dsv_hgs_pack.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.dsv_hgs_gconv.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgs_gconv_dgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]
    lib.dsv_hgs_wgrad_splits.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.dsv_hgs_wgrad_splits.restype = i32
    lib.dsv_hgs_wgrad_workspace_floats.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.dsv_hgs_wgrad_workspace_floats.restype = i64
    lib.dsv_hgs_gconv_wgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    f64 = C.c_double
    for name in ('dsv_mt_chunk_floats', 'dsv_mt_table_tensors', 'dsv_mt_table_chunks'):
        getattr(lib, name).argtypes = []
        getattr(lib, name).restype = i32
    lib.dsv_mt_set_table_limit.argtypes = [i32, i32]
    lib.dsv_mt_workspace_floats.argtypes = [vp, i64]
    lib.dsv_mt_workspace_floats.restype = i64
    lib.dsv_mt_grad_norm.argtypes = [vp, vp, i64, f64, vp, i64, vp, vp]
    lib.dsv_radam_scalars.argtypes = [i64, f64, f64, vp]
    lib.dsv_mt_radam_step.argtypes = [vp, vp, vp, vp, vp, i64, f64, f64, f64, f64, f64, i64, vp, vp]
    lib.dsv_mt_adamw_step.argtypes = [vp, vp, vp, vp, vp, i64, f64, f64, f64, f64, f64, i64, vp, vp]
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if fn.restype is C.c_int and name not in ('dsd_abi_version',):
            fn.restype = C.c_int
    if lib.dsd_abi_version() != DSD_ABI_VERSION:
        raise RuntimeError(f'libdsdenoise ABI {lib.dsd_abi_version()} != binding {DSD_ABI_VERSION}: rebuild')
    _lib = lib
    return lib


def build_id() -> str:
    """sha256 of the sources the loaded library was compiled from (dsd_build_id, include/dsd.h)."""
    return load().dsd_build_id().decode()


def check(rc: int, what: str = ''):
    if rc != 0:
        msg = load().dsd_last_error()
        raise RuntimeError(f'{what or "libdsdenoise"} failed ({rc}): {msg.decode() if msg else "?"}')


def call(name: str, dev, *args):
    """Entry point `name` on device `dev`: the arguments, then that device's current stream as the last one; raises on a refusal."""
    import torch
    lib = load()
    with torch.cuda.device(dev):
        check(getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)


def ptr(t):
    """a tensor's address, None (a null pointer) for None"""
    return t.data_ptr() if t is not None else None

"""ctypes binding of libdmad_hip.so (C ABI: include/dmad.h).

The HIP library is the product path.  There is NO fallback: if the shared object is missing or a
call fails, a DmadError is raised."""
from __future__ import annotations

import ctypes as C
import os

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG_ROOT, 'libdmad_hip.so')


class DmadError(RuntimeError):
    pass


class DmadConfig(C.Structure):
    """dmad_config of include/dmad.h; positional arguments are the fields AFTER struct_size, which is filled in here."""
    _fields_ = [(n, C.c_int32) for n in (
        'struct_size', 'res_channels', 'skip_channels', 'num_res_layers', 'dilation_cycle', 'embed_dim_in', 'embed_dim_mid',
        'embed_dim_out', 'clip_len', 'max_batch', 'num_classes', 'precision', 'with_classifier', 'recheck_batch', 'half_type',
        'with_wavenet')]

    def __init__(self, *fields, **named):
        if len(fields) < 15:
            named.setdefault('with_wavenet', 1)
        super().__init__(C.sizeof(type(self)), *fields, **named)


class DmadWaveDefense(C.Structure):
    """dmad_wave_defense of include/dmad.h (host pointers); struct_size is filled in here."""
    _PF = C.POINTER(C.c_float)
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'kind', 'window', 'order')] + [('down_ker', _PF)] +
                [(n, C.c_int32) for n in ('down_phases', 'down_taps', 'down_stride', 'down_width', 'down_len', 'up_phases', 'up_taps',
                                          'up_stride', 'up_width')] +
                [('up_ker', _PF), ('b', _PF), ('a', _PF), ('lo', C.c_float), ('hi', C.c_float)])

    def __init__(self, **named):
        super().__init__(**named)
        self.struct_size = C.sizeof(type(self))


_P = C.c_void_p
_PF = C.POINTER(C.c_float)
_SIGNATURES = {
    'dmad_create': (C.c_int, [C.POINTER(DmadConfig), C.POINTER(_P)]),
    'dmad_destroy': (None, [_P]),
    'dmad_last_error': (C.c_char_p, []),
    'dmad_version': (C.c_char_p, []),
    'dmad_last_warning': (C.c_char_p, []),
    'dmad_load_weight': (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    'dmad_finalize_weights': (C.c_int, [_P]),
    'dmad_wavenet_eps': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_one_shot': (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, C.c_int32, _P, _P]),
    'dmad_ddpm_step': (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, _P, C.c_uint64, C.c_uint64, C.c_int32, _P]),
    'dmad_diffuse': (C.c_int, [_P, _P, C.c_float, C.c_float, _P, C.c_uint64, C.c_uint64, C.c_int32, _P, _P]),
    'dmad_ddpm_purify': (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int32, _P, _P]),
    'dmad_unet_eps': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_unet_eps_tier': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_unet_p_sample': (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _P, C.c_uint64, C.c_uint64,
                                     C.c_int32, _P, _P]),
    'dmad_mel_db': (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    'dmad_mel_power': (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    'dmad_power_to_db': (C.c_int, [_P, _P, C.c_int64, _P, _P]),
    'dmad_classify': (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    'dmad_classify_tier': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_conv_h16': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, _P, _P, _P]),
    'dmad_conv_h16_up2': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_split_f16': (C.c_int, [_P, C.c_int64, _P, _P]),
    'dmad_conv_x3': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                               C.c_int32, _P, _P]),
    'dmad_conv_h16_stats': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_groupnorm16_apply': (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_qkv_attention_h16': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_groupnorm16': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_conv1ch_3x3': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_conv3x3_c128_to1': (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_float, C.c_float, _P, _P]),
    'dmad_conv3x3_c128_to1_h16': (C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    'dmad_upsample2x': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_conv_f32': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, _P, C.c_int64, C.c_int64, _P, _P, _P]),
    'dmad_conv_f32_vjp': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, _P, _P, _P, _P, _P]),
    'dmad_groupnorm_f32': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_groupnorm_bwd': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_qkv_attention_f32': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_qkv_attention_bwd': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_rx_head_bwd': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_rx_conv1_bwd': (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P]),
    'dmad_vgg_pool_relu_bwd': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_smooth_votes': (C.c_int, [_P, _P, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_int64, C.c_int32,
                                    C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P]),
    'dmad_rs_smooth_votes': (C.c_int, [_P, _P, C.c_float, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    'dmad_set_mode': (C.c_int, [_P, C.c_int32]),
    'dmad_set_waveform_tier': (C.c_int, [_P, C.c_int32]),
    'dmad_set_recheck_margin': (C.c_int, [_P, C.c_float]),
    'dmad_set_recheck_margin2': (C.c_int, [_P, C.c_float]),
    'dmad_recheck_stats': (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    'dmad_wavenet_eps_path': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_reserve_vjp': (C.c_int, [_P, C.c_int32]),
    'dmad_wavenet_eps_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    # the any-length forms of the exact-fp32 DiffWave path: their twins' arguments with `len` after B
    'dmad_wavenet_eps_len': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_wavenet_eps_vjp_len': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_philox_normal_len': (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_diffuse_len': (C.c_int, [_P, _P, C.c_float, C.c_float, _P, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, _P, _P]),
    'dmad_ddpm_step_len': (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, C.c_float, _P, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, _P]),
    'dmad_ddpm_purify_len': (C.c_int, [_P, _P, C.c_int32, C.c_float, C.c_float, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, _P,
                                       _P]),
    'dmad_reserve_unet_vjp': (C.c_int, [_P, C.c_int32]),
    'dmad_unet_eps_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_reserve_classifier_vjp': (C.c_int, [_P, C.c_int32]),
    'dmad_classify_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'dmad_mel_db_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'dmad_masking_loss_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    'dmad_masking_step': (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.c_int32, _P, _P, _P, _P]),
    'dmad_reserve_vgg_vjp': (C.c_int, [_P, C.c_int32]),
    'dmad_vgg_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'dmad_vgg_vjp_tape': (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_reserve_wrn_vjp': (C.c_int, [_P, C.c_int32]),
    'dmad_wrn_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'dmad_wrn_vjp_tape': (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_reserve_dn_vjp': (C.c_int, [_P, C.c_int32]),
    'dmad_dn_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'dmad_dn_vjp_tape': (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_dn_pw': (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int64, _P, _P, _P, _P, _P, C.c_int32, _P]),
    'dmad_dn_pw_bwd': (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P, C.c_int32,
                                 C.c_int32, _P]),
    'dmad_dn_growth': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    'dmad_dn_growth_bwd': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_dn_stem': (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    'dmad_dn_stem_bwd': (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P]),
    'dmad_dn_pool': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'dmad_dn_preact': (C.c_int, [_P, C.c_int32, _P, _P, C.c_int64, C.c_int32, _P, _P]),
    'dmad_dn_head': (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_dn_head_bwd': (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'dmad_wrn_preact': (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, _P, _P]),
    'dmad_wrn_preact_bwd': (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, _P, _P]),
    'dmad_wrn_stem': (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    'dmad_wrn_stem_bwd': (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    'dmad_vpsde_purify': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64,
                                    C.c_int32, _P, _P, _P]),
    'dmad_vpsde_purify_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    'dmad_spec_vpsde_purify': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P, C.c_uint64,
                                         C.c_uint64, C.c_int32, _P, _P, _P]),
    'dmad_spec_vpsde_purify_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P, _P, _P, _P, _P, _P]),
    'dmad_eval_samples': (C.c_int, [_P, _P, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_uint64, _P, _P, C.c_int64,
                                    C.c_int32, _P, _P, _P]),
    'dmad_debug_rounding': (C.c_int, [_P, C.POINTER(C.c_int32)]),
    'dmad_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P,
                                    C.c_uint64, C.c_uint64, _P, _P, _P]),
    'dmad_spec_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P, C.c_float, C.c_float,
                                         C.c_uint64, C.c_uint64, _P, _P, _P]),
    'dmad_spec_smooth_votes': (C.c_int, [_P, _P, C.c_float, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P, C.c_float, C.c_float,
                                         C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    'dmad_spec_eval_samples': (C.c_int, [_P, _P, C.c_float, C.c_int32, C.c_float, C.c_float, _P, _P, _P, _P, _P, C.c_float, C.c_float,
                                         C.c_uint64, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    'dmad_set_spec_recheck_margin': (C.c_int, [_P, C.c_float]),
    'dmad_spec_recheck_stats': (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    'dmad_set_spec_recheck_margin2': (C.c_int, [_P, C.c_float]),
    'dmad_spec_recheck_stats2': (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    'dmad_nes_probes': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, _P, _P]),
    'dmad_nes_grad': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int32, _P, _P]),
    'dmad_philox_uniform': (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, _P, _P]),
    'dmad_pso_init': (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_uint64, C.c_uint64, _P, _P, _P, _P, _P]),
    'dmad_pso_step': (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_uint64,
                                _P, _P, _P, _P]),
    'dmad_pso_update_best': (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P]),
    'dmad_wave_rfft': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    'dmad_wave_irfft_threshold': (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P]),
    'dmad_kenan_update': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    'dmad_wave_smooth': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_wave_smooth_vjp': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_wave_resample': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_wave_resample_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_wave_iir': (C.c_int, [_P, _P, C.c_int32, _PF, _PF, C.c_int32, C.c_float, C.c_float, _P, _P]),
    'dmad_wave_iir_vjp': (C.c_int, [_P, _P, _P, C.c_int32, _PF, _PF, C.c_int32, C.c_float, C.c_float, _P, _P, _P]),
    'dmad_defense_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(DmadWaveDefense), _P, _P, _P]),
    'dmad_m5_logits': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P]),
    'dmad_m5_vjp': (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    'dmad_m5_tape': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_m5_rs_smooth_votes': (C.c_int, [_P, _P, C.c_float, C.c_int64, C.c_uint64, C.c_uint64, _P, _P, _P, _P]),
    'dmad_kws_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_kws_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_kws_tape': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    'dmad_kws_mel_power': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_kws_mel_db': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    'dmad_kws_mel_db_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_kws_wave_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    'dmad_kws_wave_vjp': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    'dmad_kws_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P,
                                        C.c_uint64, C.c_uint64, _P, _P, _P]),
    'dmad_kws_defense_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(DmadWaveDefense), _P, _P, _P]),
    'dmad_m5_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P, _P,
                                       C.c_uint64, C.c_uint64, _P, _P, _P]),
    'dmad_m5_defense_query_logits': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(DmadWaveDefense), _P, _P, _P]),
    'dmad_vote': (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    'dmad_philox_raw': (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _P, _P]),
    'dmad_philox_normal': (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int32, _P, _P]),
    'dmad_time_layer': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), _P]),
    'dmad_device_bytes': (C.c_int64, [_P]),
    'dmad_profile_layers': (C.c_int, [_P, C.c_int32]),
    'dmad_profile_read': (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    'dmad_profile_read_final': (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
}
EXPORTS = tuple(_SIGNATURES)

_lib = None


def load():
    """Load (once) and return the ctypes library.  torch must be imported first so that the HIP
    runtime already mapped by torch (same SONAME libamdhip64.so.7) is the one the library binds to."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DmadError('HIP extension missing: %s (build it with `python -c "import __graft_entry__ as g; g.build()"` '
                        'or `make -C diffusion-model-for-audio-defense_amd/csrc`); there is no CPU fallback' % LIB_PATH)
    import torch  # noqa: F401  (maps torch's libamdhip64 first)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        msg = load().dmad_last_error()
        raise DmadError('dmad call failed (%d): %s' % (rc, msg.decode() if msg else '?'))

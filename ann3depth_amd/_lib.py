"""ctypes binding of liba3d.so (include/a3d.h).  Fails loudly when the library is missing or lacks a symbol."""
import collections
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint32, c_void_p, POINTER

# A3D_LIB points the binding at another build of the same library (tools/bench_layers.py A/B runs); there is still no
# fallback: a missing file or symbol raises.
LIB_PATH = os.environ.get('A3D_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'liba3d.so')


class A3dError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    """struct a3d_conv_desc"""
    _fields_ = [(n, c_int32) for n in ('n', 'h', 'w', 'c', 'k', 'r', 's', 'stride', 'pad_t', 'pad_l', 'ho', 'wo',
                                       'ldx', 'ldy', 'precision', 'storage', 'hints')]


class SecondOutput(ctypes.Structure):
    """struct a3d_second_output"""
    _fields_ = [('ptr', c_void_p), ('ld', c_int32), ('step', c_int32), ('offset', c_int32), ('bf16', c_int32), ('cols', c_int32)]


class ExampleView(ctypes.Structure):
    """struct a3d_example_view"""
    _fields_ = [('image_height', c_int64), ('image_width', c_int64), ('image_channels', c_int64),
                ('depth_height', c_int64), ('depth_width', c_int64), ('depth_channels', c_int64),
                ('image', c_void_p), ('image_bytes', c_size_t), ('depth', c_void_p), ('depth_bytes', c_size_t)]


class TimingRecord(ctypes.Structure):
    """struct a3d_timing_record"""
    _fields_ = [(n, c_int32) for n in ('mode', 'bm', 'bn', 'waves_m', 'nwaves', 'bk', 'avec', 'bvec', 'prec', 'lds_dma', 'splitk', 'm', 'n', 'k')] + \
               [('ms', c_float), ('flops', ctypes.c_double)]


_P = c_void_p
_D = POINTER(ConvDesc)

# name -> (restype, argtypes); every symbol include/a3d.h declares
SIGNATURES = {
    'a3d_version': (c_char_p, []),
    'a3d_last_error': (c_int, [c_char_p, c_size_t]),
    'a3d_conv2d_fwd_ws_bytes': (c_size_t, [_D]),
    'a3d_conv2d_fwd': (c_int, [_D, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    'a3d_conv2d_bwd_data_ws_bytes': (c_size_t, [_D]),
    'a3d_conv2d_bwd_data': (c_int, [_D, _P, _P, _P, _P, _P, c_size_t, _P]),
    'a3d_conv2d_bwd_filter_ws_bytes': (c_size_t, [_D]),
    'a3d_conv2d_bwd_filter': (c_int, [_D, _P, _P, _P, _P, _P, c_size_t, _P]),
    'a3d_conv2d_fwd_prepared_filter_bytes': (c_size_t, [_D]),
    'a3d_conv2d_fwd_prepare_filter': (c_int, [_D, _P, _P, c_size_t, _P]),
    'a3d_conv2d_bwd_filter_pooled_ws_bytes': (c_size_t, [_D]),
    'a3d_conv2d_bwd_filter_pooled': (c_int, [_D, _P, _P, c_int, _P, _P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    'a3d_conv2d_bwd_both_supported': (c_int, [_D]),
    'a3d_conv2d_bwd_both_ws_bytes': (c_size_t, [_D]),
    'a3d_conv2d_bwd_both': (c_int, [_D, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    'a3d_dense_fwd_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'a3d_dense_fwd': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P, _P, c_size_t, _P]),
    'a3d_dense_bwd_data_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'a3d_dense_bwd_data': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_float, _P, c_size_t, _P]),
    'a3d_dense_bwd_filter_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'a3d_dense_bwd_filter': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    'a3d_maxpool2x2_fwd': (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P]),
    'a3d_maxpool2x2_bwd': (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P]),
    'a3d_resize_bilinear_tf1': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, _P, _P]),
    'a3d_resize_bilinear_tf1_pair': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, _P, c_int, c_int, _P, _P]),
    'a3d_resize_bilinear_tf1_ex': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int, c_int,
                                           _P, _P]),
    'a3d_warp_bilinear_pair': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int, c_int,
                                       _P, _P, _P]),
    'a3d_extract_patches': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, _P, _P]),
    'a3d_silog_loss_fwd': (c_int, [c_int, c_int, _P, _P, _P, _P, _P]),
    'a3d_silog_loss_bwd': (c_int, [c_int, c_int, _P, _P, _P, _P, _P]),
    'a3d_dropout_keep_mask': (c_int, [c_size_t, ctypes.c_uint64, ctypes.c_uint64, c_float, _P, _P]),
    'a3d_adam_apply_tf1': (c_int, [c_size_t, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, c_float,
                                   c_float, _P]),
    'a3d_adam_apply_tf1_flag': (c_int, [c_size_t, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, c_float,
                                        c_float, _P, _P]),
    'a3d_dense_fwd_ex': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P, c_int, c_int, _P, c_size_t, _P]),
    'a3d_dense_bwd_data_ex': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_float, c_int, c_int, _P, c_size_t, _P]),
    'a3d_dense_fwd_ex2': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_int, c_int, _P, c_int, c_int, POINTER(SecondOutput), _P,
                                  c_size_t, _P]),
    'a3d_dense_bwd_data_ex2': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, c_float, c_int, c_int, POINTER(SecondOutput), _P,
                                       c_size_t, _P]),
    'a3d_conv2d_fwd_ex2': (c_int, [_D, _P, _P, _P, _P, c_int, POINTER(SecondOutput), _P, c_size_t, _P]),
    'a3d_silog_loss_bwd_ex': (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, _P]),
    'a3d_depth_metrics_ws_bytes': (c_size_t, [c_int, c_int, c_int]),
    'a3d_depth_metrics': (c_int, [c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, c_float, c_float, c_float, c_float, _P, _P,
                                  c_size_t, _P]),
    'a3d_cast_bf16': (c_int, [c_size_t, _P, _P, c_int, _P]),
    'a3d_cast_rows': (c_int, [c_size_t, c_int, _P, c_int, c_int, _P, c_int, c_int, _P]),
    'a3d_pad_channels_bf16': (c_int, [c_size_t, c_int, _P, c_int, _P, _P]),
    'a3d_stream_create': (c_int, [c_int, ctypes.POINTER(ctypes.c_void_p)]),
    'a3d_stream_destroy': (c_int, [_P]),
    'a3d_maxpool2x2_fwd_bf16': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, _P]),
    'a3d_maxpool2x2_bwd_bf16': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P, c_int, _P]),
    'a3d_copy_channel_bf16': (c_int, [c_size_t, _P, c_int, c_int, _P, c_int, c_int, _P]),
    'a3d_maxpool2x2_bwd_idx_bf16': (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, c_int, _P]),
    'a3d_maxpool2x2_bwd_idx_bf16s': (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, c_int, _P]),
    'a3d_dense_bwd_filter_adam_tf1': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_float, c_float, c_float,
                                              c_float, c_float, c_float, _P]),
    'a3d_dense_bwd_filter_adam_tf1_ex': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_float, c_float, c_float,
                                                 c_float, c_float, c_float, c_int, _P]),
    'a3d_superpixel_mean': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P]),
    'a3d_superpixel_hist': (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P]),
    'a3d_pair_similarity': (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, _P, c_int, _P, _P, c_float, _P, _P, _P]),
    'a3d_crf_loss': (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, c_float, _P, _P, _P, _P]),
    'a3d_crf_map': (c_int, [c_int, c_int, _P, _P, _P, _P, c_int, _P, _P, _P]),
    'a3d_sgd_apply': (c_int, [c_size_t, _P, _P, c_float, _P]),
    'a3d_conv2d_pool_fwd': (c_int, [_D, _P, _P, _P, _P, c_int, _P, c_int, _P, c_size_t, _P]),
    'a3d_maxpool2x2_bwd_idx': (c_int, [c_int, c_int, c_int, c_int, _P, _P, c_int, _P, c_int, _P, c_int, _P]),
    'a3d_copy_channel': (c_int, [c_size_t, _P, c_int, c_int, _P, c_int, c_int, _P]),
    'a3d_comm_standin': (c_int, [_P, c_size_t, _P, c_size_t, c_int, c_float, _P]),
    'a3d_timing_enable': (c_int, [c_int]),
    'a3d_timing_collect': (c_int, [POINTER(TimingRecord), c_int]),
    'a3d_timing_select': (c_int, [POINTER(TimingRecord)]),
    'a3d_crc32c': (c_uint32, [_P, c_size_t]),
    'a3d_masked_crc32c': (c_uint32, [_P, c_size_t]),
    'a3d_tfrecord_next': (c_int, [_P, c_size_t, c_int, POINTER(c_size_t), POINTER(c_size_t), POINTER(c_size_t)]),
    'a3d_example_parse': (c_int, [_P, c_size_t, POINTER(ExampleView)]),
    'a3d_decode_raw_plus_half': (c_int, [_P, c_size_t, _P]),
    'a3d_record_decode': (c_int, [_P, c_size_t, c_int, _P, c_size_t, _P, c_size_t, POINTER(ExampleView)]),
    'a3d_record_decode_u8': (c_int, [_P, c_size_t, c_int, _P, _P, c_size_t, _P, _P, c_size_t, POINTER(ExampleView),
                                     POINTER(c_int)]),
    'a3d_records_decode': (c_int, [POINTER(c_void_p), POINTER(c_size_t), c_int, c_int, POINTER(c_int64), _P, _P, _P, _P,
                                   POINTER(c_int32), c_int, POINTER(c_int32)]),
    'a3d_h2d_gather': (c_int, [_P, _P, POINTER(c_int32), c_int, c_int, c_size_t, _P]),
    'a3d_sizeof_conv_desc': (c_size_t, []),
    'a3d_example_write': (c_int64, [_P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_size_t]),
}

# name -> (restype, argtypes); every symbol include/a3d_valid.h declares (NON-REFERENCE extension, prefix a3dx_)
EXT_SIGNATURES = {
    'a3dx_resize_bilinear_tf1_valid': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int,
                                               c_int, _P, c_float, c_float, _P]),
    'a3dx_warp_bilinear_pair_valid': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int,
                                              c_int, _P, _P, c_float, c_float, _P]),
    'a3dx_silog_masked_loss_fwd': (c_int, [c_int, c_int, _P, _P, _P, _P, _P]),
    'a3dx_silog_masked_loss_bwd_ex': (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_pairwise.h declares (NON-REFERENCE extension, prefix a3dp_)
PAIR_SIGNATURES = {
    'a3dp_crf_loss_grad': (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, c_float, _P, _P, _P, _P, _P]),
    'a3dp_pair_dense_bwd': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    'a3dp_sgd_apply_floor': (c_int, [c_size_t, _P, _P, c_float, c_float, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_texture.h declares (NON-REFERENCE extension, prefix a3dt_)
TEXTURE_SIGNATURES = {
    'a3dt_superpixel_lbp_hist': (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P]),
    'a3dt_pair_similarity3': (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P, c_int, _P, _P, c_float, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_gradloss.h declares (NON-REFERENCE extension, prefix a3dg_)
GRADLOSS_SIGNATURES = {
    'a3dg_silog_grad_loss_fwd': (c_int, [c_int, c_int, c_int, _P, _P, c_int, c_float, _P, _P, _P]),
    'a3dg_silog_grad_loss_bwd_ex': (c_int, [c_int, c_int, c_int, _P, _P, c_int, c_float, _P, _P, _P, c_int, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_berhu.h declares (NON-REFERENCE extension, prefix a3dh_)
BERHU_SIGNATURES = {
    'a3dh_berhu_loss_fwd': (c_int, [c_int, c_int, _P, _P, c_int, c_float, _P, _P, _P]),
    'a3dh_berhu_loss_bwd_ex': (c_int, [c_int, c_int, _P, _P, c_int, c_float, _P, _P, _P, c_int, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_align.h declares (NON-REFERENCE extension, prefix a3da_)
ALIGN_SIGNATURES = {
    'a3da_depth_align_ws_bytes': (c_size_t, [c_int, c_int, c_int, c_int]),
    'a3da_depth_align': (c_int, [c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, c_float, c_float, c_int, _P, _P, _P, _P,
                                 c_size_t, _P]),
    'a3da_depth_metrics_aligned': (c_int, [c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, c_float, c_float, c_float, c_float,
                                           _P, _P, _P, c_size_t, _P]),
    'a3da_affine_apply': (c_int, [c_int, c_int, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_ssi.h declares (NON-REFERENCE extension, prefix a3di_)
SSI_SIGNATURES = {
    'a3di_ssi_loss_fwd': (c_int, [c_int, c_int, _P, _P, c_int, _P, _P, _P]),
    'a3di_ssi_loss_bwd_ex': (c_int, [c_int, c_int, _P, _P, c_int, _P, _P, _P, c_int, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_crf_valid.h declares (NON-REFERENCE extension, prefix a3dv_)
CRF_VALID_SIGNATURES = {
    'a3dv_superpixel_mean_valid': (c_int, [c_int, c_int, c_int, _P, c_int, c_int, _P, _P, _P]),
    'a3dv_crf_loss_observed': (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_fcsp.h declares (NON-REFERENCE extension, prefix a3df_)
FCSP_SIGNATURES = {
    'a3df_superpixel_pool_fwd': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P]),
    'a3df_superpixel_pool_bwd': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_crf_band.h declares (NON-REFERENCE extension, prefix a3db_)
CRF_BAND_SIGNATURES = {
    'a3db_crf_band_nll': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P]),
    'a3db_crf_band_map': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, c_int, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_wino.h declares (prefix a3dw_)
WINO_SIGNATURES = {
    'a3dw_conv2d_bwd_data_prepared_filter_bytes': (c_size_t, [_D]),
    'a3dw_conv2d_bwd_data_prepare_filter': (c_int, [_D, _P, _P, c_size_t, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_wino_grad.h declares (prefix a3dwg_)
WINO_GRAD_SIGNATURES = {
    'a3dwg_conv2d_bwd_filter_ws_bytes': (c_size_t, [_D]),
    'a3dwg_conv2d_bwd_filter': (c_int, [_D, _P, _P, _P, _P, _P, c_size_t, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_wino1d.h declares (prefix a3dl_)
WINO1D_SIGNATURES = {
    'a3dl_conv2d_bwd_data_ws_bytes': (c_size_t, [_D]),
    'a3dl_conv2d_bwd_data': (c_int, [_D, _P, _P, _P, _P, _P, c_size_t, _P]),
    'a3dl_conv2d_bwd_filter_ws_bytes': (c_size_t, [_D]),
    'a3dl_conv2d_bwd_filter': (c_int, [_D, _P, _P, _P, _P, _P, c_size_t, _P]),
    'a3dl_conv2d_bwd_data_prepared_filter_bytes': (c_size_t, [_D]),
    'a3dl_conv2d_bwd_data_prepare_filter': (c_int, [_D, _P, _P, c_size_t, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_optim.h declares (NON-REFERENCE extension, prefix a3do_)
OPTIM_SIGNATURES = {
    'a3do_momentum_apply': (c_int, [c_size_t, _P, _P, _P, c_float, c_float, c_float, _P]),
    'a3do_dense_bwd_filter_momentum': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_float, c_float, c_float, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_clip.h declares (NON-REFERENCE extension, prefix a3dn_)
CLIP_SIGNATURES = {
    'a3dn_grad_norm_ws_bytes': (c_size_t, [c_size_t]),
    'a3dn_grad_norm_scale': (c_int, [c_size_t, _P, c_float, c_float, _P, _P, c_size_t, _P]),
    'a3dn_momentum_apply_ctl': (c_int, [c_size_t, _P, _P, _P, c_float, c_float, _P, _P]),
    'a3dn_adam_apply_tf1_ctl': (c_int, [c_size_t, _P, _P, _P, _P, c_float, c_float, c_float, c_float, c_float, c_float, _P, _P,
                                        _P]),
    'a3dn_sgd_apply_ctl': (c_int, [c_size_t, _P, _P, c_float, _P, _P]),
    'a3dn_sgd_apply_floor_ctl': (c_int, [c_size_t, _P, _P, c_float, c_float, _P, _P]),
}
CLIP_CTL_BYTES = 32                          # A3DN_CTL_BYTES: sumsq f64, norm f32, scale f32, skip u32, skipped u32, 8 reserved
CLIP_BLOCK_ELEMS, CLIP_MAX_BLOCKS = 4096, 1024      # A3DN_BLOCK_ELEMS, A3DN_MAX_BLOCKS


class WinoBwdPool(ctypes.Structure):
    """a3dwb_pool (include/a3d_wino_bwd.h): the 2x2 max pool below a layer, as the fused forward recorded it."""
    _fields_ = [('argmax', c_void_p), ('y', c_void_p), ('ldy', c_int), ('h2', c_int), ('w2', c_int)]


# name -> (restype, argtypes); every symbol include/a3d_wino_bwd.h declares (prefix a3dwb_)
WINO_BWD_SIGNATURES = {
    'a3dwb_sizeof_pool': (c_size_t, []),
    'a3dwb_conv2d_bwd_ws_bytes': (c_size_t, [_D, c_int, c_int]),
    'a3dwb_conv2d_bwd': (c_int, [_D, _P, _P, _P, _P, _P, _P, _P, ctypes.POINTER(WinoBwdPool), _P, c_size_t, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_upsample.h declares (NON-REFERENCE extension, prefix a3du_)
UPSAMPLE_SIGNATURES = {
    'a3du_joint_bilateral_upsample': (c_int, [c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, _P, _P, _P, _P, c_int, c_float,
                                              c_float, _P, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_posterior.h declares (NON-REFERENCE extension, prefix a3dc_)
POSTERIOR_SIGNATURES = {
    'a3dc_crf_band_posterior': (c_int, [c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, _P, _P, _P, _P, _P]),
}

# name -> (restype, argtypes); every symbol include/a3d_slic.h declares (NON-REFERENCE extension, prefix a3ds_)
SLIC_SIGNATURES = {
    'a3ds_label_mean': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    'a3ds_label_hist': (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, _P]),
    'a3ds_slic_update': (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    'a3ds_slic_assign': (c_int, [c_int, c_int, c_int, _P, c_int, _P, c_float, _P, _P]),
    'a3ds_slic_segment': (c_int, [c_int, c_int, c_int, _P, c_int, c_int, c_float, _P, _P, _P, _P]),
    'a3ds_pair_similarity': (c_int, [c_int, c_int, _P, _P, _P, _P, _P, c_int, _P, _P, c_float, _P, _P, _P]),
    'a3ds_label_pool_fwd': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, _P]),
    'a3ds_label_pool_bwd': (c_int, [c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_int, _P]),
}

# Every C surface of liba3d.so, in the order load() binds them: the prefix its names share, its header under include/, its
# dict above.  A new surface is one header, one dict and one line here; tests/test_abi_surfaces.py holds the list to the
# headers and to what load() binds.
Surface = collections.namedtuple('Surface', 'prefix header signatures')
SURFACES = (
    Surface('a3d_', 'a3d.h', SIGNATURES),
    Surface('a3dx_', 'a3d_valid.h', EXT_SIGNATURES),
    Surface('a3dp_', 'a3d_pairwise.h', PAIR_SIGNATURES),
    Surface('a3dt_', 'a3d_texture.h', TEXTURE_SIGNATURES),
    Surface('a3dg_', 'a3d_gradloss.h', GRADLOSS_SIGNATURES),
    Surface('a3dv_', 'a3d_crf_valid.h', CRF_VALID_SIGNATURES),
    Surface('a3df_', 'a3d_fcsp.h', FCSP_SIGNATURES),
    Surface('a3db_', 'a3d_crf_band.h', CRF_BAND_SIGNATURES),
    Surface('a3dw_', 'a3d_wino.h', WINO_SIGNATURES),
    Surface('a3du_', 'a3d_upsample.h', UPSAMPLE_SIGNATURES),
    Surface('a3dc_', 'a3d_posterior.h', POSTERIOR_SIGNATURES),
    Surface('a3dwg_', 'a3d_wino_grad.h', WINO_GRAD_SIGNATURES),
    Surface('a3ds_', 'a3d_slic.h', SLIC_SIGNATURES),
    Surface('a3dwb_', 'a3d_wino_bwd.h', WINO_BWD_SIGNATURES),
    Surface('a3dh_', 'a3d_berhu.h', BERHU_SIGNATURES),
    Surface('a3da_', 'a3d_align.h', ALIGN_SIGNATURES),
    Surface('a3di_', 'a3d_ssi.h', SSI_SIGNATURES),
    Surface('a3dl_', 'a3d_wino1d.h', WINO1D_SIGNATURES),
    Surface('a3do_', 'a3d_optim.h', OPTIM_SIGNATURES),
    Surface('a3dn_', 'a3d_clip.h', CLIP_SIGNATURES),
)

_lib = None


def load():
    """Load liba3d.so once and bind every declared entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise A3dError(f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                       f'or `make -C ann3depth_amd/csrc` (there is no fallback path)')
    # PyTorch bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Import it first so that liba3d.so binds to
    # the runtime copy torch initialises: two HIP runtimes in one process cannot both own the device.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in ((n, sig) for surface in SURFACES for n, sig in surface.signatures.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise A3dError(f'liba3d.so lacks symbol {name}: stale build?') from e
        fn.restype = res
        fn.argtypes = args
    if lib.a3d_sizeof_conv_desc() != ctypes.sizeof(ConvDesc):
        raise A3dError(f'liba3d.so reads a {lib.a3d_sizeof_conv_desc()}-byte a3d_conv_desc, this binding passes '
                       f'{ctypes.sizeof(ConvDesc)} bytes: stale build?')
    if lib.a3dwb_sizeof_pool() != ctypes.sizeof(WinoBwdPool):
        raise A3dError(f'liba3d.so reads a {lib.a3dwb_sizeof_pool()}-byte a3dwb_pool, this binding passes '
                       f'{ctypes.sizeof(WinoBwdPool)} bytes: stale build?')
    _lib = lib
    return lib


def last_error():
    buf = ctypes.create_string_buffer(512)
    load().a3d_last_error(buf, 512)
    return buf.value.decode(errors='replace')


def check(rc, what):
    if rc != 0:
        raise A3dError(f'{what} failed ({rc}): {last_error()}')

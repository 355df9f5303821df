"""ctypes binding of libonsetfp.so (include/onsetfp.h).

The shared library is built in-tree by ``csrc/Makefile`` (hipcc, gfx950).  There
is NO CPU fallback: if the library is missing, or a call fails, an exception is
raised.  PyTorch is used only to own device memory and streams; every pointer
handed to the library is a raw device address.
"""
import ctypes
import os
import subprocess
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libonsetfp.so"


class OnsetFPError(RuntimeError):
    pass


class DetectorParams(ctypes.Structure):
    _fields_ = [
        ("n_channels", ctypes.c_int32),
        ("block_size", ctypes.c_int32),
        ("floor_db", ctypes.c_float),
        ("hp_enabled", ctypes.c_int32),
        ("hp_b", ctypes.c_float * 5),
        ("hp_a", ctypes.c_float * 5),
        ("fast_attack", ctypes.c_float),
        ("fast_release", ctypes.c_float),
        ("slow_attack", ctypes.c_float),
        ("slow_release", ctypes.c_float),
        ("alpha_min", ctypes.c_float),
        ("alpha_max", ctypes.c_float),
        ("minmin", ctypes.c_float),
        ("min0", ctypes.c_float),
        ("max0", ctypes.c_float),
        ("manual", ctypes.c_int32),
        ("cooldown", ctypes.c_int64),
        ("backtrack", ctypes.c_int32),
        ("backtrack_buffer_size", ctypes.c_int64),
        ("backtrack_alpha", ctypes.c_float),
        ("backtrack_tol", ctypes.c_float),
    ]


class DetectTuning(ctypes.Structure):
    _fields_ = [
        ("hp_chunk", ctypes.c_int64), ("hp_warm", ctypes.c_int64),
        ("ar_chunk", ctypes.c_int64), ("ar_warm", ctypes.c_int64),
        ("mm_chunk", ctypes.c_int64), ("mm_warm", ctypes.c_int64),
        ("max_passes", ctypes.c_int32),
        ("ar_coarse_warm", ctypes.c_int64),
        ("hp_candidates", ctypes.c_int64),
        ("hp_candidate_offset", ctypes.c_int64),
        ("ar_guess", ctypes.c_int64),
        ("hp_span", ctypes.c_int64),
        ("ar_span", ctypes.c_int64),
        ("mm_span", ctypes.c_int64),
        ("verify_group", ctypes.c_int64),
        ("hp_dedupe", ctypes.c_int64),
        ("hp_early", ctypes.c_int64),
        ("lane_merge", ctypes.c_int64),
        ("fuse_db_sums", ctypes.c_int64),
        ("sm_segments", ctypes.c_int64),
        ("concurrent_calls", ctypes.c_int64),
        ("scan_skip", ctypes.c_int64),
        ("host_verify", ctypes.c_int64),
        ("interleaved", ctypes.c_int64),
        ("walk_through", ctypes.c_int64),
        ("line_stores", ctypes.c_int64),
    ]


class DetectPlan(ctypes.Structure):
    """ofp_detect_plan: the geometry of a call and the kernel variants it runs (include/onsetfp.h)."""
    _fields_ = ([(n, ctypes.c_int64) for n in ("n_w", "n_wb", "Nm", "U", "V", "Nv", "hp_L", "hp_S", "hp_R", "hp_span",
                                               "ar_L", "ar_S", "mm_L", "mm_S", "tu")] +
                [(n, ctypes.c_int32) for n in ("sm_seg", "merge", "hp_early", "hp_staged", "hp_spread", "hp_lines",
                                               "ar_sym", "ar_through", "ar_lines", "db_sym", "mm_il", "mm_through",
                                               "ar_il", "use_sum")])

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class HopConfig(ctypes.Structure):
    _fields_ = [
        ("n_fft", ctypes.c_int32),
        ("ring_samples", ctypes.c_int64),
        ("n_mels", ctypes.c_int32),
        ("fb_lo", ctypes.c_void_p),
        ("fb_len", ctypes.c_void_p),
        ("fb_off", ctypes.c_void_p),
        ("fb_w", ctypes.c_void_p),
        ("fb_nnz", ctypes.c_int32),
        ("mlp", ctypes.c_void_p),
        ("want_rel", ctypes.c_int32),
        ("strength", ctypes.c_int32),
        ("strength_ring", ctypes.c_int32),
        ("max_length", ctypes.c_int32),
        ("avg_length", ctypes.c_int32),
        ("ls_max0", ctypes.c_float), ("ls_minmax", ctypes.c_float), ("ls_alpha", ctypes.c_float),
        ("oe_min0", ctypes.c_float), ("oe_minmin", ctypes.c_float), ("oe_max0", ctypes.c_float),
        ("oe_alpha", ctypes.c_float),
        ("tg_win_length", ctypes.c_int32),
    ]


LOCS_GROUPS, LOCS_MEMBERS = 64, 8  # OFP_LOCS_GROUPS, OFP_LOCS_MEMBERS
LOCF_GROUPS, LOCF_MEMBERS, LOCF_SECTION, LOCF_BAD_CALL = 1, 2, 4, 8


class LocateState(ctypes.Structure):
    _fields_ = [
        ("n_groups", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("len", ctypes.c_int32 * LOCS_GROUPS),
        ("alias", ctypes.c_int32 * LOCS_GROUPS),
        ("sensors", (ctypes.c_int32 * LOCS_MEMBERS) * LOCS_GROUPS),
        ("onsets", (ctypes.c_int64 * LOCS_MEMBERS) * LOCS_GROUPS),
    ]


class HopLocator(ctypes.Structure):
    _fields_ = [
        ("d_sensors", ctypes.c_void_p),
        ("S", ctypes.c_int32),
        ("d_maps", ctypes.c_void_p),
        ("d_min", ctypes.c_void_p),
        ("d_max", ctypes.c_void_p),
        ("r", ctypes.c_int32),
        ("samples_per_cm", ctypes.c_double), ("sr", ctypes.c_double), ("c", ctypes.c_double),
        ("radius", ctypes.c_double), ("xtol", ctypes.c_double),
        ("maxfev", ctypes.c_int32),
        ("mlp", ctypes.c_void_p),
        ("use_audio", ctypes.c_int32),
        ("max_section", ctypes.c_int32),
    ]


REG_MAX_LAYERS, REG_MAX_SIGNALS, REG_MAX_OUT, REG_MAX_FRAME, REG_QUEUE = 8, 8, 64, 4096, 8  # OFP_REG_*
REGF_QUEUE, REGF_BAD_ONSET = 1, 2
REG_KIND_CNN, REG_KIND_CCCNN, REG_KIND_CCCNN_GROUPED = 0, 1, 2
REG_NORM_NONE, REG_NORM_BATCH, REG_NORM_GROUP = 0, 1, 2


class HopRegressor(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32), ("channels", ctypes.c_int32), ("width", ctypes.c_int32), ("n_out", ctypes.c_int32),
        ("n_conv", ctypes.c_int32),
        ("cout", ctypes.c_int32 * REG_MAX_LAYERS),
        ("kernels", ctypes.c_int32 * REG_MAX_LAYERS),
        ("strides", ctypes.c_int32 * REG_MAX_LAYERS),
        ("padding", ctypes.c_int32), ("dilation", ctypes.c_int32), ("groups", ctypes.c_int32),
        ("act", ctypes.c_int32), ("norm", ctypes.c_int32), ("pool", ctypes.c_int32),
        ("gn_eps", ctypes.c_float),
        ("d_params", ctypes.c_void_p),
        ("n_params", ctypes.c_int64),
        ("frame_length", ctypes.c_int32), ("pre_samples", ctypes.c_int32), ("max_distance", ctypes.c_int32),
        ("min_channels", ctypes.c_int32),
    ]


PAIR_MAX_WINDOW = 1024          # ofppair::MAX_WINDOW: left + right of the voting locator's stage
PAIR_LDS_ENVELOPE = 96 * 1024   # ofpreg::LDS_SWITCH


def paired_lds_bytes(window, side):
    """ofppair::lds_bytes: the reductions' partials, three rows of the window and the vote bitmap."""
    return 32 + 12 * window + 4 * ((side * side + 31) // 32)


class HopPaired(ctypes.Structure):
    _fields_ = [
        ("d_starts", ctypes.c_void_p),
        ("d_sorted", ctypes.c_void_p),
        ("d_vmin", ctypes.c_void_p),
        ("n_buckets", ctypes.c_int32), ("S", ctypes.c_int32), ("side", ctypes.c_int32),
        ("radius", ctypes.c_double), ("tol", ctypes.c_double),
        ("left", ctypes.c_int32), ("right", ctypes.c_int32), ("max_distance", ctypes.c_int32),
        ("min_channels", ctypes.c_int32),
    ]


class CnnConfig(ctypes.Structure):
    _fields_ = [
        ("n_conv", ctypes.c_int32),
        ("channels", ctypes.c_int32 * 4),
        ("kernel", ctypes.c_int32), ("padding", ctypes.c_int32), ("dilation", ctypes.c_int32),
        ("groups", ctypes.c_int32),
        ("act", ctypes.c_int32), ("batch_norm", ctypes.c_int32), ("pool", ctypes.c_int32),
        ("width", ctypes.c_int32), ("n_out", ctypes.c_int32), ("loss", ctypes.c_int32),
        ("bn_momentum", ctypes.c_float),
        ("bn_eps", ctypes.c_double),
    ]


class CnnrnnConfig(ctypes.Structure):
    _fields_ = [("cnn", CnnConfig), ("hidden", ctypes.c_int32), ("heads", ctypes.c_int32)]
    width = property(lambda self: self.cnn.width)  # what model._fit compares between x and x_val


class RnnConfig(ctypes.Structure):
    _fields_ = [
        ("channels", ctypes.c_int32), ("width", ctypes.c_int32), ("hidden", ctypes.c_int32),
        ("layers", ctypes.c_int32), ("heads", ctypes.c_int32), ("n_out", ctypes.c_int32), ("loss", ctypes.c_int32),
        ("permute_input", ctypes.c_int32),
        ("weight_decay", ctypes.c_float),
        ("ln_eps", ctypes.c_double),
    ]


class CccnnConfig(ctypes.Structure):
    _fields_ = [
        ("n_conv", ctypes.c_int32),
        ("sensors", ctypes.c_int32),
        ("layer_sizes", ctypes.c_int32 * 8),
        ("kernels", ctypes.c_int32 * 8),
        ("strides", ctypes.c_int32 * 8),
        ("padding", ctypes.c_int32), ("dilation", ctypes.c_int32), ("group", ctypes.c_int32),
        ("act", ctypes.c_int32), ("norm", ctypes.c_int32), ("pool", ctypes.c_int32),
        ("width", ctypes.c_int32), ("n_out", ctypes.c_int32), ("loss", ctypes.c_int32),
        ("momentum", ctypes.c_float), ("weight_decay", ctypes.c_float),
        ("gn_eps", ctypes.c_double),
    ]


class TrainRandom(ctypes.Structure):
    _fields_ = [
        ("seed", ctypes.c_uint64),
        ("dropout_p", ctypes.c_double),
        ("epoch", ctypes.c_int32), ("max_shift", ctypes.c_int32), ("n_extractions", ctypes.c_int32),
        ("audio_channels", ctypes.c_int32),
        ("d_audio", ctypes.c_void_p),
        ("audio_len", ctypes.c_int64),
        ("d_starts", ctypes.c_void_p),
        ("n_onsets", ctypes.c_int64),
    ]


_vp, _i32, _i64, _f32, _f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
_f32p_h = ctypes.POINTER(ctypes.c_float)
_long_p = ctypes.POINTER(ctypes.c_long)

# name -> (restype, argtypes); every name here must be declared in include/onsetfp.h
SIGNATURES = {
    "ofp_abi_version": (ctypes.c_int, []),
    "ofp_last_error": (ctypes.c_char_p, []),
    "ofp_runtime_prepare": (ctypes.c_int, []),
    "ofp_device_count": (ctypes.c_int, []),
    "ofp_device_check": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "ar_envelope": (None, [_f32p_h, _f32p_h, _f32, _f32, ctypes.c_int, ctypes.c_int]),
    "minmax_envelope": (None, [_f32p_h, _f32p_h, _f32p_h, _f32, _f32, _f32, ctypes.c_int, ctypes.c_int]),
    "backtrack_onsets": (None, [_f32p_h, _long_p, _long_p, _f32, _f32, ctypes.c_long, ctypes.c_long,
                                ctypes.c_long, ctypes.c_long]),
    "ofp_lfilter": (ctypes.c_int, [_f32p_h, _f32p_h, _f32p_h, _f32p_h, ctypes.c_int, _f32p_h, ctypes.c_long,
                                   ctypes.c_int]),
    "ofp_detector_create": (ctypes.c_int, [ctypes.POINTER(DetectorParams), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_vp)]),
    "ofp_detector_destroy": (ctypes.c_int, [_vp]),
    "ofp_detector_set_tuning": (ctypes.c_int, [_vp, ctypes.POINTER(DetectTuning)]),
    "ofp_pack_records": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, ctypes.c_int32, _vp, _vp]),
    "ofp_detect_workspace_bytes": (_i64, [_vp, _i64, _i64, _i64]),
    "ofp_detect_plan_query": (ctypes.c_int, [_vp, _i64, _i64, _i64, ctypes.c_int, _vp, ctypes.POINTER(DetectPlan)]),
    "ofp_detect_plan_for": (ctypes.c_int, [ctypes.POINTER(DetectorParams), ctypes.POINTER(DetectTuning), ctypes.c_int,
                                           _i64, _i64, _i64, ctypes.c_int, _vp, ctypes.POINTER(DetectPlan)]),
    "ofp_canon_eval": (ctypes.c_int, [_i32, _vp, _vp, _i64, _f32, _f32, _f32, _vp, _vp]),
    "ofp_canon_eval_lds": (ctypes.c_int, [_i32, _vp, _i64, _f32, _vp, _vp]),
    "ofp_detect_offline": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64,
                                          ctypes.POINTER(_i64), _vp]),
    "ofp_detect_offline_enqueue": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "ofp_detect_offline_complete": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64,
                                                   ctypes.POINTER(_i64), _vp]),
    "ofp_detect_offline_finish_enqueue": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "ofp_detect_offline_begin": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "ofp_detect_offline_finish": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64,
                                                 ctypes.POINTER(_i64), _vp]),
    "ofp_detect_offline_begin_input": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "ofp_detect_offline_begin_iir": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "ofp_stream_state_bytes": (_i64, [_vp]),
    "ofp_stream_state_init": (ctypes.c_int, [_vp, _vp, _vp]),
    "ofp_stream_process": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _i64, _vp, _vp]),
    "ofp_stream_calibrate": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ofp_detector_set_thresholds": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "ofp_stft_power": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp]),
    "ofp_stft_power_mel": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                          _i64, _vp]),
    "ofp_detect_planar_input": (_vp, [_vp, _i64, _i64, _i64, _vp]),
    "ofp_detect_planar_stride": (_i64, [_vp, _i64, _i64, _i64]),
    "ofp_stft_frames": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32,
                                       _vp, _vp, _vp]),
    "ofp_extract_frames": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp]),
    "ofp_mel": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ofp_mfcc": (ctypes.c_int, [_vp, _i64, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "ofp_dense": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ofp_mlp_create": (ctypes.c_int, [_i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_vp),
                                      ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                      ctypes.POINTER(_vp)]),
    "ofp_mlp_destroy": (ctypes.c_int, [_vp]),
    "ofp_mlp_lds_bytes": (_i64, [_vp]),
    "ofp_mlp_forward": (ctypes.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "ofp_stft_power_mel_mlp": (ctypes.c_int, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32,
                                              _vp, _i64, _vp, _vp, _vp]),
    "ofp_hop_create": (ctypes.c_int, [_vp, ctypes.POINTER(HopConfig), ctypes.POINTER(_vp)]),
    "ofp_hop_destroy": (ctypes.c_int, [_vp]),
    "ofp_hop_reset": (ctypes.c_int, [_vp]),
    "ofp_hop_warmup": (ctypes.c_int, [_vp, _vp, _i64]),
    "ofp_hop_submit": (ctypes.c_int, [_vp, _vp]),
    "ofp_hop_collect": (ctypes.c_int, [_vp, ctypes.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    "ofp_hop_push": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    "ofp_hop_ring_read": (ctypes.c_int, [_vp, _i64, _vp]),
    "ofp_hop_group_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.POINTER(_vp)]),
    "ofp_hop_group_destroy": (ctypes.c_int, [_vp]),
    "ofp_hop_group_submit": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "ofp_hop_group_wait": (ctypes.c_int, [_vp]),
    "ofp_autocorr_softmax": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "ofp_conv1d": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp,
                                  _i32, _vp, _vp]),
    "ofp_groupnorm1": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _f32, _i32, _vp, _vp]),
    "ofp_rnn_layer": (ctypes.c_int, [_i32, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _i64, _vp, _i64, _i64,
                                     _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "ofp_rnn_lds_bytes": (_i64, [_i32, _i32]),
    "ofp_layernorm": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _f32, _vp, _vp]),
    "ofp_attention_mean": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "ofp_group_workspace_bytes": (_i64, [_i64, _i64]),
    "ofp_group_onsets": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i32, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _i64,
                                        _vp]),
    "ofp_group_windows": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _i64, _vp,
                                         _vp]),
    "ofp_xcorr_lag": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "ofp_adjust_onset": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "ofp_filter_direction": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "ofp_onset_region": (ctypes.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _f32, _vp, _vp]),
    "ofp_resample_windows": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "ofp_xcorr_full": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i64, _i64, _i32, _vp, _vp]),
    "ofp_spectral_flux": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "ofp_select_rank": (ctypes.c_int, [_vp, _i64, _i64, _vp, _vp]),
    "ofp_scale_inverse": (ctypes.c_int, [_vp, _i64, _vp, _vp]),
    "ofp_peak_pick": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _f32, _i64, _vp, _i64, _vp, _vp, _vp]),
    "ofp_fix_onsets_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ofp_fix_onsets": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                      _i32, _i32, _vp, _vp, _i64, _vp]),
    "ofp_lag_maps": (ctypes.c_int, [_vp, _i32, _i32, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp]),
    "ofp_locate_legal": (ctypes.c_int, [_vp, _i32, _i32, _vp, _vp, _i64, _f64, _vp, _vp]),
    "ofp_trilaterate": (ctypes.c_int, [_vp, _vp, _vp, _i64, _f64, _i32, _vp, _vp, _vp, _vp]),
    "ofp_locate_workspace_bytes": (_i64, [_i64]),
    "ofp_locate_groups": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _f64, _f64, _f64,
                                         _f64, _f64, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_locate_section": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "ofp_locate_groups_2d": (ctypes.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _f64, _f64, _f64,
                                            _f64, _f64, _i32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_locate_stream": (ctypes.c_int, [ctypes.POINTER(HopLocator), _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp,
                                         _vp]),
    "ofp_locate_stream_2d": (ctypes.c_int, [ctypes.POINTER(HopLocator), _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "ofp_hop_set_locator": (ctypes.c_int, [_vp, ctypes.POINTER(HopLocator)]),
    "ofp_hop_set_locator_2d": (ctypes.c_int, [_vp, ctypes.POINTER(HopLocator)]),
    "ofp_hop_collect_location": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_f64), ctypes.POINTER(_i32),
                                                ctypes.POINTER(_i32), ctypes.POINTER(_i64), ctypes.POINTER(_i32),
                                                ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "ofp_hop_locator_state": (ctypes.c_int, [_vp, ctypes.POINTER(LocateState)]),
    "ofp_regress_workspace_floats": (_i64, [ctypes.POINTER(HopRegressor)]),
    "ofp_regress_stream": (ctypes.c_int, [ctypes.POINTER(HopRegressor), _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _vp]),
    "ofp_hop_set_regressor": (ctypes.c_int, [_vp, ctypes.POINTER(HopRegressor)]),
    "ofp_hop_collect_hit": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i64), _vp, _vp,
                                           ctypes.POINTER(_i32)]),
    "ofp_locate_cc_stream": (ctypes.c_int, [ctypes.POINTER(HopPaired), _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ofp_hop_set_locator_paired": (ctypes.c_int, [_vp, ctypes.POINTER(HopPaired)]),
    "ofp_hop_collect_cc_hit": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i64),
                                              ctypes.POINTER(_i32), _vp, _vp, ctypes.POINTER(_i32), _vp, _vp,
                                              ctypes.POINTER(_i32)]),
    "ofp_find_lags": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp,
                                     _vp, _vp, _vp, _vp]),
    "ofp_vote_index": (ctypes.c_int, [_vp, _i64, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "ofp_paired_windows": (ctypes.c_int, [_i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32,
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    "ofp_paired_vote": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _f64, _f64,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "ofp_paired_solve": (ctypes.c_int, [_vp, _i32, _vp, _vp, _i64, _f64, _f64, _f64, _f64, _i32, _vp, _vp, _vp,
                                        _vp]),
    "ofp_intensity_maps": (ctypes.c_int, [_vp, _i32, _f64, _vp, _vp]),
    "ofp_fcnn_train_lds_bytes": (_i64, [_i32, ctypes.POINTER(_i32), _i32, _i32, _i64]),
    "ofp_fcnn_train_workspace_bytes": (_i64, [_i32, ctypes.POINTER(_i32), _i32, _i32, _i64, _i64]),
    "ofp_fcnn_train": (ctypes.c_int, [_i32, ctypes.POINTER(_i32), _i32, _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp,
                                      _i64, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_fcnn_loss_grads": (ctypes.c_int, [_i32, ctypes.POINTER(_i32), _i32, _i32, _i32, _i32, _i64, _i64, _vp, _i64,
                                           _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_tdoa_fit": (ctypes.c_int, [_i64, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _f32, _i32, _vp, _vp,
                                    _vp, _vp, _vp, _vp]),
    "ofp_tdoa_loss_grads": (ctypes.c_int, [_i64, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ofp_cnn_train_slab": (_i32, []),
    "ofp_cnn_train_workspace_bytes": (_i64, [ctypes.POINTER(CnnConfig), _i64, _i64]),
    "ofp_cnn_train": (ctypes.c_int, [ctypes.POINTER(CnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32,
                                     _vp, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp]),
    "ofp_cnn_loss_grads": (ctypes.c_int, [ctypes.POINTER(CnnConfig), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_conv1d_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "ofp_conv1d_backward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                           _vp, _vp, _i64, _vp]),
    "ofp_linear_head_train_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ofp_linear_head_train": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _vp, _i64, _vp]),
    "ofp_batchnorm_train_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ofp_batchnorm_train_forward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _f64, _f32, _vp, _vp, _vp, _vp,
                                                   _vp, _vp, _i64, _vp]),
    "ofp_batchnorm_train_backward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                    _i64, _vp]),
    "ofp_nadam_step": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "ofp_cccnn_train_workspace_bytes": (_i64, [ctypes.POINTER(CccnnConfig), _i64, _i64]),
    "ofp_cccnn_train": (ctypes.c_int, [ctypes.POINTER(CccnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32,
                                       _i32, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp]),
    "ofp_cccnn_loss_grads": (ctypes.c_int, [ctypes.POINTER(CccnnConfig), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                            _vp]),
    "ofp_conv1d_backward_strided_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "ofp_conv1d_backward_strided": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32,
                                                   _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_groupnorm1_train_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ofp_groupnorm1_train_forward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _f64, _i32, _vp, _vp, _vp, _vp]),
    "ofp_groupnorm1_train_backward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                                     _vp, _vp, _i64, _vp]),
    "ofp_autocorr_softmax_lds_bytes": (_i64, [_i32, _i32]),
    "ofp_autocorr_softmax_backward": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "ofp_sgd_step": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, _i32, _f32, _f32, _vp]),
    "ofp_cnn_train_random_workspace_bytes": (_i64, [ctypes.POINTER(CnnConfig), _i64, _i64,
                                                    ctypes.POINTER(TrainRandom)]),
    "ofp_cnn_train_random": (ctypes.c_int, [ctypes.POINTER(CnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32,
                                            _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp,
                                            ctypes.POINTER(TrainRandom)]),
    "ofp_cnn_loss_grads_random": (ctypes.c_int, [ctypes.POINTER(CnnConfig), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                                 _vp, ctypes.POINTER(TrainRandom)]),
    "ofp_cccnn_train_random_workspace_bytes": (_i64, [ctypes.POINTER(CccnnConfig), _i64, _i64,
                                                      ctypes.POINTER(TrainRandom)]),
    "ofp_cccnn_train_random": (ctypes.c_int, [ctypes.POINTER(CccnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                              _i32, _i32, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp,
                                              ctypes.POINTER(TrainRandom)]),
    "ofp_cccnn_loss_grads_random": (ctypes.c_int, [ctypes.POINTER(CccnnConfig), _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                   _i64, _vp, ctypes.POINTER(TrainRandom)]),
    "ofp_philox4x32": (ctypes.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "ofp_dropout_mask": (ctypes.c_int, [ctypes.c_uint64, _i32, _i64, _i32, _f64, _vp, _vp]),
    "ofp_shift_windows": (ctypes.c_int, [ctypes.c_uint64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _i32, _vp,
                                         _vp, _vp]),
    "ofp_stretch_windows": (ctypes.c_int, [ctypes.c_uint64, _i32, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _i32, _i32,
                                           _vp, _vp, _vp, _vp]),
    "ofp_cnn_train_stretch_workspace_bytes": (_i64, [ctypes.POINTER(CnnConfig), _i64, _i64,
                                                     ctypes.POINTER(TrainRandom), _i32]),
    "ofp_cnn_train_stretch": (ctypes.c_int, [ctypes.POINTER(CnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                             _i32, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp,
                                             ctypes.POINTER(TrainRandom), _i32]),
    "ofp_cccnn_train_stretch_workspace_bytes": (_i64, [ctypes.POINTER(CccnnConfig), _i64, _i64,
                                                       ctypes.POINTER(TrainRandom), _i32]),
    "ofp_cccnn_train_stretch": (ctypes.c_int, [ctypes.POINTER(CccnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                               _i32, _i32, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp,
                                               ctypes.POINTER(TrainRandom), _i32]),
    "ofp_linear_backward_slab": (_i32, []),
    "ofp_cnnrnn_train_stretch_workspace_bytes": (_i64, [ctypes.POINTER(CnnrnnConfig), _i64, _i64,
                                                        ctypes.POINTER(TrainRandom), _i32]),
    "ofp_cnnrnn_train_stretch": (ctypes.c_int, [ctypes.POINTER(CnnrnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                                _i32, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp,
                                                ctypes.POINTER(TrainRandom), _i32]),
    "ofp_cnnrnn_loss_grads_random_workspace_bytes": (_i64, [ctypes.POINTER(CnnrnnConfig), _i64, _i64,
                                                            ctypes.POINTER(TrainRandom)]),
    "ofp_cnnrnn_loss_grads_random": (ctypes.c_int, [ctypes.POINTER(CnnrnnConfig), _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                    _i64, _vp, ctypes.POINTER(TrainRandom)]),
    "ofp_linear_backward_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ofp_linear_backward": (ctypes.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_gru_train_forward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ofp_gru_train_forward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                             _vp]),
    "ofp_gru_train_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ofp_gru_train_backward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _i64, _vp]),
    "ofp_attention_mean_train_forward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ofp_attention_mean_train_forward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp,
                                                        ctypes.POINTER(TrainRandom), _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_attention_mean_train_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ofp_attention_mean_train_backward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                                         ctypes.POINTER(TrainRandom), _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_attention_dropout_mask": (ctypes.c_int, [ctypes.c_uint64, _i32, _i64, _i32, _i32, _f64, _vp, _vp]),
    "ofp_rnn_train_stretch_workspace_bytes": (_i64, [ctypes.POINTER(RnnConfig), _i64, _i64,
                                                     ctypes.POINTER(TrainRandom), _i32]),
    "ofp_rnn_train_stretch": (ctypes.c_int, [ctypes.POINTER(RnnConfig), _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                             _i32, _i32, _vp, _vp, _vp, ctypes.POINTER(_i32), _vp, _i64, _vp,
                                             ctypes.POINTER(TrainRandom), _i32]),
    "ofp_rnn_loss_grads_random_workspace_bytes": (_i64, [ctypes.POINTER(RnnConfig), _i64, _i64,
                                                         ctypes.POINTER(TrainRandom)]),
    "ofp_rnn_loss_grads_random": (ctypes.c_int, [ctypes.POINTER(RnnConfig), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                                 _vp, ctypes.POINTER(TrainRandom)]),
    "ofp_layernorm_train_forward": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _f64, _vp, _vp, _vp, _vp]),
    "ofp_layernorm_train_backward_workspace_bytes": (_i64, [_i64, _i32]),
    "ofp_layernorm_train_backward": (ctypes.c_int, [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                                    _vp]),
    "ofp_rnn_gru_train_forward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "ofp_rnn_gru_train_forward": (ctypes.c_int, [_vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp,
                                                 ctypes.POINTER(TrainRandom), _vp, _vp, _vp, _i64, _vp]),
    "ofp_rnn_gru_train_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "ofp_rnn_gru_train_backward": (ctypes.c_int, [_vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp,
                                                  ctypes.POINTER(TrainRandom), _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_rnn_attention_train_forward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ofp_rnn_attention_train_forward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp,
                                                       ctypes.POINTER(TrainRandom), _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_rnn_attention_train_backward_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ofp_rnn_attention_train_backward": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                                        ctypes.POINTER(TrainRandom), _vp, _vp, _vp, _vp, _i64, _vp]),
    "ofp_rnn_layer_dropout_mask": (ctypes.c_int, [ctypes.c_uint64, _i32, _i32, _i64, _i32, _i32, _f64, _vp, _vp]),
    "ofp_nadam_decay_step": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _f32, _vp]),
}

_lib = None


def build(force=False):
    """Compile csrc/*.hip into libonsetfp.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", str(_HERE / "csrc"), "-j4"]
    if force:
        subprocess.check_call(cmd + ["clean"])
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    """The loaded library with argtypes set; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OnsetFPError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        L = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here means header and library disagree
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def runtime_prepare():
    """ofp_runtime_prepare() (include/onsetfp.h): ask the HIP runtime for the hardware queues that steps in flight need,
    while it can still be asked -- before the first HIP call of the process.  -> 1 if the variable was set, 0 if the
    runtime was already up (nothing changed).  os.environ is brought in line with what the C call did, so that Python
    code and child processes started with a copy of it see the same value.  A tree that has not been built yet has
    nothing to prepare (lib() raises at the first use)."""
    if not LIB_PATH.exists():
        return 0
    done = lib().ofp_runtime_prepare()
    if done:
        libc_getenv = ctypes.CDLL(None).getenv
        libc_getenv.restype, libc_getenv.argtypes = ctypes.c_char_p, [ctypes.c_char_p]
        os.environ["GPU_MAX_HW_QUEUES"] = libc_getenv(b"GPU_MAX_HW_QUEUES").decode()
    return done


def check(status, what=""):
    if status != 0:
        msg = lib().ofp_last_error().decode(errors="replace")
        raise OnsetFPError(f"{what or 'libonsetfp'} failed with status {status}: {msg}")


def last_error():
    return lib().ofp_last_error().decode(errors="replace")


_checked = {}


def require_gpu(device=0):
    """Fail loudly unless `device` is a gfx950 GPU (checked once per device and process)."""
    if device in _checked:
        return _checked[device]
    L = lib()
    n = L.ofp_device_count()
    if n <= 0:
        raise OnsetFPError(f"no GPU visible to HIP ({last_error()}); onset_fingerprinting_amd has no CPU path")
    buf = ctypes.create_string_buffer(64)
    check(L.ofp_device_check(device, buf, 64), "ofp_device_check")
    _checked[device] = buf.value.decode()
    return _checked[device]

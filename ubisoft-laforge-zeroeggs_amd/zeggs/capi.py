"""The one ctypes binding of libzeggs_hip.so (C ABI: include/zeggs_hip.h): the mirrors of the header's structs, one prototype row
per function, and the two handles of the library.

  api()   the TYPED handle the package calls: `argtypes` and `restype` of every row are set when the library is loaded, a status
          return other than 0 raises RuntimeError("<function>: <zeggs_last_error()>"), and a device-pointer parameter takes a
          tensor (checked: on a GPU, contiguous, the element type of the header) or None -- call sites pass tensors and plain
          Python numbers.
  raw()   a second CDLL of the same file with the rows' `restype` only: no `argtypes`, no error check.  What ops.lib() returns;
          tests, tools and the benchmark call it with hand-wrapped arguments and look at the return codes themselves.  Both
          handles share the dlopen handle, and so every global of the library.

A new entry point is a declaration in the header plus one row in PROTOTYPES (tests/test_abi.py compares the two); the second
header include/zeggs_hip_live.h has its own tables, EXT_STRUCTS / EXT_PROTOTYPES (tests/test_live_push_cpu.py), the third,
include/zeggs_hip_loudness.h, LOUD_STRUCTS / LOUD_PROTOTYPES (tests/test_live_loudness_cpu.py), the fourth,
include/zeggs_hip_resample.h, RS_STRUCTS / RS_PROTOTYPES (tests/test_live_resample_cpu.py), the fifth,
include/zeggs_hip_frames.h, FR_STRUCTS / FR_PROTOTYPES (tests/test_live_frames_cpu.py), the sixth, include/zeggs_hip_retime.h,
RT_STRUCTS / RT_PROTOTYPES (tests/test_live_retime_cpu.py), the seventh, include/zeggs_hip_refilter.h, RF_STRUCTS / RF_PROTOTYPES
(tests/test_live_refilter_cpu.py), the eighth, include/zeggs_hip_snapshot.h, SNAP_STRUCTS / SNAP_PROTOTYPES
(tests/test_live_snapshot_cpu.py), the ninth, include/zeggs_hip_gaze.h, GZ_STRUCTS / GZ_PROTOTYPES (tests/test_live_gaze_cpu.py),
the tenth, include/zeggs_hip_styles.h, SB_STRUCTS / SB_PROTOTYPES (tests/test_live_styles_cpu.py), the eleventh,
include/zeggs_hip_plant.h, PL_STRUCTS / PL_PROTOTYPES (tests/test_live_plant_cpu.py), the twelfth, include/zeggs_hip_mirror.h,
MR_PROTOTYPES (tests/test_mirror_cpu.py; it has no structs): same loader.  torch is imported when a tensor is first converted, not
when this module is.
"""
import ctypes as C
import os
import threading
from pathlib import Path

LIB_PATH = Path(os.environ.get("ZEGGS_LIB") or Path(__file__).resolve().parent / "libzeggs_hip.so")   # ZEGGS_LIB: A/B builds
OPTIONS = {}             # switches set through ops.set_option / ZEGGS_OPTIONS (the library's defaults otherwise)


class HipLibraryMissing(RuntimeError):
    pass


# ----------------------------------------------------------------------------- structs (mirror zeggs_hip.h)
def _struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": [(f, t) for t, names in fields for f in names.split()]})


def _ptr_struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": [(f, C.c_void_p) for f in fields]})


SpeechDims = _struct("SpeechDims", [(C.c_int, "B T F H O KW"), (C.c_float, "dropout_p"), (C.c_uint64, "seed")])
LiveDims = _struct("LiveDims", [(C.c_int, "R F H O KW D feat_ld out_ld")])
LiveRow = _struct("LiveRow", [(C.c_long, "n_ring k0 last"), (C.c_int, "n_new n_out feat_off reserved")])
StyleDims = _struct("StyleDims", [(C.c_int, "B L C H E NH dropout"), (C.c_uint64, "seed")])
StyleGruDims = _struct("StyleGruDims", [(C.c_int, "B L C H O")])
DecDims = _struct("DecDims", [(C.c_int, "B T PI PO SP ST H"), (C.c_float, "dt"), (C.c_int, "film")])
# the per-call controls of zeggs_decoder_fwd_ex / _bwd_ex
DecCall = _struct("DecCall", [(C.c_int, "prepared defer_wgrads"), (C.c_void_p, "wgrad_stream status"), (C.c_int, "grads_zeroed")])
LossDims = _struct("LossDims", [(C.c_int, "B T J S"), (C.c_float, "dt")])
MelDims = _struct("MelDims", [(C.c_int, "n_fft hop n_mels fs"), (C.c_float, "fps min_clip"), (C.c_double, "pre_emph"), (C.c_int, "flags")])
AnimDims = _struct("AnimDims", [(C.c_int, "N J hips spine2 head"), (C.c_double, "dt"), (C.c_int, "order")])
BvhDims = _struct("BvhDims", [(C.c_int, "T J rebase"), (C.c_double * 3, "start_pos"), (C.c_double * 4, "start_rot"), (C.c_int, "order")])

SPEECH_FIELDS = ("w0", "b0", "w1", "b1", "w2", "b2")
STYLE_FIELDS = ("c0_w", "c0_b", "ln0_g", "ln0_b", "c4_w", "c4_b", "ln1_g", "ln1_b", "in_w", "in_b", "out_w", "out_b",
                "lna_g", "lna_b", "ff0_w", "ff0_b", "ff2_w", "ff2_b", "lnf_g", "lnf_b")
STYLE_GRU_FIELDS = ("c0_w", "c0_b", "c2_w", "c2_b", "w_ih", "w_hh", "b_ih", "b_hh", "w_ih_r", "w_hh_r", "b_ih_r",
                    "b_hh_r", "p_w", "p_b")
DEC_FIELDS = ("l0_w", "l0_b", "w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "l2_w", "l2_b",
              "c0_w", "c0_b", "c1_w", "c1_b", "c2_w", "c2_b",
              "l3_w", "l3_b", "g_w", "g_b", "be_w", "be_b")          # last six: rnn_cond "film" only (else NULL)
STATS_FIELDS = ("in_mean", "in_std", "out_mean", "out_std")
ANIM_OUT_FIELDS = ("root_pos", "root_rot", "root_vel", "root_vrt", "lpos", "lrot", "lvel", "lvrt", "ltxy", "cpos", "crot", "cvel",
                   "cvrt", "ctxy", "gaze_pos", "gaze_dir")
SpeechPtrs = _ptr_struct("SpeechPtrs", SPEECH_FIELDS)
StylePtrs = _ptr_struct("StylePtrs", STYLE_FIELDS)
StyleGruPtrs = _ptr_struct("StyleGruPtrs", STYLE_GRU_FIELDS)
DecPtrs = _ptr_struct("DecPtrs", DEC_FIELDS)
DecStats = _ptr_struct("DecStats", STATS_FIELDS)
AnimOut = _ptr_struct("AnimOut", ANIM_OUT_FIELDS)

# header struct -> its mirror (a parameter record and its gradient record share one)
STRUCTS = {
    "ZeggsSpeechDims": SpeechDims, "ZeggsSpeechParams": SpeechPtrs, "ZeggsSpeechGrads": SpeechPtrs, "ZeggsLiveDims": LiveDims,
    "ZeggsLiveRow": LiveRow, "ZeggsStyleDims": StyleDims, "ZeggsStyleParams": StylePtrs, "ZeggsStyleGrads": StylePtrs,
    "ZeggsStyleGruDims": StyleGruDims, "ZeggsStyleGruParams": StyleGruPtrs, "ZeggsStyleGruGrads": StyleGruPtrs,
    "ZeggsDecDims": DecDims, "ZeggsDecParams": DecPtrs, "ZeggsDecGrads": DecPtrs, "ZeggsDecStats": DecStats, "ZeggsDecCall": DecCall,
    "ZeggsLossDims": LossDims, "ZeggsMelDims": MelDims, "ZeggsAnimDims": AnimDims, "ZeggsAnimOut": AnimOut, "ZeggsBvhDims": BvhDims,
}

# ----------------------------------------------------------------------------- prototypes
# One row per function of the header: "<return>: <parameter> <parameter> ...".
#   return     status (an int, 0 = success: anything else raises with zeggs_last_error) | mask (an int >= 0, a negative one raises
#              alike) | int | long | size_t | str (as they are)
#   parameter  int long size_t uint64 float double | str (C string) | ZeggsX* (pointer to that struct; an instance is passed by
#              reference, an array as it is) | f32* f64* i32* i64* u8* any* (DEVICE pointer with the header's element type: float,
#              double, int / unsigned, int64_t / long / long long, uint8_t / unsigned char / char (uint8 or bool tensors), void) |
#              host* (a pointer the library reads or writes on the HOST: ctypes arrays, byref() of an out-parameter, an address) |
#              stream (a hipStream_t as void*)
PROTOTYPES = {
    "zeggs_version": "int:",
    "zeggs_last_error": "str:",
    "zeggs_set_option": "status: str int",
    "zeggs_timing_ms": "status: int host*",
    "zeggs_gemm": "status: f32* f32* f32* f32* int int int long long long long long long int long long long float float int stream",
    "zeggs_gemm_tn_bias": "status: f32* long f32* long f32* long int int int float f32* stream",
    "zeggs_gemm_direct_selftest": "int: int int int",
    "zeggs_gemm_direct_state": "int: int int int",
    "zeggs_gemm_direct_warm": "status:",
    "zeggs_gemm_route": "status: int int int int",
    "zeggs_gemm_route_get": "status: host*",
    "zeggs_gemm_kbatch": "status: f32* f32* f32* int int int long long long long long long int long long float stream",
    "zeggs_speech_encoder_workspace_bytes": "size_t: ZeggsSpeechDims*",
    "zeggs_speech_encoder_fwd": "status: ZeggsSpeechDims* ZeggsSpeechParams* f32* f32* any* size_t stream",
    "zeggs_speech_encoder_bwd": "status: ZeggsSpeechDims* ZeggsSpeechParams* f32* f32* f32* ZeggsSpeechGrads* any* size_t stream",
    "zeggs_speech_encoder_bwd_ex": "status: ZeggsSpeechDims* ZeggsSpeechParams* f32* f32* f32* ZeggsSpeechGrads* any* size_t stream int",
    "zeggs_speech_encoder_live_workspace_bytes": "size_t: ZeggsLiveDims*",
    "zeggs_speech_encoder_live_prepare": "status: ZeggsLiveDims* ZeggsSpeechParams* any* size_t stream",
    # rows: a HOST array of ZeggsLiveRow
    "zeggs_speech_encoder_live": "status: ZeggsLiveDims* ZeggsSpeechParams* f32* f32* ZeggsLiveRow* f32* f32* f32* any* size_t stream",
    "zeggs_style_encoder_workspace_bytes": "size_t: ZeggsStyleDims*",
    "zeggs_style_encoder_fwd": "status: ZeggsStyleDims* ZeggsStyleParams* f32* f32* f32* any* size_t stream",
    "zeggs_style_encoder_fwd_part": "status: ZeggsStyleDims* ZeggsStyleParams* f32* f32* f32* any* size_t stream int",
    "zeggs_style_encoder_input_offset": "size_t: ZeggsStyleDims*",
    "zeggs_style_encoder_bwd": "status: ZeggsStyleDims* ZeggsStyleParams* f32* ZeggsStyleGrads* any* size_t stream",
    "zeggs_style_encoder_bwd_ex": "status: ZeggsStyleDims* ZeggsStyleParams* f32* ZeggsStyleGrads* any* size_t stream int",
    "zeggs_style_encoder_bwd_part": "status: ZeggsStyleDims* ZeggsStyleParams* f32* ZeggsStyleGrads* any* size_t stream int int",
    "zeggs_style_encoder_gru_workspace_bytes": "size_t: ZeggsStyleGruDims*",
    "zeggs_style_encoder_gru_fwd": "status: ZeggsStyleGruDims* ZeggsStyleGruParams* f32* f32* any* size_t stream",
    "zeggs_style_encoder_gru_bwd": "status: ZeggsStyleGruDims* ZeggsStyleGruParams* f32* ZeggsStyleGruGrads* any* size_t stream",
    "zeggs_vae_reparam_fwd": "status: f32* f32* f32* f32* f32* int int float stream",
    "zeggs_vae_reparam_bwd": "status: f32* f32* f32* f32* f32* f32* int int float stream",
    "zeggs_decoder_workspace_bytes": "size_t: ZeggsDecDims* int",
    "zeggs_decoder_fwd": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* f32* f32* int any* "
                         "size_t stream",
    "zeggs_decoder_fwd_state": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* "
                               "f32* any* size_t stream",
    "zeggs_persistent_state": "int: int",
    "zeggs_tp_stamps": "status: ZeggsDecDims* any* size_t host*",
    "zeggs_tp_waits": "status: ZeggsDecDims* any* size_t host*",
    "zeggs_tp_dual_stamps": "status: ZeggsDecDims* any* size_t host*",
    "zeggs_bp_stamps": "status: ZeggsDecDims* any* size_t host*",
    "zeggs_bp_waits": "status: ZeggsDecDims* any* size_t host*",
    "zeggs_decoder_chain_errors": "status: ZeggsDecDims* int any* size_t host*",
    "zeggs_decoder_chain_stamps": "status: ZeggsDecDims* int any* size_t host*",
    "zeggs_decoder_bwd": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* ZeggsDecGrads* f32* "
                         "f32* any* size_t stream",
    "zeggs_decoder_fwd_ex": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* f32* f32* int any* "
                            "size_t stream ZeggsDecCall*",
    "zeggs_decoder_bwd_ex": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* ZeggsDecGrads* f32* "
                            "f32* any* size_t stream ZeggsDecCall*",
    "zeggs_decoder_fwd_state_ex": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* f32* f32* "
                                  "f32* f32* any* size_t stream ZeggsDecCall*",
    "zeggs_decoder_batch_workspace_bytes": "size_t: ZeggsDecDims*",
    "zeggs_decoder_batch_prepare": "mask: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* any* size_t stream",
    "zeggs_decoder_state_init": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* any* size_t stream",
    "zeggs_decoder_fwd_batch": "status: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* "
                               "f32* any* size_t stream ZeggsDecCall* int",
    "zeggs_decoder_batch_last_path": "int:",
    "zeggs_decoder_wgrads": "status: ZeggsDecDims* ZeggsDecGrads* any* size_t int stream",
    "zeggs_decoder_prepare": "mask: ZeggsDecDims* ZeggsDecParams* ZeggsDecStats* any* size_t stream",
    "zeggs_side_stream": "status: host*",
    "zeggs_loss_workspace_bytes": "size_t: ZeggsLossDims*",
    "zeggs_loss_fwd_bwd": "status: ZeggsLossDims* i32* f32* f32* f32* f32* f32* f32* f32* f32* f32* float f32* f32* f32* f32* f32* f32* "
                          "float any* size_t stream",
    "zeggs_loss_prepare_truth": "status: ZeggsLossDims* i32* f32* f32* f32* f32* any* size_t stream",
    "zeggs_loss_fwd_bwd_ex": "status: ZeggsLossDims* i32* f32* f32* f32* f32* f32* f32* f32* f32* f32* float f32* f32* f32* f32* f32* "
                             "f32* float any* size_t stream int",
    "zeggs_loss_eval_workspace_bytes": "size_t: ZeggsLossDims*",
    "zeggs_loss_eval": "status: ZeggsLossDims* i32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f64* any* size_t stream",
    "zeggs_eval_accumulate": "status: f64* i32* int int f64* stream",
    "zeggs_gemm_fixed_order": "int: int",                                                                       # the previous setting
    "zeggs_test_gemm_route_log": "int: int host* host* int",                                                    # the number of route ids
    "zeggs_radam_step": "status: f32* f32* f32* f32* long float float float float int stream",
    "zeggs_radam_step_guarded": "status: f32* f32* f32* f32* long float float float float int i32* f32* stream",
    "zeggs_radam_step_guarded_part": "status: f32* f32* f32* f32* long float float float float int i32* f32* int stream",
    "zeggs_radam_step_wd": "status: f32* f32* f32* f32* long float float float float int float i32* f32* int stream",
    "zeggs_radam_step_c": "status: f32* f32* f32* f32* long float float float float float float int float i32* f32* int stream",
    "zeggs_radam_step_d": "status: f32* f32* f32* f32* long double double double double float float int float i32* f32* int stream",
    "zeggs_status_flag": "status: i32* f32* stream",
    "zeggs_test_cotenant": "status: int int float f32* long stream",
    "zeggs_test_attention_fwd": "status: f32* f32* f32* int int int int float uint64 stream",
    "zeggs_test_attention_bwd": "status: f32* f32* f32* f32* f32* f32* f32* int int int int float uint64 stream",
    "zeggs_gather_windows": "status: f32* int i64* int int f32* stream",
    "zeggs_gather_rows": "status: f32* int i64* long f32* int stream",
    "zeggs_mel_stft_frames": "long: ZeggsMelDims* long",
    "zeggs_mel_workspace_bytes": "size_t: ZeggsMelDims* long",
    "zeggs_mel_features": "status: ZeggsMelDims* f32* long f64* int f32* any* size_t stream",
    "zeggs_mel_frames_ready": "long: ZeggsMelDims* long",
    "zeggs_mel_range_workspace_bytes": "size_t: ZeggsMelDims* long long",
    "zeggs_mel_features_range": "status: ZeggsMelDims* f32* long int f64* long long f32* any* size_t stream",
    "zeggs_mel_window_first_sample": "long: ZeggsMelDims* long",
    "zeggs_mel_features_window": "status: ZeggsMelDims* f32* long long int f64* long long f32* any* size_t stream",
    "zeggs_mel_last_form": "int:",
    "zeggs_loudness_workspace_bytes": "size_t: long int long",
    # coef[10] / trans[8]: prepared and read on the host
    "zeggs_loudness_gain": "status: f32* long int double host* host* long i64* i64* int int f64* f32* any* size_t stream",
    "zeggs_gather_example": "status: f32* int i64* int int f32* f32* f32* int int stream",
    "zeggs_normalize_rows": "status: f32* long int long f32* f32* float stream",
    "zeggs_fill": "status: f32* long float stream",
    "zeggs_scale_copy": "status: f32* f32* long f32* float stream",
    "zeggs_randn": "status: f32* long uint64 stream",
    "zeggs_dropout": "status: f32* long float uint64 stream",
    "zeggs_broadcast_time": "status: f32* f32* int int int stream",
    "zeggs_sum_time": "status: f32* f32* int int int stream",
    "zeggs_normalize_vec_fwd": "status: f32* f32* long int float stream",
    "zeggs_normalize_vec_bwd": "status: f32* f32* f32* long int float stream",
    "zeggs_vectorize_input_fwd": "status: int int f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* stream",
    "zeggs_vectorize_input_bwd": "status: int int f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* stream",
    "zeggs_devectorize_output_fwd": "status: int int float f32* f32* f32* f32* f32* f32* f32* f32* stream",
    "zeggs_devectorize_output_bwd": "status: int int float f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* f32* stream",
    "zeggs_kl_div_fwd": "status: f32* f32* int int f32* stream",
    "zeggs_kl_div_bwd": "status: f32* f32* int int f32* f32* f32* stream",
    "zeggs_mask_from_lengths": "status: i64* int int u8* stream",
    "zeggs_anim_features_workspace_bytes": "size_t: ZeggsAnimDims*",
    "zeggs_anim_features": "status: ZeggsAnimDims* i32* f64* f64* ZeggsAnimOut* any* size_t stream",
    "zeggs_pose_to_bvh": "status: ZeggsBvhDims* f32* f32* f32* f32* f64* f64* stream",
    "zeggs_pose_to_bvh_table": "status: ZeggsBvhDims* f32* f32* f32* f32* f32* f32* i32* f64* stream",
    "zeggs_write_table_text": "status: str int host* long int",
    "zeggs_parse_table_text": "status: host* size_t host* long int",        # text: an address inside a larger host buffer, not a whole C string
    "zeggs_format_table_text": "status: host* long int host* size_t host*",
    "zeggs_table_text_workspace_bytes": "size_t: long int",
    "zeggs_table_text_device": "status: f64* long int u8* size_t i64* i32* any* size_t stream",
    "zeggs_spline_chunk": "status: host* host* host*",
    "zeggs_spline_resample_workspace_bytes": "size_t: long int",
    "zeggs_spline_resample": "status: f64* long int long f64* any* size_t stream",
    "zeggs_rot_stretch_workspace_bytes": "size_t: long int long",
    "zeggs_rot_stretch": "status: f64* long int long int f64* any* size_t stream",
    "zeggs_audio_prepare": "status: f32* long i64* int long long f32* f64* stream",
    "zeggs_center_take": "status: f64* f64* long int int int any* size_t stream",
    "zeggs_masked_stats_workspace_bytes": "size_t: long int",
    "zeggs_masked_stats": "status: f32* u8* long int f64* f64* f64* any* size_t stream",
    "zeggs_sweep_graph_stats": "status: host* host*",
}

# ----------------------------------------------------------------------------- the second header (include/zeggs_hip_live.h)
# Per-row records with device pointers inside (the main header's set is closed: tests/test_abi.py); bound by the same loader.
MelRow = _struct("MelRow", [(C.c_void_p, "wav out"), (C.c_long, "base n_samples k0 k1"), (C.c_int, "final")])
Seg = _struct("Seg", [(C.c_void_p, "src dst"), (C.c_long, "count")])
EXT_STRUCTS = {"ZeggsMelRow": MelRow, "ZeggsSeg": Seg}
EXT_PROTOTYPES = {
    "zeggs_mel_batch_tables_bytes": "size_t: ZeggsMelDims*",
    "zeggs_mel_batch_prepare": "status: ZeggsMelDims* f64* any* size_t stream",
    "zeggs_mel_batch_workspace_bytes": "size_t: ZeggsMelDims* int long",
    # rows_host: a HOST array of ZeggsMelRow; rows_dev: the same records on the device (an address cast to the pointer type) or None
    "zeggs_mel_features_batch": "status: ZeggsMelDims* ZeggsMelRow* ZeggsMelRow* int f64* any* any* size_t stream",
    "zeggs_mel_batch_last_ops": "int:",
    "zeggs_copy_segments": "status: ZeggsSeg* ZeggsSeg* int stream",
}

# ----------------------------------------------------------------------------- the third header (include/zeggs_hip_loudness.h)
# Running loudness normalisation of live serving (tests/test_live_loudness_cpu.py compares these tables with the header).
LoudDims = _struct("LoudDims", [(C.c_int, "fs rows ring_blocks warmup"), (C.c_double, "target gain_lo gain_hi"), (C.c_double * 10, "coef")])
LoudRow = _struct("LoudRow", [(C.c_void_p, "src dst"), (C.c_long, "count"), (C.c_int, "row")])
LOUD_STRUCTS = {"ZeggsLoudDims": LoudDims, "ZeggsLoudRow": LoudRow}
LOUD_PROTOTYPES = {
    "zeggs_live_loudness_state_bytes": "size_t: ZeggsLoudDims*",
    "zeggs_live_loudness_reset": "status: ZeggsLoudDims* any* size_t int float stream",
    "zeggs_live_loudness_hold": "status: ZeggsLoudDims* any* size_t int int stream",
    # rows_host: a HOST array of ZeggsLoudRow; rows_dev: the same records on the device (an address cast to the pointer type), None for one
    "zeggs_live_loudness_push": "status: ZeggsLoudDims* ZeggsLoudRow* ZeggsLoudRow* int any* size_t stream",
    "zeggs_live_loudness_read": "status: ZeggsLoudDims* any* size_t int host* stream",
}

# ----------------------------------------------------------------------------- the fourth header (include/zeggs_hip_resample.h)
# The rate converter of live serving (tests/test_live_resample_cpu.py compares these tables with the header).
ResampleDims = _struct("ResampleDims", [(C.c_int, "rows history")])
ResampleRow = _struct("ResampleRow", [(C.c_void_p, "src dst table"), (C.c_long, "count n_in n_out outputs WL"),
                                      (C.c_int, "row format final L M")])
RS_STRUCTS = {"ZeggsResampleDims": ResampleDims, "ZeggsResampleRow": ResampleRow}
RS_PROTOTYPES = {
    "zeggs_live_resample_version": "int:",
    "zeggs_resample_state_bytes": "size_t: ZeggsResampleDims*",
    "zeggs_resample_reset": "status: ZeggsResampleDims* any* size_t int stream",
    # rows_host / rows_dev as in zeggs_live_loudness_push
    "zeggs_resample_push": "status: ZeggsResampleDims* ZeggsResampleRow* ZeggsResampleRow* int any* size_t stream",
    "zeggs_resample_flush": "status: ZeggsResampleDims* ZeggsResampleRow* any* size_t stream",
    "zeggs_resample_whole": "status: f64* int int long any* int long f32* long stream",
}

# ----------------------------------------------------------------------------- the fifth header (include/zeggs_hip_frames.h)
# The output head of live serving (tests/test_live_frames_cpu.py compares these tables with the header).
FramesDims = _struct("FramesDims", [(C.c_int, "rows J max_frames what order")])
FramesRow = _struct("FramesRow", [(C.c_void_p, "pose rpos rrot local world bvh"), (C.c_long, "pose_ld rpos_ld rrot_ld"), (C.c_int, "row count")])
FR_STRUCTS = {"ZeggsFramesDims": FramesDims, "ZeggsFramesRow": FramesRow}
FR_PROTOTYPES = {
    "zeggs_live_frames_version": "int:",
    "zeggs_live_frames_state_bytes": "size_t: ZeggsFramesDims*",
    # parents / seq: HOST arrays of int
    "zeggs_live_frames_prepare": "status: ZeggsFramesDims* host* host* any* size_t stream",
    # ref_pos[3] / ref_rot[4] (float) and start_pos[3] / start_rot[4] (double): HOST arrays
    "zeggs_live_frames_reset": "status: ZeggsFramesDims* any* size_t int host* host* host* host* int stream",
    # rows_host / rows_dev as in zeggs_live_loudness_push
    "zeggs_live_frames": "status: ZeggsFramesDims* ZeggsFramesRow* ZeggsFramesRow* int any* size_t stream",
}

# ----------------------------------------------------------------------------- the sixth header (include/zeggs_hip_retime.h)
# The output head at each stream's own frame rate (tests/test_live_retime_cpu.py compares these tables with the header).
RetimeRow = _struct("RetimeRow", [(C.c_void_p, "pose rpos rrot local world bvh"), (C.c_long, "pose_ld rpos_ld rrot_ld n_in outputs"),
                                  (C.c_int, "row count L M")])
RT_STRUCTS = {"ZeggsRetimeRow": RetimeRow}
RT_PROTOTYPES = {
    "zeggs_live_retime_version": "int:",
    "zeggs_live_retime_state_bytes": "size_t: ZeggsFramesDims*",
    # parents / seq, ref / start: HOST arrays, as in the fifth header
    "zeggs_live_retime_prepare": "status: ZeggsFramesDims* host* host* any* size_t stream",
    "zeggs_live_retime_reset": "status: ZeggsFramesDims* any* size_t int host* host* host* host* int stream",
    # rows_host / rows_dev as in zeggs_live_loudness_push
    "zeggs_live_frames_retimed": "status: ZeggsFramesDims* ZeggsRetimeRow* ZeggsRetimeRow* int any* size_t stream",
}

# ----------------------------------------------------------------------------- the seventh header (include/zeggs_hip_refilter.h)
# The filter stage of the re-timing output head (tests/test_live_refilter_cpu.py compares these tables with the header).
RefilterRow = _struct("RefilterRow", [(C.c_void_p, "pose rpos rrot local world bvh"), (C.c_long, "pose_ld rpos_ld rrot_ld n_in outputs"),
                                      (C.c_int, "row count L M"), (C.c_void_p, "table"), (C.c_int, "half final")])
RF_STRUCTS = {"ZeggsRefilterRow": RefilterRow}
RF_PROTOTYPES = {
    "zeggs_live_refilter_version": "int:",
    "zeggs_live_refilter_state_bytes": "size_t: ZeggsFramesDims* int",
    # parents / seq, ref / start: HOST arrays, as in the fifth header
    "zeggs_live_refilter_prepare": "status: ZeggsFramesDims* int host* host* any* size_t stream",
    "zeggs_live_refilter_reset": "status: ZeggsFramesDims* int any* size_t int host* host* host* host* int stream",
    # rows_host / rows_dev as in zeggs_live_loudness_push
    "zeggs_live_frames_refiltered": "status: ZeggsFramesDims* int ZeggsRefilterRow* ZeggsRefilterRow* int any* size_t stream",
}


# ----------------------------------------------------------------------------- the eighth header (include/zeggs_hip_snapshot.h)
# Snapshot and restore of a live row's state (tests/test_live_snapshot_cpu.py compares these tables with the header).
SnapSpan = _struct("SnapSpan", [(C.c_size_t, "offset bytes")])
SnapSeg = _struct("SnapSeg", [(C.c_void_p, "src"), (C.c_size_t, "dst_offset bytes")])
SNAP_STRUCTS = {"ZeggsSnapSpan": SnapSpan, "ZeggsSnapSeg": SnapSeg}
SNAP_PROTOTYPES = {
    "zeggs_live_snapshot_version": "int:",
    # the span reports (host only): the count, or -1 with zeggs_last_error() ("mask": a negative value raises)
    "zeggs_live_loudness_spans": "mask: ZeggsLoudDims* int ZeggsSnapSpan* int",
    "zeggs_resample_spans": "mask: ZeggsResampleDims* int ZeggsSnapSpan* int",
    "zeggs_live_frames_spans": "mask: ZeggsFramesDims* int ZeggsSnapSpan* int",
    "zeggs_live_retime_spans": "mask: ZeggsFramesDims* int ZeggsSnapSpan* int",
    "zeggs_live_refilter_spans": "mask: ZeggsFramesDims* int int ZeggsSnapSpan* int",
    # segs_host: a HOST array of ZeggsSnapSeg; segs_dev: the same records on the device (an address cast to the pointer type)
    "zeggs_live_pack": "status: ZeggsSnapSeg* ZeggsSnapSeg* int any* size_t stream",
    "zeggs_live_unpack": "status: ZeggsSnapSeg* ZeggsSnapSeg* int any* size_t stream",
}


# ----------------------------------------------------------------------------- the ninth header (include/zeggs_hip_gaze.h)
# A gaze target per live row that can move while speech goes on (tests/test_live_gaze_cpu.py compares these tables with the header).
GazeDims = _struct("GazeDims", [(C.c_int, "rows ST")])
GazeSet = _struct("GazeSet", [(C.c_float * 3, "target pivot"), (C.c_long, "k fade"), (C.c_int, "row space path ease has_pivot")])
GazeCond = _struct("GazeCond", [(C.c_long, "k0 k_style fade_style"), (C.c_int, "row out_row n")])
GZ_STRUCTS = {"ZeggsGazeDims": GazeDims, "ZeggsGazeSet": GazeSet, "ZeggsGazeCond": GazeCond}
GZ_PROTOTYPES = {
    "zeggs_live_gaze_version": "int:",
    "zeggs_live_gaze_state_bytes": "size_t: ZeggsGazeDims*",
    "zeggs_live_gaze_reset": "status: ZeggsGazeDims* any* size_t int f32* stream",
    # recs_host: a HOST array of ZeggsGazeSet; recs_dev: the same records on the device (an address cast to the pointer type), None for one
    "zeggs_live_gaze_set": "status: ZeggsGazeDims* ZeggsGazeSet* ZeggsGazeSet* int f32* long f32* long any* size_t stream",
    "zeggs_live_condition": "status: ZeggsGazeDims* ZeggsGazeCond* ZeggsGazeCond* int any* size_t f32* f32* f32* f32* int long stream",
    "zeggs_live_gaze_read": "status: ZeggsGazeDims* any* size_t int long host* stream",
    "zeggs_live_gaze_spans": "mask: ZeggsGazeDims* int ZeggsSnapSpan* int",
}


# ----------------------------------------------------------------------------- the tenth header (include/zeggs_hip_styles.h)
# A bank of named styles on the device, mixed per live row (tests/test_live_styles_cpu.py compares these tables with the header).
StyleBankDims = _struct("StyleBankDims", [(C.c_int, "rows ST capacity")])
StyleMix = _struct("StyleMix", [(C.c_long, "k k_style fade_style"), (C.c_float * 8, "weight"), (C.c_int * 8, "slot"), (C.c_float, "temperature"),
                                (C.c_int, "row terms eps_row reset")])
SB_STRUCTS = {"ZeggsStyleBankDims": StyleBankDims, "ZeggsStyleMix": StyleMix}
SB_PROTOTYPES = {
    "zeggs_live_styles_version": "int:",
    "zeggs_live_style_bank_bytes": "size_t: ZeggsStyleBankDims*",
    "zeggs_live_style_put": "status: ZeggsStyleBankDims* any* size_t int f32* int stream",
    # recs_host: a HOST array of ZeggsStyleMix; recs_dev: the same records on the device (an address cast to the pointer type), None for one
    "zeggs_live_style_mix": "status: ZeggsStyleBankDims* ZeggsStyleMix* ZeggsStyleMix* int any* size_t f32* int f32* f32* stream",
    "zeggs_live_style_read": "status: ZeggsStyleBankDims* any* size_t int f32* f32* int host* stream",
}


# ----------------------------------------------------------------------------- the eleventh header (include/zeggs_hip_plant.h)
# Feet that stay planted: contact lock and leg IK for live rows (tests/test_live_plant_cpu.py compares these tables with the header).
PlantDims = _struct("PlantDims", [(C.c_int, "rows J max_frames chains release pad"), (C.c_double, "dt v_on v_off h_on h_off ground slack stretch")])
PlantRow = _struct("PlantRow", [(C.c_void_p, "pose rpos rrot out contacts"), (C.c_long, "pose_ld rpos_ld rrot_ld out_ld"), (C.c_int, "row count")])
PL_STRUCTS = {"ZeggsPlantDims": PlantDims, "ZeggsPlantRow": PlantRow}
PL_PROTOTYPES = {
    "zeggs_live_plant_version": "int:",
    "zeggs_live_plant_state_bytes": "size_t: ZeggsPlantDims*",
    # parents / chains: HOST arrays of int
    "zeggs_live_plant_prepare": "status: ZeggsPlantDims* host* host* any* size_t stream",
    "zeggs_live_plant_reset": "status: ZeggsPlantDims* any* size_t int stream",
    "zeggs_live_plant_spans": "mask: ZeggsPlantDims* int ZeggsSnapSpan* int",
    # recs_host / recs_dev as in zeggs_live_frames
    "zeggs_live_plant": "status: ZeggsPlantDims* ZeggsPlantRow* ZeggsPlantRow* int any* size_t stream",
}


# ----------------------------------------------------------------------------- the twelfth header (include/zeggs_hip_mirror.h)
# The signed column gather behind left/right mirroring (tests/test_mirror_cpu.py compares this table with the header).
MR_PROTOTYPES = {
    "zeggs_mirror_version": "int:",
    "zeggs_mirror_table_check": "status: host* int",              # table: a HOST array of int32
    "zeggs_mirror_plan_create": "status: host* int host*",        # table (HOST), cols, void** plan
    "zeggs_mirror_plan_free": "status: host*",
    "zeggs_mirror_plan_cols": "mask: host*",
    "zeggs_mirror_rows": "status: host* any* any* long int stream",
}


# ----------------------------------------------------------------------------- parameter types
class DevicePointer(C.c_void_p):
    """A device-pointer parameter: takes a tensor (on a GPU, contiguous, one of `dtypes`), None, a c_void_p or an address."""
    dtypes = None        # names of the torch dtypes it takes (None: any)
    _ok = None           # the dtypes themselves, once torch is there

    @classmethod
    def from_param(cls, t):
        if t is None:
            return None
        try:
            on_gpu = t.is_cuda
        except AttributeError:
            if isinstance(t, (int, C.c_void_p)):
                return C.c_void_p.from_param(t)
            raise TypeError(f"zeggs: a tensor, None or an address where the library reads a device pointer, not {type(t).__name__}") from None
        if not on_gpu:
            raise RuntimeError("zeggs: tensor is not on a GPU (the HIP engine has no CPU path)")
        if cls.dtypes is not None:
            if cls._ok is None:
                import torch
                cls._ok = tuple(getattr(torch, n) for n in cls.dtypes)
            if t.dtype not in cls._ok:
                raise TypeError(f"zeggs: {t.dtype} tensor where the library reads {' / '.join(cls.dtypes)}")
        if not t.is_contiguous():
            raise RuntimeError("zeggs: tensor must be contiguous")
        return C.c_void_p(t.data_ptr())


def _device_pointer(name, dtypes):
    return type(name, (DevicePointer,), {"dtypes": dtypes})


KINDS = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "uint64": C.c_uint64, "float": C.c_float, "double": C.c_double,
         "str": C.c_char_p, "host*": C.c_void_p, "stream": C.c_void_p,
         "f32*": _device_pointer("f32_p", ("float32",)), "f64*": _device_pointer("f64_p", ("float64",)),
         "i32*": _device_pointer("i32_p", ("int32",)), "i64*": _device_pointer("i64_p", ("int64",)),
         "u8*": _device_pointer("u8_p", ("uint8", "bool")), "any*": _device_pointer("any_p", None)}
KINDS.update({name + "*": C.POINTER(cls) for name, cls in {**STRUCTS, **EXT_STRUCTS, **LOUD_STRUCTS, **RS_STRUCTS, **FR_STRUCTS, **RT_STRUCTS, **RF_STRUCTS, **SNAP_STRUCTS, **GZ_STRUCTS, **SB_STRUCTS, **PL_STRUCTS}.items()})
RETURNS = {"status": C.c_int, "mask": C.c_int, "int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "str": C.c_char_p}


def signature(name):
    """-> (return kind, [parameter kinds]) of a row"""
    ret, _, params = (PROTOTYPES.get(name) or EXT_PROTOTYPES.get(name) or LOUD_PROTOTYPES.get(name) or RS_PROTOTYPES.get(name) or
                       FR_PROTOTYPES.get(name) or RT_PROTOTYPES.get(name) or RF_PROTOTYPES.get(name) or SNAP_PROTOTYPES.get(name) or GZ_PROTOTYPES.get(name) or SB_PROTOTYPES.get(name) or PL_PROTOTYPES.get(name) or MR_PROTOTYPES[name]).partition(":")
    return ret, params.split()


# ----------------------------------------------------------------------------- the two handles
class _Typed(C.CDLL):
    """CDLL whose functions hand on what a parameter type's from_param raised (ctypes wraps it in an ArgumentError) as the
    RuntimeError / TypeError it was, with the function's name in front."""

    def __init__(self, path):
        super().__init__(path)
        base = self._FuncPtr

        class _Fn(base):
            _flags_, _restype_ = base._flags_, base._restype_

            def __call__(self, *args, _call=base.__call__):
                try:
                    return _call(self, *args)
                except C.ArgumentError as e:
                    raise (TypeError if ": TypeError: " in str(e) else RuntimeError)(f"{self.__name__}: {e}") from None
        self._FuncPtr = _Fn


_HANDLES = None
_LOCK = threading.Lock()


def _load():
    global _HANDLES
    with _LOCK:
        if _HANDLES is not None:
            return _HANDLES
        if not LIB_PATH.exists():
            raise HipLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The ZeroEGGS MI355X engine has no CPU fallback.")
        typed, plain = _Typed(str(LIB_PATH)), C.CDLL(str(LIB_PATH))
        missing = [n for n in (*PROTOTYPES, *EXT_PROTOTYPES, *LOUD_PROTOTYPES, *RS_PROTOTYPES, *FR_PROTOTYPES, *RT_PROTOTYPES, *RF_PROTOTYPES, *SNAP_PROTOTYPES, *GZ_PROTOTYPES, *SB_PROTOTYPES, *PL_PROTOTYPES, *MR_PROTOTYPES) if not hasattr(plain, n)]
        if missing:
            raise HipLibraryMissing(f"{LIB_PATH} is older than this package (no {', '.join(missing)}): rebuild it")
        last_error = typed.zeggs_last_error

        def status(rc, fn, args):
            if rc != 0:
                raise RuntimeError(f"{fn.__name__}: {last_error().decode()}")
            return rc

        def mask(rc, fn, args):
            return rc if rc >= 0 else status(rc, fn, args)
        for name in (*PROTOTYPES, *EXT_PROTOTYPES, *LOUD_PROTOTYPES, *RS_PROTOTYPES, *FR_PROTOTYPES, *RT_PROTOTYPES, *RF_PROTOTYPES, *SNAP_PROTOTYPES, *GZ_PROTOTYPES, *SB_PROTOTYPES, *PL_PROTOTYPES, *MR_PROTOTYPES):
            ret, params = signature(name)
            fn = getattr(typed, name)
            fn.argtypes, fn.restype = [KINDS[k] for k in params], RETURNS[ret]
            if ret in ("status", "mask"):
                fn.errcheck = status if ret == "status" else mask
            getattr(plain, name).restype = RETURNS[ret]
        # tuning switches for experiments, e.g. ZEGGS_OPTIONS="bwd_chunks=4,stage_variant=0" (see zeggs_set_option)
        for kv in filter(None, os.environ.get("ZEGGS_OPTIONS", "").split(",")):
            k, v = kv.split("=")
            try:
                typed.zeggs_set_option(k.strip().encode(), int(v))
            except RuntimeError as e:
                raise RuntimeError(f"ZEGGS_OPTIONS: {str(e).partition(': ')[2]}") from None
            OPTIONS[k.strip()] = int(v)
        _HANDLES = (typed, plain)
        return _HANDLES


def api():
    """The typed handle (loads the library built by __graft_entry__.build() / csrc/build.sh on first use)."""
    return (_HANDLES or _load())[0]


def raw():
    """The handle without argument types or error checks (ops.lib())."""
    return (_HANDLES or _load())[1]

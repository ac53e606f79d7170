"""ctypes binding of libfacodec_hip.so (C ABI declared in include/facodec_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, the product path
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FAC_LIB_PATH", os.path.join(_HERE, "libfacodec_hip.so"))

PAD_ZERO, PAD_REFLECT = 0, 1
ACT_NONE, ACT_TANH, ACT_MISH, ACT_LOG_MEL = 0, 1, 2, 3
ACT_GATE, ACT_WN_RES_SKIP = 4, 5          # epilogues of the few-column split-reduction launches only (facodec_hip.h)

_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64
_f = C.c_float


class ConvDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("w", _p), ("bias", _p), ("alpha_in", _p), ("alpha_out", _p), ("res", _p), ("y", _p), ("y2", _p), ("alpha_y2", _p), ("w_k1", _p), ("bias_k1", _p),
        ("x_bs", _i64), ("x_cs", _i64), ("y_bs", _i64), ("y_cs", _i64),
        ("B", C.c_int32), ("C_in", C.c_int32), ("T_in", C.c_int32), ("C_out", C.c_int32),
        ("C_out_pad", C.c_int32), ("T_out", C.c_int32),
        ("K", C.c_int32), ("stride", C.c_int32), ("dilation", C.c_int32), ("pad_left", C.c_int32),
        ("pad_mode", C.c_int32), ("n_phase", C.c_int32), ("y_tstride", C.c_int32), ("phase_shift", C.c_int32),
        ("act", C.c_int32),
        ("w_batched", C.c_int32), ("w_bs", _i64), ("ws", _p), ("ws_bytes", _i64), ("w_split", _p),
        ("K1", C.c_int32), ("dilation2", C.c_int32), ("row_phases", C.c_int32),
        ("x_p8", _p), ("x_p8_plane_bytes", _i64), ("y2_p8", _p), ("y2_p8_plane_bytes", _i64),
        ("pw_split", C.c_int32), ("split_rows", C.c_int32),
        ("gate_cond", _p), ("gate_cond_bs", _i64),
        ("keep_tile160", C.c_int32), ("gsplit_p8_cols", C.c_int32),
    ]


class VqDesc(C.Structure):
    _fields_ = [
        ("residual", _p), ("z_in", _p), ("zq_acc", _p), ("zq_out", _p), ("w_in", _p), ("b_in", _p),
        ("codebook", _p), ("w_out", _p), ("w_out_scale", _p), ("b_out", _p), ("mask", _p), ("codes", _p), ("z_e", _p),
        ("loss_part", _p), ("codes_bs", _i64),
        ("B", C.c_int32), ("D", C.c_int32), ("T", C.c_int32), ("Kc", C.c_int32),
    ]



VQ_DECODE_MAX_Q = 16


class VqDecodeDesc(C.Structure):
    _fields_ = [
        ("codes", _p * 3), ("codes_bs", _i64 * 3), ("codes_qs", _i64 * 3), ("n_q", C.c_int32 * 3),
        ("codebook", _p * VQ_DECODE_MAX_Q), ("w_out", _p * VQ_DECODE_MAX_Q), ("w_out_scale", _p * VQ_DECODE_MAX_Q),
        ("b_out", _p * VQ_DECODE_MAX_Q), ("style", _p), ("outs", _p), ("z", _p * 3),
        ("B", C.c_int32), ("D", C.c_int32), ("T", C.c_int32), ("Kc", C.c_int32),
    ]


class VqDecodeMaskedDesc(C.Structure):
    _fields_ = [("base", VqDecodeDesc), ("n_use", _p), ("n_use_bs", _i64), ("n_use_ts", _i64)]


PLC_MAX_FRAMES = 16                      # FAC_PLC_MAX_FRAMES
PLC_PRIMARY, PLC_REDUNDANT, PLC_LOST = 0, 1, 2


class PlcSelectDesc(C.Structure):
    _fields_ = [
        ("prim", _p * 3), ("prim_bs", _i64 * 3), ("prim_qs", _i64 * 3),
        ("red", _p * 3), ("red_bs", _i64 * 3), ("red_qs", _i64 * 3),
        ("dst", _p * 3), ("dst_bs", _i64 * 3), ("dst_qs", _i64 * 3),
        ("n_q", C.c_int32 * 3), ("n_red", C.c_int32 * 3),
        ("status", _p), ("last_codes", _p), ("last_n", _p), ("g", _p), ("run", _p),
        ("n_use", _p), ("n_use_bs", _i64), ("n_use_ts", _i64), ("ramp", _p),
        ("B", C.c_int32), ("k", C.c_int32), ("hold", C.c_int32), ("fade", C.c_int32), ("recover", C.c_int32),
        ("reserved", C.c_int32),
    ]


VAD_MAX_FRAME, VAD_MAX_WINDOW = 4096, 2048          # FAC_VAD_MAX_FRAME, FAC_VAD_MAX_WINDOW
SID_PASS, SID_STORE, SID_FILL = 0, 1, 2


class VadEnergyDesc(C.Structure):
    _fields_ = [
        ("carry_in", _p), ("carry_out", _p), ("x", _p), ("lens", _p), ("e", _p),
        ("x_bs", _i64), ("e_bs", _i64), ("f0", _i64),
        ("B", C.c_int32), ("k", C.c_int32), ("frame", C.c_int32), ("carry_n", C.c_int32), ("is_final", C.c_int32), ("R", C.c_int32),
    ]


class VadDecideDesc(C.Structure):
    _fields_ = [
        ("e", _p), ("lens", _p), ("flags", _p), ("ring", _p),
        ("e_bs", _i64), ("flags_bs", _i64), ("ring_bs", _i64), ("f0", _i64),
        ("margin", C.c_double), ("thr_abs", C.c_double),
        ("B", C.c_int32), ("n_new", C.c_int32), ("R", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("frame", C.c_int32),
    ]


AGC_MAX_WINDOW, AGC_MAX_LOOKAHEAD = 1024, 1024       # FAC_AGC_MAX_WINDOW, FAC_AGC_MAX_LOOKAHEAD


class AgcGainsDesc(C.Structure):
    _fields_ = [
        ("e", _p), ("lens", _p), ("j_start", _p), ("G", _p), ("g", _p),
        ("e_bs", _i64), ("g_bs", _i64), ("j0", _i64),
        ("target_db", C.c_double), ("max_boost_db", C.c_double), ("max_cut_db", C.c_double),
        ("B", C.c_int32), ("n_new", C.c_int32), ("R", C.c_int32), ("W", C.c_int32), ("S", C.c_int32), ("reserved", C.c_int32),
    ]


class AgcApplyDesc(C.Structure):
    _fields_ = [
        ("carry_in", _p), ("carry_out", _p), ("x", _p), ("lens", _p), ("j_start", _p), ("g", _p), ("y", _p),
        ("x_bs", _i64), ("g_bs", _i64), ("y_bs", _i64), ("n0", _i64),
        ("ceiling", C.c_double),
        ("B", C.c_int32), ("k", C.c_int32), ("n_out", C.c_int32), ("S", C.c_int32), ("LA", C.c_int32), ("R", C.c_int32),
    ]


NS_N, NS_H, NS_BINS, NS_CARRY, NS_MAX_M, NS_MAX_W = 512, 256, 257, 1023, 64, 256      # FAC_NS_*


class NsPowerDesc(C.Structure):
    _fields_ = [
        ("carry_in", _p), ("carry_out", _p), ("x", _p), ("lens", _p), ("starts", _p), ("P", _p), ("X", _p),
        ("x_bs", _i64), ("p_bs", _i64), ("n0", _i64), ("f0", _i64),
        ("B", C.c_int32), ("k", C.c_int32), ("n_new", C.c_int32), ("R", C.c_int32),
    ]


class NsGainsDesc(C.Structure):
    _fields_ = [
        ("P", _p), ("starts", _p), ("G", _p),
        ("p_bs", _i64), ("g_bs", _i64), ("f0", _i64),
        ("over", C.c_double), ("g_min", C.c_double),
        ("B", C.c_int32), ("n_new", C.c_int32), ("R", C.c_int32), ("M", C.c_int32), ("W", C.c_int32), ("reserved", C.c_int32),
    ]


class NsSynthDesc(C.Structure):
    _fields_ = [
        ("carry_in", _p), ("x", _p), ("lens", _p), ("starts", _p), ("G", _p), ("X", _p), ("y", _p),
        ("x_bs", _i64), ("g_bs", _i64), ("y_bs", _i64), ("n0", _i64), ("m0", _i64),
        ("B", C.c_int32), ("k", C.c_int32), ("n_out", C.c_int32), ("R", C.c_int32),
    ]


AEC_N, AEC_H, AEC_BINS, AEC_MAX_P, AEC_LDS_P, AEC_MAX_DELAY, AEC_MIC_CARRY, AEC_FAR_CARRY = 512, 256, 257, 32, 8, 16384, 255, 511     # FAC_AEC_*


class AecDesc(C.Structure):
    _fields_ = [
        ("mic_carry_in", _p), ("mic_carry_out", _p), ("far_carry_in", _p), ("far_carry_out", _p), ("mic", _p), ("far", _p),
        ("lens", _p), ("starts", _p), ("adapt", _p), ("W", _p), ("X", _p), ("e_ring", _p), ("y", _p), ("stats", _p),
        ("mic_bs", _i64), ("far_bs", _i64), ("y_bs", _i64), ("w_bs", _i64), ("xr_bs", _i64), ("s_bs", _i64),
        ("n0", _i64), ("m0", _i64), ("blk0", _i64),
        ("mu", C.c_double), ("c", C.c_double), ("delta", C.c_double),
        ("B", C.c_int32), ("k", C.c_int32), ("n_out", C.c_int32), ("n_blk", C.c_int32), ("P", C.c_int32), ("delay", C.c_int32),
        ("far_cn", C.c_int32), ("reserved", C.c_int32),
    ]


EDELAY_MAX_DELAY, EDELAY_MAX_LAGS, EDELAY_MIC_RING, EDELAY_POL = 16384, 65, 511, 4     # FAC_EDELAY_*


class EdelayDesc(C.Structure):
    _fields_ = [
        ("mic", _p), ("far", _p), ("lens", _p), ("starts", _p), ("mic_ring", _p), ("far_ring", _p), ("C", _p), ("X", _p), ("act", _p),
        ("pol", _p), ("conf_last", _p), ("y", _p), ("raw", _p), ("locked", _p), ("used", _p), ("conf", _p), ("ok", _p), ("score", _p),
        ("mic_bs", _i64), ("far_bs", _i64), ("y_bs", _i64), ("c_bs", _i64), ("xr_bs", _i64), ("f_bs", _i64), ("n0", _i64), ("frm0", _i64),
        ("a", C.c_double), ("eps", C.c_double), ("gate", C.c_double), ("thr", C.c_double),
        ("B", C.c_int32), ("k", C.c_int32), ("n_frm", C.c_int32), ("f_ring", C.c_int32), ("max_delay", C.c_int32), ("far_rn", C.c_int32),
        ("k_lo", C.c_int32), ("k_hi", C.c_int32), ("hold", C.c_int32), ("tol", C.c_int32), ("move", C.c_int32), ("margin", C.c_int32),
        ("delay0", C.c_int32), ("reserved", C.c_int32),
    ]


class SidApplyDesc(C.Structure):
    _fields_ = [
        ("dst", _p * 3), ("dst_bs", _i64 * 3), ("dst_qs", _i64 * 3), ("n_q", C.c_int32 * 3), ("B", C.c_int32),
        ("mode", _p), ("sid_codes", _p), ("k", C.c_int32), ("reserved", C.c_int32),
    ]


class CodesPackDesc(C.Structure):
    _fields_ = [
        ("codes", _p * 3), ("codes_bs", _i64 * 3), ("codes_qs", _i64 * 3), ("n_q", C.c_int32 * 3),
        ("lens", _p), ("out", _p), ("out_bs", _i64),
        ("B", C.c_int32), ("T", C.c_int32), ("bits", C.c_int32),
    ]


class CodesUnpackDesc(C.Structure):
    _fields_ = [
        ("in_", _p), ("in_bs", _i64), ("codes", _p * 3), ("codes_bs", _i64 * 3), ("codes_qs", _i64 * 3), ("n_q", C.c_int32 * 3),
        ("lens", _p),
        ("B", C.c_int32), ("T", C.c_int32), ("bits", C.c_int32),
    ]


class ResampleDesc(C.Structure):
    _fields_ = [
        ("hist", _p), ("x", _p), ("lens", _p), ("y", _p), ("hist_out", _p), ("table", _p), ("offs", _p),
        ("hist_bs", _i64), ("x_bs", _i64), ("y_bs", _i64), ("q0", _i64), ("m_lo", _i64),
        ("B", C.c_int32), ("n_hist", C.c_int32), ("T", C.c_int32), ("n_out", C.c_int32),
        ("o", C.c_int32), ("n", C.c_int32), ("taps", C.c_int32),
    ]


class KweightDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("lens", _p), ("e", _p), ("state_in", _p), ("state_out", _p), ("peak", _p), ("ws", _p),
        ("x_bs", _i64), ("e_bs", _i64),
        ("B", C.c_int32), ("T", C.c_int32), ("S", C.c_int32), ("offset", C.c_int32), ("peak_accumulate", C.c_int32),
        ("reserved", C.c_int32),
        ("coef", C.c_double * 10), ("pw", C.c_double * 16 * 7),
    ]


SI_SDR_CHUNK = 4096                      # FAC_SI_SDR_CHUNK


class StoiDesc(C.Structure):
    _fields_ = [
        ("x", _p), ("y", _p), ("lens", _p), ("kept_idx", _p), ("n_frames", _p), ("n_kept", _p), ("n_segments", _p),
        ("stoi", _p), ("estoi", _p), ("ws", _p),
        ("x_bs", _i64), ("y_bs", _i64), ("ws_bytes", _i64),
        ("B", C.c_int32), ("T", C.c_int32),
    ]


SLOT_MAX_DST, SLOT_TILE = 8, 4096        # FAC_SLOT_MAX_DST, FAC_SLOT_TILE


class SlotSeg(C.Structure):
    _fields_ = [
        ("base", _p), ("slot_hi", _i64),
        ("rows", C.c_int32), ("row_stride", C.c_int32), ("row_len", C.c_int32), ("slot_lo", C.c_int32),
        ("elems", C.c_int32), ("reserved", C.c_int32),
    ]


# name -> (restype, argtypes); must list every symbol include/facodec_hip.h declares
SIGNATURES = {
    "fac_version": (_i, []),
    "fac_last_error": (C.c_char_p, []),
    "fac_wn_scale": (_i, [_p, _p, _p, _i, _i, _p]),
    "fac_pack_conv_w": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_pack_convtr_w_rows": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_conv_w_split_bytes": (_i64, [_i, _i, _i]),
    "fac_conv_w_split2_bytes": (_i64, [_i, _i, _i, _i]),
    "fac_pack_conv_w_split2": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_gemm_w_split_bytes": (_i64, [_i, _i, _i, _i]),
    "fac_pack_gemm_w_split": (_i, [_p, _i64, _i64, _i64, _p, _p, _i, _i, _i, _i, _p]),
    "fac_pack_conv_w_split": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_conv_w_split_rows_bytes": (_i64, [_i, _i, _i, _i]),
    "fac_pack_conv_w_split_rows": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_flip_transpose_w": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_prep_begin": (_i, []),
    "fac_prep_set_phase": (_i, [_i]),
    "fac_prep_abort": (_i, []),
    "fac_prep_end": (_i, []),
    "fac_prep_replay": (_i, [_i, _p]),
    "fac_prep_info": (_i, [_i, _p, _p]),
    "fac_prep_free": (_i, [_i]),
    "fac_pack_conv_w_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_pad_fold_bwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "fac_conv1d_bwd_weight_ws_bytes": (_i64, [_i, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_conv1d_bwd_weight_split_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_split_form": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int)]),
    "fac_conv1d_bwd_weight_k1_ws_bytes": (_i64, [_i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_k1_ws_bytes_for": (_i64, [_p, _p, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_taps_tx": (_i64, [_i, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_taps_ws_bytes": (_i64, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_taps_ws_bytes_for": (_i64, [_p, _i, _i, _i, _i, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_taps": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_conv1d_bwd_weight_k1": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "fac_conv1d_bwd_weight_split": (_i, [_p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_conv1d_bwd_weight_split_db_ok": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i]),
    "fac_conv1d_bwd_weight_split_db": (_i, [_p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_weight_norm_bwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _p]),
    "fac_snake_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_pack_lstm_whh_t": (_i, [_p, _p, _i, _p]),
    "fac_lstm_layer_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_to_p8": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_lstm_persist_ok": (_i, [_i, _i]),
    "fac_lstm_persist_stream_ok": (_i, [_p]),
    "fac_pack_lstm_whh16": (_i, [_p, _p, _i, _i, _p]),
    "fac_lstm_layer_fwd_persist": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_lstm_layer_bwd_persist": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_lstm_persist_split_ok": (_i, [_i, _i]),
    "fac_lstm_persist_timeouts": (_i, []),
    "fac_lstm_persist_arm": (_i, [_p]),
    "fac_lstm_abort_flag": (_i, [_p, _p]),
    "fac_mask_flags_if": (_i, [_p, _i, _p, _p]),
    "fac_pack_lstm_whh_split": (_i, [_p, _p, _i, _p]),
    "fac_lstm_layer_fwd_persist_split": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_snake_bwd_fused": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_bias_grad": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_snake_bwd_fused_rs": (_i, [_p, _p, _p, _i64, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_pad_fold_edges": (_i, [_p, _i, _i, _i, _i, _i, _p]),
    "fac_pack_convtr_w": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_conv1d_fwd": (_i, [C.POINTER(ConvDesc), _p]),
    "fac_conv1d_variant": (_i, [C.POINTER(ConvDesc), C.c_char_p, _i]),
    "fac_gsplit_p8_tile_cols": (_i, [_i64, _i64, _i64, _i]),
    "fac_snake_fwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_lstm_to_time_major": (_i, [_p, _p, _i, _i, _i, _p]),
    "fac_lstm_from_time_major": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_pack_lstm_whh": (_i, [_p, _p, _i, _p]),
    "fac_lstm_layer_fwd": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_lstm_layer_fwd_from": (_i, [_p, _p, _p, _p, _i, _i, _i, _i64, _p]),
    "fac_lstm_layer_fwd_train": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i64, _p]),
    "fac_lstm_gate_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i64, _i, _p]),
    "fac_tanh_bwd": (_i, [_p, _p, _p, _i64, _p]),
    "fac_pair_bwd": (_i, [_p, _p, _p, _i64, _i, C.c_float, C.c_float, _i, _p]),
    "fac_spec_power_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_stft_frames_bwd": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_vq_latent_bwd": (_i, [_p, _p, _p, _i64, _p, _p, _p, _p, _i, _i, _p]),
    "fac_vq_codebook_grad": (_i, [_p, _p, _p, _i64, _p, _p, _i, _i, _i, _i, _p]),
    "fac_layernorm_c_affine_bwd": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_rows_fma": (_i, [_p, _p, _p, _p, _i, _i64, _f, _p]),
    "fac_grad_norm_clip": (_i, [_p, _i64, _f, _p, _p, _p]),
    "fac_adamw_step": (_i, [_p, _p, _p, _p, _i64, _f, _f, _f, _f, _f, _i64, _p, _p]),
    "fac_logdiff_rms_bwd": (_i, [_p, _p, _p, _i, _i, _i, _f, _f, _i, _p]),
    "fac_gather_copy": (_i, [_p, _p, _p, _i, _p]),
    "fac_adamw_step_masked": (_i, [_p, _p, _p, _p, _i64, _p, _i, _p, _p, _p, _f, _f, _f, _f, _f, _p, _p]),
    "fac_gate_bwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_mish_fwd": (_i, [_p, _p, _i64, _p]),
    "fac_mish_bwd": (_i, [_p, _p, _p, _i64, _p]),
    "fac_glu_bwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_mul_scaled": (_i, [_p, _p, _p, _f, _i64, _p]),
    "fac_embed_sum_bwd": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_gate_bwd_cond": (_i, [_p, _p, _i64, _p, _p, _p, _i64, _i, _i, _i, _p]),
    "fac_masked_mean_bwd": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_attention_probs": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_pv": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_bwd_pv": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_bwd_qk": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_aa_snakebeta_bwd": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_leaky_relu": (_i, [_p, _p, _p, _i64, _f, _i, _i, _i, _i, _i, _p]),
    "fac_spec_to_cat": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_period_fold": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "fac_zero_insert": (_i, [_p, _p, _i64, _i, _i, _p]),
    "fac_row_stack3": (_i, [_p, _p, _i64, _i, _i, _i, _i, _p]),
    "fac_spec_to_rows": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "fac_pad_reflect": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "fac_disc_preprocess": (_i, [_p, _p, _p, _p, _i, _i, _p]),
    "fac_cross_entropy": (_i, [_p, _p, _p, _p, _p, _i64, _i, _f, _p]),
    "fac_focal_scalar": (_i, [_p, _p, _f, _p]),
    "fac_crop_rows": (_i, [_p, _p, _p, _i, _i, _i64, _i, _i, _p]),
    "fac_stream_push": (_i, [_p, _p, _i64, _i64, _i, _i, _i, _p]),
    "fac_vq_fwd": (_i, [C.POINTER(VqDesc), _p]),
    "fac_vq_loss_tiles": (_i, [_i]),
    "fac_vq_decode": (_i, [C.POINTER(VqDecodeDesc), _p]),
    "fac_vq_decode_masked": (_i, [C.POINTER(VqDecodeMaskedDesc), _p]),
    "fac_plc_select": (_i, [C.POINTER(PlcSelectDesc), _p]),
    "fac_plc_gain": (_i, [_p, _i64, _p, _i64, _p, _i, _i, _i, _p]),
    "fac_vad_energy": (_i, [C.POINTER(VadEnergyDesc), _p]),
    "fac_vad_decide": (_i, [C.POINTER(VadDecideDesc), _p]),
    "fac_vad_take": (_i, [_p, _i64, _i, _i64, _i, _p, _i64, _i, _p]),
    "fac_sid_apply": (_i, [C.POINTER(SidApplyDesc), _p]),
    "fac_agc_gains": (_i, [C.POINTER(AgcGainsDesc), _p]),
    "fac_agc_apply": (_i, [C.POINTER(AgcApplyDesc), _p]),
    "fac_ns_power": (_i, [C.POINTER(NsPowerDesc), _p]),
    "fac_ns_gains": (_i, [C.POINTER(NsGainsDesc), _p]),
    "fac_ns_synth": (_i, [C.POINTER(NsSynthDesc), _p]),
    "fac_aec_run": (_i, [C.POINTER(AecDesc), _p]),
    "fac_aec_state_sizes": (_i, [_i, _i, C.POINTER(_i64)]),
    "fac_edelay_run": (_i, [C.POINTER(EdelayDesc), _p]),
    "fac_edelay_state_sizes": (_i, [_i, C.POINTER(_i64)]),
    "fac_true_peak_ws_bytes": (_i64, [_i, _i]),
    "fac_true_peak": (_i, [C.POINTER(ResampleDesc), _p, _p, _p]),
    "fac_codes_pack": (_i, [C.POINTER(CodesPackDesc), _p]),
    "fac_codes_unpack": (_i, [C.POINTER(CodesUnpackDesc), _p]),
    "fac_codes_row_bytes": (_i64, [_i, _i, _i]),
    "fac_rccl_available": (_i, []),
    "fac_rccl_unique_id": (_i, [_p]),
    "fac_rccl_comm_init": (_i, [C.POINTER(_p), _p, _i, _i]),
    "fac_rccl_comm_destroy": (_i, [_p]),
    "fac_allreduce_arena": (_i, [_p, _p, _i64, _i, _p]),
    "fac_vq_search": (_i, [_p, _p, _p, _i64, _i, _p]),
    "fac_gate_tanh_sigmoid": (_i, [_p, _p, _i64, _p, _i, _i, _i, _p]),
    "fac_embed_sum": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_glu_residual": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_add": (_i, [_p, _p, _p, _i64, _p]),
    "fac_sub2": (_i, [_p, _p, _p, _p, _i64, _p]),
    "fac_mul_mask": (_i, [_p, _p, _i, _i, _i, _p]),
    "fac_wn_res_skip": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_stream": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_route": (_i, [_i, _i]),
    "fac_attention_form": (_i, [_i, _i]),
    "fac_attention_tiled_fits": (_i, [_i, _i]),
    "fac_attention_tiled": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_serial": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_attention_stream_tile": (_i, [_i]),
    "fac_masked_mean": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_layernorm_c_affine": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_stft_frames": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_stft_frames_ragged": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_mask_tail": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "fac_mask_tail_i64": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "fac_edge_tail": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "fac_frame_mask": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "fac_resample": (_i, [C.POINTER(ResampleDesc), _p]),
    "fac_resample_form": (_i, [C.POINTER(ResampleDesc), _p]),
    "fac_kweight_ws_bytes": (_i64, [_i, _i]),
    "fac_kweight_energy": (_i, [C.POINTER(KweightDesc), _p]),
    "fac_loudness_chunk": (_i, [_i]),
    "fac_loudness_gate": (_i, [_p, _i64, _p, _i64, _i, _i, _p, _i, _p, _p, _i, _p]),
    "fac_loudness_gain": (_i, [_p, _i64, _p, _p, _p, _p, C.c_double, _i, _p, _i64, _p, _i, _i, _p]),
    "fac_si_sdr_ws_bytes": (_i64, [_i, _i]),
    "fac_si_sdr": (_i, [_p, _i64, _p, _i64, _p, _p, _p, _i64, _i, _i, _p]),
    "fac_stoi_geometry": (_i, [_i, C.POINTER(_i64)]),
    "fac_stoi_select": (_i, [C.POINTER(StoiDesc), _p]),
    "fac_stoi_bands": (_i, [C.POINTER(StoiDesc), _p]),
    "fac_stoi_score": (_i, [C.POINTER(StoiDesc), _p]),
    "fac_slot_copy": (_i, [_p, _i, _p, _i, _i, _i, C.POINTER(C.c_int32), _i, _p]),
    "fac_rows_pick": (_i, [_p, _i64, _p, _p, _i, _i, _i, _p]),
    "fac_spec_power": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "fac_reduce_pair": (_i, [_p, _p, _p, _p, _i64, _i, _f, _f, _i, _p]),
    "fac_aa_snakebeta_fwd": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "fac_logdiff_rms": (_i, [_p, _p, _p, _p, _i, _i, _i, _f, _f, _i, _p]),
    "fac_jdc_affine_lrelu_pool": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _p]),
    "fac_jdc_layout_in": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "fac_jdc_to_time_major": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "fac_jdc_to_nchw": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "fac_jdc_head": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "fac_f0_normalize": (_i, [_p, _p, _p, _i, _i, _p]),
    "fac_mel_log_norm": (_i, [_p, _p, _i, _i, _i, _p]),
}

_lib = None


class FacodecHipError(RuntimeError):
    pass


def load():
    """Loads the shared library (once).  Raises FacodecHipError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FacodecHipError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m facodec_amd.build` (needs hipcc, cross-compiles gfx950).")
    # One HIP runtime per process: torch bundles its own libamdhip64, and a second copy (the system one, pulled
    # in if this library were loaded first) initialises with "no ROCm-capable device".  Import torch first so
    # that our DT_NEEDED entry resolves to the copy already in the process.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().fac_last_error().decode("utf-8", "replace")
        raise FacodecHipError(f"{what} failed (rc={rc}): {msg}")

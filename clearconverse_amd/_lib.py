"""ctypes binding of libccx.so (the C ABI declared in include/ccx.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, a
`CcxError` is raised.  Tensors are torch ROCm tensors; only `data_ptr()` and the current HIP
stream cross the boundary.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libccx.so"


class CcxError(RuntimeError):
    pass


class WhisperDims(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
        "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]


class SepformerDims(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "n_filters", "kernel", "stride", "d_model", "n_head", "d_ffn", "n_layers", "n_blocks", "segment", "n_spk")]


class DecodeRules(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "eot", "sot", "sot_prev", "no_speech", "no_timestamps", "timestamp_begin", "blank",
        "max_initial_timestamp_index", "n_suppress")] + [("suppress", C.POINTER(C.c_int))]


class DecodeOptions(C.Structure):
    """ccx_decode_options (include/ccx.h): the per-call decoding options; ccx_decode_options_default fills the defaults."""
    _fields_ = [("without_timestamps", C.c_int), ("suppress_blank", C.c_int), ("max_initial_timestamp_index", C.c_int),
                ("n_suppress", C.c_int), ("suppress", C.POINTER(C.c_int))]


class GemmDesc(C.Structure):
    """ccx_gemm_desc (include/ccx.h): csrc/gemm_bf16.h GemmParams field for field, then the element count of every buffer."""
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("lda", C.c_int64), ("ldw", C.c_int64),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("ntaps", C.c_int), ("a_tap_stride", C.c_int64),
        ("bias", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int64), ("resid", C.c_void_p), ("ldr", C.c_int64),
        ("resid_mod", C.c_int), ("scale", C.c_void_p), ("shift", C.c_void_p), ("slope", C.c_float),
        ("rpb_in", C.c_int), ("rpb_out", C.c_int), ("roff", C.c_int), ("rpb_valid", C.c_int),
        ("img_rows_in", C.c_int), ("img_rows_valid", C.c_int), ("img_rows_out", C.c_int),
        ("resid_bf16", C.c_void_p), ("ldrb", C.c_int64),
        ("hq", C.c_void_p), ("hk", C.c_void_p), ("hv", C.c_void_p),
        ("d_model", C.c_int), ("n_head", C.c_int), ("S", C.c_int), ("Spad", C.c_int),
        ("v_transposed", C.c_int), ("first_block", C.c_int),
        ("a_elems", C.c_int64), ("w_elems", C.c_int64), ("out_elems", C.c_int64), ("resid_elems", C.c_int64),
        ("resid_bf16_elems", C.c_int64), ("heads_elems", C.c_int64)]


class DecAttnDesc(C.Structure):
    """ccx_dec_attn_desc (include/ccx.h): one decode attention form on its own."""
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p),
        ("rows", C.c_int), ("n_seq", C.c_int), ("H", C.c_int), ("kv_T", C.c_int), ("T", C.c_int),
        ("pos", C.POINTER(C.c_int)), ("row_seq", C.POINTER(C.c_int)), ("rows_per_seq", C.c_int),
        ("nsplit", C.c_int), ("combine", C.c_int), ("lds_pad", C.c_int),
        ("x", C.c_void_p), ("pend", C.c_void_p), ("pend_n", C.c_int), ("pend_stride", C.c_int64),
        ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("eps", C.c_float),
        ("wq_host", C.c_void_p), ("bq", C.c_void_p),
        ("out", C.c_void_p), ("part_o", C.c_void_p), ("part_ml", C.c_void_p), ("q_x_out", C.c_void_p),
        ("q_elems", C.c_int64), ("kv_elems", C.c_int64), ("out_elems", C.c_int64), ("part_o_elems", C.c_int64),
        ("part_ml_elems", C.c_int64), ("x_elems", C.c_int64), ("pend_elems", C.c_int64), ("q_x_out_elems", C.c_int64),
        ("ind", C.POINTER(C.c_uint16)), ("ind_ld", C.c_int)]


DEC_ATTN_SELF, DEC_ATTN_SPLIT, DEC_ATTN_STREAM, DEC_ATTN_PREFILL, DEC_ATTN_FUSED_Q, DEC_ATTN_TWO_LAUNCH_Q = range(6)
DEC_ATTN_STREAM_MAPPED = 7       # (6 is no form)
DEC_ATTN_SELF_IND = 8            # the self form through a cache indirection (beam search)


class DecMidChainDesc(C.Structure):
    """ccx_dec_mid_chain_desc (include/ccx.h): self attention .. cross-attention out projection of the X-stream decode chain on its own."""
    _fields_ = [
        ("M", C.c_int), ("D", C.c_int), ("H", C.c_int), ("S", C.c_int), ("kv_T", C.c_int), ("packed", C.c_int),
        ("q", C.c_void_p), ("self_k", C.c_void_p), ("self_v", C.c_void_p), ("x", C.c_void_p), ("shift", C.c_void_p), ("xa", C.c_void_p),
        ("pos", C.c_void_p),
        ("wo", C.c_void_p), ("bo", C.c_void_p),
        ("lnc_g", C.c_void_p), ("lnc_b", C.c_void_p), ("cq_w", C.c_void_p), ("cq_b", C.c_void_p),
        ("ck_w", C.c_void_p), ("cv_w", C.c_void_p), ("cv_b", C.c_void_p),
        ("co_w", C.c_void_p), ("co_b", C.c_void_p),
        ("out", C.c_void_p), ("packed_used", C.POINTER(C.c_int)),
        ("q_elems", C.c_int64), ("kv_elems", C.c_int64), ("x_elems", C.c_int64), ("xa_elems", C.c_int64), ("out_elems", C.c_int64)]


class DecLnLinearDesc(C.Structure):
    """ccx_dec_ln_linear_desc (include/ccx.h): a LayerNorm -> linear pair of the > 16-row decode chain on its own."""
    _fields_ = [
        ("M", C.c_int), ("K", C.c_int), ("F", C.c_int), ("N", C.c_int), ("epi", C.c_int), ("packed", C.c_int),
        ("x", C.c_void_p), ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("eps", C.c_float),
        ("w1_host", C.c_void_p), ("b1", C.c_void_p), ("w_host", C.c_void_p), ("bias", C.c_void_p),
        ("out", C.c_void_p), ("x_elems", C.c_int64), ("out_elems", C.c_int64)]


class DecLinearDesc(C.Structure):
    """ccx_dec_linear_desc (include/ccx.h): one launch of dec_linear_kernel on its own, every device buffer the caller's."""
    _fields_ = [
        ("act", C.c_int), ("epi", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("w_host", C.c_void_p), ("bias", C.c_void_p),
        ("x", C.c_void_p), ("pend", C.c_void_p), ("pend_n", C.c_int), ("pend_stride", C.c_int64), ("x_out", C.c_void_p),
        ("ln_g", C.c_void_p), ("ln_b", C.c_void_p), ("eps", C.c_float), ("ln_mean_out", C.c_void_p),
        ("act_rows", C.c_void_p), ("lda", C.c_int64),
        ("part_o", C.c_void_p), ("part_ml", C.c_void_p), ("nsplit", C.c_int),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("out_stride", C.c_int64),
        ("cache_k", C.c_void_p), ("cache_v", C.c_void_p), ("cache_T", C.c_int), ("n_seq", C.c_int),
        ("pos", C.POINTER(C.c_int)), ("row_seq", C.POINTER(C.c_int)),
        ("bias_elems", C.c_int64), ("x_elems", C.c_int64), ("pend_elems", C.c_int64), ("x_out_elems", C.c_int64),
        ("ln_elems", C.c_int64), ("ln_mean_out_elems", C.c_int64), ("act_elems", C.c_int64), ("part_o_elems", C.c_int64),
        ("part_ml_elems", C.c_int64), ("out_elems", C.c_int64), ("cache_elems", C.c_int64)]


DEC_ACT_LN, DEC_ACT_BF16, DEC_ACT_COMBINE = range(3)
DEC_EPI_PARTIAL, DEC_EPI_F32, DEC_EPI_SELF_QKV, DEC_EPI_GELU = range(4)


class DecodeSamplingOptions(C.Structure):
    """ccx_decode_sampling_options (include/ccx.h): top_k, top_p and min_p; the defaults are {0, 1.0, 0.0}."""
    _fields_ = [("top_k", C.c_int), ("top_p", C.c_float), ("min_p", C.c_float)]


class DecodeLogprobOptions(C.Structure):
    """ccx_decode_logprob_options (include/ccx.h): top_n in [0, LOGPROB_MAX_TOP]; a NULL pointer is off."""
    _fields_ = [("top_n", C.c_int)]


LOGPROB_MAX_TOP = 8     # CCX_LOGPROB_MAX_TOP


class DecSeqState(C.Structure):
    """ccx_dec_seq_state: the select kernel's per-sequence state."""
    _fields_ = [(n, C.c_int) for n in ("pos", "prompt_len", "n_gen", "done", "last_tok", "pen_tok", "last_ts_tok", "n_tokens")] + [
        ("sum_logprob", C.c_float), ("no_speech_prob", C.c_float)]


class DecSelectDesc(C.Structure):
    """ccx_dec_select_desc (include/ccx.h): one launch of the select kernel."""
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("n_vocab", C.c_int), ("B", C.c_int),
        ("rules", C.POINTER(DecodeRules)), ("state", C.POINTER(DecSeqState)),
        ("prompt", C.POINTER(C.c_int)), ("max_prompt", C.c_int), ("sample_len", C.c_int),
        ("gen", C.POINTER(C.c_int)), ("cur_tok", C.POINTER(C.c_int)), ("pos", C.POINTER(C.c_int)), ("n_done", C.POINTER(C.c_int)),
        ("tok_emb", C.c_void_p), ("pos_emb", C.c_void_p), ("x", C.c_void_p), ("D", C.c_int),
        ("sample", C.c_int), ("temperature", C.c_float), ("seed", C.c_uint64), ("row0", C.c_int),
        ("logits_elems", C.c_int64), ("tok_emb_elems", C.c_int64), ("pos_emb_elems", C.c_int64), ("x_elems", C.c_int64),
        ("stream_ids", C.POINTER(C.c_int)), ("opts", C.POINTER(DecodeOptions)),
        ("sampling", C.POINTER(DecodeSamplingOptions)), ("cut_out", C.POINTER(C.c_float)), ("kept_out", C.POINTER(C.c_int)),
        ("kept_mass_out", C.POINTER(C.c_float)),
        ("logprobs", C.POINTER(DecodeLogprobOptions)), ("tok_logprob_out", C.POINTER(C.c_float)),
        ("top_id_out", C.POINTER(C.c_int)), ("top_lp_out", C.POINTER(C.c_float))]


class DecBeamDesc(C.Structure):
    """ccx_dec_beam_desc (include/ccx.h): one beam-search step (top-k kernel + update kernel) on its own."""
    _fields_ = [
        ("logits", C.c_void_p), ("ld", C.c_int64), ("n_vocab", C.c_int),
        ("G", C.c_int), ("beam_size", C.c_int), ("max_candidates", C.c_int),
        ("rules", C.POINTER(DecodeRules)), ("state", C.POINTER(DecSeqState)), ("sample_len", C.c_int),
        ("hist", C.POINTER(C.c_int)), ("cur_tok", C.POINTER(C.c_int)), ("pos", C.POINTER(C.c_int)), ("n_done", C.POINTER(C.c_int)),
        ("tok_emb", C.c_void_p), ("pos_emb", C.c_void_p), ("x", C.c_void_p), ("D", C.c_int),
        ("ind", C.POINTER(C.c_uint16)), ("ind_ld", C.c_int),
        ("fin_tok", C.POINTER(C.c_int)), ("fin_score", C.POINTER(C.c_float)), ("fin_n", C.POINTER(C.c_int)),
        ("fin_count", C.POINTER(C.c_int)),
        ("cand_id", C.POINTER(C.c_int)), ("cand_lp", C.POINTER(C.c_float)), ("tok_out", C.POINTER(C.c_int)),
        ("parent_out", C.POINTER(C.c_int)),
        ("logits_elems", C.c_int64), ("tok_emb_elems", C.c_int64), ("pos_emb_elems", C.c_int64), ("x_elems", C.c_int64),
        ("opts", C.POINTER(DecodeOptions))]


class DecodeHistoryOptions(C.Structure):
    """ccx_decode_history_options (include/ccx.h): repetition_penalty and no_repeat_ngram_size; the defaults are {1.0, 0}."""
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int)]


class DecHistoryDesc(C.Structure):
    """ccx_dec_history_desc (include/ccx.h): one launch of the history kernel on its own."""
    _fields_ = [
        ("logits", C.c_void_p), ("logits_elems", C.c_int64), ("ld", C.c_int64), ("n_vocab", C.c_int), ("rows", C.c_int),
        ("state", C.POINTER(DecSeqState)), ("hist", C.POINTER(C.c_int)), ("sample_len", C.c_int), ("text_end", C.c_int),
        ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int)]


class DecodeBiasOptions(C.Structure):
    """ccx_decode_bias_options (include/ccx.h): a sequence-bias table as three HOST arrays; all zero: off."""
    _fields_ = [("n_entries", C.c_int), ("offsets", C.POINTER(C.c_int)), ("ids", C.POINTER(C.c_int)), ("bias", C.POINTER(C.c_float))]


class DecBiasDesc(C.Structure):
    """ccx_dec_bias_desc (include/ccx.h): one launch of the sequence-bias kernel on its own."""
    _fields_ = [
        ("logits", C.c_void_p), ("logits_elems", C.c_int64), ("ld", C.c_int64), ("n_vocab", C.c_int), ("rows", C.c_int),
        ("state", C.POINTER(DecSeqState)), ("hist", C.POINTER(C.c_int)), ("sample_len", C.c_int), ("text_end", C.c_int),
        ("table", DecodeBiasOptions)]


class BeamTrace(C.Structure):
    """ccx_beam_trace (include/ccx.h): host buffers a traced ccx_whisper_decode_beam fills."""
    _fields_ = [("n_steps", C.c_int), ("cand_id", C.POINTER(C.c_int32)), ("cand_lp", C.POINTER(C.c_float)),
                ("tok", C.POINTER(C.c_int32)), ("parent", C.POINTER(C.c_int32)), ("score", C.POINTER(C.c_float))]


class DecTokenProbsDesc(C.Structure):
    """ccx_dec_token_probs_desc (include/ccx.h): the ranged softmax over logit rows on its own."""
    _fields_ = [
        ("logits", C.c_void_p), ("logits_elems", C.c_int64), ("ld", C.c_int64), ("n_vocab", C.c_int), ("rows", C.c_int),
        ("lo", C.c_int), ("hi", C.c_int), ("pick", C.c_int),
        ("argmax", C.POINTER(C.c_int)), ("pick_prob", C.POINTER(C.c_float)),
        ("probs", C.c_void_p), ("probs_elems", C.c_int64)]


class DecPickProbsDesc(C.Structure):
    """ccx_dec_pick_probs_desc (include/ccx.h): the probability of one picked id per logit row on its own."""
    _fields_ = [
        ("logits", C.c_void_p), ("logits_elems", C.c_int64), ("ld", C.c_int64), ("rows", C.c_int), ("hi", C.c_int),
        ("picks", C.c_void_p), ("picks_elems", C.c_int64), ("pick_stride", C.c_int64),
        ("out", C.c_void_p), ("out_elems", C.c_int64), ("out_stride", C.c_int64)]


class SepDesc(C.Structure):
    """ccx_sep_desc (include/ccx.h): one SepFormer layer kernel on its own."""
    _fields_ = (
        [(n, C.c_void_p) for n in ("h", "xin", "y", "qkv", "att", "feats", "fc")]
        + [(n, C.c_int64) for n in ("h_elems", "xin_elems", "y_elems", "qkv_elems", "att_elems", "feats_elems", "fc_elems")]
        + [("rows", C.c_int), ("seq_start", C.POINTER(C.c_int)), ("seq_len", C.POINTER(C.c_int)), ("n_seq", C.c_int),
           ("n_tok", C.c_int), ("d_ffn", C.c_int)]
        + [(n, C.c_void_p) for n in ("ln_g", "ln_b", "gln_g", "gln_b", "wqkv", "bqkv", "wo", "bo", "w1", "b1", "w2", "b2", "wdec")]
        + [(n, C.c_int64) for n in ("ln_elems", "gln_elems", "wqkv_elems", "bqkv_elems", "wo_elems", "bo_elems", "w1_elems",
                                    "b1_elems", "w2_elems", "b2_elems", "wdec_elems")]
        + [("utt_tok0", C.POINTER(C.c_int)), ("utt_L", C.POINTER(C.c_int)), ("utt_T", C.POINTER(C.c_int)), ("n_utt", C.c_int),
           ("segment", C.c_int), ("out", C.c_void_p), ("out_stride", C.c_int64), ("out_elems", C.c_int64), ("n_spk", C.c_int)])


SEP_ATTN_BLOCK, SEP_ATTENTION, SEP_FFN, SEP_FINAL_NORM, SEP_DECODER = range(5)


class DualPathDims(C.Structure):
    """ccx_dualpath_dims (include/ccx.h)."""
    _fields_ = [(n, C.c_int) for n in (
        "n_filters", "kernel", "stride", "d_model", "n_head", "d_ffn", "n_layers", "n_blocks", "segment", "n_spk")]


class DualPathDesc(C.Structure):
    """ccx_dualpath_desc (include/ccx.h): one dual-path SepFormer kernel on its own."""
    _fields_ = (
        [(n, C.c_void_p) for n in ("in", "in2", "out", "w", "w2")]
        + [(n, C.c_int64) for n in ("in_elems", "in2_elems", "out_elems", "w_elems", "w2_elems")]
        + [("rows", C.c_int), ("frames", C.c_int), ("mode", C.c_int)]
        + [("seq_first", C.POINTER(C.c_int)), ("seq_stride", C.POINTER(C.c_int)), ("seq_len", C.POINTER(C.c_int)), ("n_seq", C.c_int)]
        + [("utt_row0", C.POINTER(C.c_int)), ("utt_rows", C.POINTER(C.c_int))]
        + [(n, C.POINTER(C.c_int)) for n in ("utt_tok0", "utt_frame0", "utt_L", "utt_gap", "utt_S", "utt_T")]
        + [("n_utt", C.c_int), ("segment", C.c_int), ("kernel", C.c_int), ("n_spk", C.c_int),
           ("in_stride", C.c_int64), ("out_stride", C.c_int64)])


(DP_ATTENTION, DP_GROUP_NORM, DP_SEGMENT, DP_OVERLAP_ADD, DP_PE_ADD, DP_GATE, DP_ENCODER, DP_DECODER, DP_PRELU) = range(9)


class EcapaDesc(C.Structure):
    """ccx_ecapa_desc (include/ccx.h): one ECAPA-TDNN kernel on its own."""
    _fields_ = [
        ("n", C.c_int), ("row_off", C.POINTER(C.c_int)), ("frames", C.POINTER(C.c_int)), ("rows", C.c_int),
        ("wav", C.c_void_p), ("wav_elems", C.c_int64), ("offsets", C.POINTER(C.c_int64)), ("n_samples", C.POINTER(C.c_int)),
        ("window", C.c_void_p), ("window_elems", C.c_int64), ("filters", C.c_void_p), ("filters_elems", C.c_int64),
        ("feats", C.c_void_p), ("feats_elems", C.c_int64),
        ("x", C.c_void_p), ("x_elems", C.c_int64), ("ldx", C.c_int64), ("y", C.c_void_p), ("y_elems", C.c_int64), ("ldy", C.c_int64),
        ("dilation", C.c_int), ("w_host", C.POINTER(C.c_float)), ("aff_host", C.POINTER(C.c_float)),
        ("resid", C.c_void_p), ("resid_elems", C.c_int64), ("ld_resid", C.c_int64),
        ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
        ("w1_elems", C.c_int64), ("b1_elems", C.c_int64), ("w2_elems", C.c_int64), ("b2_elems", C.c_int64),
        ("gates", C.c_void_p), ("gates_elems", C.c_int64),
        ("channels", C.c_int), ("hidden", C.c_void_p), ("hidden_elems", C.c_int64),
        ("wa", C.c_void_p), ("ba", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p),
        ("wa_elems", C.c_int64), ("ba_elems", C.c_int64), ("bn_elems", C.c_int64),
        ("pooled", C.c_void_p), ("pooled_elems", C.c_int64)]


ECAPA_FBANK, ECAPA_RES2NET, ECAPA_SE, ECAPA_ASP_POOL = range(4)
ECAPA_R2_TILE = 128              # csrc/ecapa.h ECAPA_R2_TILE: output frames of one Res2Net block
ECAPA_MIN_SAMPLES = 8000         # csrc/ecapa.h ECAPA_MIN_SAMPLES


class ResnetDesc(C.Structure):
    """ccx_resnet_desc (include/ccx.h): one ResNet-34 kernel on its own."""
    _fields_ = [
        ("n_chunks", C.c_int),
        ("wav", C.c_void_p), ("wav_elems", C.c_int64), ("stride", C.c_int64), ("n_samples", C.c_int),
        ("feats_t", C.c_void_p), ("feats_t_elems", C.c_int64), ("fmean", C.c_void_p), ("fmean_elems", C.c_int64),
        ("T", C.c_int), ("c1w", C.c_void_p), ("c1w_elems", C.c_int64), ("c1b", C.c_void_p), ("c1b_elems", C.c_int64),
        ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int), ("conv_stride", C.c_int), ("H", C.c_int), ("W", C.c_int), ("epi", C.c_int),
        ("w_host", C.POINTER(C.c_float)), ("scale_host", C.POINTER(C.c_float)), ("shift_host", C.POINTER(C.c_float)),
        ("in_", C.c_void_p), ("in_elems", C.c_int64), ("out", C.c_void_p), ("out_elems", C.c_int64),
        ("resid", C.c_void_p), ("resid_elems", C.c_int64),
        ("halo0", C.c_void_p), ("halo1", C.c_void_p), ("halo2", C.c_void_p), ("halo0_elems", C.c_int64),
        ("c0", C.c_int), ("n", C.c_int), ("Wp", C.c_int), ("C", C.c_int),
        ("act", C.c_void_p), ("act_elems", C.c_int64), ("W4", C.c_int),
        ("weights", C.c_void_p), ("weights_elems", C.c_int64), ("n_w", C.c_int), ("mask_chunk", C.POINTER(C.c_int)), ("n_masks", C.c_int),
        ("pooled", C.c_void_p), ("pooled_elems", C.c_int64),
        ("lin_w", C.c_void_p), ("lin_w_elems", C.c_int64), ("lin_b", C.c_void_p), ("lin_b_elems", C.c_int64),
        ("emb", C.c_void_p), ("emb_elems", C.c_int64)]


RESNET_FBANK, RESNET_CONV1, RESNET_CONV, RESNET_HALO_ZERO, RESNET_TSTP, RESNET_LINEAR = range(6)
RESNET_EPI_PLAIN, RESNET_EPI_RELU, RESNET_EPI_ADD_RELU = range(3)


class SpeakerDesc(C.Structure):
    """ccx_speaker_desc (include/ccx.h): one SincNet / x-vector / PyanNet kernel on its own."""
    _fields_ = [
        ("n", C.c_int),
        ("wav", C.c_void_p), ("wav_elems", C.c_int64), ("crop_off", C.POINTER(C.c_int64)), ("crop_len", C.POINTER(C.c_int)),
        ("norm_w", C.c_float), ("norm_b", C.c_float),
        ("filters_host", C.POINTER(C.c_float)),
        ("frames", C.POINTER(C.c_int)),
        ("in_", C.c_void_p), ("in_elems", C.c_int64), ("ld_in", C.c_int64), ("in_off", C.POINTER(C.c_int)),
        ("out", C.c_void_p), ("out_elems", C.c_int64), ("ld_out", C.c_int64), ("out_off", C.POINTER(C.c_int)),
        ("pool", C.c_int), ("C", C.c_int), ("gamma", C.c_void_p), ("gamma_elems", C.c_int64), ("beta", C.c_void_p), ("beta_elems", C.c_int64),
        ("weights", C.c_void_p), ("weights_elems", C.c_int64), ("w_off", C.POINTER(C.c_int64)), ("w_len", C.POINTER(C.c_int)),
        ("whh_host", C.POINTER(C.c_float)),
        ("rows", C.c_int), ("powerset", C.c_int)]


SPEAKER_WAV_STATS, SPEAKER_SINC_POOL, SPEAKER_INORM, SPEAKER_STATS_POOL, SPEAKER_LSTM, SPEAKER_ACTIVATION = range(6)


class AlignDesc(C.Structure):
    """ccx_align_desc (include/ccx.h): one word-alignment kernel on its own."""
    _fields_ = [
        ("q", C.c_void_p), ("k", C.c_void_p), ("q_elems", C.c_int64), ("k_elems", C.c_int64),
        ("n_seq", C.c_int), ("H", C.c_int), ("Spad", C.c_int),
        ("heads", C.POINTER(C.c_int)), ("n_heads", C.c_int), ("head0", C.c_int), ("t", C.c_int),
        ("Hsel", C.c_int), ("T", C.c_int), ("Mmax", C.c_int),
        ("n_keys", C.POINTER(C.c_int)), ("n_rows", C.POINTER(C.c_int)), ("r0", C.c_int),
        ("P", C.c_void_p), ("A", C.c_void_p), ("P_elems", C.c_int64), ("A_elems", C.c_int64),
        ("text_idx", C.c_void_p), ("time_idx", C.c_void_p), ("path_len", C.c_void_p), ("jump_frame", C.c_void_p),
        ("text_idx_elems", C.c_int64), ("time_idx_elems", C.c_int64), ("path_len_elems", C.c_int64), ("jump_frame_elems", C.c_int64)]


ALIGN_SCORES, ALIGN_MATRIX, ALIGN_DTW = range(3)


class SpecgateOpts(C.Structure):
    """ccx_specgate_opts (include/ccx.h): mode, tunables and noise clip of one spectral-gate call; ccx_specgate_opts_default fills
    upstream's defaults."""
    _fields_ = [
        ("stationary", C.c_int), ("prop_decrease", C.c_float), ("n_std_thresh", C.c_float), ("time_constant_s", C.c_float),
        ("thresh_n_mult", C.c_float), ("sigmoid_slope", C.c_float),
        ("noise_dev", C.c_void_p), ("noise_stride", C.c_int64), ("n_noise", C.POINTER(C.c_int)), ("noise_rows", C.c_int)]


_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
_ip = C.POINTER(C.c_int)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes); every symbol declared in include/ccx.h
PROTOTYPES = {
    "ccx_version": (C.c_char_p, []),
    "ccx_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "ccx_ctx_destroy": (None, [_vp]),
    "ccx_last_error": (C.c_char_p, [_vp]),
    "ccx_prof_enable": (_i, [_vp, _i]),
    "ccx_prof_count": (_i, [_vp]),
    "ccx_prof_get": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _fp]),
    "ccx_gemm_bf16": (_i, [_vp, _i, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _vp]),
    "ccx_gemm_bf16_desc": (_i, [_vp, _i, C.POINTER(GemmDesc), _vp]),
    "ccx_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "ccx_gather_rows": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i64, _vp]),
    "ccx_peak_normalize": (_i, [_vp, _vp, _vp, _i64, _vp, _i, _f, _vp]),
    "ccx_row_variance": (_i, [_vp, _vp, _i64, _vp, _i, _vp, _vp]),
    "ccx_cross_attention_xa": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ccx_cross_attention_xa_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "ccx_cross_attention_xa_keys": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "ccx_cross_attention_xa_fp8_keys": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ccx_cosine_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ccx_speaker_profiles": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ccx_resample_sinc": (_i, [_vp, _vp, _i64, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i, _vp]),
    "ccx_enc_attention": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "ccx_enc_attention_keys": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "ccx_whisper_create": (_i, [_vp, C.POINTER(WhisperDims), _i, C.POINTER(_vp)]),
    "ccx_whisper_destroy": (None, [_vp]),
    "ccx_whisper_set_tensor": (_i, [_vp, C.c_char_p, _vp, _i, _i, _i64p]),
    "ccx_whisper_set_max_audio": (_i, [_vp, C.c_double]),
    "ccx_whisper_set_cross_fp8": (_i, [_vp, _i]),
    "ccx_whisper_cross_fp8": (_i, [_vp]),
    "ccx_whisper_set_audio_ctx": (_i, [_vp, _i]),
    "ccx_whisper_audio_ctx": (_i, [_vp]),
    "ccx_whisper_share_encoder_scratch": (_i, [_vp, _vp]),
    "ccx_whisper_finalize": (_i, [_vp]),
    "ccx_whisper_set_rules": (_i, [_vp, C.POINTER(DecodeRules)]),
    "ccx_whisper_logmel": (_i, [_vp, _vp, _i64, _ip, _ip, _i, _vp, _vp]),
    "ccx_whisper_logmel_ex": (_i, [_vp, _vp, _i64, _ip, _ip, _ip, _i, _vp, _vp]),
    "ccx_decode_options_default": (None, [C.POINTER(DecodeOptions)]),
    "ccx_whisper_set_decode_options": (_i, [_vp, C.POINTER(DecodeOptions)]),
    "ccx_whisper_graph_count": (_i, [_vp, _i]),
    "ccx_decode_history_options_default": (None, [C.POINTER(DecodeHistoryOptions)]),
    "ccx_whisper_set_history_options": (_i, [_vp, C.POINTER(DecodeHistoryOptions)]),
    "ccx_whisper_history_graph_count": (_i, [_vp]),
    "ccx_dec_history_step": (_i, [_vp, C.POINTER(DecHistoryDesc), _vp]),
    "ccx_decode_bias_options_default": (None, [C.POINTER(DecodeBiasOptions)]),
    "ccx_whisper_set_bias_options": (_i, [_vp, C.POINTER(DecodeBiasOptions)]),
    "ccx_whisper_bias_graph_count": (_i, [_vp]),
    "ccx_dec_bias_step": (_i, [_vp, C.POINTER(DecBiasDesc), _vp]),
    "ccx_decode_sampling_options_default": (None, [C.POINTER(DecodeSamplingOptions)]),
    "ccx_whisper_set_sampling_options": (_i, [_vp, C.POINTER(DecodeSamplingOptions)]),
    "ccx_whisper_sampling_graph_count": (_i, [_vp]),
    "ccx_whisper_set_token_logprobs": (_i, [_vp, _i]),
    "ccx_whisper_set_logprob_options": (_i, [_vp, C.POINTER(DecodeLogprobOptions)]),
    "ccx_whisper_token_logprobs": (_i, [_vp, _i, _i, C.POINTER(C.c_float), _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _vp]),
    "ccx_whisper_logprob_graph_count": (_i, [_vp]),
    "ccx_whisper_set_mel": (_i, [_vp, _vp, _i, _vp]),
    "ccx_whisper_encode": (_i, [_vp, _i, _vp, _vp]),
    "ccx_whisper_encode_ctx": (_i, [_vp, _i, _vp, _vp, _vp]),
    "ccx_whisper_decoder_logits": (_i, [_vp, _i32p, _i, _i, _vp, _vp]),
    "ccx_whisper_decode_greedy": (_i, [_vp, _i32p, _i32p, _i, _i, _i, _i32p, _i32p, _fp, _fp, _vp]),
    "ccx_dec_attention_desc": (_i, [_vp, _i, C.POINTER(DecAttnDesc), _vp]),
    "ccx_dec_ln_linear": (_i, [_vp, C.POINTER(DecLnLinearDesc), _vp]),
    "ccx_dec_linear_op": (_i, [_vp, C.POINTER(DecLinearDesc), _vp]),
    "ccx_dec_mid_chain_out_elems": (_i64, [_i, _i, _i]),
    "ccx_dec_mid_chain": (_i, [_vp, C.POINTER(DecMidChainDesc), _vp]),
    "ccx_dec_select_step": (_i, [_vp, C.POINTER(DecSelectDesc), _vp]),
    "ccx_dec_beam_step": (_i, [_vp, C.POINTER(DecBeamDesc), _vp]),
    "ccx_whisper_decode_beam": (_i, [_vp, _i32p, _i32p, _i, _i, _i32p, _i, _i, _i, _i, _i32p, _i32p, _fp, _i32p, _fp,
                                     C.POINTER(BeamTrace), _vp]),
    "ccx_dec_token_probs": (_i, [_vp, C.POINTER(DecTokenProbsDesc), _vp]),
    "ccx_dec_pick_probs": (_i, [_vp, C.POINTER(DecPickProbsDesc), _vp]),
    "ccx_align_op": (_i, [_vp, _i, C.POINTER(AlignDesc), _vp]),
    "ccx_whisper_align": (_i, [_vp, _i32p, _i32p, _i, _i, _i32p, _i32p, _i, _i, _vp, _vp, _i32p, _vp]),
    "ccx_whisper_align_probs": (_i, [_vp, _i32p, _i32p, _i, _i, _i32p, _i32p, _i, _i, _vp, _vp, _i32p, _i, _fp, _vp]),
    "ccx_whisper_last_cross_path": (_i, [_vp]),
    "ccx_whisper_set_sot_tail": (_i, [_vp, _i]),
    "ccx_whisper_set_prefix_len": (_i, [_vp, _i]),
    "ccx_whisper_detect_language": (_i, [_vp, _i, _i, _i, _i32p, _fp, _vp]),
    "ccx_whisper_prepare_lanes": (_i, [_vp, _vp]),
    "ccx_whisper_trace_lanes": (_i, [_vp, C.c_char_p, _i]),
    "ccx_whisper_decode": (_i, [_vp, _i32p, _i32p, _i, _i, _i, _f, C.c_uint64, _i32p, _i32p, _fp, _fp, _vp]),
    "ccx_whisper_decode_rows": (_i, [_vp, _i32p, _i32p, _i, _i, _i32p, _i, _i32p, _i, _f, C.c_uint64, _i32p, _i32p, _fp, _fp, _vp]),
    "ccx_sepformer_create": (_i, [_vp, C.POINTER(SepformerDims), _i, _i, C.POINTER(_vp)]),
    "ccx_sepformer_destroy": (None, [_vp]),
    "ccx_sepformer_set_tensor": (_i, [_vp, C.c_char_p, _vp, _i64]),
    "ccx_sepformer_finalize": (_i, [_vp]),
    "ccx_sepformer_separate": (_i, [_vp, _vp, _i64, _ip, _i, _vp, _vp]),
    "ccx_sep_op": (_i, [_vp, _i, C.POINTER(SepDesc), _vp]),
    "ccx_dualpath_create": (_i, [_vp, C.POINTER(DualPathDims), _i, _i, C.POINTER(_vp)]),
    "ccx_dualpath_destroy": (None, [_vp]),
    "ccx_dualpath_set_tensor": (_i, [_vp, C.c_char_p, _vp, _i64]),
    "ccx_dualpath_finalize": (_i, [_vp]),
    "ccx_dualpath_separate": (_i, [_vp, _vp, _i64, _ip, _i, _vp, _vp]),
    "ccx_dualpath_op": (_i, [_vp, _i, C.POINTER(DualPathDesc), _vp]),
    "ccx_speaker_create": (_i, [_vp, _i, _i, _i, _i, _i64, C.POINTER(_vp)]),
    "ccx_speaker_destroy": (None, [_vp]),
    "ccx_speaker_set_tensor": (_i, [_vp, C.c_char_p, _vp, _i64]),
    "ccx_speaker_finalize": (_i, [_vp]),
    "ccx_speaker_embed": (_i, [_vp, _vp, _i64p, _ip, _i, _vp, _i64p, _ip, _vp, _vp]),
    "ccx_speaker_segment": (_i, [_vp, _vp, _i64p, _ip, _i, _vp, _i64, _ip, _vp]),
    "ccx_speaker_op": (_i, [_vp, _i, C.POINTER(SpeakerDesc), _vp]),
    "ccx_ecapa_create": (_i, [_vp, _i, _i64, C.POINTER(_vp)]),
    "ccx_ecapa_destroy": (None, [_vp]),
    "ccx_ecapa_set_tensor": (_i, [_vp, C.c_char_p, _vp, _i64]),
    "ccx_ecapa_finalize": (_i, [_vp]),
    "ccx_ecapa_embed": (_i, [_vp, _vp, _i64p, _ip, _i, _vp, _vp]),
    "ccx_ecapa_op": (_i, [_vp, _i, C.POINTER(EcapaDesc), _vp]),
    "ccx_resnet_create": (_i, [_vp, _i, _i64, _i, C.POINTER(_vp)]),
    "ccx_resnet_destroy": (None, [_vp]),
    "ccx_resnet_set_tensor": (_i, [_vp, C.c_char_p, _vp, _i64]),
    "ccx_resnet_finalize": (_i, [_vp]),
    "ccx_resnet_embed": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i, _ip, _i, _vp, _vp]),
    "ccx_resnet_op": (_i, [_vp, _i, C.POINTER(ResnetDesc), _vp]),
    "ccx_specgate_create": (_i, [_vp, _i64, _i, _i, C.POINTER(_vp)]),
    "ccx_specgate_destroy": (None, [_vp]),
    "ccx_specgate_reduce": (_i, [_vp, _vp, _i64, _ip, _i, _f, _vp, _vp]),
    "ccx_specgate_reduce_long": (_i, [_vp, _vp, _i64, _f, _vp, _vp]),
    "ccx_specgate_set_clip_noise": (_i, [_vp, _i]),
    "ccx_specgate_opts_default": (None, [C.POINTER(SpecgateOpts)]),
    "ccx_specgate_reduce_ex": (_i, [_vp, C.POINTER(SpecgateOpts), _vp, _i64, _ip, _i, _vp, _vp]),
    "ccx_specgate_reduce_long_ex": (_i, [_vp, C.POINTER(SpecgateOpts), _vp, _i64, _vp, _vp]),
    "ccx_specgate_time_smooth": (_i, [_vp, _vp, _vp, _ip, _i, _i64, _f, _vp]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen libccx.so and bind every prototype.  Raises CcxError when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise CcxError(f"{LIB_PATH} is missing: run `python -m clearconverse_amd.build` "
                       "(there is no CPU fallback for the HIP path)")
    # torch first: libccx.so needs libamdhip64, and the process must end up with ONE HIP runtime.  PyTorch's ROCm wheels carry
    # their own copy; if libccx were loaded before torch, it would bind /opt/rocm's copy and torch would later load a second
    # runtime -- ccx_ctx_create then reports "no ROCm-capable device" (seen with build() and smoke() in one process).
    import torch  # noqa: F401
    try:
        lib = C.CDLL(str(LIB_PATH))
    except OSError as e:
        raise CcxError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise CcxError(f"libccx.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class Context:
    """One ccx_ctx per process/device (created after fork, reference back/api.py:2045-2049)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = _vp()
        rc = self.lib.ccx_ctx_create(device, C.byref(h))
        if rc != 0:
            raise CcxError(f"ccx_ctx_create({device}) failed: {self.lib.ccx_last_error(None).decode()}")
        self.handle = h
        self.device = device

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            raise CcxError(f"{what or 'ccx call'} failed ({rc}): {self.lib.ccx_last_error(self.handle).decode()}")

    prof_on = False

    def prof_enable(self, on: bool = True):
        self.check(self.lib.ccx_prof_enable(self.handle, 1 if on else 0), "ccx_prof_enable")
        self.prof_on = bool(on)

    def prof_records(self):
        """[(kernel name, algorithmic flops, algorithmic bytes, ms)] for every recorded launch."""
        out = []
        buf = C.create_string_buffer(64)
        fl, by, ms = C.c_double(), C.c_double(), C.c_float()
        for i in range(self.lib.ccx_prof_count(self.handle)):
            self.check(self.lib.ccx_prof_get(self.handle, i, buf, 64, C.byref(fl), C.byref(by), C.byref(ms)), "ccx_prof_get")
            out.append((buf.value.decode(), fl.value, by.value, ms.value))
        return out

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ccx_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def current_stream_ptr() -> int:
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def ptr(t) -> int:
    """Device (or host) address of a contiguous torch tensor; None -> NULL."""
    if t is None:
        return 0
    if not t.is_contiguous():
        raise CcxError("tensor passed to libccx must be contiguous")
    return int(t.data_ptr())

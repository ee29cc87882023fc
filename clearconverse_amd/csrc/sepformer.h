// sepformer.h -- launchers of the SepFormer layer kernels (sepformer.hip): the model handle (run_block, ccx_sepformer_separate) and
// the stand-alone operators of sep_ops.hip launch through these, so a kernel parity test runs the product's grid rule, LDS opt-in
// and profile label.  All pointers are device pointers; nothing is checked here (the handle builds its tables itself, sep_ops.hip
// checks a caller's on the host).
#pragma once
#include "../../include/ccx.h"
#include "ccx_common.h"

constexpr int CCX_SEP_FUSED_MAX_TOK = 160;   // longest sequence of sep_attn_block_kernel (ten 16-token tiles resident in registers)

// h [rows][128] f32 in place: h += out_proj(attention(LayerNorm(h) Wqkv^T + bqkv)) + bo for every sequence (start, len <= 160).
// n_tok / max_len only size the profile record.
int ccx_launch_sep_attn_block(ccx_ctx* ctx, float* h, const float* ln_g, const float* ln_b, const bf16_t* Wqkv, const float* bqkv,
                              const bf16_t* Wo, const float* bo, const int* seq_start, const int* seq_len, int n_seq, int n_tok,
                              int max_len, hipStream_t st);
// qkv [rows][384] bf16 (q | k | v) -> out [rows][128] bf16, sequences of any length; n_head a multiple of 4 (one block per four heads)
int ccx_launch_sep_attention(ccx_ctx* ctx, const bf16_t* qkv, const int* seq_start, const int* seq_len, int n_seq, int n_head,
                             bf16_t* out, hipStream_t st);
// h [n_tok][128] f32 in place: h += W2 relu(W1 LayerNorm(h) + b1) + b2.  W1 [d_ffn][128], W2 [128][d_ffn] bf16; d_ffn a multiple of
// 64 in [64, 1024].  Owns the kernel's LDS opt-in.
int ccx_launch_sep_ffn(ccx_ctx* ctx, float* h, const float* ln_g, const float* ln_b, const bf16_t* W1, const float* b1,
                       const bf16_t* W2, const float* b2, int n_tok, int d_ffn, hipStream_t st);
// y = gLN(LayerNorm(h)) + xin per sequence (statistics over len x 128)
int ccx_launch_sep_final_norm(ccx_ctx* ctx, const float* h, const float* xin, const int* seq_start, const int* seq_len, int n_seq,
                              const float* ln_g, const float* ln_b, const float* gln_g, const float* gln_b, float* y, hipStream_t st);
// out [n_utt][out_stride][n_spk] f32 from fc [rows][128 n_spk] (channel-major, source-minor): mask * features, transposed
// convolution, trimmed / zero-padded to utt_T.  n_spk in [1, 4] (one instantiation each; anything else is CCX_ERR_ARG); out needs
// no more than float alignment
int ccx_launch_sep_decoder(ccx_ctx* ctx, const float* feats, const float* fc, const int* utt_tok0, const int* utt_L, const int* utt_T,
                           const float* wdec, float* out, long out_stride, int n_utt, int n_spk, hipStream_t st);

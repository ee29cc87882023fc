// dualpath.h -- launchers of the dual-path SepFormer kernels (dualpath.hip): the model handle (ccx_dualpath_separate) and the
// stand-alone operators (ccx_dualpath_op) launch through these, so a kernel parity test runs the product's grid rule and profile
// label.  All pointers are device pointers; nothing is checked here (the handle builds its tables itself, ccx_dualpath_op checks a
// caller's on the host).  Every token / frame buffer is [rows][256]: d_model = n_filters = 256, 8 heads of 32.
#pragma once
#include "../../include/ccx.h"
#include "ccx_common.h"

constexpr int CCX_DP_D = 256;           // n_filters == d_model
constexpr int CCX_DP_KEY_BLOCK = 64;    // dp_attention_kernel: online softmax over blocks of four 16-key tiles
constexpr int CCX_DP_GN_PARTS = 32;     // dp_gn_*: partial sums per utterance (fixed order, no atomics)

// one utterance of a call: its first token row, first frame row, frames L, zero frames `gap` behind them, chunks S, samples T
struct ccx_dp_utt { int tok0, frame0, L, gap, S, T, pad0, pad1; };

// qkv [rows][768] bf16 (q | k | v, heads contiguous inside each 256) -> out [rows][256] bf16.  seq [n_seq][3]: first row, row
// stride, length >= 1; non-causal, any length (max_len sizes the grid)
int ccx_launch_dp_attention(ccx_ctx* ctx, const bf16_t* qkv, const int* seq, int n_seq, int max_len, bf16_t* out, hipStream_t st);
// GroupNorm(1, 256, eps 1e-8) per utterance over rows [tab[u][0], + tab[u][1]) of x f32, two passes; part: 2 * n_utt * CCX_DP_GN_PARTS
// floats of scratch.  out_f32 = gamma (x - mean) rstd + beta + skip (skip may be out_f32 itself), or out_bf16 without a skip
int ccx_launch_dp_group_norm(ccx_ctx* ctx, const float* x, const int* tab, int n_utt, int max_rows, const float* gamma, const float* beta,
                             const float* skip, float* out_f32, bf16_t* out_bf16, float* part, hipStream_t st);
// tok [tok0 + s K + k][:] = frames[frame0 + s K/2 + k - K/2][:] where that frame exists, zero elsewhere; every row of every chunk is written
int ccx_launch_dp_segment(ccx_ctx* ctx, const float* frames, const ccx_dp_utt* utt, int n_utt, int K, int max_S, float* tok, hipStream_t st);
// out [(frame0 + l) n_spk + s][:] bf16 = the two chunk entries of frame l in columns 256 s .. of fc [rows][256 n_spk] f32, summed
int ccx_launch_dp_overlap_add(ccx_ctx* ctx, const float* fc, const ccx_dp_utt* utt, int n_utt, int K, int max_L, int n_spk, bf16_t* out,
                              hipStream_t st);
// out = x + pe[axis == 0 ? position in the chunk : chunk index][:]
int ccx_launch_dp_pe_add(ccx_ctx* ctx, const float* x, const ccx_dp_utt* utt, int n_utt, int K, int max_S, int axis, const float* pe,
                         float* out, hipStream_t st);
// out bf16 [rows][256] = tanh(g[r][c]) * sigmoid(g[r][256 + c]) from g f32 [rows][512]
int ccx_launch_dp_gate(ccx_ctx* ctx, const float* g, bf16_t* out, long rows, hipStream_t st);
// frames [frame0 + l][c] = relu(sum_k w[c][k] mix[u][stride l + k]), stride = kernel / 2, l < L
int ccx_launch_dp_encoder(ccx_ctx* ctx, const float* mix, long mix_stride, const ccx_dp_utt* utt, int n_utt, int max_L, int kernel,
                          const float* w, float* frames, hipStream_t st);
// out [u][t][s] = sum_l sum_c feats[l][c] relu(mask[l n_spk + s][c]) wdec[c][t - stride l], zero from T on; n_spk in [1, 3]
int ccx_launch_dp_decoder(ccx_ctx* ctx, const float* feats, const float* mask, const ccx_dp_utt* utt, int n_utt, int kernel, int n_spk,
                          const float* wdec, float* out, long out_stride, hipStream_t st);

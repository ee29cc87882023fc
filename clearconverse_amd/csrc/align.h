// align.h -- parameter blocks and launchers of the word-alignment kernels (align.hip): cross-attention probabilities of the alignment
// heads, their normalisation into the DTW cost source, and the dynamic-time-warping pass [UPSTREAM-RECALL: whisper/timing.py
// find_alignment / median_filter / dtw].  Behind transcribe(word_timestamps=True) of the reference (back/api.py:1435, 1477).
#pragma once
#include "ccx_common.h"

#define CCX_ALIGN_MAX_HEADS 96     // selected heads: the matrix kernel keeps (mean, std) of every head's 70 columns in 54 KB of LDS
#define CCX_ALIGN_MAX_TOK 448      // token rows (n_text_ctx): the DTW block has one thread per text row
#define CCX_ALIGN_MAX_FRAMES 1500  // encoder positions (n_audio_ctx): the scores block keeps one row of scores in LDS

// P[seq][hsel[i]][t][0 .. n_keys[seq]) = softmax_j(q[seq][heads[i]] . k[seq][heads[i]][j] / 8) for i < n_heads; columns [n_keys, Mmax)
// are written as 0.  Keys at and behind n_keys[seq] are never read.
struct AlignScoresParams {
  const float* q;        // [n_seq][H][64] f32
  const bf16_t* k;       // [n_seq][H][Spad][64] bf16 (project_cross_kv's crossK)
  int H, Spad;
  const int* heads;      // device [n_heads]: head of k / q
  const int* hsel;       // device [n_heads]: its index among the Hsel heads of P
  int n_heads;
  const int* n_keys;     // device [n_seq], 1 .. min(Mmax, Spad)
  float* P;              // [n_seq][Hsel][T][Mmax] f32
  int Hsel, T, Mmax, t;
};
int ccx_launch_align_scores(ccx_ctx* ctx, const AlignScoresParams& p, int n_seq, hipStream_t stream);

// A[seq][t][j] = mean_h median7_j((P[seq][h][t][j] - mean_t) / std_t) for t < n_rows[seq], j < n_keys[seq]: population statistics over
// all n_rows token rows, the median over frames with reflect padding 3 (unfiltered when n_keys <= 3).
struct AlignMatrixParams {
  const float* P; float* A;   // [n_seq][Hsel][T][Mmax], [n_seq][T][Mmax]
  int Hsel, T, Mmax;
  const int* n_rows;     // device [n_seq], 2 .. T
  const int* n_keys;     // device [n_seq], 1 .. Mmax
};
int ccx_launch_align_matrix(ccx_ctx* ctx, const AlignMatrixParams& p, int n_seq, hipStream_t stream);

// DTW over x = -A[seq][r0 : r1[seq]][: n_keys[seq]], one block per sequence.
struct AlignDtwParams {
  const float* A; int T, Mmax;
  int r0; const int* r1; // device [n_seq], r0 < r1 <= T
  const int* n_keys;     // device [n_seq]
  unsigned char* trace; long trace_stride;   // 8-bit cells [n_seq][trace_stride], trace_stride >= (N + 1) * (M + 1)
  int* text_idx; int* time_idx; int path_cap; // [n_seq][path_cap], path_cap >= N + M
  int* path_len;         // [n_seq]
  int* jump_frame;       // [n_seq][T]: time index of the first path cell of text index i (i < N), -1 behind
};
int ccx_launch_align_dtw(ccx_ctx* ctx, const AlignDtwParams& p, int n_seq, hipStream_t stream);

// logmel.h -- launcher for the log-mel front end (see logmel.hip).
#pragma once
#include "ccx_common.h"

struct LogmelTables {
  const float* dft_cos;   // [400][208] cos(2*pi*n*k/400) * hann[n]
  const float* dft_sin;   // [400][208]
  const float* mel_fb;    // [n_mels][208]
  const int* mel_range;   // [n_mels][2]
  int n_mels;             // 80 or 128 (the kernels are instantiated for these two)
};

// row length of the conv1 im2col matrix: 3 taps x n_mels, padded to the GEMM's 128-element K granule (80 -> 256, 128 -> 384)
inline int ccx_logmel_kpad(int n_mels) { return (3 * n_mels + 127) / 128 * 128; }

// audio: [B][audio_stride] f32 device; n_samples_dev/seek_dev/seg_len_dev: [B] int device (seek and
// seg_len may be null = 0 / 3000).  Window frames t >= seg_len[b] are written as zeros.
// raw: [B][n_mels][Fraw] scratch of which frames [0, Fcomp) are computed (the rest is all-zero padding = -10), gmax_bits: [B] scratch.  mel_out [B][n_mels][3000] f32 and
// im2col [B*3000][ccx_logmel_kpad(n_mels)] bf16 are optional outputs.
int ccx_launch_logmel(ccx_ctx* ctx, const LogmelTables& tb, const float* audio, long audio_stride,
                      const int* n_samples_dev, const int* seek_dev, const int* seg_len_dev, int B, int Fraw, int Fcomp, float* raw,
                      unsigned int* gmax_bits, float* mel_out, bf16_t* im2col, hipStream_t stream);
// mel [B][n_mels][3000] f32 (a caller's own log-mel) -> the same im2col matrix
int ccx_launch_mel_to_im2col(ccx_ctx* ctx, int n_mels, const float* mel, int B, bf16_t* im2col, hipStream_t stream);

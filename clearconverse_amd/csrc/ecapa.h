// ecapa.h -- launchers of the ECAPA-TDNN kernels (csrc/ecapa.hip).  The product path (ccx_ecapa_embed) and the kernel-parity entry
// (ccx_ecapa_op) call the same functions.
//
// Row layout shared by every kernel: activations are bf16 [rows][C] row-major; crop i owns rows row_off[i] .. row_off[i] + T_i + 8:
// four halo rows, its T_i frames, four halo rows.  A halo holds the reflection x[-j] = x[j], x[T-1+j] = x[T-1-j] (j = 1..4), so
// T_i >= 5.  `row_off` / `frames` are DEVICE tables of n crops.
#pragma once
#include "ccx_common.h"

#define ECAPA_HALO 4
#define ECAPA_MIN_FRAMES 5
#define ECAPA_MIN_SAMPLES 8000      // the shortest crop the reference embeds (0.5 s, back/api.py:864)
#define ECAPA_NFFT 400
#define ECAPA_HOP 160
#define ECAPA_BINS 201
#define ECAPA_BINS_LD 208
#define ECAPA_MELS 80
#define ECAPA_PIECES 16             // pieces of a crop's time axis in the two-pass kernels
#define ECAPA_R2_TILE 128           // F: output frames of one Res2Net block
#define ECAPA_R2_MARGIN 28          // 7 stages x the largest dilation (4): recomputed halo on each side
#define ECAPA_R2_STAGES 7
#define ECAPA_R2_WFRAG (3 * 4 * 8 * 64 * 8)   // bf16 elements of one stage's packed weights (96 KB)

struct EcapaCrops {
  const int* row_off; const int* frames;   // device
  int n, max_frames;
};

// window [400] and mel filters [80][201] (host) -> window-folded DFT tables [400][208] x 2 and the padded filter matrix [80][208]
void ccx_ecapa_fbank_tables(const float* window, const float* filters, std::vector<float>& dft_cos, std::vector<float>& dft_sin,
                            std::vector<float>& filt);
// Conv1d weights [7][128][128][3] of one SE-Res2Net block (host) -> MFMA fragment order [7][3 taps][4 k steps][8 tiles][64 lanes][8]
void ccx_ecapa_pack_res2net(const float* w, std::vector<float>& frag);

// crop samples -> normalised log-mel features bf16 [rows][80] with halos.  raw f32 [rows][80], gmax [n], part f32 [n][16][80]: scratch
int ccx_launch_ecapa_fbank(ccx_ctx* ctx, const float* wav, const long* crop_off, const int* crop_len, const EcapaCrops& cr,
                           const float* dft_cos, const float* dft_sin, const float* filt, float* raw, unsigned int* gmax, float* part,
                           bf16_t* feats, hipStream_t st);
// reflection halos of a [rows][C] buffer (C % 8 == 0) from its valid rows
int ccx_launch_ecapa_halo(ccx_ctx* ctx, bf16_t* buf, long ld, int C, const EcapaCrops& cr, hipStream_t st);
// the seven dependent dilated convolutions of one SE-Res2Net block: x [rows][ldx] (1024 live columns) -> y [rows][ldy], halos written
int ccx_launch_ecapa_res2net(ccx_ctx* ctx, const bf16_t* x, long ldx, bf16_t* y, long ldy, const EcapaCrops& cr, const bf16_t* wfrag,
                             const float* aff /* [7][bias|scale|shift][128] */, int dilation, hipStream_t st);
// squeeze-excitation: mean over valid rows -> gates = sigmoid(W2 relu(W1 mean + b1) + b2) -> y = gates * x + resid (all rows, halos too)
int ccx_launch_ecapa_se(ccx_ctx* ctx, const bf16_t* x, long ldx, const bf16_t* resid, long ldr, bf16_t* y, long ldy, const EcapaCrops& cr,
                        const float* w1, const float* b1, const float* w2, const float* b2, float* mean /* [n][1024] */,
                        float* gates /* [n][1024] */, hipStream_t st);
// per-crop column mean and std = sqrt(max(sum (x - mean)^2 / T, 1e-12)) over valid rows -> stat f32 [n][2 C] (mean | std)
int ccx_launch_ecapa_ctx_stats(ccx_ctx* ctx, const bf16_t* x, long ldx, int C, const EcapaCrops& cr, float* stat, hipStream_t st);
// attentive statistics pooling: logits = hidden W^T + b formed on the MFMA, softmax over the crop's frames per channel, weighted mean and
// std of x, then the affine of asp_bn -> out bf16 [n][2 C] (mean | std).  C % 64 == 0.
int ccx_launch_ecapa_asp_pool(ccx_ctx* ctx, const bf16_t* hidden, const bf16_t* x, long ldx, int C, const EcapaCrops& cr, const bf16_t* wa,
                              const float* ba, const float* bn_scale, const float* bn_shift, bf16_t* out, hipStream_t st);
